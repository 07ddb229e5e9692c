// screen_bound.h -- how far the two-digit screen of the int8 PSS correlation (pss_xcorr_i8.hip: k_xcorr_i8x3<2, .>) can lie from the
// three-digit kernel, as one function that the flag kernel and tests/test_screen_bound_host.py share.  Plain C++, no HIP, no context.
//
// The screen drops digit 0 of the 24-bit template integers: per tap component an integer in [-128, 127].  A window's complex integer
// correlation therefore moves by at most  E = sqrt(2) * 128 * sum_k (|a_re| + |a_im|) <= sqrt(2) * 128 * 274 * 128  (each of the two
// output components by at most 128 * sum; 137 taps, samples in [-128, 127]).  With x_w the exact and x_w + d_w the screened
// correlation of window w, P = sum_w |x_w|^2 over n windows:
//     |P' - P| <= 2 sum |x_w| |d_w| + sum |d_w|^2 <= 2 E sqrt(n P) + n E^2                                   (Cauchy-Schwarz)
// In the kernel's output units v = P sc^2 / n (sc = 1 / (128 q), the column's scale) and with e = E sc this reads
//     |v' - v| <= 2 e sqrt(v) + e^2 =: B_e(v),
// independent of n.  B_e is increasing and concave in v, so the bound survives the box filter over 2 ds + 1 lags (mean of the bounds
// <= bound of the mean) and, taken with the largest e of a buffer's columns, the maximum over the hypotheses (both monotone).  Hence
// for a collapsed power V and its screened twin V':  V >= Z  implies  V' >= Z - B_e(Z)  wherever v - B_e(v) is increasing, that is
// for Z > e^2.  What the fp32 arithmetic of the two epilogues adds is covered by an explicit relative slack (below).
#pragma once
#include <cmath>

#if defined(__HIP__) || defined(__host__)
#define LCS_SCREEN_HD __host__ __device__
#else
#define LCS_SCREEN_HD
#endif

// e = E sc for a column (or a buffer's largest) scale; the constant is sqrt(2) rounded up
LCS_SCREEN_HD static inline double lcs_screen_err(double sc) { return (1.4142135623730951 * 128.0 * 274.0 * 128.0) * sc; }
// B_e(v): how far a screened value of exact power v (a single element, a box-filtered one, a collapsed one) can lie from it
LCS_SCREEN_HD static inline double lcs_screen_bound(double e, double v) { return 2.0 * e * sqrt(v) + e * e; }
// The fp32 roundings: per window an epilogue rounds at most 4 times (the integer to float, the recombination, two fused
// multiply-adds into the running sum), then twice for scale and division, and the collapse 2 ds + 2 times (box filter, division);
// every partial sum is a sum of non-negative terms, so each rounding costs at most 2^-24 of the value, in each of the two kernels:
// (4 n + 2 ds + 4) 2^-23 in all.  The function grants 4 (n + 2 ds + 1) + 16 units of 2^-23, and 4e-7 for the ~1e-7 between the kernel's
// arithmetic and the reference's at positions the tie repair rewrites (k_frq_repair).
LCS_SCREEN_HD static inline double lcs_screen_slack(int n_comb, int ds) { return ldexp(4.0 * (double)(n_comb + 2 * ds + 1) + 16.0, -23) + 4e-7; }
// T(Z): a screened collapsed power below T belongs to an exact collapsed power that is certainly below Z.  Negative: no such value
// exists -- Z is not above e^2 (v - B_e(v) is not increasing there: a silent buffer), T would not be positive, or an input is not a
// positive finite number -- and the caller flags everything.
LCS_SCREEN_HD static inline double lcs_screen_threshold(int n_comb, int ds, double sc, double Z) {
  const double e = lcs_screen_err(sc);
  if (!(Z > 0.0) || !(sc > 0.0) || !(Z < INFINITY) || !(e < INFINITY)) return -1.0;
  if (!(Z > e * e)) return -1.0;
  const double T = (Z - lcs_screen_bound(e, Z)) * (1.0 - lcs_screen_slack(n_comb, ds));
  return T > 0.0 ? T : -1.0;
}

// ---------------------------------------------------------------- the theta rule: refine down to theta, not to the smallest threshold
// The other direction of the same inequality.  |v' - v| <= 2 e sqrt(v) + e^2 gives v' <= (sqrt(v) + e)^2, so sqrt(v) >= sqrt(v') - e and
//     v >= L_e(v') := max(sqrt(v') - e, 0)^2:
// a LOWER bound of the exact power from the screened one.  It carries through the box filter and the maximum like B_e does: with
// m = mean of the box's exact values and m' of their screened twins, m' <= mean (sqrt(v_i) + e)^2 = m + 2 e mean sqrt(v_i) + e^2
// <= (sqrt(m) + e)^2 (sqrt is concave), hence m >= L_e(m'); and with the largest e of the buffer's columns (L_e decreases in e) the
// hypothesis that holds the screened maximum V' has an exact box value >= L_e(V'), so the exact maximum V >= L_e(V') (L_e increases in v').
// The fp32 roundings: the screened kernel's float is at most (1 + s) times its real-arithmetic value and the exact kernel's float at
// least (1 - s) times its own, s = (4 n + 2 ds + 4) 2^-24 each (lcs_screen_slack's count); the repaired positions add the 4e-7.  A
// relative slack does not pass through sqrt(v') - e unchanged, so it is applied on both sides of it -- to the argument and to the result,
// lcs_screen_slack each time (1 / (1 + s) >= 1 - slack, and L_e increases in its argument).
LCS_SCREEN_HD static inline double lcs_screen_lower(int n_comb, int ds, double sc, double vs) {
  const double e = lcs_screen_err(sc), k = 1.0 - lcs_screen_slack(n_comb, ds);
  const double r = sqrt(vs * k) - e;
  return r > 0.0 ? r * r * k : 0.0;      // (a NaN gives 0: theta <= e^2, everything is flagged)
}
// The rule of a buffer, with its largest column scale sc.  S = the entries (PSS, lag) whose screened collapsed power V'
// is not below T(z[lag]) -- hot against their OWN threshold; theta = the smallest L_e(V') over S, rounded down to float; an entry is hot
// when V' is not below T(theta).  The three steps below are the text both k_screen_flag and the host tests run.
// step 1, per entry: is it in S?  (No usable T(z): it is.)
LCS_SCREEN_HD static inline bool lcs_screen_in_s(int n_comb, int ds, double sc, double z, double vs) {
  return !(vs < lcs_screen_threshold(n_comb, ds, sc, z));
}
// step 2, per buffer: from lmin = the minimum of lcs_screen_lower over S (INFINITY: S is empty) to theta and T(theta).
// 0: S is empty -- nothing can be recorded, nothing is flagged; 1: *T > 0 decides; 2: flag every tile (theta <= e^2 or T(theta) not positive).
// Whoever found a z or a V' that is not a positive finite number flags every tile without asking.
#define LCS_SCREEN_NONE 0
#define LCS_SCREEN_BY_T 1
#define LCS_SCREEN_ALL 2
LCS_SCREEN_HD static inline int lcs_screen_decide(int n_comb, int ds, double sc, double lmin, float *theta, double *T) {
  *theta = 0.f;
  *T = -1.0;
  if (lmin == INFINITY) return LCS_SCREEN_NONE;
  if (!(lmin > 0.0) || !(lmin < 3.0e38)) return LCS_SCREEN_ALL;
  float tf = (float)lmin;
  if ((double)tf > lmin) tf = nextafterf(tf, 0.f);      // rounded DOWN: theta stays a lower bound of every exact value in S
  if (!(tf > 0.f)) return LCS_SCREEN_ALL;
  *T = lcs_screen_threshold(n_comb, ds, sc, (double)tf);      // -1: theta <= e^2, or T not positive
  if (!(*T > 0.0)) return LCS_SCREEN_ALL;
  *theta = tf;
  return LCS_SCREEN_BY_T;
}
// step 3, per entry: hot -- its box is redone with three digits (a NaN is hot)
LCS_SCREEN_HD static inline bool lcs_screen_hot(double T, double vs) { return !(vs < T); }
