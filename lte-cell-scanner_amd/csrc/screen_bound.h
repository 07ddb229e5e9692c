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
