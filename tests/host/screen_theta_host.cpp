// Host-side calls of the batch screen's theta rule (screen_bound.h): the functions k_screen_flag (pss_xcorr_i8.hip) decides by --
// lcs_screen_in_s, lcs_screen_lower, lcs_screen_decide, lcs_screen_hot -- and, around them, a buffer's rule as a serial loop in the
// kernel's order of steps.  The header is all this file includes.  tests/test_screen_theta_host.py and tests/test_gpu_screen_theta.py
// model the kernel with it.  Test infrastructure.
#include "../../lte-cell-scanner_amd/csrc/screen_bound.h"

extern "C" double theta_lower(int n_comb, int ds, double sc, double vs) { return lcs_screen_lower(n_comb, ds, sc, vs); }
extern "C" int theta_in_s(int n_comb, int ds, double sc, double z, double vs) { return lcs_screen_in_s(n_comb, ds, sc, z, vs) ? 1 : 0; }
extern "C" int theta_decide(int n_comb, int ds, double sc, double lmin, float *theta, double *T) { return lcs_screen_decide(n_comb, ds, sc, lmin, theta, T); }
extern "C" int theta_hot(double T, double vs) { return lcs_screen_hot(T, vs) ? 1 : 0; }

static void flag_entry(int idx, int ds, int n_idx, int tile_lags, int *flags) {
  const int lo = idx - ds < 0 ? idx - ds + n_idx : idx - ds, hi = idx + ds >= n_idx ? idx + ds - n_idx : idx + ds;
  flags[idx / tile_lags] = 1; flags[lo / tile_lags] = 1; flags[hi / tile_lags] = 1;
}
static void flag_all(int n_idx, int tile_lags, int *flags) {
  for (int t = 0; t < (n_idx + tile_lags - 1) / tile_lags; ++t) flags[t] = 1;
}

// One buffer by the theta rule.  z[n_idx]: the thresholds; vs[3 * n_idx]: the screened collapsed powers (PSS-major); sc: the buffer's
// largest column scale.  flags[ceil(n_idx / tile_lags)] <- 0 / 1; *theta, *T as lcs_screen_decide leaves them; *n_s = |S|.  Returns the mode.
extern "C" int theta_rule(int n_comb, int ds, double sc, const double *z, const float *vs, int n_idx, int tile_lags, int *flags, float *theta, double *T,
                          int *n_s) {
  const int n_tiles = (n_idx + tile_lags - 1) / tile_lags;
  for (int t = 0; t < n_tiles; ++t) flags[t] = 0;
  *theta = 0.f; *T = -1.0; *n_s = 0;
  double zm = INFINITY;
  bool bad = false;
  for (int i = 0; i < n_idx; ++i) { bad |= !(z[i] > 0.0 && z[i] < INFINITY); zm = fmin(zm, z[i]); }
  for (int e = 0; e < 3 * n_idx; ++e) bad |= !(vs[e] > 0.f && vs[e] < INFINITY);
  if (bad || !(lcs_screen_threshold(n_comb, ds, sc, zm) > 0.0)) { flag_all(n_idx, tile_lags, flags); return LCS_SCREEN_ALL; }
  double lm = INFINITY;
  for (int e = 0; e < 3 * n_idx; ++e)
    if (lcs_screen_in_s(n_comb, ds, sc, z[e % n_idx], (double)vs[e])) { lm = fmin(lm, lcs_screen_lower(n_comb, ds, sc, (double)vs[e])); ++*n_s; }
  const int mode = lcs_screen_decide(n_comb, ds, sc, lm, theta, T);
  if (mode == LCS_SCREEN_ALL) flag_all(n_idx, tile_lags, flags);
  else if (mode == LCS_SCREEN_BY_T)
    for (int e = 0; e < 3 * n_idx; ++e)
      if (lcs_screen_hot(*T, (double)vs[e])) flag_entry(e % n_idx, ds, n_idx, tile_lags, flags);
  return mode;
}

// The rule this one replaces, for comparison: hot = not below T(the buffer's smallest threshold).  Returns 1 if it flagged everything.
extern "C" int zmin_rule(int n_comb, int ds, double sc, const double *z, const float *vs, int n_idx, int tile_lags, int *flags, double *T) {
  const int n_tiles = (n_idx + tile_lags - 1) / tile_lags;
  for (int t = 0; t < n_tiles; ++t) flags[t] = 0;
  double zm = INFINITY;
  bool bad = false;
  for (int i = 0; i < n_idx; ++i) { bad |= !(z[i] > 0.0); zm = fmin(zm, z[i]); }
  *T = bad ? -1.0 : lcs_screen_threshold(n_comb, ds, sc, zm);
  if (!(*T > 0.0)) { flag_all(n_idx, tile_lags, flags); return 1; }
  for (int e = 0; e < 3 * n_idx; ++e)
    if (!((double)vs[e] < *T)) flag_entry(e % n_idx, ds, n_idx, tile_lags, flags);
  return 0;
}
