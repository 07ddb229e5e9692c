// Host-side calls of the batch screen's bound (screen_bound.h), the very functions k_screen_flag (pss_xcorr_i8.hip) decides by.  The
// header is all this file includes.  tests/test_screen_bound_host.py sets them against brute-force integer correlations.  Test
// infrastructure.
#include "../../lte-cell-scanner_amd/csrc/screen_bound.h"

extern "C" double screen_err(double sc) { return lcs_screen_err(sc); }
extern "C" double screen_bound(double e, double v) { return lcs_screen_bound(e, v); }
extern "C" double screen_slack(int n_comb, int ds) { return lcs_screen_slack(n_comb, ds); }
extern "C" double screen_threshold(int n_comb, int ds, double sc, double Z) { return lcs_screen_threshold(n_comb, ds, sc, Z); }
