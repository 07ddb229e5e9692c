// Host-side harness for foe_coarse.h (the same __host__ __device__ code k_foe_fin_unwrap runs; its lanes reduce in foe_half_sum's order): the half sums of one
// PSS window, the coarse estimate of a sum of terms and the decision that unwraps pss_sss_foe with it.  tests/test_foe_coarse_host.py
// compares them with the numpy reference (tests/pss_coarse_ref.py).  Test infrastructure.
#include "../../lte-cell-scanner_amd/csrc/foe_coarse.h"

// win, p: 128 complex samples (the capture at P_k .., the template behind its cyclic prefix); kph = -2 pi freq / fs.
// -> A, B (2 doubles each), *sum_abs = sum |z|
extern "C" void foe_host_halves(const double *win, double kph, const double *p, double *A, double *B, double *sum_abs) {
  cd2 z[2 * FOE_HALF];
  double s = 0;
  for (int t = 0; t < 2 * FOE_HALF; ++t) {
    z[t] = foe_halves_z(mk(win[2 * t], win[2 * t + 1]), mk(cos(kph * t), sin(kph * t)), mk(p[2 * t], p[2 * t + 1]));
    s += sqrt(z[t].re * z[t].re + z[t].im * z[t].im);
  }
  const cd2 a = foe_half_sum(z), b = foe_half_sum(z + FOE_HALF);
  A[0] = a.re; A[1] = a.im; B[0] = b.re; B[1] = b.im;
  *sum_abs = s;
}
// C = sum_k conj(A_k) B_k in occurrence order -> f_coarse; *usable as k_foe_fin_unwrap decides it
extern "C" double foe_host_coarse(const double *A, const double *B, int n_occ, double fs, double *C, int *usable) {
  cd2 c = mk(0, 0);
  for (int k = 0; k < n_occ; ++k) {
    const cd2 t = foe_halves_term(mk(A[2 * k], A[2 * k + 1]), mk(B[2 * k], B[2 * k + 1]));
    c.re += t.re; c.im += t.im;
  }
  C[0] = c.re; C[1] = c.im;
  *usable = foe_coarse_usable(c, n_occ) ? 1 : 0;
  return foe_coarse_hz(c, fs);
}
extern "C" int foe_host_usable(double c_re, double c_im, int n_occ) { return foe_coarse_usable(mk(c_re, c_im), n_occ) ? 1 : 0; }
extern "C" double foe_host_unwrap(double native, double freq, double f_coarse, double fs, int dist, int usable, int *n) {
  *n = foe_unwrap_n(native, freq, f_coarse, fs, dist, usable != 0);
  return foe_unwrap(native, freq, f_coarse, fs, dist, usable != 0);
}
