// Host-side harness for pss_ref.h: the window geometry, the grid packing and the PSS correlation "in the reference's own arithmetic"
// are __host__ __device__ (or plain host) code, so the text the kernels compile is compiled here for the CPU and
// tests/test_pss_ref_host.py pins it to NumPy and the oracle.  Test infrastructure.
#include "../../lte-cell-scanner_amd/csrc/pss_ref.h"

// out[w * n_f + i] = lcs_win_start(p, f[i], w)
extern "C" void pss_ref_win_start(double fc_req, double fc_prog, double fs_prog, const double *f, int n_f, int n_w, int *out) {
  const SlotParams p{fc_req, fc_prog, fs_prog};
  for (int w = 0; w < n_w; ++w)
    for (int i = 0; i < n_f; ++i) out[w * n_f + i] = lcs_win_start(p, f[i], w);
}

// the geometry of n_f hypotheses packed cpg columns per group: out[(w * G + g) * 2 + {0, 1}] = {min, max} of lcs_group_span.
// Returns G; *n_comb = windows.
extern "C" int pss_ref_group_span(unsigned n_cap, int n_f, int ds, int cpg, const double *fset, double fc_req, double fc_prog, double fs_prog,
                                  int *n_comb, int *out) {
  const XcGeom geo = make_geo(n_cap, n_f, ds, cpg);
  const SlotParams p{fc_req, fc_prog, fs_prog};
  *n_comb = geo.n_comb;
  if (out)
    for (int w = 0; w < geo.n_comb; ++w)
      for (int g = 0; g < geo.G; ++g) {
        const WinSpan s = lcs_group_span(geo, p, fset, g, w);
        out[(w * geo.G + g) * 2] = s.mn;
        out[(w * geo.G + g) * 2 + 1] = s.mx;
      }
  return geo.G;
}

// the library's own decision for one buffer: out = {cpg, G, n_narrow, n_comb}
extern "C" void pss_ref_pack_grid(unsigned n_cap, int n_f, int ds, const double *fset, double fc_req, double fc_prog, double fs_prog, int max_taps,
                                  int *out) {
  const XcGeom geo = pack_grid(n_cap, n_f, ds, fset, &fc_req, &fc_prog, 1, fs_prog, max_taps);
  out[0] = geo.cpg; out[1] = geo.G; out[2] = geo.n_narrow; out[3] = geo.n_comb;
}
extern "C" void pss_ref_limits(int *out) { out[0] = LCS_I8_MAX_TAPS; out[1] = 2 * (LCS_KP2_MAX - LCS_KP2_UNROLL); out[2] = LCS_NARROW_SPREAD; out[3] = LCS_NW_MAX; }

// n_pos correlations of 137 taps over samples x[k .. k + 136] of the given kind (0: int8 pairs 127 - u8 as uint16, 1: float2, 2: double2):
// xc[k] = the rounded complex<float>, sq[k] = its square in double; both loop forms of pss_tap_sum
template <int KIND> static void tap_sq(const double2 *tmpl, const void *x, int n_pos, int unroll8, float *xc, double *sq) {
  const typename CapKind<KIND>::T *s = static_cast<const typename CapKind<KIND>::T *>(x);
  for (int k = 0; k < n_pos; ++k) {
    const double2 a = unroll8 ? pss_tap_sum<KIND, true>(tmpl, s + k) : pss_tap_sum<KIND, false>(tmpl, s + k);
    const float2 r = pss_xc_round(a);
    xc[2 * k] = r.x; xc[2 * k + 1] = r.y;
    sq[k] = pss_xc_sq(a);
  }
}
extern "C" void pss_ref_tap_sq(int kind, const double *tmpl, const void *x, int n_pos, int unroll8, float *xc, double *sq) {
  const double2 *t = reinterpret_cast<const double2 *>(tmpl);
  if (kind == 0) tap_sq<0>(t, x, n_pos, unroll8, xc, sq);
  else if (kind == 1) tap_sq<1>(t, x, n_pos, unroll8, xc, sq);
  else tap_sq<2>(t, x, n_pos, unroll8, xc, sq);
}

// out[m] = pss_tmpl_tap(p, f_off, pss_td[m], m), m = 0 .. 136 (re, im interleaved)
extern "C" void pss_ref_tmpl(double fc_req, double fc_prog, double fs_prog, double f_off, const double *pss_td, double *out) {
  const SlotParams p{fc_req, fc_prog, fs_prog};
  for (int m = 0; m < 137; ++m) {
    const double2 v = pss_tmpl_tap(p, f_off, make_double2(pss_td[2 * m], pss_td[2 * m + 1]), m);
    out[2 * m] = v.x; out[2 * m + 1] = v.y;
  }
}
