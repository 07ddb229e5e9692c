// pss_ref.h -- the pieces of the reference's PSS arithmetic that several kernels, and the host, must form IDENTICALLY: each is written
// here once, __host__ __device__, and tests/test_pss_ref_host.py pins the host compilation of the same text to NumPy and the oracle.
//   window geometry   lcs_win_start / lcs_group_span: the window starts the host packs a grid by (pack_grid) are the ones the
//                     kernels subtract from an LDS row base (k_prep_tables, k_frq_repair's remote winner)
//   correlation       pss_tmpl_tap / pss_tap_sum / pss_xc_round / pss_xc_sq: "the reference's own arithmetic" of DESIGN 3.2a
//                     (k_prep_tables, k_xc_debug, k_frq_repair, k_single_exact)
//   threshold         SpArgs / make_sp_args / lcs_z_th1 (k_sp_fold, k_sp_i8, k_foe_unpack)
#pragma once
#include <algorithm>
#include <cmath>
#include "lcs_internal.h"

// ---- window geometry --------------------------------------------------------------------------------------------------------
// round_i(w*.005*k_factor*fs_programmed), evaluated left to right (ref src/searcher.cpp:298)
__host__ __device__ static inline int lcs_win_start(const SlotParams &p, double f_off, int w) {
  return (int)rint((((double)w * .005) * ((p.fc_req - f_off) / p.fc_prog)) * p.fs_prog);
}
// smallest and largest window start among the hypotheses that have a template in group g, in window w (a group spans at most 7)
struct WinSpan { int mn, mx; };
__host__ __device__ static inline WinSpan lcs_group_span(const XcGeom &geo, const SlotParams &p, const double *fset, int g, int w) {
  const int c_end = g * geo.cpg + geo.cpg - 1, c_hi = c_end < geo.n_tmpl - 1 ? c_end : geo.n_tmpl - 1;
  const int f_lo = (g * geo.cpg) / 3, f_hi = c_hi / 3;
  WinSpan r;
  r.mn = r.mx = lcs_win_start(p, fset[f_lo], w);
  for (int f = f_lo + 1; f <= f_hi; ++f) {
    const int s = lcs_win_start(p, fset[f], w);
    r.mn = s < r.mn ? s : r.mn;
    r.mx = s > r.mx ? s : r.mx;
  }
  return r;
}

inline XcGeom make_geo(uint32_t n_cap, int n_f, int ds, int cpg = LCS_TG) {
  XcGeom g;
  g.n_cap = n_cap;
  g.n_f = n_f;
  g.n_tmpl = 3 * n_f;
  g.cpg = cpg;
  g.G = (g.n_tmpl + cpg - 1) / cpg;
  g.n_comb = (int)((n_cap - 136 - 100) / 9600);   // ref src/searcher.cpp:276
  g.ds = ds;
  g.foi0 = 0;
  g.n_narrow = (n_f == 1 || cpg == 3) ? g.n_comb : 0;     // one hypothesis per group: no spread at all; otherwise pack_grid looks at the grid
  return g;
}

// One walk over the (window, group) pairs of a frequency grid packed `cpg` template columns per group: the largest spread of the
// window starts inside one template group (the correlation kernels hold 137 taps + that spread), and the number of leading
// combining windows in which every group's spread stays within LCS_NARROW_SPREAD samples (the spread grows with the window
// index; the count stops at the first window that exceeds it).
struct GridSpread { int worst, n_narrow; };
inline GridSpread grid_spread(const XcGeom &geo, const double *fset, const SlotParams &p) {
  GridSpread r{0, geo.n_comb};
  for (int w = 0; w < geo.n_comb; ++w)
    for (int g = 0; g < geo.G; ++g) {
      const WinSpan s = lcs_group_span(geo, p, fset, g, w);
      r.worst = std::max(r.worst, s.mx - s.mn);
      if (s.mx - s.mn > LCS_NARROW_SPREAD) r.n_narrow = std::min(r.n_narrow, w);
    }
  return r;
}

// Choose how the 3 n_f templates are packed into 16-column groups: densely when the window starts of a group's
// hypotheses stay within `max_taps` - 137 samples of each other over the whole buffer (every grid the CLI builds), else
// with fewer whole hypotheses per group -- one per group always fits (its three templates share a window start).
inline XcGeom pack_grid(uint32_t n_cap, int n_f, int ds, const double *fset, const double *fc_req, const double *fc_prog, int n_buf,
                        double fs_prog, int max_taps) {
  static const int packings[] = {LCS_TG, 15, 12, 9, 6, 3};
  for (int cpg : packings) {
    XcGeom geo = make_geo(n_cap, n_f, ds, cpg);
    GridSpread all{0, geo.n_comb};
    for (int i = 0; i < n_buf && (cpg == 3 || 137 + all.worst <= max_taps); ++i)      // (a packing that does not fit is left at once)
      if (i == 0 || fc_req[i] != fc_req[i - 1] || fc_prog[i] != fc_prog[i - 1]) {
        const GridSpread s = grid_spread(geo, fset, SlotParams{fc_req[i], fc_prog[i], fs_prog});
        all = GridSpread{std::max(all.worst, s.worst), std::min(all.n_narrow, s.n_narrow)};
      }
    if (137 + all.worst <= max_taps || cpg == 3) {
      geo.n_narrow = all.n_narrow;
      return geo;
    }
  }
  return make_geo(n_cap, n_f, ds, 3);
}

// ---- PSS correlation in the reference's arithmetic ----------------------------------------------------------------------------
// tap m of conj(fshift(pss_td, f_off, fs_programmed * k_factor)) / 137 in double (ref :146-151, dsp.h:40-53); s = pss_td[t][m]
__host__ __device__ __forceinline__ double2 pss_tmpl_tap(const SlotParams &p, double f_off, double2 s, int m) {
  const double kf = (p.fc_req - f_off) / p.fc_prog;
  const double k = M_PI * f_off / ((p.fs_prog * kf) / 2);
  double sn, cs;
  sincos(k * (double)m, &sn, &cs);
  return make_double2((s.x * cs - s.y * sn) / 137, -(s.x * sn + s.y * cs) / 137);      // seq * coeff, conjugated
}
// xc[t][k][foi] before it is stored: the 137 terms added in tap order in double (ref :160-169).  x: samples in the source's own
// format (CapKind<KIND>::T).  UNROLL8: eight taps' operand reads in flight; the sums stay in tap order either way.
template <int KIND> __host__ __device__ __forceinline__ void pss_tap(double2 &acc, double2 a, typename CapKind<KIND>::T raw) {
  const double2 b = CapKind<KIND>::cvt(raw);
  acc.x += a.x * b.x - a.y * b.y;
  acc.y += a.x * b.y + a.y * b.x;
}
template <int KIND, bool UNROLL8>
__host__ __device__ __forceinline__ double2 pss_tap_sum(const double2 *tmpl, const typename CapKind<KIND>::T *x) {
  double2 acc = make_double2(0.0, 0.0);
  if (UNROLL8) {
#pragma unroll 8
    for (int m = 0; m < 137; ++m) pss_tap<KIND>(acc, tmpl[m], x[m]);
  } else {
    for (int m = 0; m < 137; ++m) pss_tap<KIND>(acc, tmpl[m], x[m]);
  }
  return acc;
}
// xc is complex<float> (:136); xc_incoherent_single adds its square formed in double (:299-305)
__host__ __device__ __forceinline__ float2 pss_xc_round(double2 acc) { return make_float2((float)acc.x, (float)acc.y); }
__host__ __device__ __forceinline__ double pss_xc_sq(double2 acc) {
  const float2 f = pss_xc_round(acc);
  return (double)f.x * (double)f.x + (double)f.y * (double)f.y;
}

// ---- detection threshold (ref src/CellSearch.cpp:500-503) ---------------------------------------------------------------------
struct SpArgs {
  int n_comb_sp;
  double R_th1, rx_cutoff;
  int n_comb_xc, ds;
};
inline SpArgs make_sp_args(const XcGeom &geo) {
  SpArgs a;
  a.n_comb_sp = (int)((geo.n_cap - 136 - 137) / 9600);
  a.n_comb_xc = geo.n_comb;
  a.ds = geo.ds;
  a.R_th1 = lcs_tables::chi2cdf_inv(1 - pow(10.0, -12), 2.0 * geo.n_comb * (2 * geo.ds + 1));
  a.rx_cutoff = (6 * 12 * 15e3 / 2 + 4 * 15e3) / (FS_LTE / 16 / 2);
  return a;
}
// Z_th1 of a position whose sp_incoherent is v
__host__ __device__ __forceinline__ double lcs_z_th1(const SpArgs &a, double v) {
  return a.R_th1 * v / a.rx_cutoff / 137 / 2 / a.n_comb_xc / (2 * a.ds + 1);
}
