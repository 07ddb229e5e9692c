// cell_meas.h -- RSRP, RSSI, RSRQ and the noise power of a cell from its cell-specific reference signals (36.214 5.1.1, 5.1.3;
// lcs_set_cell_meas, lcs_cell_meas; the rule is stated in include/lcs.h), over n_rb resource blocks: six here, more in
// cell_meas_wide.h.
//
// Of the grid tfg[n_ofdm][12 n_rb] (row 0 = slot 0 symbol 0 of a frame) only port 0's reference rows take part, enumerated as
// tdd_config.h does: reference row q is grid row tdd_grid_row(q, n_symb) and falls into bin b = q mod 40 = 4 s + j (subframe s, row j
// of the subframe); a bin takes part iff bit s of the 10-bit dl_mask is set.  Ports 0 and 1 have their reference signals on these
// rows, with the row's RS_DL sequence rs and first subcarriers shift_0, shift_1.  Per used row and port p, with N = 2 n_rb entries,
//   h_m = tfg[row][shift_p + 6 m] conj(rs[m]) (m < N),  a_p = sum_{m<N-1} h_m conj(h_{m+1}),  e_p = sum_{m<N} |h_m|^2
// and per used row w = sum_k |tfg[row][k]|^2.  Over the n_rows used rows A_p, E_p, W are their sums, and (meas_numbers)
//   rsrp[p] = |A_p| / ((N - 1) n_rows),  noise[p] = E_p / (N n_rows) - rsrp[p],  rssi = W / n_rows,  rsrq = n_rb rsrp[0] / rssi.
//
// THE ORDER OF EVERY SUM IS FIXED HERE, so that the kernels (cell_meas.hip: k_cell_meas; tfg_wide.hip: k_cell_meas_wide) and the
// host twins (tests/host/cell_meas_host.cpp, meas_wide_host.cpp) perform the same additions.  A row has L lanes, a power of two
// (the kernels: lanes of a wave): 16 here, and N = 12 of them hold an entry.  Entry m < N holds the subcarriers 6 m .. 6 m + 5
// and contributes MEAS_NV = 7 values (meas_entry):
//   a_p       h_m conj(h_{m+1}) for m < N - 1, else 0 (re and im: two values per port)
//   e_p       h_m.re^2 + h_m.im^2
//   w         ((((|x_0|^2 + |x_1|^2) + |x_2|^2) + |x_3|^2) + |x_4|^2) + |x_5|^2 over the entry's six subcarriers, |x|^2 = re^2 + im^2
// a lane without an entry holds zeros.  Then, for each of the seven values on its own:
//   per row   the butterfly over the L lanes: v[i] += v[i ^ off] for off = L / 2, .., 2, 1 (meas_row_sum, meas_row_sum_lanes)
//   per bin   the bin's rows in row order (q = b, b + 40, ..), starting from the first row itself (meas_bin_sum)
//   total     0 + the bins of the mask in increasing b (meas_total)
// Plain fp64, compiled with -ffp-contract=off on both sides.
#pragma once
#include <math.h>
#include "tdd_config.h"

#define MEAS_NV 7            // values a row is reduced to: A_0 (re, im), A_1 (re, im), E_0, E_1, W
enum { MEAS_A0_RE = 0, MEAS_A0_IM, MEAS_A1_RE, MEAS_A1_IM, MEAS_E0, MEAS_E1, MEAS_W };

// 36.211 table 4.2-2: the downlink subframes of an uplink-downlink configuration as a mask (bit s = subframe s), special subframes
// excluded; -1 for anything that is no configuration
__host__ __device__ __forceinline__ int meas_tdd_dl_mask(int ul_dl_config) {
  switch (ul_dl_config) {
    case 0: return 0x021;      // DSUUUDSUUU
    case 1: return 0x231;      // DSUUDDSUUD
    case 2: return 0x339;      // DSUDDDSUDD
    case 3: return 0x3e1;      // DSUUUDDDDD
    case 4: return 0x3f1;      // DSUUDDDDDD
    case 5: return 0x3f9;      // DSUDDDDDDD
    case 6: return 0x221;      // DSUUUDSUUD
    default: return -1;
  }
}
__host__ __device__ __forceinline__ bool meas_mask_ok(int dl_mask) { return dl_mask > 0 && dl_mask <= 0x3ff; }
__host__ __device__ __forceinline__ bool meas_bin_used(int b, int dl_mask) { return (dl_mask >> (b >> 2)) & 1; }
// ports measured by the cell's antenna ports (0 / unknown: port 0 alone)
__host__ __device__ __forceinline__ int meas_ports(int n_ports) { return n_ports >= 2 ? 2 : 1; }

__host__ __device__ __forceinline__ double meas_abs2(double re, double im) { return re * re + im * im; }
// The entry's six subcarriers travel as six values, never as an array: one of them is picked by selects, and the compiler turns
// selects among the elements of an array into a run-time index, which sends the array to scratch.
struct meas_x6 { cd2 x0, x1, x2, x3, x4, x5; };
__host__ __device__ __forceinline__ cd2 meas_sel(bool take, cd2 a, cd2 b) { return mk(take ? a.re : b.re, take ? a.im : b.im); }
__host__ __device__ __forceinline__ cd2 meas_pick(const meas_x6 &x, int k) {
  cd2 v = x.x0;
  v = meas_sel(k == 1, x.x1, v); v = meas_sel(k == 2, x.x2, v); v = meas_sel(k == 3, x.x3, v);
  v = meas_sel(k == 4, x.x4, v); v = meas_sel(k == 5, x.x5, v);
  return v;
}
// h of entry m for one port: x = the entry's six subcarriers, shift = the port's first subcarrier (0 .. 5)
__host__ __device__ __forceinline__ cd2 meas_h(const meas_x6 &x, int shift, cd2 rs) { return tdd_h(meas_pick(x, shift), rs); }
// the seven values of entry m (< n_ent) from its h and its right neighbour's (h_next: entry m + 1's, anything for the last), per port;
// n_ent = 2 n_rb: twelve for the chain's grid, the spelling the 6-RB host twin keeps
__host__ __device__ __forceinline__ void meas_entry(const meas_x6 &x, int m, int ports, cd2 h0, cd2 h0_next, cd2 h1, cd2 h1_next,
                                                    double (&v)[MEAS_NV], int n_ent = 12) {
  const cd2 p0 = tdd_pair(h0, h0_next), p1 = tdd_pair(h1, h1_next);
  const bool pair = m < n_ent - 1, two = ports >= 2;
  v[MEAS_A0_RE] = pair ? p0.re : 0.0;
  v[MEAS_A0_IM] = pair ? p0.im : 0.0;
  v[MEAS_A1_RE] = (pair && two) ? p1.re : 0.0;
  v[MEAS_A1_IM] = (pair && two) ? p1.im : 0.0;
  v[MEAS_E0] = meas_abs2(h0.re, h0.im);
  v[MEAS_E1] = two ? meas_abs2(h1.re, h1.im) : 0.0;
  double w = meas_abs2(x.x0.re, x.x0.im);
  w = w + meas_abs2(x.x1.re, x.x1.im); w = w + meas_abs2(x.x2.re, x.x2.im); w = w + meas_abs2(x.x3.re, x.x3.im);
  w = w + meas_abs2(x.x4.re, x.x4.im); w = w + meas_abs2(x.x5.re, x.x5.im);
  v[MEAS_W] = w;
}
// one value of a row from its LANES lanes (host form; the kernels' is meas_row_sum_lanes)
template <int LANES = TDD_ROW_LANES> __host__ __device__ inline double meas_row_sum(const double *p) {
  double v[LANES], w[LANES];
  for (int i = 0; i < LANES; ++i) v[i] = p[i];
  for (int off = LANES / 2; off >= 1; off >>= 1) {
    for (int i = 0; i < LANES; ++i) w[i] = v[i] + v[i ^ off];
    for (int i = 0; i < LANES; ++i) v[i] = w[i];
  }
  return v[0];
}
#ifdef __HIPCC__
template <int LANES> __device__ __forceinline__ double meas_row_sum_lanes(double v) {
#pragma unroll
  for (int off = LANES / 2; off >= 1; off >>= 1) v = v + __shfl_xor(v, off);
  return v;
}
#endif
// one value of bin b from the per-row values r[q], q < n_q
__host__ __device__ __forceinline__ double meas_bin_sum(const double *r, int b, int n_q) {
  if (b >= n_q) return 0.0;
  double s = r[b];
  for (int q = b + TDD_BINS; q < n_q; q += TDD_BINS) s = s + r[q];
  return s;
}
// one value's total over the bins of the mask
__host__ __device__ __forceinline__ double meas_total(const double *bin /*[40]*/, int dl_mask) {
  double s = 0.0;
  for (int b = 0; b < TDD_BINS; ++b) if (meas_bin_used(b, dl_mask)) s = s + bin[b];
  return s;
}
// used rows among n_q reference rows
__host__ __device__ __forceinline__ int meas_n_rows(int n_q, int dl_mask) {
  int n = 0;
  for (int b = 0; b < TDD_BINS; ++b) if (meas_bin_used(b, dl_mask)) n += tdd_bin_count(b, n_q);
  return n;
}

__host__ __device__ __forceinline__ void meas_clear(lcs_meas_info *o, int status) {
  o->status = status; o->n_rows = status; o->n_ports = status; o->dl_mask = status;
  o->rsrp[0] = o->rsrp[1] = o->noise[0] = o->noise[1] = o->rssi = o->rsrq = 0.0;
  for (int i = 0; i < 4; ++i) { o->a_re_im[i] = 0.0; o->reserved[i] = 0.0; }
}
// The numbers of a record (lcs_meas_info, lcs_meas_wide_info: the fields have the same names) from the totals over n_ent = 2 n_rb
// entries per row, and status 0 with them: that field says whether there is a number.  There is none -- the record stays as it is --
// without a used row, with an rssi of zero, or when a total or a result is not finite.  (Port 1's totals are exact zeros where it
// is not measured: meas_entry.)  It returns nothing: with a verdict for a return value k_cell_meas's one-thread tail compiles to
// other code than it always had, and read from the status k_cell_meas_wide_fin's does -- the stage's launch-bound last kernel.
template <class Rec> __host__ __device__ __forceinline__ void meas_numbers(const double *tot /*[MEAS_NV]*/, int n_rows, int n_ent, int n_rb, Rec *o) {
  if (n_rows <= 0) return;
  const double a0r = tot[MEAS_A0_RE], a0i = tot[MEAS_A0_IM], a1r = tot[MEAS_A1_RE], a1i = tot[MEAS_A1_IM];
  const double rssi = tot[MEAS_W] / (double)n_rows;
  const double rsrp0 = sqrt(a0r * a0r + a0i * a0i) / (double)((n_ent - 1) * n_rows), rsrp1 = sqrt(a1r * a1r + a1i * a1i) / (double)((n_ent - 1) * n_rows);
  const double noise0 = tot[MEAS_E0] / (double)(n_ent * n_rows) - rsrp0, noise1 = tot[MEAS_E1] / (double)(n_ent * n_rows) - rsrp1;
  const double rsrq = (double)n_rb * rsrp0 / rssi;
  const bool ok = isfinite(a0r) && isfinite(a0i) && isfinite(a1r) && isfinite(a1i) && isfinite(tot[MEAS_E0]) && isfinite(tot[MEAS_E1]) &&
                  isfinite(tot[MEAS_W]) && rssi > 0.0 && isfinite(rssi) && isfinite(rsrp0) && isfinite(rsrp1) && isfinite(noise0) &&
                  isfinite(noise1) && isfinite(rsrq);
  if (!ok) return;
  o->status = 0;
  o->rsrp[0] = rsrp0; o->rsrp[1] = rsrp1;
  o->noise[0] = noise0; o->noise[1] = noise1;
  o->rssi = rssi;
  o->rsrq = rsrq;
  o->a_re_im[0] = a0r; o->a_re_im[1] = a0i; o->a_re_im[2] = a1r; o->a_re_im[3] = a1i;
}
// The record from the totals: without a number status -1, every double 0, the integers as they are
__host__ __device__ inline void meas_finish(const double *tot /*[MEAS_NV]*/, int n_rows, int ports, int dl_mask, lcs_meas_info *o) {
  meas_clear(o, -1);
  o->n_rows = n_rows; o->n_ports = ports; o->dl_mask = dl_mask;
  meas_numbers(tot, n_rows, 12, 6, o);
}
