// cell_meas_wide.h -- RSRP, RSSI, RSRQ and the noise power of a cell over n_rb resource blocks, with a per-RB profile
// (lcs_cell_meas_wide; the rule is stated in include/lcs.h).  cell_meas.h's rule on a grid tfg[rows][12 n_rb] taken from wide
// samples (tfg_wide.hip: k_tfg_wide) instead of the chain's 72 centre subcarriers.
//
// Only port 0's reference rows take part, enumerated as cell_meas.h does: reference row q is grid row tdd_grid_row(q, n_symb) and
// falls into bin b = q mod 40 = 4 s + j; a bin takes part iff bit s of the 10-bit dl_mask is set.  A row's RS sequence rs is
// 36.211 6.10.1.1 for N_RB = n_rb (lte_device.h: rs_dl_row_wide), shift_0 and shift_1 the ports' first subcarriers.  Per used row
// and port p, with N = 2 n_rb entries,
//   h_m = tfg[row][shift_p + 6 m] conj(rs[m]) (m < N),  a_p = sum_{m<N-1} h_m conj(h_{m+1}),  e_p = sum_{m<N} |h_m|^2,
//   w = sum_k |tfg[row][k]|^2, and per resource block i < n_rb:  b_p[i] = h_{2i} conj(h_{2i+1}),  w[i] = the power of its 12 columns.
// Over the n_rows used rows A_p, E_p, W, B_p[i], W[i] are their sums, and
//   rsrp[p] = |A_p| / ((N - 1) n_rows),  noise[p] = E_p / (N n_rows) - rsrp[p],  rssi = W / n_rows,  rsrq = n_rb rsrp[0] / rssi,
//   rsrp_rb[p][i] = |B_p[i]| / n_rows,  rssi_rb[i] = W[i] / n_rows.
//
// THE ORDER OF EVERY SUM IS FIXED HERE, so that the kernels (tfg_wide.hip: k_cell_meas_wide, k_cell_meas_wide_fin) and the host
// twin (tests/host/meas_wide_host.cpp) perform the same additions.  A row has MEASW_LANES = 64 lanes (the kernel: one wave) and is
// taken in n_pass = ceil(N / 64) passes; lane l holds the entries m = l + 64 t, t < n_pass.  Entry m < N holds the subcarriers
// 6 m .. 6 m + 5 and contributes the MEAS_NV = 7 values of cell_meas.h (measw_entry: the pair product where m < N - 1, |h_m|^2,
// and w as ((((|x_0|^2 + |x_1|^2) + |x_2|^2) + |x_3|^2) + |x_4|^2) + |x_5|^2); an entry m >= N is seven zeros.  Then, for each of
// the seven values on its own:
//   per lane  pass 0's value, + pass 1's, + .. in pass order (measw_lane_sum)
//   per row   the butterfly over the 64 lanes: v[i] += v[i ^ off] for off = 32, 16, 8, 4, 2, 1
//   per bin   the bin's rows in row order (q = b, b + 40, ..), starting from the first row itself (meas_bin_sum)
//   total     0 + the bins of the mask in increasing b (meas_total)
// With n_rb = 6 that is cell_meas.h's sum term for term: twelve entries, and the offsets 32 and 16 add zeros.
// The per-RB values have no sum inside a row but one: w[i] = w(entry 2 i) + w(entry 2 i + 1).  Their sums over the rows run as
// above: per bin in row order starting from the first row itself, then 0 + the bins of the mask in increasing b.
// Plain fp64, compiled with -ffp-contract=off on both sides.
#pragma once
#include <math.h>
#include "cell_meas.h"

#define MEASW_MAX_RB 100     // resource blocks of a 20 MHz carrier: the per-RB arrays of lcs_meas_wide_info
#define MEASW_LANES 64       // lanes of a row's butterfly
#define MEASW_MAX_PASSES 4   // ceil(2 * 100 / 64)
#define MEASW_NRB 5          // per-RB values: B_0 (re, im), B_1 (re, im), W
enum { MEASW_B0_RE = 0, MEASW_B0_IM, MEASW_B1_RE, MEASW_B1_IM, MEASW_WRB };
static_assert(sizeof(lcs_meas_wide_info) == 128 + 3 * MEASW_MAX_RB * 8 && LCS_MEAS_WIDE_MAX_RB == MEASW_MAX_RB, "include/lcs.h: lcs_meas_wide_info");

// n_fft = 128 R with R in {1, 2, 4, 8, 16}: log2 R, or -1
__host__ __device__ __forceinline__ int measw_log2r(int n_fft) {
  return n_fft == 128 ? 0 : n_fft == 256 ? 1 : n_fft == 512 ? 2 : n_fft == 1024 ? 3 : n_fft == 2048 ? 4 : -1;
}
// the most resource blocks a grid of that length holds (the LTE bandwidth that fits the rate)
__host__ __device__ __forceinline__ int measw_max_rb(int n_fft) {
  switch (measw_log2r(n_fft)) { case 0: return 6; case 1: return 15; case 2: return 25; case 3: return 50; case 4: return 100; default: return -1; }
}
__host__ __device__ __forceinline__ bool measw_rb_ok(int n_fft, int n_rb) { return measw_log2r(n_fft) >= 0 && n_rb >= 6 && n_rb <= measw_max_rb(n_fft); }
__host__ __device__ __forceinline__ int measw_passes(int n_rb) { return (2 * n_rb + MEASW_LANES - 1) / MEASW_LANES; }
// column of the grid row that holds DFT bin k (0 .. n_fft - 1), or -1: concat(dft.right(6 n_rb), dft.mid(1, 6 n_rb));
// *cn = the bin's signed subcarrier number, -6 n_rb .. -1, 1 .. 6 n_rb
__host__ __device__ __forceinline__ int measw_col_of_bin(int k, int n_fft, int n_rb, int *cn) {
  const int half = 6 * n_rb;
  if (k >= 1 && k <= half) { *cn = k; return half + k - 1; }
  if (k >= n_fft - half && k < n_fft) { *cn = k - n_fft; return k - (n_fft - half); }
  *cn = 0;
  return -1;
}

// the seven values of entry m (< n_ent = 2 n_rb) from its h and its right neighbour's (h_next: entry m + 1's, anything for the last)
__host__ __device__ __forceinline__ void measw_entry(const meas_x6 &x, int m, int n_ent, int ports, cd2 h0, cd2 h0_next, cd2 h1, cd2 h1_next,
                                                     double (&v)[MEAS_NV]) {
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
// The per-RB values of resource block i from entry m = 2 i's seven values and entry m + 1's w: the pair product of an even entry IS
// b_p[i] (m = 2 i < n_ent - 1 always)
__host__ __device__ __forceinline__ void measw_rb_values(const double (&v)[MEAS_NV], double w_next, double (&r)[MEASW_NRB]) {
  r[MEASW_B0_RE] = v[MEAS_A0_RE]; r[MEASW_B0_IM] = v[MEAS_A0_IM];
  r[MEASW_B1_RE] = v[MEAS_A1_RE]; r[MEASW_B1_IM] = v[MEAS_A1_IM];
  r[MEASW_WRB] = v[MEAS_W] + w_next;
}
// a running sum "starting from the first itself": the lane's passes, a bin's rows
__host__ __device__ __forceinline__ double measw_acc(bool first, double acc, double v) { return first ? v : acc + v; }
// one value of a row from its entries e[m], m < 64 n_pass (host form; the kernel's is measw_row_sum_lanes on the lanes' sums)
__host__ __device__ inline double measw_row_sum(const double *e, int n_pass) {
  double v[MEASW_LANES], w[MEASW_LANES];
  for (int l = 0; l < MEASW_LANES; ++l) {
    v[l] = 0.0;
    for (int t = 0; t < n_pass; ++t) v[l] = measw_acc(t == 0, v[l], e[l + MEASW_LANES * t]);
  }
  for (int off = MEASW_LANES / 2; off >= 1; off >>= 1) {
    for (int l = 0; l < MEASW_LANES; ++l) w[l] = v[l] + v[l ^ off];
    for (int l = 0; l < MEASW_LANES; ++l) v[l] = w[l];
  }
  return v[0];
}
#ifdef __HIPCC__
__device__ __forceinline__ double measw_row_sum_lanes(double v) {
#pragma unroll
  for (int off = MEASW_LANES / 2; off >= 1; off >>= 1) v = v + __shfl_xor(v, off);
  return v;
}
#endif
// one per-RB value's total from its bins: bin[b * stride], b < 40
__host__ __device__ __forceinline__ double measw_total_strided(const double *bin, size_t stride, int n_q, int dl_mask) {
  double s = 0.0;
  for (int b = 0; b < TDD_BINS; ++b) if (meas_bin_used(b, dl_mask) && b < n_q) s = s + bin[(size_t)b * stride];
  return s;
}

__host__ __device__ __forceinline__ void measw_clear_head(lcs_meas_wide_info *o, int status) {
  o->status = status; o->n_rows = status; o->n_ports = status; o->dl_mask = status;
  o->n_rb = status; o->n_fft = status; o->reserved_i[0] = o->reserved_i[1] = 0;
  o->rsrp[0] = o->rsrp[1] = o->noise[0] = o->noise[1] = o->rssi = o->rsrq = 0.0;
  for (int i = 0; i < 4; ++i) o->a_re_im[i] = 0.0;
  o->reserved[0] = o->reserved[1] = 0.0;
}
// The record's head from the totals; the conditions under which there is no number are meas_finish's -- status -1, every double 0,
// the integers as they are -- without a used row, with an rssi of zero, or when a total or a result is not finite.  Returns whether
// there is a number: the per-RB arrays are filled (measw_finish_rb) only then, and are zero otherwise.
__host__ __device__ inline bool measw_finish_head(const double *tot /*[MEAS_NV]*/, int n_rows, int ports, int dl_mask, int n_rb, int n_fft,
                                                  lcs_meas_wide_info *o) {
  measw_clear_head(o, -1);
  o->n_rows = n_rows; o->n_ports = ports; o->dl_mask = dl_mask; o->n_rb = n_rb; o->n_fft = n_fft;
  if (n_rows <= 0) return false;
  const int n_ent = 2 * n_rb;
  const double a0r = tot[MEAS_A0_RE], a0i = tot[MEAS_A0_IM], a1r = tot[MEAS_A1_RE], a1i = tot[MEAS_A1_IM];
  const double rssi = tot[MEAS_W] / (double)n_rows;
  const double rsrp0 = sqrt(a0r * a0r + a0i * a0i) / (double)((n_ent - 1) * n_rows), rsrp1 = sqrt(a1r * a1r + a1i * a1i) / (double)((n_ent - 1) * n_rows);
  const double noise0 = tot[MEAS_E0] / (double)(n_ent * n_rows) - rsrp0, noise1 = tot[MEAS_E1] / (double)(n_ent * n_rows) - rsrp1;
  const double rsrq = (double)n_rb * rsrp0 / rssi;
  const bool ok = isfinite(a0r) && isfinite(a0i) && isfinite(a1r) && isfinite(a1i) && isfinite(tot[MEAS_E0]) && isfinite(tot[MEAS_E1]) &&
                  isfinite(tot[MEAS_W]) && rssi > 0.0 && isfinite(rssi) && isfinite(rsrp0) && isfinite(rsrp1) && isfinite(noise0) &&
                  isfinite(noise1) && isfinite(rsrq);
  if (!ok) return false;
  o->status = 0;
  o->rsrp[0] = rsrp0; o->rsrp[1] = rsrp1;
  o->noise[0] = noise0; o->noise[1] = noise1;
  o->rssi = rssi;
  o->rsrq = rsrq;
  o->a_re_im[0] = a0r; o->a_re_im[1] = a0i; o->a_re_im[2] = a1r; o->a_re_im[3] = a1i;
  return true;
}
// resource block i of the record from its five totals (ok: measw_finish_head's verdict; port 1's are exact zeros where it is not measured)
__host__ __device__ __forceinline__ void measw_finish_rb(const double (&t)[MEASW_NRB], bool ok, int n_rows, int i, lcs_meas_wide_info *o) {
  o->rsrp_rb[0][i] = ok ? sqrt(t[MEASW_B0_RE] * t[MEASW_B0_RE] + t[MEASW_B0_IM] * t[MEASW_B0_IM]) / (double)n_rows : 0.0;
  o->rsrp_rb[1][i] = ok ? sqrt(t[MEASW_B1_RE] * t[MEASW_B1_RE] + t[MEASW_B1_IM] * t[MEASW_B1_IM]) / (double)n_rows : 0.0;
  o->rssi_rb[i] = ok ? t[MEASW_WRB] / (double)n_rows : 0.0;
}
