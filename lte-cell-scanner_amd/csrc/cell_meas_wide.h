// cell_meas_wide.h -- RSRP, RSSI, RSRQ and the noise power of a cell over n_rb resource blocks, with a per-RB profile
// (lcs_cell_meas_wide; the rule is stated in include/lcs.h).  cell_meas.h's rule, with its entries, its seven values and the order
// of its sums, on a grid tfg[rows][12 n_rb] taken from wide samples (tfg_wide.hip: k_tfg_wide) instead of the chain's 72 centre
// subcarriers; a row's RS sequence rs is 36.211 6.10.1.1 for N_RB = n_rb (lte_device.h: rs_dl_row_wide).  What this file adds:
//
// The passes.  A row has MEASW_LANES = 64 lanes (the kernel: one wave) and its N = 2 n_rb entries are taken in n_pass =
// ceil(N / 64) passes; lane l holds the entries m = l + 64 t, t < n_pass, an entry m >= N being seven zeros.  Before the row's
// butterfly every lane adds up its own entries, for each of the seven values on its own:
//   per lane  pass 0's value, + pass 1's, + .. in pass order (measw_acc)
// With n_rb = 6 there is one pass and the butterfly's offsets 32 and 16 add zeros: cell_meas.h's sum over 16 lanes, term for term.
//
// The per-RB values.  Per used row and resource block i < n_rb:  b_p[i] = h_{2i} conj(h_{2i+1}),  w[i] = the power of its 12 columns
// = w(entry 2 i) + w(entry 2 i + 1), the one sum inside a row.  B_p[i], W[i] are their sums over the used rows, in the order of the
// other sums over rows: per bin in row order starting from the first row itself, then 0 + the bins of the mask in increasing b; and
//   rsrp_rb[p][i] = |B_p[i]| / n_rows,  rssi_rb[i] = W[i] / n_rows.
//
// The column map of the grid (measw_col_of_bin) and the bandwidths a rate holds (measw_max_rb).
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

// cell_meas.h's entry with the wide rule's argument order (the host twin's spelling)
__host__ __device__ __forceinline__ void measw_entry(const meas_x6 &x, int m, int n_ent, int ports, cd2 h0, cd2 h0_next, cd2 h1, cd2 h1_next,
                                                     double (&v)[MEAS_NV]) {
  meas_entry(x, m, ports, h0, h0_next, h1, h1_next, v, n_ent);
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
// one value of a row from its entries e[m], m < 64 n_pass (host form; the kernel's is meas_row_sum_lanes<64> on the lanes' sums)
__host__ __device__ inline double measw_row_sum(const double *e, int n_pass) {
  double v[MEASW_LANES];
  for (int l = 0; l < MEASW_LANES; ++l) {
    v[l] = 0.0;
    for (int t = 0; t < n_pass; ++t) v[l] = measw_acc(t == 0, v[l], e[l + MEASW_LANES * t]);
  }
  return meas_row_sum<MEASW_LANES>(v);
}
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
// The record's head from the totals, as meas_finish.  Returns whether there is a number: the per-RB arrays are filled
// (measw_finish_rb) only then, and are zero otherwise.
__host__ __device__ inline bool measw_finish_head(const double *tot /*[MEAS_NV]*/, int n_rows, int ports, int dl_mask, int n_rb, int n_fft,
                                                  lcs_meas_wide_info *o) {
  measw_clear_head(o, -1);
  o->n_rows = n_rows; o->n_ports = ports; o->dl_mask = dl_mask; o->n_rb = n_rb; o->n_fft = n_fft;
  meas_numbers(tot, n_rows, 2 * n_rb, n_rb, o);
  return o->status == 0;
}
// resource block i of the record from its five totals (ok: measw_finish_head's verdict; port 1's are exact zeros where it is not measured)
__host__ __device__ __forceinline__ void measw_finish_rb(const double (&t)[MEASW_NRB], bool ok, int n_rows, int i, lcs_meas_wide_info *o) {
  o->rsrp_rb[0][i] = ok ? sqrt(t[MEASW_B0_RE] * t[MEASW_B0_RE] + t[MEASW_B0_IM] * t[MEASW_B0_IM]) / (double)n_rows : 0.0;
  o->rsrp_rb[1][i] = ok ? sqrt(t[MEASW_B1_RE] * t[MEASW_B1_RE] + t[MEASW_B1_IM] * t[MEASW_B1_IM]) / (double)n_rows : 0.0;
  o->rssi_rb[i] = ok ? t[MEASW_WRB] / (double)n_rows : 0.0;
}
