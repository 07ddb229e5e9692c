// tdd_config.h -- the uplink-downlink configuration of a TDD cell (36.211 table 4.2-2) read off its cell-specific reference
// signals (lcs_set_tdd_config, lcs_tdd_config; the rule is stated in include/lcs.h).
//
// CRS are sent in every downlink subframe and in the DwPTS and never in an uplink subframe, and subframes 0 and 5 are downlink in
// every configuration.  Of the grid tfg[n_ofdm][72] (row 0 = slot 0 symbol 0 of a frame) only port 0's reference rows take part:
// reference row q = 0, 1, .. is grid row (q >> 1) n_symb + ((q & 1) ? n_symb - 3 : 0), and it falls into bin b = q mod 40 =
// 4 s + j (subframe s, row j of the subframe).  Per row, with rs the row's 12 values of RS_DL and shift its first subcarrier,
//   h_m = tfg[row][shift + 6 m] conj(rs[m]),  p_m = h_m conj(h_{m+1}) (m < 11),  c = sum_m p_m
// a neighbour product that a common phase of the row (the frequency correction) leaves alone and a timing offset turns by one
// angle for every row.  C[b] = sum of c over the bin's rows, N[b] their number; ref = C[0] + C[5] over whole subframes, and
//   T[s] = Re(C[s] conj(ref)) / |ref|^2  n_ref / N[s]
// reads about 1 for a subframe with CRS and about 0 for one without, whatever the uplink carries.
//
// THE ORDER OF EVERY SUM IS FIXED HERE, so that the kernel (tfg_mib.hip: k_tdd_config) and the host twin
// (tests/host/tdd_config_host.cpp) perform the same additions:
//   c      a butterfly over 16 entries, p_11 .. p_15 = 0: v[i] += v[i ^ off] for off = 8, 4, 2, 1 (the kernel: 16 lanes of a wave)
//   C[b]   the bin's rows in row order (q = b, b + 40, ..), starting from the first row itself
//   C[s]   ((C[s][0] + C[s][1]) + C[s][2]) + C[s][3];  ref = C[0] + C[5]
// Plain fp64, compiled with -ffp-contract=off on both sides.
#pragma once
#include <math.h>
#include "lte_device.h"

#define TDD_BINS 40          // (subframe, reference row of the subframe) pairs of a frame
#define TDD_ROW_LANES 16     // entries of a row's butterfly: 12 subcarriers, 11 products, padded with zeros

// where reference row q lies: the grid row, and the bin's slot and symbol flag
__host__ __device__ __forceinline__ int tdd_n_ref_rows(int n_ofdm, int n_symb) {
  if (n_ofdm <= 0) return 0;
  const int full = n_ofdm / n_symb, rem = n_ofdm - full * n_symb;      // whole slots, rows of a partial last one
  return 2 * full + (rem > 0) + (rem > n_symb - 3);
}
__host__ __device__ __forceinline__ int tdd_grid_row(int q, int n_symb) { return (q >> 1) * n_symb + ((q & 1) ? n_symb - 3 : 0); }
// rows of bin b among n_q reference rows
__host__ __device__ __forceinline__ int tdd_bin_count(int b, int n_q) { return n_q > b ? (n_q - 1 - b) / TDD_BINS + 1 : 0; }

__host__ __device__ __forceinline__ cd2 tdd_h(cd2 x, cd2 rs) { return cmul(x, cconj(rs)); }
__host__ __device__ __forceinline__ cd2 tdd_pair(cd2 h, cd2 h_next) { return cmul(h, cconj(h_next)); }
// c of one row from its 16 entries (host form; the kernel's is tdd_row_sum_lanes)
__host__ __device__ inline cd2 tdd_row_sum(const cd2 *p) {
  cd2 v[TDD_ROW_LANES], w[TDD_ROW_LANES];
  for (int i = 0; i < TDD_ROW_LANES; ++i) v[i] = p[i];
  for (int off = TDD_ROW_LANES / 2; off >= 1; off >>= 1) {
    for (int i = 0; i < TDD_ROW_LANES; ++i) w[i] = cadd(v[i], v[i ^ off]);
    for (int i = 0; i < TDD_ROW_LANES; ++i) v[i] = w[i];
  }
  return v[0];
}
#ifdef __HIPCC__
__device__ __forceinline__ cd2 tdd_row_sum_lanes(cd2 v) {
#pragma unroll
  for (int off = TDD_ROW_LANES / 2; off >= 1; off >>= 1) v = mk(v.re + __shfl_xor(v.re, off), v.im + __shfl_xor(v.im, off));
  return v;
}
#endif
// C[b] from the per-row values c[q], q < n_q
__host__ __device__ __forceinline__ cd2 tdd_bin_sum(const cd2 *c, int b, int n_q) {
  if (b >= n_q) return mk(0, 0);
  cd2 s = c[b];
  for (int q = b + TDD_BINS; q < n_q; q += TDD_BINS) s = cadd(s, c[q]);
  return s;
}

__host__ __device__ __forceinline__ double tdd_stat(cd2 c, cd2 ref, double den, int n_ref, int n) {
  const double num = c.re * ref.re + c.im * ref.im;
  return num / den * (double)n_ref / (double)n;
}
// 36.211 table 4.2-2 by the pattern of subframes (3, 4, 7, 8, 9) read as a binary number, D = 1, subframe 3 first; -1: no such row
__host__ __device__ __forceinline__ int tdd_config_of_pattern(int pat) {
  switch (pat) {
    case 0x00: return 0;      // UUUUU
    case 0x09: return 1;      // UDUUD
    case 0x1b: return 2;      // DDUDD
    case 0x07: return 3;      // UUDDD
    case 0x0f: return 4;      // UDDDD
    case 0x1f: return 5;      // DDDDD
    case 0x01: return 6;      // UUUUD
    default: return -1;
  }
}
__host__ __device__ __forceinline__ void tdd_info_clear(lcs_tdd_info *o, int code) {
  o->ul_dl_config = code; o->dwpts_rs_rows = code; o->margin = 0.0;
  for (int s = 0; s < 10; ++s) o->T[s] = 0.0;
  for (int j = 0; j < 4; ++j) o->R[j] = 0.0;
}
// The decision from the bins.  Nothing is decided -- configuration -1, DwPTS class -1, margin 0 -- when ref is zero or not
// finite, when a subframe has no row, or when a T is not finite (a NaN in the grid); T and R keep what could be computed.
__host__ __device__ inline void tdd_decide(const cd2 *C /*[40]*/, const int *N /*[40]*/, lcs_tdd_info *o) {
  tdd_info_clear(o, -1);
  cd2 Cs[10];
  int Ns[10];
  for (int s = 0; s < 10; ++s) {
    Cs[s] = cadd(cadd(cadd(C[4 * s], C[4 * s + 1]), C[4 * s + 2]), C[4 * s + 3]);
    Ns[s] = ((N[4 * s] + N[4 * s + 1]) + N[4 * s + 2]) + N[4 * s + 3];
  }
  const cd2 ref = cadd(Cs[0], Cs[5]);
  const int n_ref = Ns[0] + Ns[5];
  const double den = ref.re * ref.re + ref.im * ref.im;
  if (!(isfinite(ref.re) && isfinite(ref.im)) || !isfinite(den) || den == 0.0 || n_ref == 0) return;
  bool ok = true;
  for (int s = 0; s < 10; ++s) {
    if (Ns[s] == 0) { ok = false; continue; }
    o->T[s] = tdd_stat(Cs[s], ref, den, n_ref, Ns[s]);
    ok = ok && isfinite(o->T[s]);
  }
  // the special subframe's rows: subframe 1 alone first (what a grid without a configuration keeps)
  int config = -1;
  if (ok) {
    const int sf[5] = {3, 4, 7, 8, 9};
    int pat = 0;
    for (int k = 0; k < 5; ++k) pat |= (o->T[sf[k]] > 0.5) ? (1 << (4 - k)) : 0;
    config = (o->T[2] > 0.5) ? -1 : tdd_config_of_pattern(pat);      // subframe 2 is uplink in every configuration
    const int ms[6] = {2, 3, 4, 7, 8, 9};
    double m = fabs(o->T[ms[0]] - 0.5);
    for (int k = 1; k < 6; ++k) { const double d = fabs(o->T[ms[k]] - 0.5); m = d < m ? d : m; }
    o->margin = m;
  }
  o->ul_dl_config = config;
  const bool join6 = config == 0 || config == 1 || config == 2 || config == 6;      // subframe 6 is special there
  bool r_ok = true;
  int present = 0;
  for (int j = 0; j < 4; ++j) {
    const cd2 cj = join6 ? cadd(C[4 + j], C[24 + j]) : C[4 + j];
    const int nj = join6 ? N[4 + j] + N[24 + j] : N[4 + j];
    if (nj == 0) { r_ok = false; continue; }
    o->R[j] = tdd_stat(cj, ref, den, n_ref, nj);
    r_ok = r_ok && isfinite(o->R[j]);
    present |= (o->R[j] > 0.5) ? (1 << j) : 0;
  }
  // rows present must be a prefix that starts with row 0: 1, 11, 111, 1111 read from j = 0
  int rows = -1;
  if (present == 1) rows = 1; else if (present == 3) rows = 2; else if (present == 7) rows = 3; else if (present == 15) rows = 4;
  o->dwpts_rs_rows = (ok && r_ok && config >= 0) ? rows : -1;
}
