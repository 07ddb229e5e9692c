// pcfich.h -- the control format indicator of every downlink subframe of a full-bandwidth grid (36.211 6.7, 36.212 5.3.4;
// lcs_pcfich_wide, lcs_pcfich; the rule is stated in include/lcs.h: lcs_pcfich_info).  Host and device: the kernels (pcfich.hip:
// k_pcfich, k_pcfich_fin) and the host twin (tests/host/pcfich_host.cpp) run the functions of this file.
//
// A subframe has PCF_LANES = 64 lanes (the kernel: one wave), of which lane e < 16 holds resource element e = 4 i + j, element j
// of quadruplet i.  Elements 2 u and 2 u + 1 are a pair of the transmit diversity; a pair's ports are (a, b) = (0, -) with one
// port, (0, 1) with two, and (q, q + 2) for the quadruplet's pair q with four.  A lane works out, from its own column k alone,
//   y = tfg[row0][k],  ha = h_a(k),  hb = h_b(k)        (pcf_elem; h_b is zero with one port)
// takes hb and y of the other lane of its pair, and combines (pcf_soft):
//   s = conj(ha) y  [ + hb' conj(y') on the even lane | - hb' conj(y') on the odd one ]
// h_p(k) = h[m0] + (h[m0 + 1] - h[m0]) (k - (shift_p + 6 m0)) / 6 with m0 = floor((k - shift_p) / 6) clipped to 0 .. 2 n_rb - 2.
//
// THE ORDER OF EVERY SUM IS FIXED HERE.  A lane's four values (pcf_lane_values) are, with d0 = Re s (1 - 2 c(2 e)) and
// d1 = Im s (1 - 2 c(2 e + 1)):  n_c = +-d0 +- d1 for the three codewords (the sign is + iff the bit index mod 3 is c), and
// |d0| + |d1|; a lane without an element holds zeros.  Each value goes through cell_meas.h's butterfly over the 64 lanes, and
// pcf_decide divides.  The summary (pcf_summary) walks the subframes in order.  Plain fp64, -ffp-contract=off on both sides.
#pragma once
#include <math.h>
#include "cell_meas.h"

#define PCF_LANES 64
#define PCF_NV 4             // values a subframe is reduced to: the three numerators and the sum of |b_i|
#define PCF_MAX_SF LCS_PCFICH_MAX_SF
static_assert(sizeof(lcs_pcfich_info) == 48 + PCF_MAX_SF * (4 + 24 + 8) && PCF_MAX_SF * 12 >= LCS_TFG_MAX_OFDM, "include/lcs.h: lcs_pcfich_info");

__host__ __device__ __forceinline__ bool pcf_rb_ok(int n_rb) { return n_rb == 6 || n_rb == 15 || n_rb == 25 || n_rb == 50 || n_rb == 75 || n_rb == 100; }
__host__ __device__ __forceinline__ int pcf_ports(int n_ports) { return n_ports == 4 ? 4 : n_ports == 2 ? 2 : 1; }
// subframes a grid of n_ofdm rows reaches into
__host__ __device__ __forceinline__ int pcf_n_sf(int n_ofdm, int n_symb) { return n_ofdm <= 0 ? 0 : (n_ofdm + 2 * n_symb - 1) / (2 * n_symb); }
// is grid subframe g read at all: its bit of the mask, and its one or two rows inside the grid
__host__ __device__ __forceinline__ bool pcf_sf_used(int g, int n_ofdm, int n_symb, int ports, int dl_mask) {
  const int r0 = 2 * g * n_symb;
  return ((dl_mask >> (g % 10)) & 1) && r0 + (ports == 4 ? 1 : 0) < n_ofdm;
}
// column of element e = 4 i + j
__host__ __device__ __forceinline__ int pcf_col(int e, int id, int n_rb) {
  const int i = e >> 2, j = e & 3, v = id % 3;
  const int reg = (6 * (id % (2 * n_rb)) + 6 * ((i * n_rb) / 2)) % (12 * n_rb);
  // the REG starts on a multiple of 6, so column reg + o is = o (mod 3): o runs over 0 .. 5 without v and v + 3
  const int o = 3 * (j >> 1) + ((j & 1) ? (v == 2 ? 1 : 2) : (v == 0 ? 1 : 0));
  return reg + o;
}
// the pair's ports for element e: *a on row 0; *b on row 0 (two ports) or row 1 (four), -1 with one port
__host__ __device__ __forceinline__ void pcf_pair_ports(int e, int ports, int *a, int *b) {
  const int q = (e >> 1) & 1;
  *a = ports == 4 ? q : 0;
  *b = ports == 4 ? q + 2 : ports == 2 ? 1 : -1;
}
// the 32 scrambling bits of subframe sf (0 .. 9): jump = the jump-ahead table for 1600 clocks
__host__ __device__ __forceinline__ uint32_t pcf_scramble(int sf, int id, const uint32_t *__restrict__ jump) {
  const uint32_t c_init = (uint32_t)(sf + 1) * (uint32_t)(2 * id + 1) * 512u + (uint32_t)id;
  uint32_t x1 = jump[31], x2 = 0, word = 0;
  for (int b = 0; b < 31; ++b) if ((c_init >> b) & 1u) x2 ^= jump[b];
  for (int i = 0; i < 32; ++i) {
    word |= ((x1 ^ x2) & 1u) << i;
    const uint32_t n1 = ((x1 >> 3) ^ x1) & 1u;
    const uint32_t n2 = ((x2 >> 3) ^ (x2 >> 2) ^ (x2 >> 1) ^ x2) & 1u;
    x1 = (x1 >> 1) | (n1 << 30);
    x2 = (x2 >> 1) | (n2 << 30);
  }
  return word;
}
// h_p at column k of a reference row: row = [12 n_rb] (re, im) pairs, bits = the row's sequence (rs_dl_row_wide), shift = the
// port's first subcarrier.  Only the two reference elements around k are read.
__host__ __device__ __forceinline__ cd2 pcf_h_at(const double *__restrict__ row, const uint32_t *bits, int shift, int k, int n_rb) {
  int m0 = (k - shift + 6) / 6 - 1;                   // floor((k - shift) / 6) for k - shift >= -6
  m0 = m0 < 0 ? 0 : m0 > 2 * n_rb - 2 ? 2 * n_rb - 2 : m0;
  const int c0 = shift + 6 * m0;
  const cd2 h0 = tdd_h(mk(row[2 * c0], row[2 * c0 + 1]), rs_dl_wide_value(bits, m0));
  const cd2 h1 = tdd_h(mk(row[2 * (c0 + 6)], row[2 * (c0 + 6) + 1]), rs_dl_wide_value(bits, m0 + 1));
  const double t = (double)(k - c0) / 6.0;
  return mk(h0.re + (h1.re - h0.re) * t, h0.im + (h1.im - h0.im) * t);
}
// what element e brings by itself.  row1 / bits1 are read with four ports only.
__host__ __device__ __forceinline__ void pcf_elem(int e, int id, int n_rb, int ports, const double *__restrict__ row0, const double *__restrict__ row1,
                                                  const uint32_t *bits0, const uint32_t *bits1, const double *shift4, cd2 *y, cd2 *ha, cd2 *hb) {
  const int k = pcf_col(e, id, n_rb);
  int a, b;
  pcf_pair_ports(e, ports, &a, &b);
  // (selects, not an index into shift4: a run-time index would send it to scratch)
  const int sa = (int)(a == 1 ? shift4[1] : shift4[0]);
  const int sb = (int)(b == 3 ? shift4[3] : b == 2 ? shift4[2] : shift4[1]);
  *y = mk(row0[2 * k], row0[2 * k + 1]);
  *ha = pcf_h_at(row0, bits0, sa, k, n_rb);
  *hb = mk(0.0, 0.0);
  if (ports == 4) *hb = pcf_h_at(row1, bits1, sb, k, n_rb);
  else if (ports == 2) *hb = pcf_h_at(row0, bits0, sb, k, n_rb);
}
// the element's symbol from its own values and hb, y of the other element of its pair
__host__ __device__ __forceinline__ cd2 pcf_soft(int e, int ports, cd2 y, cd2 ha, cd2 hb_pair, cd2 y_pair) {
  const cd2 t1 = cmul(cconj(ha), y), t2 = cmul(hb_pair, cconj(y_pair));
  if (ports == 1) return t1;
  return (e & 1) ? csub(t1, t2) : cadd(t1, t2);
}
// the lane's four values from its symbol
__host__ __device__ __forceinline__ void pcf_lane_values(int e, uint32_t scr, cd2 s, double (&v)[PCF_NV]) {
  const int i0 = 2 * e, i1 = 2 * e + 1;
  const double d0 = ((scr >> i0) & 1u) ? -s.re : s.re, d1 = ((scr >> i1) & 1u) ? -s.im : s.im;
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = ((i0 % 3 == c) ? d0 : -d0) + ((i1 % 3 == c) ? d1 : -d1);
  v[3] = fabs(d0) + fabs(d1);
}
// the subframe's entry from the four sums; returns the cfi (0: not decoded, corr and margin zero)
__host__ __device__ __forceinline__ int pcf_decide(const double (&tot)[PCF_NV], double (&corr)[3], double *margin) {
  corr[0] = corr[1] = corr[2] = 0.0;
  *margin = 0.0;
  const double den = tot[3];
  if (!(den > 0.0) || !isfinite(den) || !isfinite(tot[0]) || !isfinite(tot[1]) || !isfinite(tot[2])) return 0;
  const double c0 = tot[0] / den, c1 = tot[1] / den, c2 = tot[2] / den;
  corr[0] = c0; corr[1] = c1; corr[2] = c2;
  int best = 0;
  double vb = c0, second = c1 > c2 ? c1 : c2;
  if (c1 > vb) { best = 1; vb = c1; second = c0 > c2 ? c0 : c2; }
  if (c2 > vb) { best = 2; vb = c2; second = c0 > c1 ? c0 : c1; }
  *margin = vb - second;
  return best + 1;
}
// the head of the record from its per-subframe entries g < n_sf, in subframe order (the caller has zeroed the entries beyond)
__host__ __device__ inline void pcf_summary(lcs_pcfich_info *o, int n_sf, int dl_mask, int n_rb, int ports) {
  int n = 0, k[3] = {0, 0, 0}, sum = 0;
  double mm = 0.0;
  for (int g = 0; g < n_sf; ++g) {
    const int cfi = o->cfi[g];
    if (cfi < 1 || cfi > 3) continue;
    k[cfi - 1] += 1;
    sum += cfi + (n_rb <= 10 ? 1 : 0);
    mm = (n == 0 || o->margin[g] < mm) ? o->margin[g] : mm;
    n += 1;
  }
  o->n_sf = n_sf; o->n_decoded = n; o->n_cfi[0] = k[0]; o->n_cfi[1] = k[1]; o->n_cfi[2] = k[2];
  o->dl_mask = dl_mask; o->n_rb = n_rb; o->n_ports = ports;
  o->mean_n_ctrl_sym = n > 0 ? (double)sum / (double)n : 0.0;
  o->min_margin = mm;
}
