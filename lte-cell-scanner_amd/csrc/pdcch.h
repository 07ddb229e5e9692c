// pdcch.h -- the PDCCH common search space of every downlink subframe of a full-bandwidth grid (36.211 6.2.4, 6.8, 6.9.3; 36.212
// 5.1.4.2, 5.3.3; 36.213 9.1.1; lcs_pdcch_wide, lcs_pdcch; the rule is stated in include/lcs.h: lcs_pdcch_info).  Host and device:
// the kernels (pdcch.hip: k_pdcch_llr, k_pdcch_dec, k_pdcch_fin) and the host twin (tests/host/pdcch_host.cpp) run the functions of
// this file, and the tables the kernels read are built on the host by its functions (pdc_build_map, pdc_derm_build).
//
// TABLES.  A map is made for (n_rb, ports, CP, n_id_cell, PHICH duration and Ng) and every (m_i, cfi): PdcMap::re[4 q + j] is the
// resource element (l << 16 | k) that carries element j of quadruplet q < 144 of the multiplexed stream (CCE 0 .. 15), -1 beyond
// 9 N_CCE.  A map that the rule refuses (extended PHICH duration with n_ctrl < 3, PHICH units that do not fit their symbol) has
// n_reg = n_cce = 0: a subframe with that (m_i, cfi) is not read.  A de-rate-matching list names, for coded bit b = 3-stream s K + t,
// the positions among the E rate-matched bits that carry it, ascending, -1 padded.
//
// THE ORDER OF EVERY SUM IS FIXED HERE.  An element's symbol is pcfich.h's (pcf_h_at, pcf_soft) with the channel of the subframe's
// symbol 0 (ports 0, 1) and symbol 1 (ports 2, 3) at the element's column, whatever its own symbol.  A coded bit is 0 + its soft bits
// in ascending position.  sum |coded bit|: lane i < 64 adds |d[i]| + |d[i + 64]| + |d[i + 128]| (0 for b >= 3 K), then cell_meas.h's
// butterfly over the 64 lanes.  The decoder is lte_device.h's length-n form.  Plain fp64, -ffp-contract=off on both sides.
#pragma once
#include <math.h>
#include <algorithm>
#include <vector>
#include "pcfich.h"

#define PDC_MAX_QUAD 144                 // quadruplets the receiver reads: CCE 0 .. 15
#define PDC_NRE (4 * PDC_MAX_QUAD)
#define PDC_NLLR (2 * PDC_NRE)           // 1152 soft bits per subframe
#define PDC_SCR_WORDS (PDC_NLLR / 32)
#define PDC_SLOTS LCS_PDCCH_SLOTS
#define PDC_SIZES LCS_PDCCH_MAX_SIZES
#define PDC_MAX_CODED 192                // 3 K, K = A + 16 <= 64
#define PDC_DERM_W 8                     // 72 L / (3 K) <= 576 / 72
#define PDC_MAX_SYM 4
static_assert(sizeof(lcs_pdcch_cfg) == 68 && sizeof(lcs_pdcch_dec) == 24 &&
              sizeof(lcs_pdcch_info) == 40 + PCF_MAX_SF * 12 + PCF_MAX_SF * PDC_SLOTS * PDC_SIZES * 24, "include/lcs.h: lcs_pdcch_info");

// a map of the first NQ quadruplets: the PDCCH stage reads PDC_MAX_QUAD of them, the blind search (pdcch_scan.h) every one
template <int NQ> struct PdcMapT { int n_reg, n_cce; int re[4 * NQ]; };
typedef PdcMapT<PDC_MAX_QUAD> PdcMap;

__host__ __device__ __forceinline__ int pdc_n_ctrl(int cfi, int n_rb) { return cfi + (n_rb <= 10 ? 1 : 0); }
__host__ __device__ __forceinline__ int pdc_n_ctrl_max(int n_rb) { return n_rb <= 10 ? 4 : 3; }
// REGs per resource block of symbol l of the first slot
__host__ __device__ __forceinline__ int pdc_regs_per_rb(int l, int ports, int cp_type) {
  return l == 0 ? 2 : l == 1 ? (ports == 4 ? 2 : 3) : l == 2 ? 3 : (cp_type == LCS_CP_NORMAL ? 3 : 2);
}
// column of element j of the REG (k', l): four consecutive ones, or the four of six that are not = id (mod 3) (as pcf_col)
__host__ __device__ __forceinline__ int pdc_reg_col(int kp, int per_rb, int j, int id) {
  if (per_rb == 3) return kp + j;
  const int v = id % 3;
  return kp + 3 * (j >> 1) + ((j & 1) ? (v == 2 ? 1 : 2) : (v == 0 ? 1 : 0));
}
// the candidate of slot s with n_cce CCEs: its level and first CCE; false beyond the subframe's candidates
__host__ __device__ __forceinline__ bool pdc_slot(int s, int n_cce, int *L, int *cce) {
  const bool l8 = s >= 4;
  const int m = l8 ? s - 4 : s, lv = l8 ? 8 : 4, cap = l8 ? 2 : 4, have = n_cce / lv;
  *L = lv; *cce = lv * m;
  return s >= 0 && s < PDC_SLOTS && m < (have < cap ? have : cap);
}
// the 32 scrambling bits 32 w .. 32 w + 31 of subframe sf: jump = the jump-ahead table for 1600 clocks
__host__ __device__ __forceinline__ uint32_t pdc_scramble_word(int sf, int id, int w, const uint32_t *__restrict__ jump) {
  const uint32_t c_init = (uint32_t)sf * 512u + (uint32_t)id;
  uint32_t x1 = jump[31], x2 = 0, word = 0;
  for (int b = 0; b < 31; ++b) if ((c_init >> b) & 1u) x2 ^= jump[b];
  for (int i = 0; i < 32 * w + 32; ++i) {
    if (i >= 32 * w) word |= ((x1 ^ x2) & 1u) << (i - 32 * w);
    const uint32_t n1 = ((x1 >> 3) ^ x1) & 1u;
    const uint32_t n2 = ((x2 >> 3) ^ (x2 >> 2) ^ (x2 >> 1) ^ x2) & 1u;
    x1 = (x1 >> 1) | (n1 << 30);
    x2 = (x2 >> 1) | (n2 << 30);
  }
  return word;
}
// what element e (4 q + j of the stream) at column k of row rowy brings by itself: pcf_elem with the column given
__host__ __device__ __forceinline__ void pdc_elem(int e, int k, int n_rb, int ports, const double *__restrict__ rowy, const double *__restrict__ row0,
                                                  const double *__restrict__ row1, const uint32_t *bits0, const uint32_t *bits1, const double *shift4,
                                                  cd2 *y, cd2 *ha, cd2 *hb) {
  int a, b;
  pcf_pair_ports(e, ports, &a, &b);
  const int sa = (int)(a == 1 ? shift4[1] : shift4[0]);
  const int sb = (int)(b == 3 ? shift4[3] : b == 2 ? shift4[2] : shift4[1]);
  *y = mk(rowy[2 * k], rowy[2 * k + 1]);
  *ha = pcf_h_at(row0, bits0, sa, k, n_rb);
  *hb = mk(0.0, 0.0);
  if (ports == 4) *hb = pcf_h_at(row1, bits1, sb, k, n_rb);
  else if (ports == 2) *hb = pcf_h_at(row0, bits0, sb, k, n_rb);
}
// the element's two soft bits from its symbol and its scrambling word
__host__ __device__ __forceinline__ void pdc_llr(int e, uint32_t word /*of bits 2 e, 2 e + 1*/, cd2 s, double *l0, double *l1) {
  const int i0 = (2 * e) & 31;
  *l0 = ((word >> i0) & 1u) ? -s.re : s.re;
  *l1 = ((word >> (i0 + 1)) & 1u) ? -s.im : s.im;
}
// coded bit b of a candidate: llr = the candidate's first soft bit, lst = the bit's PDC_DERM_W positions
__host__ __device__ __forceinline__ double pdc_coded_bit(const double *__restrict__ llr, const int16_t *__restrict__ lst) {
  double v[PDC_DERM_W];
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < PDC_DERM_W; ++k) { const int t = lst[k]; v[k] = (t >= 0) ? llr[t] : 0.0; cnt += (t >= 0); }
  double s = 0;
#pragma unroll
  for (int k = 0; k < PDC_DERM_W; ++k) if (k < cnt) s += v[k];
  return s;
}
// CRC-16 (x^16 + x^12 + x^5 + 1, zero initial state: pbch_crc_ok's generator) of the first A decoded bits ^ the sixteen received
// after them, bit 15 - t of the result from decoded bit A + t: the RNTI the parity was masked with, MSB first
__host__ __device__ __forceinline__ uint32_t pdc_rnti_x(unsigned long long bits, int A) {
  unsigned crc = 0;
  for (int i = 0; i < A; ++i) {
    const unsigned msb = ((crc >> 15) & 1u) ^ (unsigned)((bits >> i) & 1ull);
    crc = (crc << 1) & 0xffffu;
    if (msb) crc ^= 0x1021u;
  }
  unsigned rx = 0;
  for (int t = 0; t < 16; ++t) rx |= (unsigned)((bits >> (A + t)) & 1ull) << (15 - t);
  return crc ^ rx;
}
// 1 SI, 2 paging, 4 random-access response, 0 none of them
__host__ __device__ __forceinline__ int pdc_kind(uint32_t rnti_x) {
  return rnti_x == 0xffffu ? 1 : rnti_x == 0xfffeu ? 2 : (rnti_x >= 1u && rnti_x <= 60u) ? 4 : 0;
}
// the entry of one decode from the winner's bits (all K of them), its end metric and sum |coded bit|
__host__ __device__ __forceinline__ lcs_pdcch_dec pdc_entry(unsigned long long bitsK, int A, double best, double den, int rnti_mask) {
  lcs_pdcch_dec d;
  d.bits = bitsK & ((1ull << A) - 1ull);
  d.rnti_x = pdc_rnti_x(bitsK, A);
  d.flags = 1 | ((pdc_kind(d.rnti_x) & rnti_mask) ? 2 : 0);
  d.quality = den > 0.0 ? -best / den : 0.0;
  return d;
}
__host__ __device__ __forceinline__ lcs_pdcch_dec pdc_entry_zero() {
  lcs_pdcch_dec d;
  d.bits = 0ull; d.rnti_x = 0u; d.flags = 0; d.quality = 0.0;
  return d;
}
// the head of the record from its entries g < n_sf, in subframe, slot and size order (the caller has zeroed the entries beyond)
__host__ __device__ inline void pdc_summary(lcs_pdcch_info *o, int n_sf, int dl_mask, int n_rb, int ports) {
  int n_read = 0, n_acc = 0, k[3] = {0, 0, 0};
  for (int g = 0; g < n_sf; ++g) {
    if (o->cfi[g] >= 1 && o->cfi[g] <= 3) n_read += 1;
    for (int s = 0; s < PDC_SLOTS; ++s)
      for (int i = 0; i < PDC_SIZES; ++i) {
        const lcs_pdcch_dec &d = o->dec[g][s][i];
        if (!(d.flags & 2)) continue;
        const int kind = pdc_kind(d.rnti_x);
        n_acc += 1;
        k[kind == 1 ? 0 : kind == 2 ? 1 : 2] += 1;
      }
  }
  o->n_sf = n_sf; o->n_read = n_read; o->n_accepted = n_acc; o->n_si = k[0]; o->n_paging = k[1]; o->n_ra = k[2];
  o->dl_mask = dl_mask; o->n_rb = n_rb; o->n_ports = ports; o->reserved = 0;
}

// ------------------------------------------------------------------ the tables (host)
// the sub-block interleaver's column permutation (36.212 table 5.1.4-2: the PBCH's)
static const int PDC_PERM[32] = {1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31, 0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30};
// w[0 .. n - 1]: the interleaver's output order of the inputs 0 .. n - 1 (nulls in front, row by row, permuted columns, column by column)
inline std::vector<int> pdc_interleave(int n) {
  const int R = (n + 31) / 32, nd = 32 * R - n;
  std::vector<int> w;
  w.reserve((size_t)n);
  for (int c = 0; c < 32; ++c)
    for (int r = 0; r < R; ++r) {
      const int v = 32 * r + PDC_PERM[c] - nd;
      if (v >= 0) w.push_back(v);
    }
  return w;
}
// Ng n_rb / 8 rounded up, Ng = 1/6, 1/2, 1, 2 for phich_resource 1 .. 4
inline int pdc_phich_units(int phich_resource, int n_rb) {
  const int num = phich_resource == 4 ? 2 : 1, den = phich_resource == 1 ? 6 : phich_resource == 2 ? 2 : 1;
  return (num * n_rb + 8 * den - 1) / (8 * den);
}
struct PdcReg { int k, l; };
// every REG of symbol l, ascending k'
inline std::vector<PdcReg> pdc_regs_of_symbol(int l, int n_rb, int ports, int cp_type) {
  const int per = pdc_regs_per_rb(l, ports, cp_type);
  std::vector<PdcReg> v;
  for (int n = 0; n < n_rb; ++n)
    for (int j = 0; j < per; ++j) v.push_back(PdcReg{12 * n + (per == 2 ? 6 : 4) * j, l});
  return v;
}
// The map of (m_i, cfi).  phich_duration 1 / 2, phich_resource 1 .. 4 as lcs_cell's.  pcfich / phich / order (each may be null):
// the REGs of the three kinds as (k' << 2 | l'), order in the PDCCH's REG order.  false: refused (the map is empty)
template <int NQ>
inline bool pdc_build_map_t(int n_rb, int ports, int cp_type, int id, int phich_duration, int phich_resource, int mi, int cfi, PdcMapT<NQ> *m,
                            std::vector<int> *pcfich = nullptr, std::vector<int> *phich = nullptr, std::vector<int> *order = nullptr) {
  m->n_reg = m->n_cce = 0;
  for (int i = 0; i < 4 * NQ; ++i) m->re[i] = -1;
  const int n_ctrl = pdc_n_ctrl(cfi, n_rb);
  if (cfi < 1 || cfi > 3 || mi < 0 || mi > 2) return false;
  if (phich_duration == 2 && n_ctrl < 3) return false;
  std::vector<PdcReg> sym[PDC_MAX_SYM];
  for (int l = 0; l < n_ctrl; ++l) sym[l] = pdc_regs_of_symbol(l, n_rb, ports, cp_type);
  // the PCFICH's four leave symbol 0's list
  std::vector<int> taken;          // k' << 2 | l'
  for (int i = 0; i < 4; ++i) {
    const int kp = (6 * (id % (2 * n_rb)) + 6 * ((i * n_rb) / 2)) % (12 * n_rb);
    taken.push_back(kp << 2);
    if (pcfich) pcfich->push_back(kp << 2);
  }
  std::vector<PdcReg> free_[PDC_MAX_SYM];
  for (int l = 0; l < n_ctrl; ++l)
    for (const PdcReg &r : sym[l])
      if (l != 0 || std::find(taken.begin(), taken.end(), r.k << 2) == taken.end()) free_[l].push_back(r);
  const int U = mi * pdc_phich_units(phich_resource, n_rb), n0 = (int)free_[0].size();
  for (int mp = 0; mp < U; ++mp)
    for (int i = 0; i < 3; ++i) {
      const int li = phich_duration == 2 ? i : 0, nl = (int)free_[li].size();
      const int num = ((id * nl) / n0 + mp + (i * nl) / 3) % nl;
      const int key = (free_[li][num].k << 2) | li;
      if (std::find(taken.begin(), taken.end(), key) != taken.end()) return false;     // the units do not fit their symbol
      taken.push_back(key);
      if (phich) phich->push_back(key);
    }
  std::vector<PdcReg> regs;
  for (int l = 0; l < n_ctrl; ++l)
    for (const PdcReg &r : free_[l])
      if (std::find(taken.begin() + 4, taken.end(), (r.k << 2) | l) == taken.end()) regs.push_back(r);
  std::sort(regs.begin(), regs.end(), [](const PdcReg &a, const PdcReg &b) { return a.k != b.k ? a.k < b.k : a.l < b.l; });
  const int n = (int)regs.size();
  if (order) for (const PdcReg &r : regs) order->push_back((r.k << 2) | r.l);
  m->n_reg = n;
  m->n_cce = n / 9;
  if (n == 0) return true;
  const std::vector<int> w = pdc_interleave(n);
  for (int i = 0; i < n; ++i) {
    const int q = w[(size_t)((i + id) % n)];          // REG i carries quadruplet q
    if (q >= NQ || q >= 9 * m->n_cce) continue;
    const int per = pdc_regs_per_rb(regs[i].l, ports, cp_type);
    for (int j = 0; j < 4; ++j) m->re[4 * q + j] = (regs[i].l << 16) | pdc_reg_col(regs[i].k, per, j, id);
  }
  return true;
}
inline bool pdc_build_map(int n_rb, int ports, int cp_type, int id, int phich_duration, int phich_resource, int mi, int cfi, PdcMap *m,
                          std::vector<int> *pcfich = nullptr, std::vector<int> *phich = nullptr, std::vector<int> *order = nullptr) {
  return pdc_build_map_t<PDC_MAX_QUAD>(n_rb, ports, cp_type, id, phich_duration, phich_resource, mi, cfi, m, pcfich, phich, order);
}
// out[3 K][width]: the positions among the E rate-matched bits that carry coded bit s K + t, ascending, -1 padded (36.212 5.1.4.2:
// three sub-block interleavers of 32 columns, the streams one after the other, read cyclically without the nulls).  false when a
// coded bit has more than width positions.
inline bool pdc_derm_build(int K, int E, int width, int16_t *out) {
  const int R = (K + 31) / 32, Kp = 32 * R, nd = Kp - K;
  std::vector<int> w((size_t)3 * Kp, -1);
  for (int s = 0; s < 3; ++s)
    for (int c = 0; c < 32; ++c)
      for (int r = 0; r < R; ++r) {
        const int v = 32 * r + PDC_PERM[c] - nd;
        w[(size_t)s * Kp + (size_t)c * R + r] = v >= 0 ? s * K + v : -1;
      }
  std::vector<int> cnt((size_t)3 * K, 0);
  for (int i = 0; i < 3 * K * width; ++i) out[i] = -1;
  int k = 0, j = 0;
  while (k < E) {
    const int b = w[(size_t)j];
    if (b >= 0) {
      if (cnt[(size_t)b] >= width) return false;
      out[b * width + cnt[(size_t)b]++] = (int16_t)k;
      k += 1;
    }
    j = (j + 1) % (3 * Kp);
  }
  return true;
}
