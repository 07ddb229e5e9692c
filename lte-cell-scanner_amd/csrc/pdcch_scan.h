// pdcch_scan.h -- the blind search of every CCE of the control region (lcs_pdcch_scan_wide, lcs_pdcch_scan; the rule is stated in
// include/lcs.h: lcs_pdcch_scan_info).  Host and device: the kernels (pdcch_scan.hip: k_pscan_llr, k_pscan_dec, k_pscan_acc, k_pscan_fin) and the
// host twin (tests/host/pdcch_scan_host.cpp) run the functions of this file, and the tables are built on the host by its functions.
//
// Everything up to the soft bit is pdcch.h's, at the cap of 792 quadruplets (pdc_build_map_t, pdc_elem, pdc_llr, pdc_coded_bit): the
// first 1152 soft bits of a subframe are the PDCCH stage's bit for bit.  The scrambling word w is reached with jump-ahead tables
// (psc_build_jump: by 1600 clocks, then by 32 2^k clocks for the bits of w) and not by clocking from zero.
//
// THE DECODER IS INTEGER.  The coded bits are sums in fp64 in pdcch.h's order; their quantisation is one fp64 multiplication, one
// division and one rint; from there the path metrics, the decisions, the re-encoded word and the sums of the quality are integers, so
// host, device and numpy agree bit for bit.  The wave's form keeps one state per lane with lte_device.h's rotating lane map
// (vit_lane_desc, vit_lane_step<int>): after n steps state s lives in lane rotl6(s, n mod 6), a step is one exchange across one lane
// bit.  The metrics run on through the three passes, so the map keeps rotating through all 3 K steps.
#pragma once
#include <cstddef>
#include "pdcch.h"

#define PSC_MAX_CCE LCS_PDCCH_SCAN_MAX_CCE
#define PSC_MAX_QUAD (9 * PSC_MAX_CCE)          // 792
#define PSC_NRE (4 * PSC_MAX_QUAD)              // 3168
#define PSC_NLLR (2 * PSC_NRE)                  // 6336 soft bits per subframe
#define PSC_SCR_WORDS (PSC_NLLR / 32)           // 198
#define PSC_SIZES LCS_PDCCH_SCAN_MAX_SIZES
#define PSC_MAX_CAND LCS_PDCCH_SCAN_MAX_CAND
#define PSC_MAX_K 80                            // A + 16, A <= 64
#define PSC_MAX_CODED (3 * PSC_MAX_K)
#define PSC_MAX_MSG LCS_PDCCH_SCAN_MAX_MSG
#define PSC_JUMP_WORDS (32 + 8 * 64)
#define PSC_N_RNTI 65536
#define PSC_PASSES 3                            // over the K steps, the metrics carried from pass to pass
static_assert(sizeof(lcs_pdcch_scan_cfg) == 104 && sizeof(lcs_pdcch_scan_dec) == 32 && sizeof(lcs_pdcch_scan_msg) == 40 && sizeof(lcs_pdcch_scan_sf) == 36 &&
              sizeof(lcs_pdcch_scan_info) == 64 + PCF_MAX_SF * 36 + PSC_MAX_MSG * 40 && offsetof(lcs_pdcch_scan_cfg, min_quality) == 96 &&
              offsetof(lcs_pdcch_scan_msg, d) == 8 && offsetof(lcs_pdcch_scan_dec, quality) == 24, "include/lcs.h: lcs_pdcch_scan_info");
static_assert(PSC_MAX_CAND == PSC_MAX_CCE + PSC_MAX_CCE / 2 + PSC_MAX_CCE / 4 + PSC_MAX_CCE / 8, "every L and every start");

typedef PdcMapT<PSC_MAX_QUAD> PscMap;

// ------------------------------------------------------------------ candidates
__host__ __device__ __forceinline__ int psc_n_cand(int n_cce) { return n_cce + n_cce / 2 + n_cce / 4 + n_cce / 8; }
// candidate i of a subframe with n_cce CCEs, by L ascending and then c: its level index (L = 1 << lv) and first CCE
__host__ __device__ __forceinline__ bool psc_cand(int i, int n_cce, int *lv, int *cce) {
  int v = 0, base = 0;
  while (v < 3 && i >= base + (n_cce >> v)) { base += n_cce >> v; v += 1; }
  *lv = v; *cce = (i - base) << v;
  return i >= 0 && i < psc_n_cand(n_cce);
}
// formed only at a code rate of 3/4 at most
__host__ __device__ __forceinline__ bool psc_rate_ok(int K, int L) { return 4 * K <= 3 * 72 * L; }
// 36.213 9.1.1
__host__ __device__ __forceinline__ uint32_t psc_yk(uint32_t rnti, int k) {
  uint32_t y = rnti;
  for (int i = 0; i <= k; ++i) y = (39827u * y) % 65537u;
  return y;
}
__host__ __device__ __forceinline__ int psc_m_of(int L) { return L <= 2 ? 6 : 2; }
__host__ __device__ __forceinline__ bool psc_in_space(uint32_t rnti_x, int sf, int n_cce, int L, int cce) {
  const int nl = n_cce / L;
  if (rnti_x < 0x003du || rnti_x > 0xfff3u || nl == 0) return false;
  const uint32_t y = psc_yk(rnti_x, sf);
  bool in = false;
  for (int m = 0; m < psc_m_of(L); ++m) in = in || (L * (int)((y + (uint32_t)m) % (uint32_t)nl) == cce);
  return in;
}

// ------------------------------------------------------------------ scrambling with jump-ahead tables
__host__ __device__ __forceinline__ uint32_t psc_clock1(uint32_t x) { return (x >> 1) | ((((x >> 3) ^ x) & 1u) << 30); }
__host__ __device__ __forceinline__ uint32_t psc_clock2(uint32_t x) { return (x >> 1) | ((((x >> 3) ^ (x >> 2) ^ (x >> 1) ^ x) & 1u) << 30); }
// the image of state x under the linear map whose columns (the images of the 31 unit states) are cols[0 .. 30]
__host__ __device__ __forceinline__ uint32_t psc_apply(const uint32_t *__restrict__ cols, uint32_t x) {
  uint32_t r = 0;
  for (int b = 0; b < 31; ++b) if ((x >> b) & 1u) r ^= cols[b];
  return r;
}
// jump[0 .. 31]: lcs_tables::pn_jump_table(1600) (columns of the second register's map, and the first register 1600 clocks after its
// start); then for k < 8 the columns of the maps by 32 2^k clocks, the second register's [32 + 64 k ..], the first's [64 + 64 k ..]
inline void psc_build_jump(uint32_t *jump /*[PSC_JUMP_WORDS]*/) {
  for (int i = 0; i < PSC_JUMP_WORDS; ++i) jump[i] = 0u;
  for (int b = 0; b < 32; ++b) {
    uint32_t x = b < 31 ? (1u << b) : 1u;
    for (int i = 0; i < 1600; ++i) x = b < 31 ? psc_clock2(x) : psc_clock1(x);
    jump[b] = x;
  }
  for (int k = 0; k < 8; ++k)
    for (int b = 0; b < 31; ++b) {
      uint32_t x2 = 1u << b, x1 = 1u << b;
      for (int i = 0; i < (32 << k); ++i) { x2 = psc_clock2(x2); x1 = psc_clock1(x1); }
      jump[32 + 64 * k + b] = x2;
      jump[64 + 64 * k + b] = x1;
    }
}
// the 32 scrambling bits 32 w .. 32 w + 31 of subframe sf (pdc_scramble_word's, reached by jumps)
__host__ __device__ __forceinline__ uint32_t psc_scramble_word(int sf, int id, int w, const uint32_t *__restrict__ jump) {
  const uint32_t c_init = (uint32_t)sf * 512u + (uint32_t)id;
  uint32_t x1 = jump[31], x2 = psc_apply(jump, c_init), word = 0;
  for (int k = 0; k < 8; ++k)
    if ((w >> k) & 1) { x2 = psc_apply(jump + 32 + 64 * k, x2); x1 = psc_apply(jump + 64 + 64 * k, x1); }
  for (int i = 0; i < 32; ++i) {
    word |= ((x1 ^ x2) & 1u) << i;
    x1 = psc_clock1(x1); x2 = psc_clock2(x2);
  }
  return word;
}

// ------------------------------------------------------------------ the 8-bit decoder's pieces
__host__ __device__ __forceinline__ int psc_quant(double d, double m) { return (int)rint((127.0 * d) / m); }
// the four branch values of a step for the output words o0 + 2 o1 (o2 = 0), as vit_branch; the other four are their negatives
__host__ __device__ __forceinline__ void psc_branch(int r0, int r1, int r2, int (&d)[4]) {
  d[0] = (-r2 + -r1) + -r0; d[1] = (-r2 + -r1) + r0; d[2] = (-r2 + r1) + -r0; d[3] = (-r2 + r1) + r0;
}
// the K decoded bits: bit t < 64 in lo, bit t >= 64 in hi
__host__ __device__ __forceinline__ int psc_bit(unsigned long long lo, unsigned long long hi, int t) {
  return (int)(((t < 64) ? (lo >> t) : (hi >> (t - 64))) & 1ull);
}
// coded bit (stream j, step t) of the tail-biting code word of the K bits
__host__ __device__ __forceinline__ int psc_reencode(unsigned long long lo, unsigned long long hi, int K, int j, int t) {
  int p = 0;
  for (int i = 1; i <= 6; ++i) { const int u = (t - i < 0) ? t - i + K : t - i; p |= psc_bit(lo, hi, u) << (6 - i); }
  return (vit_word(psc_bit(lo, hi, t), p) >> j) & 1;
}
// pdc_rnti_x on K = A + 16 <= 80 bits
__host__ __device__ __forceinline__ uint32_t psc_rnti_x(unsigned long long lo, unsigned long long hi, int A) {
  unsigned crc = 0;
  for (int i = 0; i < A; ++i) {
    const unsigned msb = ((crc >> 15) & 1u) ^ (unsigned)psc_bit(lo, hi, i);
    crc = (crc << 1) & 0xffffu;
    if (msb) crc ^= 0x1021u;
  }
  unsigned rx = 0;
  for (int t = 0; t < 16; ++t) rx |= (unsigned)psc_bit(lo, hi, A + t) << (15 - t);
  return crc ^ rx;
}
__host__ __device__ __forceinline__ lcs_pdcch_scan_dec psc_entry_zero() {
  lcs_pdcch_scan_dec d;
  d.bits = 0ull; d.rnti_x = 0u; d.flags = 0; d.n_err = 0; d.n_obs = 0; d.n_repeat = 0; d.quality = 0.0;
  return d;
}
// the entry of one decode before the recurrence rule: flags 1, 4, 8, 16, and 2 for an accepted common one.  num = sum q (1 - 2 c),
// den = sum |q| (0: the silent candidate)
__host__ __device__ __forceinline__ lcs_pdcch_scan_dec psc_entry(unsigned long long lo, unsigned long long hi, int A, bool tb_ok, int n_obs, int n_err, int num, int den,
                                                                 int sf, int n_cce, int L, int cce, int rnti_mask) {
  lcs_pdcch_scan_dec d = psc_entry_zero();
  d.flags = 1;
  if (den <= 0) return d;
  d.bits = A >= 64 ? lo : (lo & ((1ull << A) - 1ull));
  d.rnti_x = psc_rnti_x(lo, hi, A);
  d.n_obs = (int16_t)n_obs; d.n_err = (int16_t)n_err;
  d.quality = (double)num / (double)den;
  const bool common = (pdc_kind(d.rnti_x) & rnti_mask) && L >= 4 && cce < 16;
  d.flags |= (tb_ok ? 8 : 0) | (psc_in_space(d.rnti_x, sf, n_cce, L, cce) ? 4 : 0) | (common ? 16 | 2 : 0);
  return d;
}
// an entry that is in space with sufficient quality: what the recurrence rule counts and what the list holds beside the common accepts
__host__ __device__ __forceinline__ bool psc_ue_hit(const lcs_pdcch_scan_dec &d, double min_quality) { return (d.flags & 4) && d.quality >= min_quality; }

// ------------------------------------------------------------------ the decoder, lane by lane on the host
// q[3][K] -> the K bits, the end state and the traced start state.  The wave's form (pdcch_scan.hip: psc_wava_wave) with an array
// index for the lane: the same steps in the same lanes.
inline void psc_wava_host(const int *q, int K, unsigned long long *lo, unsigned long long *hi, int *end_state, int *start_state) {
  int pm[64], nx[64];
  unsigned dec[64][3];
  for (int l = 0; l < 64; ++l) { pm[l] = 0; dec[l][0] = dec[l][1] = dec[l][2] = 0u; }
  const int n_tot = PSC_PASSES * K, last = (PSC_PASSES - 1) * K;
  for (int n = 0; n < n_tot; ++n) {
    const int t = n % K, k = n % 6;
    int br[4];
    psc_branch(q[t], q[K + t], q[2 * K + t], br);
    for (int l = 0; l < 64; ++l) {
      bool tk;
      nx[l] = vit_lane_step(vit_lane_desc(VIT_ROTR6(l, k)), pm[l], pm[l ^ (1 << k)], br, &tk);
      if (n >= last) dec[l][t >> 5] |= (tk ? 1u : 0u) << (t & 31);
    }
    for (int l = 0; l < 64; ++l) pm[l] = nx[l];
  }
  const int kr = n_tot % 6;
  int best = 0, bs = -1;
  for (int s = 0; s < 64; ++s) {
    const int v = pm[VIT_ROTL6(s, kr)];
    if (bs < 0 || v < best) { best = v; bs = s; }
  }
  *end_state = bs;
  *lo = *hi = 0ull;
  int s = bs;
  for (int t = K - 1; t >= 0; --t) {
    const int l = VIT_ROTL6(s, (last + t + 1) % 6);
    if (t < 64) *lo |= (unsigned long long)((s >> 5) & 1) << t; else *hi |= (unsigned long long)((s >> 5) & 1) << (t - 64);
    s = ((s << 1) & 63) | (int)((dec[l][t >> 5] >> (t & 31)) & 1u);
  }
  *start_state = s;
}
// n_obs, n_err and the two sums of the quality from q and the re-encoded word
inline void psc_score_host(const int *q, int K, unsigned long long lo, unsigned long long hi, int *n_obs, int *n_err, int *num, int *den) {
  *n_obs = *n_err = *num = *den = 0;
  for (int b = 0; b < 3 * K; ++b) {
    const int c = psc_reencode(lo, hi, K, b / K, b % K), v = q[b];
    *n_obs += v != 0;
    *n_err += (v != 0) && ((v < 0) != (c != 0));
    *num += c ? -v : v;
    *den += v < 0 ? -v : v;
  }
}

// ------------------------------------------------------------------ the acceptance, in order (what k_pscan_acc and k_pscan_fin do with prefix sums)
// tab [n_sf][PSC_MAX_CAND][PSC_SIZES]: the entries as psc_entry left them; sf[g] with cfi, n_reg, n_cce filled.  Fills n_repeat and
// flag 2 of the entries, the rest of sf[g], the list (msg_cap <= PSC_MAX_MSG of it) and the head.
inline void psc_finish_host(lcs_pdcch_scan_info *o, lcs_pdcch_scan_dec *tab, int n_sf, int n_sizes, double min_quality, int min_repeat, int msg_cap, int dl_mask,
                            int n_rb, int ports) {
  std::vector<unsigned char> pres((size_t)PSC_N_RNTI * PCF_MAX_SF, 0);
  auto ent = [&](int g, int i, int si) -> lcs_pdcch_scan_dec & { return tab[((size_t)g * PSC_MAX_CAND + i) * PSC_SIZES + si]; };
  for (int g = 0; g < n_sf; ++g) {
    o->sf[g].n_cand = o->sf[g].cfi ? psc_n_cand(o->sf[g].n_cce) : 0;
    for (int i = 0; i < o->sf[g].n_cand; ++i)
      for (int si = 0; si < n_sizes; ++si)
        if (psc_ue_hit(ent(g, i, si), min_quality)) pres[(size_t)ent(g, i, si).rnti_x * PCF_MAX_SF + g] = 1;
  }
  int n_read = 0, n_acc = 0, k[3] = {0, 0, 0}, n_ue = 0, n_rnti = 0, n_list = 0;
  std::vector<unsigned char> counted(PSC_N_RNTI, 0);
  for (int g = 0; g < n_sf; ++g) {
    lcs_pdcch_scan_sf &s = o->sf[g];
    if (s.cfi) n_read += 1;
    for (int i = 0; i < s.n_cand; ++i) {
      int lv, cce;
      psc_cand(i, s.n_cce, &lv, &cce);
      for (int si = 0; si < n_sizes; ++si) {
        lcs_pdcch_scan_dec &d = ent(g, i, si);
        const bool hit = psc_ue_hit(d, min_quality), common = (d.flags & 2) != 0;
        if (hit) {
          int rep = 0;
          for (int h = 0; h < n_sf; ++h) rep += pres[(size_t)d.rnti_x * PCF_MAX_SF + h];
          d.n_repeat = rep;
          if (rep >= min_repeat) d.flags |= 2;
        }
        if (d.flags & 2) {
          n_acc += 1;
          for (int c = cce; c < cce + (1 << lv); ++c) s.cce_mask[c >> 5] |= 1u << (c & 31);
          if (common) { const int kind = pdc_kind(d.rnti_x); k[kind == 1 ? 0 : kind == 2 ? 1 : 2] += 1; s.n_common += 1; }
          else { n_ue += 1; s.n_ue += 1; if (!counted[d.rnti_x]) { counted[d.rnti_x] = 1; n_rnti += 1; } }
        }
        if (hit || common) {
          if (n_list < msg_cap) {
            lcs_pdcch_scan_msg &m = o->msg[n_list];
            m.g = (int16_t)g; m.L = (uint8_t)(1 << lv); m.cce = (uint8_t)cce; m.size_index = (uint8_t)si; m.pad[0] = m.pad[1] = m.pad[2] = 0;
            m.d = d;
          }
          n_list += 1;
        }
      }
    }
  }
  o->n_sf = n_sf; o->n_read = n_read; o->n_accepted = n_acc; o->n_si = k[0]; o->n_paging = k[1]; o->n_ra = k[2];
  o->dl_mask = dl_mask; o->n_rb = n_rb; o->n_ports = ports; o->n_ue = n_ue; o->n_rnti = n_rnti;
  o->n_msg = n_list < msg_cap ? n_list : msg_cap; o->n_dropped = n_list - o->n_msg; o->n_sizes = n_sizes; o->reserved[0] = o->reserved[1] = 0;
}
