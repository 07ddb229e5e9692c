// pdcch_scan.hip -- the blind search of every CCE of a wide cell's control region on the device (lcs_pdcch_scan_wide, lcs_pdcch_scan;
// the rule: pdcch_scan.h, include/lcs.h).  A translation unit of its own beside pdcch.hip: a context that never calls the stage runs
// no kernel of this file and allocates none of its buffers.  No atomics, no scratch, nothing depends on the order in which workgroups
// run: every entry is written by exactly one lane, the presence bytes are only ever set to 1, and the list is placed by ordered prefix
// sums (k_pscan_acc within a subframe, k_pscan_fin across them).  Bit-equal to the host twin (tests/host/pdcch_scan_host.cpp).
#include <cstring>
#include "lcs_internal.h"
#include "lte_device.h"
#include "pdcch_scan.h"
#include "wide_call.h"

// pcfich.hip's kernels, launched here into a record of this stage's own (as pdcch.hip does)
__global__ void k_pcfich(const double2 *__restrict__ grid, const int *__restrict__ rows, const uint32_t *__restrict__ jump, lcs_pcfich_info *__restrict__ out,
                         int n_sf, int id, int cp_type, int n_symb, int ports, int n_rb);
__global__ void k_pcfich_fin(lcs_pcfich_info *__restrict__ out, int n_sf, int dl_mask, int n_rb, int ports);

#define PSC_LLR_THREADS 256
#define PSC_DEC_WAVES 4
#define PSC_FIN_THREADS 1024
#define PSC_FIN_WAVES (PSC_FIN_THREADS / 64)
static_assert(PSC_MAX_CAND * PSC_SIZES <= PSC_FIN_THREADS, "k_pscan_fin: one thread per entry of a subframe");

struct PscSizes { int a[PSC_SIZES]; };

// ------------------------------------------------------------------ the soft bits: one workgroup per subframe
// As k_pdcch_llr at the larger cap: threads 0 and 1 build the reference sequences, threads 58 .. 255 one scrambling word each (by
// jumps), then every thread takes the resource elements e = tid + 256 i of quadruplets 0 .. 791.  An element and the other of its
// pair are live together and sit in neighbouring lanes.  Thread 0 writes what the subframe is read with.
__global__ __launch_bounds__(PSC_LLR_THREADS) void k_pscan_llr(const double2 *__restrict__ grid, const int *__restrict__ sf4, const uint32_t *__restrict__ jump,
                                                               const lcs_pcfich_info *__restrict__ pcf, const PscMap *__restrict__ maps, double *__restrict__ llr,
                                                               lcs_pdcch_scan_info *__restrict__ out, int n_sf, int id, int cp_type, int n_symb, int ports, int n_rb,
                                                               int cfi_force) {
  const int g = blockIdx.x, tid = threadIdx.x;
  if (g >= n_sf) return;
  __shared__ uint32_t s_bits[2][RS_DL_WIDE_WORDS];
  __shared__ double s_shift[4];
  __shared__ uint32_t s_scr[PSC_SCR_WORDS];
  const int r0 = sf4[4 * g];
  int cfi = 0, n_reg = 0, n_cce = 0;
  const PscMap *map = nullptr;
  if (r0 >= 0) {
    cfi = cfi_force ? cfi_force : pcf->cfi[g];
    if (cfi >= 1 && cfi <= 3) {
      const int mi = sf4[4 * n_sf + g % 10];
      map = maps + (3 * mi + cfi - 1);
      n_reg = map->n_reg; n_cce = map->n_cce;
    }
    if (n_cce == 0) cfi = 0;
  }
  if (tid == 0) { out->sf[g].cfi = cfi; out->sf[g].n_reg = cfi ? n_reg : 0; out->sf[g].n_cce = n_cce; }
  if (cfi == 0) return;
  const int sf = g % 10;
  if (tid < 4) s_shift[tid] = 0.0;
  __syncthreads();
  if (tid < (ports == 4 ? 2 : 1)) rs_dl_row_wide(2 * sf, tid, id, cp_type, n_symb, n_rb, jump, s_bits[tid], s_shift);
  if (tid >= PSC_LLR_THREADS - PSC_SCR_WORDS) s_scr[tid - (PSC_LLR_THREADS - PSC_SCR_WORDS)] = psc_scramble_word(sf, id, tid - (PSC_LLR_THREADS - PSC_SCR_WORDS), jump + 32);
  __syncthreads();
  const size_t ncol = (size_t)12 * n_rb;
  const double *row0 = reinterpret_cast<const double *>(grid + (size_t)r0 * ncol);
  const double *row1 = reinterpret_cast<const double *>(grid + (size_t)(ports == 4 ? sf4[4 * g + 1] : r0) * ncol);
#pragma unroll 1
  for (int e = tid; e < ((PSC_NRE + PSC_LLR_THREADS - 1) / PSC_LLR_THREADS) * PSC_LLR_THREADS; e += PSC_LLR_THREADS) {
    const int re = e < PSC_NRE ? map->re[e] : -1;
    const bool live = re >= 0;
    const int l = live ? (re >> 16) : 0, k = live ? (re & 0xffff) : 0;
    const double *rowy = reinterpret_cast<const double *>(grid + (size_t)sf4[4 * g + l] * ncol);
    cd2 y, ha, hb;
    pdc_elem(e, k, n_rb, ports, rowy, row0, row1, s_bits[0], s_bits[1], s_shift, &y, &ha, &hb);
    const cd2 hb_pair = mk(__shfl_xor(hb.re, 1), __shfl_xor(hb.im, 1)), y_pair = mk(__shfl_xor(y.re, 1), __shfl_xor(y.im, 1));
    const cd2 s = pcf_soft(e, ports, y, ha, hb_pair, y_pair);
    double l0 = 0.0, l1 = 0.0;
    if (live) pdc_llr(e, s_scr[(2 * (e < PSC_NRE ? e : 0)) >> 5], s, &l0, &l1);
    if (e < PSC_NRE) {
      llr[(size_t)g * PSC_NLLR + 2 * e] = l0;
      llr[(size_t)g * PSC_NLLR + 2 * e + 1] = l1;
    }
  }
}

// ------------------------------------------------------------------ the 8-bit wrap-around decoder of one wave
// q [3][K] in the wave's LDS; all 64 lanes call it.  One state per lane on lte_device.h's rotating map; the metrics are carried
// through the three passes, so the map rotates through all 3 K steps (3 K mod 6 is 0 or 3).  The decisions of the last pass sit in
// three 32-bit words per lane; the traceback runs on the scalar unit, its decision word comes by v_readlane.
static __device__ __forceinline__ void psc_wava_wave(const int *q, int K, int lane, unsigned long long *lo, unsigned long long *hi, int *end_state, int *start_state) {
  int desc[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) desc[k] = vit_lane_desc(VIT_ROTR6(lane, k));
  int pm = 0;
  unsigned d0 = 0u, d1 = 0u, d2 = 0u;
  static_assert(PSC_PASSES == 3, "the step's pass is told by two comparisons");
  const int n_tot = PSC_PASSES * K, last = (PSC_PASSES - 1) * K, rem = n_tot % 6, full = n_tot - rem;
#define PSC_R(KK, N) do { const int n_ = (N), t_ = n_ >= last ? n_ - last : n_ >= K ? n_ - K : n_;                            \
                          int br_[4]; bool tk_;                                                                                \
                          psc_branch(q[t_], q[K + t_], q[2 * K + t_], br_);                                                    \
                          pm = vit_lane_step(desc[KK], pm, __shfl_xor(pm, 1 << (KK)), br_, &tk_);                              \
                          const unsigned bit_ = (tk_ && n_ >= last) ? (1u << (t_ & 31)) : 0u;                                  \
                          d0 |= t_ < 32 ? bit_ : 0u; d1 |= (t_ >= 32 && t_ < 64) ? bit_ : 0u; d2 |= t_ >= 64 ? bit_ : 0u; } while (0)
#pragma unroll 1
  for (int n6 = 0; n6 < full; n6 += 6) { PSC_R(0, n6); PSC_R(1, n6 + 1); PSC_R(2, n6 + 2); PSC_R(3, n6 + 3); PSC_R(4, n6 + 4); PSC_R(5, n6 + 5); }
  if (rem > 0) { PSC_R(0, full); PSC_R(1, full + 1); PSC_R(2, full + 2); }
#undef PSC_R
  // the lowest state among the smallest metrics: this lane holds state rotr6(lane, 3 K mod 6)
  int best = pm, bs = rem ? VIT_ROTR6(lane, 3) : lane;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int ov = __shfl_xor(best, off), os = __shfl_xor(bs, off);
    if (ov < best || (ov == best && os < bs)) { best = ov; bs = os; }
  }
  int s = __builtin_amdgcn_readfirstlane(bs);
  *end_state = s;
  unsigned long long blo = 0ull, bhi = 0ull;
  for (int t = K - 1; t >= 0; --t) {
    const unsigned w = (unsigned)__builtin_amdgcn_readlane((int)(t < 32 ? d0 : t < 64 ? d1 : d2), VIT_ROTL6(s, (last + t + 1) % 6));
    const unsigned long long b = (unsigned long long)((s >> 5) & 1);
    if (t < 64) blo |= b << t; else bhi |= b << (t - 64);
    s = ((s << 1) & 63) | (int)((w >> (t & 31)) & 1u);
  }
  *lo = blo; *hi = bhi; *start_state = s;
}

// ------------------------------------------------------------------ the decodes: one wave per (subframe, candidate), every size
// Four independent waves share a workgroup.  The wave loads the candidate's 72 L soft bits into its LDS once; per size lane b (and
// b + 64, ..) sums coded bit b from the size's list, the wave takes the largest magnitude, quantises into its LDS, decodes, and
// scores the re-encoded word; lane 0 forms the entry, writes it and, for an in-space entry of sufficient quality, sets the presence
// byte of (rnti_x, g).  Candidates beyond the subframe's leave their entries unwritten: nothing reads them.
__global__ __launch_bounds__(64 * PSC_DEC_WAVES) void k_pscan_dec(const double *__restrict__ llr, const int16_t *__restrict__ derm /*[6][4][240][8]*/,
                                                                  const lcs_pdcch_scan_info *__restrict__ rec, lcs_pdcch_scan_dec *__restrict__ tab,
                                                                  unsigned char *__restrict__ pres, int n_sf, int cand_cap, int n_sizes, PscSizes sizes, int rnti_mask,
                                                                  double min_quality) {
  __shared__ double s_llr[PSC_DEC_WAVES][576];
  __shared__ int s_q[PSC_DEC_WAVES][PSC_MAX_CODED];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int w = blockIdx.x * PSC_DEC_WAVES + wv;
  const int g = w / cand_cap, ci = w % cand_cap;
  if (g >= n_sf) return;
  const int cfi = rec->sf[g].cfi, n_cce = rec->sf[g].n_cce;
  int lv, cce;
  if (cfi == 0 || n_cce > PSC_MAX_CCE || !psc_cand(ci, n_cce, &lv, &cce)) return;
  const int L = 1 << lv;
  double *cl = s_llr[wv];
  int *q = s_q[wv];
  for (int i = lane; i < 72 * L; i += 64) cl[i] = llr[(size_t)g * PSC_NLLR + 72 * cce + i];
  lcs_wave_sync();
#pragma unroll 1
  for (int si = 0; si < n_sizes; ++si) {
    const int A = sizes.a[si], K = A + 16;
    lcs_pdcch_scan_dec ent = psc_entry_zero();
    if (psc_rate_ok(K, L)) {
      const int16_t *lst = derm + (size_t)((4 * si + lv) * PSC_MAX_CODED) * PDC_DERM_W;
      double v[4], mx = 0.0;
      bool fin_in = true;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int b = lane + 64 * u;
        v[u] = 0.0;
        if (b < 3 * K) {
          v[u] = pdc_coded_bit(cl, lst + b * PDC_DERM_W);
          fin_in = fin_in && vit_finite(v[u]);
        }
        mx = fmax(mx, fabs(v[u]));
      }
      if (!__any(!fin_in)) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off));
        unsigned long long lo = 0ull, hi = 0ull;
        int n_obs = 0, n_err = 0, num = 0, den = 0;
        bool tb_ok = false;
        if (mx > 0.0) {
          lcs_wave_sync();                                     // the last size's readers are done
#pragma unroll
          for (int u = 0; u < 4; ++u) if (lane + 64 * u < 3 * K) q[lane + 64 * u] = psc_quant(v[u], mx);
          lcs_wave_sync();
          int es, ss;
          psc_wava_wave(q, K, lane, &lo, &hi, &es, &ss);
          tb_ok = es == ss;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int b = lane + 64 * u;
            if (b < 3 * K) {
              const int c = psc_reencode(lo, hi, K, b / K, b % K), x = q[b];
              n_obs += x != 0;
              n_err += (x != 0) && ((x < 0) != (c != 0));
              num += c ? -x : x;
              den += x < 0 ? -x : x;
            }
          }
#pragma unroll
          for (int off = 32; off >= 1; off >>= 1) {
            n_obs += __shfl_xor(n_obs, off); n_err += __shfl_xor(n_err, off); num += __shfl_xor(num, off); den += __shfl_xor(den, off);
          }
        }
        ent = psc_entry(lo, hi, A, tb_ok, n_obs, n_err, num, den, g % 10, n_cce, L, cce, rnti_mask);
      }
    }
    if (lane == 0) {
      tab[((size_t)g * PSC_MAX_CAND + ci) * PSC_SIZES + si] = ent;
      if (psc_ue_hit(ent, min_quality)) pres[(size_t)ent.rnti_x * PCF_MAX_SF + g] = 1;
    }
  }
}

// ------------------------------------------------------------------ the acceptance: one workgroup per subframe
// Thread i takes entry (candidate i / 6, size i mod 6) of the subframe: the recurrence count of its RNTI from the presence bytes, flag
// 2, its place among the subframe's listed entries by an ordered prefix sum over the workgroup, and its share of the subframe's
// counts, which are added by wave and then across the waves in a fixed order.  The listed entries go to the subframe's stage in
// order; thread 0 writes the subframe's part of the record and its counts (sfc[g]: listed, accepted common, accepted UE, SI, paging,
// RA, RNTIs first seen accepted here, read) for k_pscan_fin.  Nothing here needs another workgroup's result.
#define PSC_SFC 8
static __device__ __forceinline__ int psc_block_scan(int v, int *s_w, int tid, int *total) {
  const int lane = tid & 63, wv = tid >> 6;
  int inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(inc, off); if (lane >= off) inc += o; }
  if (lane == 63) s_w[wv] = inc;
  __syncthreads();
  int before = 0, tot = 0;
  for (int i = 0; i < PSC_FIN_WAVES; ++i) { const int x = s_w[i]; tot += x; if (i < wv) before += x; }
  *total = tot;
  return before + inc - v;
}
__global__ __launch_bounds__(PSC_FIN_THREADS) void k_pscan_acc(lcs_pdcch_scan_info *__restrict__ out, lcs_pdcch_scan_dec *__restrict__ tab,
                                                               const unsigned char *__restrict__ pres, lcs_pdcch_scan_msg *__restrict__ stage /*[n_sf][990]*/,
                                                               int *__restrict__ sfc /*[n_sf][PSC_SFC]*/, int n_sf, int n_sizes, double min_quality, int min_repeat) {
  __shared__ int s_w[PSC_FIN_WAVES];
  __shared__ uint32_t s_rnti[PSC_FIN_THREADS];
  __shared__ uint32_t s_part[PSC_FIN_WAVES][9];
  __shared__ uint32_t s_tot[9];
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (g >= n_sf) return;
  const int ci = tid / PSC_SIZES, si = tid % PSC_SIZES;
  const int cfi = out->sf[g].cfi, n_cce = out->sf[g].n_cce;
  const int n_cand = (cfi && n_cce <= PSC_MAX_CCE) ? psc_n_cand(n_cce) : 0;
  const bool valid = ci < n_cand && si < n_sizes;
  lcs_pdcch_scan_dec *ep = tab + ((size_t)g * PSC_MAX_CAND + (valid ? ci : 0)) * PSC_SIZES + (valid ? si : 0);
  lcs_pdcch_scan_dec d = psc_entry_zero();
  if (valid) d = *ep;
  const bool hit = valid && psc_ue_hit(d, min_quality), common = valid && (d.flags & 2);
  int first = -1;
  if (hit) {
    int rep = 0;
    for (int h = 0; h < n_sf; ++h) { const int p = pres[(size_t)d.rnti_x * PCF_MAX_SF + h]; if (p && first < 0) first = h; rep += p; }
    d.n_repeat = rep;
    if (rep >= min_repeat) d.flags |= 2;
    ep->n_repeat = d.n_repeat; ep->flags = d.flags;
  }
  const bool acc = (d.flags & 2) != 0, listed = hit || common, ue = acc && !common;
  int lv = 0, cce = 0;
  if (valid) psc_cand(ci, n_cce, &lv, &cce);
  int tot;
  const int rank = psc_block_scan(listed ? 1 : 0, s_w, tid, &tot);
  if (listed) s_rnti[rank] = ue ? d.rnti_x : 0xffffffffu;
  __syncthreads();
  bool fresh = ue && first == g;
  if (fresh) for (int j = 0; j < rank; ++j) fresh = fresh && s_rnti[j] != d.rnti_x;
  const int kind = common ? pdc_kind(d.rnti_x) : 0;
  uint32_t part[9] = {(uint32_t)(acc && common), (uint32_t)ue, (uint32_t)(kind == 1), (uint32_t)(kind == 2), (uint32_t)(kind == 4), (uint32_t)fresh, 0u, 0u, 0u};
  if (acc) {
    const unsigned long long lo = ((cce < 64 ? (~0ull >> (64 - (1 << lv))) : 0ull)) << (cce & 63);      // L <= 8 divides 64: no straddle
    if (cce < 64) { part[6] = (uint32_t)lo; part[7] = (uint32_t)(lo >> 32); }
    else part[8] = ((1u << (1 << lv)) - 1u) << (cce - 64);
  }
#pragma unroll
  for (int u = 0; u < 9; ++u) {
    uint32_t x = part[u];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)x, off); x = u < 6 ? x + o : (x | o); }
    part[u] = x;
  }
  if (lane == 0) for (int u = 0; u < 9; ++u) s_part[wv][u] = part[u];
  __syncthreads();
  if (tid < 9) {
    uint32_t x = 0;
    for (int i = 0; i < PSC_FIN_WAVES; ++i) x = tid < 6 ? x + s_part[i][tid] : (x | s_part[i][tid]);
    s_tot[tid] = x;
  }
  if (listed) {                                                // rank < the subframe's PSC_MAX_CAND * PSC_SIZES entries
    lcs_pdcch_scan_msg m;
    m.g = (int16_t)g; m.L = (uint8_t)(1 << lv); m.cce = (uint8_t)cce; m.size_index = (uint8_t)si; m.pad[0] = m.pad[1] = m.pad[2] = 0;
    m.d = d;
    stage[(size_t)g * (PSC_MAX_CAND * PSC_SIZES) + rank] = m;
  }
  __syncthreads();
  if (tid == 0) {
    lcs_pdcch_scan_sf &s = out->sf[g];
    s.n_cand = n_cand; s.n_common = (int)s_tot[0]; s.n_ue = (int)s_tot[1];
    s.cce_mask[0] = s_tot[6]; s.cce_mask[1] = s_tot[7]; s.cce_mask[2] = s_tot[8];
    int *o = sfc + PSC_SFC * g;
    o[0] = tot; o[1] = (int)s_tot[0]; o[2] = (int)s_tot[1]; o[3] = (int)s_tot[2]; o[4] = (int)s_tot[3]; o[5] = (int)s_tot[4]; o[6] = (int)s_tot[5]; o[7] = cfi != 0;
  }
}
// ------------------------------------------------------------------ the record: one workgroup
// The list is the subframes' stages one after the other, cut at msg_cap: every thread walks the subframes with the number listed before
// each (the same sums in the same order on every thread) and copies its share; thread 0 adds the head in subframe order.
__global__ __launch_bounds__(PSC_FIN_THREADS) void k_pscan_fin(lcs_pdcch_scan_info *__restrict__ out, const lcs_pdcch_scan_msg *__restrict__ stage,
                                                               const int *__restrict__ sfc, int n_sf, int n_sizes, int msg_cap, int dl_mask, int n_rb, int ports) {
  __shared__ int s_c[PCF_MAX_SF * PSC_SFC];
  const int tid = threadIdx.x;
  for (int i = tid; i < n_sf * PSC_SFC; i += PSC_FIN_THREADS) s_c[i] = sfc[i];
  __syncthreads();
  int base = 0;
  for (int g = 0; g < n_sf; ++g) {
    const int n = s_c[PSC_SFC * g];
    for (int i = tid; i < n && base + i < msg_cap; i += PSC_FIN_THREADS) out->msg[base + i] = stage[(size_t)g * (PSC_MAX_CAND * PSC_SIZES) + i];
    base += n;
  }
  if (tid == 0) {
    int t[PSC_SFC] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int g = 0; g < n_sf; ++g)
      for (int u = 0; u < PSC_SFC; ++u) t[u] += s_c[PSC_SFC * g + u];
    out->n_sf = n_sf; out->n_read = t[7]; out->n_accepted = t[1] + t[2]; out->n_si = t[3]; out->n_paging = t[4]; out->n_ra = t[5];
    out->dl_mask = dl_mask; out->n_rb = n_rb; out->n_ports = ports; out->n_ue = t[2]; out->n_rnti = t[6];
    out->n_msg = t[0] < msg_cap ? t[0] : msg_cap; out->n_dropped = t[0] - out->n_msg; out->n_sizes = n_sizes;
    out->reserved[0] = out->reserved[1] = 0;
  }
}

// ------------------------------------------------------------------ launcher
int lcs_launch_pdcch_scan(lcs_ctx *c, const lcs_cell &cell, const int *rows4, int n_sf, int n_rb, int dl_mask, const PdcchScanPlan &plan) {
  lcs_ctx::MeasWide &w = c->meas_wide;
  lcs_ctx::PdcchScan &p = c->pdcch_scan;
  int rc;
  if (n_sf <= 0 || n_sf > PCF_MAX_SF) { c->err = "pdcch_scan: no such number of subframes"; return LCS_ERR_BAD_ARG; }
  p.last_n_sf = 0;
  const int n_symb = cell.cp_type == LCS_CP_NORMAL ? 7 : 6, id = cell.n_id_2 + 3 * cell.n_id_1, ports = pcf_ports(cell.n_ports);
  const size_t map_ints = 9 * sizeof(PscMap) / sizeof(int), derm_n = (size_t)PSC_SIZES * 4 * PSC_MAX_CODED * PDC_DERM_W;
  const size_t tab_n = (size_t)PCF_MAX_SF * PSC_MAX_CAND * PSC_SIZES, pres_n = (size_t)PSC_N_RNTI * PCF_MAX_SF;
  if ((rc = p.map.reserve(c, map_ints)) || (rc = p.derm.reserve(c, derm_n)) || (rc = p.jump.reserve(c, 32 + PSC_JUMP_WORDS)) ||
      (rc = p.sf.reserve(c, sizeof(p.h_sf) / sizeof(int))) || (rc = p.llr.reserve(c, (size_t)PCF_MAX_SF * PSC_NLLR)) || (rc = p.tab.reserve(c, tab_n)) ||
      (rc = p.pres.reserve(c, pres_n)) || (rc = p.stage.reserve(c, tab_n)) || (rc = p.sfc.reserve(c, (size_t)PCF_MAX_SF * PSC_SFC)) || (rc = p.rec.reserve(c, 1)) || (rc = p.pcf_rec.reserve(c, 1))) return rc;
  int key[13] = {n_rb, ports, (int)cell.cp_type, id, plan.sh.phich_duration, plan.sh.phich_resource, plan.n_sizes, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < plan.n_sizes; ++i) key[7 + i] = plan.size[i];
  if (std::memcmp(key, p.key, sizeof(key)) != 0) {
    p.key[0] = 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));              // nothing reads the host blocks that are rewritten
    p.h_map.assign(map_ints, 0);
    p.h_derm.assign(derm_n, (int16_t)-1);
    PscMap *maps = reinterpret_cast<PscMap *>(p.h_map.data());
    int max_cce = 0;
    for (int mi = 0; mi < 3; ++mi)
      for (int cfi = 1; cfi <= 3; ++cfi) {
        PscMap &m = maps[3 * mi + cfi - 1];
        pdc_build_map_t<PSC_MAX_QUAD>(n_rb, ports, (int)cell.cp_type, id, plan.sh.phich_duration, plan.sh.phich_resource, mi, cfi, &m);
        if (m.n_cce > PSC_MAX_CCE) { c->err = "pdcch_scan: more CCEs than the stage reads"; return LCS_ERR_BAD_ARG; }
        max_cce = m.n_cce > max_cce ? m.n_cce : max_cce;
      }
    for (int si = 0; si < plan.n_sizes; ++si)
      for (int lv = 0; lv < 4; ++lv)
        if (psc_rate_ok(plan.size[si] + 16, 1 << lv) &&
            !pdc_derm_build(plan.size[si] + 16, 72 << lv, PDC_DERM_W, p.h_derm.data() + (size_t)(4 * si + lv) * PSC_MAX_CODED * PDC_DERM_W)) {
          c->err = "pdcch_scan: a de-rate-matching list does not fit";
          return LCS_ERR_BAD_ARG;
        }
    HIPCHK(c, hipMemcpyAsync(p.map, p.h_map.data(), sizeof(int) * map_ints, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(p.derm, p.h_derm.data(), sizeof(int16_t) * derm_n, hipMemcpyHostToDevice, c->stream));
    p.cand_cap = psc_n_cand(max_cce);
    std::memcpy(p.key, key, sizeof(key));
  }
  if (p.jump_rb != n_rb) {
    p.jump_rb = 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    lcs_tables::pn_jump_table(1600 + 2 * (110 - n_rb), p.h_jump);
    psc_build_jump(p.h_jump + 32);
    HIPCHK(c, hipMemcpyAsync(p.jump, p.h_jump, sizeof(p.h_jump), hipMemcpyHostToDevice, c->stream));
    p.jump_rb = n_rb;
  }
  for (int i = 0; i < 4 * n_sf; ++i) p.h_sf[i] = rows4[i];
  for (int i = 0; i < 10; ++i) p.h_sf[4 * n_sf + i] = plan.sh.mi[i];
  int *rows2 = p.h_sf + 4 * n_sf + 10;
  for (int g = 0; g < n_sf; ++g) { rows2[2 * g] = rows4[4 * g]; rows2[2 * g + 1] = (ports == 4 && rows4[4 * g] >= 0) ? rows4[4 * g + 1] : -1; }
  HIPCHK(c, hipMemcpyAsync(p.sf, p.h_sf, sizeof(int) * (6 * n_sf + 10), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(p.rec.get(), 0, sizeof(lcs_pdcch_scan_info), c->stream));
  HIPCHK(c, hipMemsetAsync(p.pres.get(), 0, pres_n, c->stream));
  if (!plan.sh.cfi_force) {
    hipLaunchKernelGGL(k_pcfich, dim3(n_sf), dim3(PCF_LANES), 0, c->stream, (const double2 *)w.grid.get(), (const int *)(p.sf.get() + 4 * n_sf + 10),
                       (const uint32_t *)p.jump.get(), p.pcf_rec.get(), n_sf, id, (int)cell.cp_type, n_symb, ports, n_rb);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_pcfich_fin, dim3(1), dim3(PCF_LANES), 0, c->stream, p.pcf_rec.get(), n_sf, dl_mask, n_rb, ports);
    HIPCHK(c, hipGetLastError());
  }
  hipLaunchKernelGGL(k_pscan_llr, dim3(n_sf), dim3(PSC_LLR_THREADS), 0, c->stream, (const double2 *)w.grid.get(), (const int *)p.sf.get(),
                     (const uint32_t *)p.jump.get(), (const lcs_pcfich_info *)p.pcf_rec.get(), reinterpret_cast<const PscMap *>(p.map.get()), p.llr.get(),
                     p.rec.get(), n_sf, id, (int)cell.cp_type, n_symb, ports, n_rb, plan.sh.cfi_force);
  HIPCHK(c, hipGetLastError());
  PscSizes sizes;
  for (int i = 0; i < PSC_SIZES; ++i) sizes.a[i] = i < plan.n_sizes ? plan.size[i] : 0;
  if (p.cand_cap > 0) {
    const int n_waves = n_sf * p.cand_cap;
    hipLaunchKernelGGL(k_pscan_dec, dim3((n_waves + PSC_DEC_WAVES - 1) / PSC_DEC_WAVES), dim3(64 * PSC_DEC_WAVES), 0, c->stream, (const double *)p.llr.get(),
                       (const int16_t *)p.derm.get(), (const lcs_pdcch_scan_info *)p.rec.get(), p.tab.get(), p.pres.get(), n_sf, p.cand_cap, plan.n_sizes, sizes,
                       plan.sh.rnti_mask, plan.min_quality);
    HIPCHK(c, hipGetLastError());
  }
  hipLaunchKernelGGL(k_pscan_acc, dim3(n_sf), dim3(PSC_FIN_THREADS), 0, c->stream, p.rec.get(), p.tab.get(), (const unsigned char *)p.pres.get(), p.stage.get(),
                     p.sfc.get(), n_sf, plan.n_sizes, plan.min_quality, plan.min_repeat);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_pscan_fin, dim3(1), dim3(PSC_FIN_THREADS), 0, c->stream, p.rec.get(), (const lcs_pdcch_scan_msg *)p.stage.get(), (const int *)p.sfc.get(), n_sf,
                     plan.n_sizes, PSC_MAX_MSG, dl_mask, n_rb, ports);
  HIPCHK(c, hipGetLastError());
  return LCS_OK;
}
