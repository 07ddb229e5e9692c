// pdcch.hip -- the PDCCH common search space of a wide cell on the device (lcs_pdcch_wide, lcs_pdcch; the rule: pdcch.h,
// include/lcs.h).  A translation unit of its own, like pcfich.hip whose kernels decide its CFI: a context that never calls the stage runs
// no kernel of this file and allocates none of its buffers, and the code objects of the chain, of the measurement and of the PCFICH
// are what they are without it.  No atomics, no scratch, every result written by exactly one lane, nothing depends on the order in
// which workgroups run; fp64 throughout and bit-equal to the host twin (tests/host/pdcch_host.cpp).
#include <cstring>
#include "lcs_internal.h"
#include "lte_device.h"
#include "pdcch.h"
#include "wide_call.h"

// pcfich.hip's kernels, launched here into a record of this stage's own (their definitions and code objects are that file's)
__global__ void k_pcfich(const double2 *__restrict__ grid, const int *__restrict__ rows, const uint32_t *__restrict__ jump, lcs_pcfich_info *__restrict__ out,
                         int n_sf, int id, int cp_type, int n_symb, int ports, int n_rb);
__global__ void k_pcfich_fin(lcs_pcfich_info *__restrict__ out, int n_sf, int dl_mask, int n_rb, int ports);

#define PDC_LLR_THREADS 256
#define PDC_DEC_WAVES 4

// ------------------------------------------------------------------ the soft bits: one workgroup per subframe
// Workgroup g takes grid subframe g: sf4[4 g + l] is the row of `grid` that holds its symbol l, -1 for a subframe that is not read.
// Its CFI is cfi_force or the PCFICH record's, on the device; the map is the one of (m_i of the subframe, cfi).  Threads 0 and 1
// build the reference sequences of symbols 0 and 1 (the second with four ports only), threads 64 .. 99 one scrambling word each.
// Then every thread takes resource elements e = tid, tid + 256, tid + 512 of quadruplets 0 .. 143 -- its y at (l, k) of the map and
// the two channel values at column k --, the lanes of a pair trade hb and y, and the thread writes the element's two soft bits
// (zeros for an element beyond 9 N_CCE).  Thread 0 writes the subframe's cfi, n_reg and n_cce into the record.
__global__ __launch_bounds__(PDC_LLR_THREADS) void k_pdcch_llr(const double2 *__restrict__ grid, const int *__restrict__ sf4 /*[n_sf][4], m_i[10]*/,
                                                               const uint32_t *__restrict__ jump /*[2][32]*/, const lcs_pcfich_info *__restrict__ pcf,
                                                               const PdcMap *__restrict__ maps /*[3][3]*/, double *__restrict__ llr /*[n_sf][1152]*/,
                                                               lcs_pdcch_info *__restrict__ out, int n_sf, int id, int cp_type, int n_symb, int ports, int n_rb,
                                                               int cfi_force) {
  const int g = blockIdx.x, tid = threadIdx.x;
  if (g >= n_sf) return;
  __shared__ uint32_t s_bits[2][RS_DL_WIDE_WORDS];
  __shared__ double s_shift[4];
  __shared__ uint32_t s_scr[PDC_SCR_WORDS];
  const int r0 = sf4[4 * g];                                 // the same for the whole workgroup
  int cfi = 0, n_reg = 0, n_cce = 0;
  const PdcMap *map = nullptr;
  if (r0 >= 0) {
    cfi = cfi_force ? cfi_force : pcf->cfi[g];
    if (cfi >= 1 && cfi <= 3) {
      const int mi = sf4[4 * n_sf + g % 10];
      map = maps + (3 * mi + cfi - 1);
      n_reg = map->n_reg; n_cce = map->n_cce;
    }
    if (n_cce == 0) cfi = 0;                                 // a refused (m_i, cfi), or no CCE at all: not read
  }
  if (tid == 0) { out->cfi[g] = cfi; out->n_reg[g] = cfi ? n_reg : 0; out->n_cce[g] = n_cce; }
  if (cfi == 0) return;
  const int sf = g % 10;
  if (tid < 4) s_shift[tid] = 0.0;
  __syncthreads();
  if (tid < (ports == 4 ? 2 : 1)) rs_dl_row_wide(2 * sf, tid, id, cp_type, n_symb, n_rb, jump, s_bits[tid], s_shift);
  if (tid >= 64 && tid < 64 + PDC_SCR_WORDS) s_scr[tid - 64] = pdc_scramble_word(sf, id, tid - 64, jump + 32);
  __syncthreads();
  const size_t ncol = (size_t)12 * n_rb;
  const double *row0 = reinterpret_cast<const double *>(grid + (size_t)r0 * ncol);
  const double *row1 = reinterpret_cast<const double *>(grid + (size_t)(ports == 4 ? sf4[4 * g + 1] : r0) * ncol);
#pragma unroll 1
  for (int e = tid; e < ((PDC_NRE + PDC_LLR_THREADS - 1) / PDC_LLR_THREADS) * PDC_LLR_THREADS; e += PDC_LLR_THREADS) {
    const int re = e < PDC_NRE ? map->re[e] : -1;            // an element and the other of its pair are live together
    const bool live = re >= 0;
    const int l = live ? (re >> 16) : 0, k = live ? (re & 0xffff) : 0;
    const double *rowy = reinterpret_cast<const double *>(grid + (size_t)sf4[4 * g + l] * ncol);
    cd2 y, ha, hb;
    pdc_elem(e, k, n_rb, ports, rowy, row0, row1, s_bits[0], s_bits[1], s_shift, &y, &ha, &hb);
    const cd2 hb_pair = mk(__shfl_xor(hb.re, 1), __shfl_xor(hb.im, 1)), y_pair = mk(__shfl_xor(y.re, 1), __shfl_xor(y.im, 1));
    const cd2 s = pcf_soft(e, ports, y, ha, hb_pair, y_pair);
    double l0 = 0.0, l1 = 0.0;
    if (live) pdc_llr(e, s_scr[(2 * (e < PDC_NRE ? e : 0)) >> 5], s, &l0, &l1);
    if (e < PDC_NRE) {
      llr[(size_t)g * PDC_NLLR + 2 * e] = l0;
      llr[(size_t)g * PDC_NLLR + 2 * e + 1] = l1;
    }
  }
}

// ------------------------------------------------------------------ the decodes: one wave per (subframe, slot, size)
// Four independent waves share a workgroup, as in k_pbch.  Wave w = (g, slot, size i): a slot beyond the subframe's candidates, or of
// a subframe that is not read, gets a zero entry.  Otherwise lane b (and b + 64, b + 128) sums the soft bits of coded bit b from the
// candidate's list into the wave's LDS; the 64 tail-biting trellises run one per lane (end metrics), the lowest start state among
// the best runs once more one state per lane (decisions, traceback); lane 0 forms the entry and writes it.  Only wave-level
// synchronisation inside.  The trellis pass stays in a function of its own, as pbch_trellis_pass.
static __device__ __forceinline__ double pdc_trellis_pass(const double *d, int K, int ss) {
  return vit_end_metric_n<true>(d, d + K, d + 2 * K, K, ss);
}
__global__ __launch_bounds__(64 * PDC_DEC_WAVES) void k_pdcch_dec(const double *__restrict__ llr, const int16_t *__restrict__ derm /*[2][2][192][8]*/,
                                                                  lcs_pdcch_info *__restrict__ out, int n_sf, int n_sizes, int size0, int size1, int rnti_mask) {
  __shared__ double s_d[PDC_DEC_WAVES][PDC_MAX_CODED];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int w = blockIdx.x * PDC_DEC_WAVES + wv;
  if (w >= n_sf * PDC_SLOTS * PDC_SIZES) return;
  const int g = w / (PDC_SLOTS * PDC_SIZES), slot = (w / PDC_SIZES) % PDC_SLOTS, si = w % PDC_SIZES;
  int L, cce;
  const bool cand = si < n_sizes && out->cfi[g] != 0 && pdc_slot(slot, out->n_cce[g], &L, &cce);
  lcs_pdcch_dec ent = pdc_entry_zero();
  if (cand) {
    const int A = si ? size1 : size0, K = A + 16;
    double *d = s_d[wv];
    const double *cl = llr + (size_t)g * PDC_NLLR + 72 * cce;
    const int16_t *lst = derm + (size_t)((2 * si + (L == 8 ? 1 : 0)) * PDC_MAX_CODED) * PDC_DERM_W;
    double part = 0.0;
    bool fin_in = true;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int b = lane + 64 * q;
      double v = 0.0;
      if (b < 3 * K) {
        v = pdc_coded_bit(cl, lst + b * PDC_DERM_W);
        d[b] = v;
        fin_in = fin_in && vit_finite(v);
      }
      part = part + fabs(v);
    }
    lcs_wave_sync();
    const double den = meas_row_sum_lanes<64>(part);
    if (!__any(!fin_in)) {
      const double fin = pdc_trellis_pass(d, K, lane);
      double best = (fin < INFINITY) ? fin : INFINITY;
      int best_ss = lane;
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(best, off);
        const int oi = __shfl_xor(best_ss, off);
        if (ov < best || (ov == best && oi < best_ss)) { best = ov; best_ss = oi; }
      }
      if (best < INFINITY) {
        const unsigned long long bits = vit_retrace_wave_n(d, d + K, d + 2 * K, K, __builtin_amdgcn_readfirstlane(best_ss), lane);
        ent = pdc_entry(bits, A, best, den, rnti_mask);
      }
    }
  }
  if (lane == 0) out->dec[g][slot][si] = ent;
}

// the entries beyond n_sf, and the record's head from the entries in subframe order: one thread, no atomics
__global__ __launch_bounds__(256) void k_pdcch_fin(lcs_pdcch_info *__restrict__ out, int n_sf, int dl_mask, int n_rb, int ports) {
  const int tid = threadIdx.x;
  for (int i = n_sf * PDC_SLOTS * PDC_SIZES + tid; i < PCF_MAX_SF * PDC_SLOTS * PDC_SIZES; i += 256) (&out->dec[0][0][0])[i] = pdc_entry_zero();
  for (int g = n_sf + tid; g < PCF_MAX_SF; g += 256) { out->cfi[g] = 0; out->n_reg[g] = 0; out->n_cce[g] = 0; }
  if (tid == 0) pdc_summary(out, n_sf, dl_mask, n_rb, ports);
}

// ------------------------------------------------------------------ launcher
int lcs_launch_pdcch(lcs_ctx *c, const lcs_cell &cell, const int *rows4, int n_sf, int n_rb, int dl_mask, const PdcchPlan &plan) {
  return lcs_launch_pdcch_in(c, c->pdcch, cell, rows4, n_sf, n_rb, dl_mask, plan);
}
// the same into the blocks p: the stage's own, or those the PDSCH stage keeps for its grants (pdsch.hip)
int lcs_launch_pdcch_in(lcs_ctx *c, lcs_ctx::Pdcch &p, const lcs_cell &cell, const int *rows4, int n_sf, int n_rb, int dl_mask, const PdcchPlan &plan) {
  lcs_ctx::MeasWide &w = c->meas_wide;
  int rc;
  if (n_sf <= 0 || n_sf > PCF_MAX_SF) { c->err = "pdcch: no such number of subframes"; return LCS_ERR_BAD_ARG; }
  const int n_symb = cell.cp_type == LCS_CP_NORMAL ? 7 : 6, id = cell.n_id_2 + 3 * cell.n_id_1, ports = pcf_ports(cell.n_ports);
  const size_t map_ints = 9 * sizeof(PdcMap) / sizeof(int), derm_n = (size_t)PDC_SIZES * 2 * PDC_MAX_CODED * PDC_DERM_W;
  if ((rc = p.map.reserve(c, map_ints)) || (rc = p.derm.reserve(c, derm_n)) || (rc = p.jump.reserve(c, 64)) ||
      (rc = p.sf.reserve(c, sizeof(p.h_sf) / sizeof(int))) || (rc = p.llr.reserve(c, (size_t)PCF_MAX_SF * PDC_NLLR)) || (rc = p.rec.reserve(c, 1)) ||
      (rc = p.pcf_rec.reserve(c, 1))) return rc;
  // the tables: host work that grows with N_REG, so built when their key changes and not per call
  const int key[9] = {n_rb, ports, (int)cell.cp_type, id, plan.sh.phich_duration, plan.sh.phich_resource, plan.n_sizes, plan.size[0], plan.n_sizes > 1 ? plan.size[1] : 0};
  if (std::memcmp(key, p.key, sizeof(key)) != 0) {
    p.key[0] = 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));              // nothing reads the host blocks that are rewritten
    p.h_map.assign(map_ints, 0);
    p.h_derm.assign(derm_n, (int16_t)-1);
    PdcMap *maps = reinterpret_cast<PdcMap *>(p.h_map.data());
    for (int mi = 0; mi < 3; ++mi)
      for (int cfi = 1; cfi <= 3; ++cfi)
        pdc_build_map(n_rb, ports, (int)cell.cp_type, id, plan.sh.phich_duration, plan.sh.phich_resource, mi, cfi, &maps[3 * mi + cfi - 1]);
    for (int si = 0; si < plan.n_sizes; ++si)
      for (int lv = 0; lv < 2; ++lv)
        if (!pdc_derm_build(plan.size[si] + 16, lv ? 576 : 288, PDC_DERM_W, p.h_derm.data() + (size_t)(2 * si + lv) * PDC_MAX_CODED * PDC_DERM_W)) {
          c->err = "pdcch: a de-rate-matching list does not fit";
          return LCS_ERR_BAD_ARG;
        }
    HIPCHK(c, hipMemcpyAsync(p.map, p.h_map.data(), sizeof(int) * map_ints, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(p.derm, p.h_derm.data(), sizeof(int16_t) * derm_n, hipMemcpyHostToDevice, c->stream));
    std::memcpy(p.key, key, sizeof(key));
  }
  if (p.jump_rb != n_rb) {
    p.jump_rb = 0;
    lcs_tables::wide_jump_block(n_rb, p.h_jump);
    HIPCHK(c, hipMemcpyAsync(p.jump, p.h_jump, sizeof(p.h_jump), hipMemcpyHostToDevice, c->stream));
    p.jump_rb = n_rb;
  }
  for (int i = 0; i < 4 * n_sf; ++i) p.h_sf[i] = rows4[i];
  for (int i = 0; i < 10; ++i) p.h_sf[4 * n_sf + i] = plan.sh.mi[i];
  // ... and the PCFICH's two rows of every subframe behind them
  int *rows2 = p.h_sf + 4 * n_sf + 10;
  for (int g = 0; g < n_sf; ++g) { rows2[2 * g] = rows4[4 * g]; rows2[2 * g + 1] = (ports == 4 && rows4[4 * g] >= 0) ? rows4[4 * g + 1] : -1; }
  HIPCHK(c, hipMemcpyAsync(p.sf, p.h_sf, sizeof(int) * (6 * n_sf + 10), hipMemcpyHostToDevice, c->stream));
  if (!plan.sh.cfi_force) {
    // the PCFICH of the same rows into a record of this stage's own: the PCFICH stage's blocks are not touched
    hipLaunchKernelGGL(k_pcfich, dim3(n_sf), dim3(PCF_LANES), 0, c->stream, (const double2 *)w.grid.get(), (const int *)(p.sf.get() + 4 * n_sf + 10),
                       (const uint32_t *)p.jump.get(), p.pcf_rec.get(), n_sf, id, (int)cell.cp_type, n_symb, ports, n_rb);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_pcfich_fin, dim3(1), dim3(PCF_LANES), 0, c->stream, p.pcf_rec.get(), n_sf, dl_mask, n_rb, ports);
    HIPCHK(c, hipGetLastError());
  }
  hipLaunchKernelGGL(k_pdcch_llr, dim3(n_sf), dim3(PDC_LLR_THREADS), 0, c->stream, (const double2 *)w.grid.get(), (const int *)p.sf.get(),
                     (const uint32_t *)p.jump.get(), (const lcs_pcfich_info *)p.pcf_rec.get(), reinterpret_cast<const PdcMap *>(p.map.get()), p.llr.get(),
                     p.rec.get(), n_sf, id, (int)cell.cp_type, n_symb, ports, n_rb, plan.sh.cfi_force);
  HIPCHK(c, hipGetLastError());
  const int n_waves = n_sf * PDC_SLOTS * PDC_SIZES;
  hipLaunchKernelGGL(k_pdcch_dec, dim3((n_waves + PDC_DEC_WAVES - 1) / PDC_DEC_WAVES), dim3(64 * PDC_DEC_WAVES), 0, c->stream, (const double *)p.llr.get(),
                     (const int16_t *)p.derm.get(), p.rec.get(), n_sf, plan.n_sizes, plan.size[0], plan.n_sizes > 1 ? plan.size[1] : 0, plan.sh.rnti_mask);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_pdcch_fin, dim3(1), dim3(256), 0, c->stream, p.rec.get(), n_sf, dl_mask, n_rb, ports);
  HIPCHK(c, hipGetLastError());
  return LCS_OK;
}
