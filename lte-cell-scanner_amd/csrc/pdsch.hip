// pdsch.hip -- the PDSCH behind the format 1A grants of the PDCCH common search space, on the device (lcs_pdsch_wide, lcs_pdsch,
// lcs_turbo_decode; the rule: pdsch.h, include/lcs.h).  A translation unit of its own, like pdcch.hip whose kernels find its grants: a
// context that never calls the stage runs no kernel of this file and allocates none of its buffers, and the code objects of the
// chain, of the measurement, of the PCFICH and of the PDCCH are what they are without it.  No atomics, no scratch, every result
// written by exactly one lane, nothing depends on the order in which workgroups run; fp64 throughout and bit-equal to the host twin
// (tests/host/pdsch_host.cpp).  lcs_pdsch_comb_wide and lcs_pdsch_comb add three kernels between the decode and the record
// (k_pdsch_comb_group, k_pdsch_comb_dec, k_pdsch_comb_fin; the rule: pdsch_comb.h): the SI blocks that repeat one transport block are
// grouped and decoded once more from the sum of their soft bits.  k_pdsch_dec and k_pdsch_comb_dec are one function, pds_dec_block,
// behind two gathers.
//
// WHAT LIVES WHERE in k_pdsch_dec.  LDS (about 100 KB of the CU's 160): the three de-rate-matched streams (3 x 2244 doubles, every
// window of 32 steps one double further on so that the lanes of a wave read different banks), the extrinsics (one array in natural
// order, rewritten in place: a step reads and writes its own entry, the second decoder through the interleaver), the windows'
// boundary metrics of both constituent decoders, the interleaver and the decisions.  HBM: the soft bits (read once, by the gather)
// and the forward metrics of the window a lane is in, 256 doubles per lane laid out [step][state][lane] so that a wave's accesses
// coalesce -- they are written and read back once per half iteration and stay in the L2.  The eight state metrics of a window are in
// registers.
#include <cstring>
#include "lcs_internal.h"
#include "lte_device.h"
#include "pdsch.h"
#include "pdsch_comb.h"

#define PDS_LLR_THREADS 256
#define PDS_DEC_THREADS 128
#define PDS_WS_LANES 72                   // lanes of the forward-metric workspace (>= PDS_MAX_WIN)
#define PDS_WS_DOUBLES (PDS_WIN * 8 * PDS_WS_LANES)
static_assert(PDS_MAX_WIN <= PDS_WS_LANES && PDS_MAX_WIN <= PDS_DEC_THREADS, "one lane per window");
static_assert(PDS_COMB_GROUPS * sizeof(PdsCombJob) / sizeof(int) <= 256, "k_pdsch_comb_fin copies the jobs with one thread per word");

// ------------------------------------------------------------------ the plan: one thread per subframe
// Thread g reads the PDCCH record of grid subframe g on the device and writes the subframe's two grant slots: the public block and
// the job (K, F, G, k0's rank, the status).  No host round trip between the PDCCH and the PDSCH.
__global__ __launch_bounds__(128) void k_pdsch_plan(const lcs_pdcch_info *__restrict__ pdc, const int *__restrict__ sfrow, const int *__restrict__ tabs /*tbs [54], qpp [254]*/,
                                                    const PdsTabHead *__restrict__ heads, lcs_pdsch_block *__restrict__ blk, PdsJob *__restrict__ job, int n_sf, PdsPlanIn in) {
  const int g = blockIdx.x * 128 + threadIdx.x;
  if (g >= n_sf) return;
  pds_plan_sf(in, g, sfrow[g], pdc, tabs, tabs + 2 * PDS_N_MCS, heads, blk + PDS_GRANTS * g, job + PDS_GRANTS * g);
}
// The same with a non-zero lcs_set_pdsch_alloc: format 1C's entries, 1A's distributed grants and the two sets of PRBs of every grant slot.
// A kernel of its own, so that k_pdsch_plan is the code it was.
__global__ __launch_bounds__(128) void k_pdsch_plan_alloc(const lcs_pdcch_info *__restrict__ pdc, const int *__restrict__ sfrow,
                                                    const int *__restrict__ tabs /*tbs [54], qpp [254], 1C's tbs [32]*/, const PdsTabHead *__restrict__ heads,
                                                    lcs_pdsch_block *__restrict__ blk, PdsJob *__restrict__ job, unsigned long long *__restrict__ sets,
                                                    int n_sf, PdsPlanIn in, PdsAllocIn al) {
  const int g = blockIdx.x * 128 + threadIdx.x;
  if (g >= n_sf) return;
  pds_plan_sf_alloc<true>(in, al, g, sfrow[g], pdc, tabs, tabs + 2 * PDS_N_MCS + 2 * PDS_N_K, tabs + 2 * PDS_N_MCS, heads, blk + PDS_GRANTS * g, job + PDS_GRANTS * g,
                    sets ? sets + (size_t)PDS_GRANTS * PDS_SET_WORDS * g : nullptr);
}

// ------------------------------------------------------------------ the soft bits: one workgroup per grant slot
// Threads 0 .. 5 build the sequences of the subframe's six reference rows (4 and 5 with four ports only), thread 6 the elements before
// every symbol; thread j makes scrambling words 5 j .. 5 j + 4 from the registers 1600 + 160 j clocks on (the first register's from
// x1s, the second by jumping: 1600 clocks, then 160 2^b for every bit b of j).  Then every thread takes elements e = tid, tid + 256,
// .. -- its (l, k) from the rank, its y and the two channel values --, the lanes of a pair trade hb and y, and the thread writes the
// element's two soft bits.
__global__ __launch_bounds__(PDS_LLR_THREADS) void k_pdsch_llr(const double2 *__restrict__ grid, const PdsJob *__restrict__ jobs, const uint32_t *__restrict__ jump /*[320]*/,
                                                               const uint32_t *__restrict__ x1s /*[256]*/, double *__restrict__ llr, size_t llr_stride, int id, int cp_type,
                                                               int n_symb, int ports, int n_rb) {
  const int slot = blockIdx.x, tid = threadIdx.x;
  __shared__ uint32_t s_bits[6][RS_DL_WIDE_WORDS];
  __shared__ double s_shift[6][4];
  __shared__ uint32_t s_scr[PDS_SCR_WORDS];
  __shared__ int s_base[PDS_MAX_SYM + 1];
  const PdsJob job = jobs[slot];
  if (job.status != LCS_PDSCH_FOLLOW || job.reserved != 0) return;      // the same for the whole workgroup; a set-based grant is k_pdsch_llr_set's
  PdsGeom q;
  q.n_rb = n_rb; q.ports = ports; q.n_symb = n_symb; q.id = id; q.sf = job.sf; q.tdd = job.tdd; q.n_ctrl = job.n_ctrl; q.k_lo = job.k_lo; q.k_hi = job.k_hi;
  if (tid < 24) s_shift[tid >> 2][tid & 3] = 0.0;
  __syncthreads();
  if (tid < (ports == 4 ? 6 : 4)) pds_ref_row(tid, job.sf, id, cp_type, n_symb, n_rb, jump, s_bits[tid], s_shift[tid]);
  if (tid == 6) pds_bases(q, s_base);
  const int n_re = job.n_re, n_chunk = (2 * n_re + 32 * PDS_SCR_CHUNK - 1) / (32 * PDS_SCR_CHUNK);
  if (tid < n_chunk) {
    uint32_t x2 = pds_x2_jump((uint32_t)job.c_init, jump + 32);
#pragma unroll 1
    for (int b = 0; b < 8; ++b) if ((tid >> b) & 1) x2 = pds_x2_jump(x2, jump + 64 + 32 * b);
    pds_scr_chunk(x1s[tid], x2, s_scr + PDS_SCR_CHUNK * tid);
  }
  __syncthreads();
  const double *sfrow = reinterpret_cast<const double *>(grid + (size_t)job.row0 * 12 * n_rb);
  double *out = llr + (size_t)slot * llr_stride;
#pragma unroll 1
  for (int e = tid; e < ((n_re + PDS_LLR_THREADS - 1) / PDS_LLR_THREADS) * PDS_LLR_THREADS; e += PDS_LLR_THREADS) {
    const bool live = e < n_re;
    int l = q.n_ctrl, k = q.k_lo;
    if (live) pds_elem_at(q, s_base, e, &l, &k);
    cd2 y, ha, hb;
    pds_elem(e, l, k, n_rb, ports, n_symb, sfrow, s_bits, s_shift, &y, &ha, &hb);
    if (!live) { y = mk(0.0, 0.0); hb = mk(0.0, 0.0); }
    const cd2 hb_pair = mk(__shfl_xor(hb.re, 1), __shfl_xor(hb.im, 1)), y_pair = mk(__shfl_xor(y.re, 1), __shfl_xor(y.im, 1));
    const cd2 s = pcf_soft(e, ports, y, ha, hb_pair, y_pair);
    if (live) {
      double l0, l1;
      pdc_llr(e, s_scr[(2 * e) >> 5], s, &l0, &l1);
      out[2 * e] = l0;
      out[2 * e + 1] = l1;
    }
  }
}

// The same for a grant whose resource blocks are two sets (a distributed 1A or a 1C grant; launched only with a non-zero
// lcs_set_pdsch_alloc): thread 6 counts the sets' half blocks below and inside the central columns and the elements before every
// symbol, threads 7 and 8 list the PRBs of slot 0 and slot 1 in ascending order; element e's (l, k) comes from pds_set_elem_at.  A
// kernel of its own, so that k_pdsch_llr is the code it was.
__global__ __launch_bounds__(PDS_LLR_THREADS) void k_pdsch_llr_set(const double2 *__restrict__ grid, const PdsJob *__restrict__ jobs, const uint32_t *__restrict__ jump /*[320]*/,
                                                               const uint32_t *__restrict__ x1s /*[256]*/, double *__restrict__ llr, size_t llr_stride, int id, int cp_type,
                                                               int n_symb, int ports, int n_rb, const unsigned long long *__restrict__ sets) {
  const int slot = blockIdx.x, tid = threadIdx.x;
  __shared__ uint32_t s_bits[6][RS_DL_WIDE_WORDS];
  __shared__ double s_shift[6][4];
  __shared__ uint32_t s_scr[PDS_SCR_WORDS];
  __shared__ int s_base[PDS_MAX_SYM + 1];
  __shared__ uint8_t s_prb[2 * PDS_SET_RB];                // a distributed grant's resource blocks, ascending, per slot of the subframe
  __shared__ int s_cut[4];
  const PdsJob job = jobs[slot];
  if (job.status != LCS_PDSCH_FOLLOW || !(job.reserved & PDS_MODE_SET)) return;      // the same for the whole workgroup
  const int n_prb_set = (int)__popcll(sets[PDS_SET_WORDS * slot]) + (int)__popcll(sets[PDS_SET_WORDS * slot + 1]);
  PdsGeom q;
  q.n_rb = n_rb; q.ports = ports; q.n_symb = n_symb; q.id = id; q.sf = job.sf; q.tdd = job.tdd; q.n_ctrl = job.n_ctrl; q.k_lo = job.k_lo; q.k_hi = job.k_hi;
  if (tid < 24) s_shift[tid >> 2][tid & 3] = 0.0;
  __syncthreads();
  if (tid < (ports == 4 ? 6 : 4)) pds_ref_row(tid, job.sf, id, cp_type, n_symb, n_rb, jump, s_bits[tid], s_shift[tid]);
  if (tid == 6) {
    const unsigned long long *m = sets + PDS_SET_WORDS * slot;
    int cut[4];
    pds_set_cut(n_rb, m[0], m[1], cut);
    pds_set_cut(n_rb, m[2], m[3], cut + 2);
    for (int i = 0; i < 4; ++i) s_cut[i] = cut[i];
    pds_set_bases(q, n_prb_set, cut, s_base);
  }
  if (tid == 7 || tid == 8) pds_set_list(n_rb, sets[PDS_SET_WORDS * slot + 2 * (tid - 7)], sets[PDS_SET_WORDS * slot + 2 * (tid - 7) + 1], s_prb + PDS_SET_RB * (tid - 7));
  const int n_re = job.n_re, n_chunk = (2 * n_re + 32 * PDS_SCR_CHUNK - 1) / (32 * PDS_SCR_CHUNK);
  if (tid < n_chunk) {
    uint32_t x2 = pds_x2_jump((uint32_t)job.c_init, jump + 32);
#pragma unroll 1
    for (int b = 0; b < 8; ++b) if ((tid >> b) & 1) x2 = pds_x2_jump(x2, jump + 64 + 32 * b);
    pds_scr_chunk(x1s[tid], x2, s_scr + PDS_SCR_CHUNK * tid);
  }
  __syncthreads();
  const double *sfrow = reinterpret_cast<const double *>(grid + (size_t)job.row0 * 12 * n_rb);
  double *out = llr + (size_t)slot * llr_stride;
#pragma unroll 1
  for (int e = tid; e < ((n_re + PDS_LLR_THREADS - 1) / PDS_LLR_THREADS) * PDS_LLR_THREADS; e += PDS_LLR_THREADS) {
    const bool live = e < n_re;
    int l = q.n_ctrl, k = 0;
    if (live) pds_set_elem_at(q, s_prb, s_cut, s_base, e, &l, &k);
    cd2 y, ha, hb;
    pds_elem(e, l, k, n_rb, ports, n_symb, sfrow, s_bits, s_shift, &y, &ha, &hb);
    if (!live) { y = mk(0.0, 0.0); hb = mk(0.0, 0.0); }
    const cd2 hb_pair = mk(__shfl_xor(hb.re, 1), __shfl_xor(hb.im, 1)), y_pair = mk(__shfl_xor(y.re, 1), __shfl_xor(y.im, 1));
    const cd2 s = pcf_soft(e, ports, y, ha, hb_pair, y_pair);
    if (live) {
      double l0, l1;
      pdc_llr(e, s_scr[(2 * e) >> 5], s, &l0, &l1);
      out[2 * e] = l0;
      out[2 * e + 1] = l1;
    }
  }
}

// ------------------------------------------------------------------ the decode: one workgroup per grant slot
// All threads gather the three streams from the soft bits (din: the streams themselves, the turbo entry point) and fill the
// interleaver; a block whose values are all zero or not all finite is not decoded.  Then lane w < ceil(K / 32) runs window w of the
// first decoder, of the second, .. with the window's eight forward and backward metrics in registers: a window starts from the
// metrics its neighbours left in the previous iteration (read by every lane before any lane writes).  After every iteration the
// lanes pack the decisions, thread 0 takes the CRC, and the workgroup stops together.
// what a decode workgroup keeps in LDS
struct PdsDecLds {
  double d[3][PDS_PAD_D];
  double ext[PDS_PAD_D];
  double ab[2][2][PDS_MAX_WIN + 1][8];                   // [decoder][forward, backward][window boundary][state]
  uint16_t perm[PDS_MAX_K];
  uint8_t hard[PDS_MAX_K];
  uint32_t word[PDS_MAX_WIN];
  int stop;
};
// One block through the decoder by one workgroup of PDS_DEC_THREADS: value(s, k, i) is value k of stream s (i = s (K + 4) + k), ws
// the workgroup's forward-metric room, res -> {n_iter, status}, hard_out the decisions.  k_pdsch_dec and k_pdsch_comb_dec differ in
// what they gather and in the words for the three outcomes; everything from the gather on is this function.
template <class Value>
__device__ __forceinline__ void pds_dec_block(PdsDecLds &L, int K, int F, int f1, int f2, int max_iter, Value value, double *__restrict__ ws_block, int *__restrict__ res,
                                              uint8_t *__restrict__ hard_out, int st_ok, int st_crc, int st_silent) {
  const int tid = threadIdx.x;
  const int D = K + 4, n_win = (K + PDS_WIN - 1) / PDS_WIN;
  int any = 0, bad = 0;
#pragma unroll 1
  for (int i = tid; i < 3 * D; i += PDS_DEC_THREADS) {
    const int s = i / D, k = i - s * D;
    const double v = value(s, k, i);
    L.d[s][pds_pad(k)] = v;
    any |= v != 0.0;
    bad |= !vit_finite(v);
  }
  for (int i = tid; i < K; i += PDS_DEC_THREADS) { L.perm[i] = (uint16_t)pds_qpp(f1, f2, K, i); L.hard[i] = 0; L.ext[pds_pad(i)] = 0.0; }
  for (int i = tid; i < 2 * 2 * (PDS_MAX_WIN + 1) * 8; i += PDS_DEC_THREADS) {
    const int st = i & 7, w = (i >> 3) % (PDS_MAX_WIN + 1), fb = (i >> 3) / (PDS_MAX_WIN + 1) & 1;
    (&L.ab[0][0][0][0])[i] = (fb == 0 && w == 0 && st != 0) ? -INFINITY : 0.0;
  }
  any = __syncthreads_or(any);
  bad = __syncthreads_or(bad);
  if (!any || bad) {
    if (tid == 0) { res[0] = 0; res[1] = st_silent; }
    return;
  }
  if (tid < 2) {                                           // the tail of decoder tid: its values lie at K + 2 tid, K + 2 tid + 1 of the streams
    const int o = K + 2 * tid;
    const double x[3] = {L.d[0][pds_pad(o)], L.d[2][pds_pad(o)], L.d[1][pds_pad(o + 1)]};
    const double z[3] = {L.d[1][pds_pad(o)], L.d[0][pds_pad(o + 1)], L.d[2][pds_pad(o + 1)]};
    double b[8];
    pds_tail_beta(x, z, b);
#pragma unroll
    for (int s = 0; s < 8; ++s) L.ab[tid][1][n_win][s] = b[s];
  }
  __syncthreads();
  const bool lane_on = tid < n_win;
  const int k0 = PDS_WIN * tid, n = lane_on ? (K - k0 < PDS_WIN ? K - k0 : PDS_WIN) : 0;
  double *ws = ws_block + tid;
  int n_iter = 0, ok = 0;
#pragma unroll 1
  for (int it = 1; it <= max_iter; ++it) {
#pragma unroll 1
    for (int dec = 0; dec < 2; ++dec) {
      double a[8], b[8];
#pragma unroll
      for (int s = 0; s < 8; ++s) { a[s] = lane_on ? L.ab[dec][0][tid][s] : 0.0; b[s] = lane_on ? L.ab[dec][1][tid + 1][s] : 0.0; }
      __syncthreads();
      if (lane_on) {
        pds_window(L.d[0], L.d[1 + dec], L.ext, dec ? L.perm : nullptr, dec ? L.hard : nullptr, F, k0, n, a, b, ws, PDS_WS_LANES);
        if (tid + 1 < n_win) {
#pragma unroll
          for (int s = 0; s < 8; ++s) L.ab[dec][0][tid + 1][s] = a[s];
        }
        if (tid > 0) {
#pragma unroll
          for (int s = 0; s < 8; ++s) L.ab[dec][1][tid][s] = b[s];
        }
      }
      __syncthreads();
    }
    if (lane_on) {
      uint32_t word = 0;
      for (int t = 0; t < n; ++t) word |= (uint32_t)((k0 + t >= F) ? (L.hard[k0 + t] & 1) : 0) << t;
      L.word[tid] = word;
    }
    __syncthreads();
    if (tid == 0) L.stop = pds_crc24a(L.word, K) == 0u;
    __syncthreads();
    n_iter = it;
    ok = L.stop;
    if (ok) break;
  }
  for (int i = tid; i < K; i += PDS_DEC_THREADS) hard_out[i] = i >= F ? (L.hard[i] & 1) : 0;
  if (tid == 0) { res[0] = n_iter; res[1] = ok ? st_ok : st_crc; }
}

__global__ __launch_bounds__(PDS_DEC_THREADS) void k_pdsch_dec(const PdsJob *__restrict__ jobs, const double *__restrict__ llr, size_t llr_stride, const double *__restrict__ din,
                                                               const int16_t *__restrict__ rank /*[PDS_TABS][3][PDS_MAX_D]*/, double *__restrict__ ws_all,
                                                               int *__restrict__ res /*[slots][2]: n_iter, status*/, uint8_t *__restrict__ hard_out /*[slots][2240]*/) {
  const int slot = blockIdx.x, tid = threadIdx.x;
  __shared__ PdsDecLds L;
  const PdsJob job = jobs[slot];
  if (job.status != LCS_PDSCH_FOLLOW) {                    // the same for the whole workgroup
    if (tid == 0) { res[2 * slot] = 0; res[2 * slot + 1] = job.status; }
    return;
  }
  const double *sl = llr + (size_t)slot * llr_stride;
  const int16_t *rk = rank + (size_t)job.tab * 3 * PDS_MAX_D;
  pds_dec_block(L, job.K, job.F, job.f1, job.f2, job.max_iter,
                [&](int s, int k, int i) { return job.direct ? din[i] : pds_derm_value(sl, job.G, job.N, job.base, rk[s * PDS_MAX_D + k]); },
                ws_all + (size_t)slot * PDS_WS_DOUBLES, res + 2 * slot, hard_out + (size_t)slot * PDS_MAX_K, LCS_PDSCH_OK, LCS_PDSCH_CRC, LCS_PDSCH_SILENT);
}

// ------------------------------------------------------------------ the redundancy versions combined (pdsch_comb.h)
// The grouping: one workgroup.  Thread 0 lists the slots that hold a grant as k_pdsch_fin does; thread i reads block i as the grouping
// sees it (its status is what the decode left); thread 0 forms the groups; thread g completes group slot g: its members' grant slots,
// the sizes and the table of its first member, whether it is decoded and whose decisions its payload is.  No atomics.
__global__ __launch_bounds__(64) void k_pdsch_comb_group(const lcs_pdsch_block *__restrict__ blk, const PdsJob *__restrict__ jobs, const int *__restrict__ res,
                                                         PdsCombJob *__restrict__ cjobs, int n_sf, int si_window, int no_sib1) {
  const int tid = threadIdx.x;
  __shared__ int s_map[LCS_PDSCH_MAX_BLOCKS], s_n[3], s_work[PDS_COMB_WORK];
  __shared__ PdsCombBlock s_blk[LCS_PDSCH_MAX_BLOCKS];
  __shared__ PdsCombJob s_job[PDS_COMB_GROUPS];
  if (tid == 0) {
    int n = 0;
    for (int i = 0; i < PDS_GRANTS * n_sf && n < LCS_PDSCH_MAX_BLOCKS; ++i)
      if (jobs[i].status != 0) s_map[n++] = i;
    s_n[0] = n;
  }
  __syncthreads();
  const int n = s_n[0];
  if (tid < n) {
    const lcs_pdsch_block &b = blk[s_map[tid]];
    PdsCombBlock v;
    v.kind = b.kind; v.status = res[2 * s_map[tid] + 1]; v.subframe = b.subframe; v.tbs = b.tbs; v.rv = b.rv;
    s_blk[tid] = v;
  }
  __syncthreads();
  if (tid == 0) s_n[1] = pds_comb_groups(s_blk, n, si_window, no_sib1, s_work, s_job, &s_n[2]);
  __syncthreads();
  if (tid < PDS_COMB_GROUPS) {
    PdsCombJob *o = &cjobs[tid];
    if (tid >= s_n[1]) {
      o->status = 0; o->n_members = 0; o->rule = o->tbs = o->K = o->F = o->f1 = o->f2 = o->tab = o->N = o->max_iter = o->rv_mask = o->n_ok = 0; o->src = -1;
      for (int m = 0; m < PDS_COMB_MEMBERS; ++m) o->slot[m] = o->block[m] = -1;
    } else {
      const PdsCombJob &g = s_job[tid];
      int src = -1;
      for (int m = 0; m < PDS_COMB_MEMBERS; ++m) {
        const int sl = m < g.n_members ? s_map[g.block[m]] : -1;
        o->slot[m] = sl; o->block[m] = m < g.n_members ? g.block[m] : -1;
        if (sl >= 0 && src < 0 && (g.n_ok == 0 || res[2 * sl + 1] == LCS_PDSCH_OK)) src = sl;
      }
      const PdsJob &j0 = jobs[s_map[g.block[0]]];
      o->n_members = g.n_members; o->rule = g.rule; o->tbs = g.tbs; o->K = j0.K; o->F = j0.F; o->f1 = j0.f1; o->f2 = j0.f2; o->tab = j0.tab; o->N = j0.N;
      o->max_iter = j0.max_iter; o->rv_mask = g.rv_mask; o->n_ok = g.n_ok;
      const bool decode = g.n_ok == 0 && g.n_members >= 2;
      o->status = g.n_ok > 0 ? LCS_PDSCH_COMB_MEMBER : decode ? LCS_PDSCH_FOLLOW : LCS_PDSCH_COMB_CRC;
      o->src = decode ? -1 : src;
    }
    o->n_overflow = s_n[2]; o->reserved = 0;
  }
}

// Combine and decode: one workgroup per group slot, laid out as k_pdsch_dec.  A group that needs no decode ends before any LDS set-up.
// The gather sums the members' de-rate-matched values in member order (pds_comb_value); from there on it is pds_dec_block.
__global__ __launch_bounds__(PDS_DEC_THREADS) void k_pdsch_comb_dec(const PdsCombJob *__restrict__ cjobs, const PdsJob *__restrict__ jobs, const double *__restrict__ llr,
                                                                    size_t llr_stride, const int16_t *__restrict__ rank, double *__restrict__ ws_all,
                                                                    int *__restrict__ res /*[groups][2]*/, uint8_t *__restrict__ hard_out /*[groups][2240]*/) {
  const int g = blockIdx.x, tid = threadIdx.x;
  __shared__ PdsDecLds L;
  const PdsCombJob job = cjobs[g];
  if (job.status != LCS_PDSCH_FOLLOW) {                    // the same for the whole workgroup
    if (tid == 0) { res[2 * g] = 0; res[2 * g + 1] = job.status; }
    return;
  }
  const double *ml[PDS_COMB_MEMBERS];
  int mG[PDS_COMB_MEMBERS], mbase[PDS_COMB_MEMBERS];
#pragma unroll
  for (int m = 0; m < PDS_COMB_MEMBERS; ++m) {
    const int sl = m < job.n_members ? job.slot[m] : job.slot[0];
    ml[m] = llr + (size_t)sl * llr_stride; mG[m] = jobs[sl].G; mbase[m] = jobs[sl].base;
  }
  const int16_t *rk = rank + (size_t)job.tab * 3 * PDS_MAX_D;
  pds_dec_block(L, job.K, job.F, job.f1, job.f2, job.max_iter,
                [&](int s, int k, int) { return pds_comb_value(ml, mG, mbase, job.n_members, job.N, rk[s * PDS_MAX_D + k]); },
                ws_all + (size_t)g * PDS_WS_DOUBLES, res + 2 * g, hard_out + (size_t)g * PDS_MAX_K, LCS_PDSCH_COMB_OK, LCS_PDSCH_COMB_CRC, LCS_PDSCH_COMB_SILENT);
}

// The combined record: one workgroup.  Thread g writes group g's fields and counts the OK members whose payload equals the first's;
// all threads form the payload bytes (from the decisions of the member named by the grouping, or the group's own); thread 0 the head.
__global__ __launch_bounds__(256) void k_pdsch_comb_fin(const PdsCombJob *__restrict__ cjobs, const int *__restrict__ res, const uint8_t *__restrict__ hard,
                                                        const int *__restrict__ cres, const uint8_t *__restrict__ chard, lcs_pdsch_comb_info *__restrict__ out) {
  const int tid = threadIdx.x;
  constexpr int JOB_INTS = (int)(sizeof(PdsCombJob) / sizeof(int));
  __shared__ PdsCombJob s_job[PDS_COMB_GROUPS];          // the eight jobs, read once: every loop bound and barrier below depends on LDS alone
  __shared__ int s_ok[PDS_COMB_GROUPS][PDS_COMB_MEMBERS], s_same[PDS_COMB_GROUPS];
  if (tid < PDS_COMB_GROUPS * JOB_INTS) reinterpret_cast<int *>(s_job)[tid] = reinterpret_cast<const int *>(cjobs)[tid];
  __syncthreads();
  if (tid < PDS_COMB_GROUPS * PDS_COMB_MEMBERS) {
    const int gi = tid / PDS_COMB_MEMBERS, m = tid % PDS_COMB_MEMBERS, sl = s_job[gi].slot[m];
    s_ok[gi][m] = s_job[gi].n_ok > 0 && m < s_job[gi].n_members && sl >= 0 && res[2 * sl + 1] == LCS_PDSCH_OK;
  }
  __syncthreads();
  // n_same: all threads compare the tbs decisions of every OK member with the first OK member's (the payload bytes are those bits)
#pragma unroll 1
  for (int gi = 0; gi < PDS_COMB_GROUPS; ++gi) {
    const PdsCombJob &j = s_job[gi];
    int same = 0;
#pragma unroll 1
    for (int m = 0; m < PDS_COMB_MEMBERS; ++m) {
      if (!s_ok[gi][m]) continue;                          // (the same for the whole workgroup)
      int diff = 0;
      for (int i = tid; i < j.tbs; i += 256) diff |= hard[(size_t)j.slot[m] * PDS_MAX_K + j.F + i] != hard[(size_t)j.src * PDS_MAX_K + j.F + i];
      same += !__syncthreads_or(diff);
    }
    if (tid == 0) s_same[gi] = same;
  }
  __syncthreads();
  if (tid < PDS_COMB_GROUPS) {
    const PdsCombJob &j = s_job[tid];
    lcs_pdsch_comb_group *o = &out->group[tid];
    o->n_members = j.n_members; o->rule = j.rule; o->tbs = j.tbs; o->K = j.K; o->F = j.F; o->rv_mask = j.rv_mask; o->n_ok_members = j.n_ok;
    for (int m = 0; m < PDS_COMB_MEMBERS; ++m) o->member[m] = j.status ? j.block[m] : 0;
    o->n_iter = cres[2 * tid]; o->status = cres[2 * tid + 1]; o->reserved[0] = o->reserved[1] = 0;
    o->n_same = s_same[tid];
  }
  for (int i = tid; i < PDS_COMB_GROUPS * LCS_PDSCH_PAYLOAD; i += 256) {
    const int gi = i / LCS_PDSCH_PAYLOAD, t = i - gi * LCS_PDSCH_PAYLOAD;
    const PdsCombJob &j = s_job[gi];
    const int st = cres[2 * gi + 1];
    uint8_t v = 0;
    if (st == LCS_PDSCH_COMB_MEMBER || st == LCS_PDSCH_COMB_OK || st == LCS_PDSCH_COMB_CRC)
      v = pds_payload_byte(j.src >= 0 ? hard + (size_t)j.src * PDS_MAX_K : chard + (size_t)gi * PDS_MAX_K, j.F, j.tbs, t);
    out->group[gi].payload[t] = v;
  }
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int gi = 0; gi < PDS_COMB_GROUPS; ++gi) n += s_job[gi].status != 0;
    pds_comb_summary(out, n, s_job[0].n_overflow);
  }
}

// ------------------------------------------------------------------ the record: one workgroup
// Thread 0 lists the slots that hold a grant, in (subframe, candidate slot) order; thread i copies block i with what the decode left;
// all threads form the payload bytes and zero the blocks beyond; thread 0 writes the head.  No atomics.
__global__ __launch_bounds__(256) void k_pdsch_fin(const lcs_pdsch_block *__restrict__ blk, const PdsJob *__restrict__ jobs, const int *__restrict__ res,
                                                   const uint8_t *__restrict__ hard, lcs_pdsch_info *__restrict__ out, int n_sf, int dl_mask, int n_rb, int ports) {
  const int tid = threadIdx.x;
  __shared__ int s_map[LCS_PDSCH_MAX_BLOCKS], s_n[2];
  if (tid == 0) {
    int n = 0, over = 0;
    for (int i = 0; i < PDS_GRANTS * n_sf; ++i) {
      if (jobs[i].status == 0) continue;
      if (n < LCS_PDSCH_MAX_BLOCKS) s_map[n++] = i; else over += 1;
    }
    s_n[0] = n; s_n[1] = over;
  }
  __syncthreads();
  const int n = s_n[0];
  if (tid < LCS_PDSCH_MAX_BLOCKS) {
    lcs_pdsch_block *o = &out->block[tid];
    if (tid < n) {
      const lcs_pdsch_block &b = blk[s_map[tid]];
      o->subframe = b.subframe; o->slot = b.slot; o->rnti = b.rnti; o->kind = b.kind; o->rb_start = b.rb_start; o->n_prb = b.n_prb; o->mcs = b.mcs; o->rv = b.rv;
      o->tbs = b.tbs; o->n_re = b.n_re; o->K = b.K; o->F = b.F; o->n_iter = res[2 * s_map[tid]]; o->status = res[2 * s_map[tid] + 1];
    } else {
      o->subframe = o->slot = o->rnti = o->kind = o->rb_start = o->n_prb = o->mcs = o->rv = o->tbs = o->n_re = o->K = o->F = o->n_iter = o->status = 0;
    }
  }
  for (int i = tid; i < LCS_PDSCH_MAX_BLOCKS * LCS_PDSCH_PAYLOAD; i += 256) {
    const int bi = i / LCS_PDSCH_PAYLOAD, t = i - bi * LCS_PDSCH_PAYLOAD;
    uint8_t v = 0;
    if (bi < n) {
      const int sl = s_map[bi], st = res[2 * sl + 1];
      if (st == LCS_PDSCH_OK || st == LCS_PDSCH_CRC) v = pds_payload_byte(hard + (size_t)sl * PDS_MAX_K, blk[sl].F, blk[sl].tbs, t);
    }
    out->block[bi].payload[t] = v;
  }
  __syncthreads();
  if (tid == 0) pds_summary(out, n_sf, n, s_n[1], dl_mask, n_rb, ports);
}

// ------------------------------------------------------------------ launchers
namespace {
// the tables that do not depend on the call: transport block sizes, interleaver parameters, the rank tables of the 54 (column, mcs)
int pdsch_tables(lcs_ctx *c) {
  lcs_ctx::Pdsch &p = c->pdsch;
  int rc;
  const size_t n_tabs = 2 * PDS_N_MCS + 2 * PDS_N_K + PDS_N_1C, n_heads = (size_t)(PDS_TABS + PDS_N_1C) * sizeof(PdsTabHead) / sizeof(int),
               n_rank = (size_t)(PDS_TABS + PDS_N_1C) * 3 * PDS_MAX_D;
  if ((rc = p.tabs.reserve(c, n_tabs)) || (rc = p.heads.reserve(c, n_heads)) || (rc = p.rank.reserve(c, n_rank)) || (rc = p.x1s.reserve(c, 256)) ||
      (rc = p.res.reserve(c, 2 * PDS_GRANTS * PCF_MAX_SF)) || (rc = p.hard.reserve(c, (size_t)PDS_GRANTS * PCF_MAX_SF * PDS_MAX_K)) ||
      (rc = p.job.reserve(c, (size_t)PDS_GRANTS * PCF_MAX_SF * sizeof(PdsJob) / sizeof(int))) || (rc = p.blk.reserve(c, (size_t)PDS_GRANTS * PCF_MAX_SF)) ||
      (rc = p.rec.reserve(c, 1)) || (rc = p.sfrow.reserve(c, PCF_MAX_SF)) || (rc = p.jump.reserve(c, PDS_JUMP_WORDS)) || (rc = p.din.reserve(c, 3 * PDS_MAX_D))) return rc;
  if (p.tables_ready) return LCS_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  p.h_tabs.assign(n_tabs, 0);
  for (int i = 0; i < 2 * PDS_N_MCS; ++i) p.h_tabs[(size_t)i] = PDS_TBS[i / PDS_N_MCS][i % PDS_N_MCS];
  for (int i = 0; i < 2 * PDS_N_K; ++i) p.h_tabs[(size_t)(2 * PDS_N_MCS + i)] = PDS_QPP[i / 2][i % 2];
  for (int i = 0; i < PDS_N_1C; ++i) p.h_tabs[(size_t)(2 * PDS_N_MCS + 2 * PDS_N_K + i)] = PDS_TBS_1C[i];
  p.h_heads.assign(n_heads, 0);
  p.h_rank.assign(n_rank, (int16_t)-1);
  PdsTabHead *heads = reinterpret_cast<PdsTabHead *>(p.h_heads.data());
  for (int t = 0; t < 2 * PDS_N_MCS; ++t) {
    const int ki = pds_k_ceil_index(PDS_TBS[t / PDS_N_MCS][t % PDS_N_MCS] + 24), K = pds_k_at(ki);
    pds_rank_build(K, K - (PDS_TBS[t / PDS_N_MCS][t % PDS_N_MCS] + 24), &heads[t], p.h_rank.data() + (size_t)t * 3 * PDS_MAX_D);
  }
  pds_x1_states(p.h_x1s);
  HIPCHK(c, hipMemcpyAsync(p.tabs, p.h_tabs.data(), sizeof(int) * n_tabs, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(p.x1s, p.h_x1s, sizeof(p.h_x1s), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(p.heads, p.h_heads.data(), sizeof(int) * n_heads, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(p.rank, p.h_rank.data(), sizeof(int16_t) * n_rank, hipMemcpyHostToDevice, c->stream));
  p.tables_ready = true;
  p.tables_1c_ready = false;
  for (int f = 0; f < LCS_PDSCH_MAX_FORCED; ++f) p.forced_key[f][0] = p.forced_key[f][1] = 0;
  return LCS_OK;
}
// the rank table of slot 2 * 27 + f for (K, F), rebuilt when they change
int pdsch_forced_table(lcs_ctx *c, int f, int K, int F) {
  lcs_ctx::Pdsch &p = c->pdsch;
  if (p.forced_key[f][0] == K && p.forced_key[f][1] == F + 1) return LCS_OK;
  p.forced_key[f][0] = 0;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int t = 2 * PDS_N_MCS + f;
  PdsTabHead *heads = reinterpret_cast<PdsTabHead *>(p.h_heads.data());
  pds_rank_build(K, F, &heads[t], p.h_rank.data() + (size_t)t * 3 * PDS_MAX_D);
  HIPCHK(c, hipMemcpyAsync(reinterpret_cast<PdsTabHead *>(p.heads.get()) + t, &heads[t], sizeof(PdsTabHead), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(p.rank.get() + (size_t)t * 3 * PDS_MAX_D, p.h_rank.data() + (size_t)t * 3 * PDS_MAX_D, sizeof(int16_t) * 3 * PDS_MAX_D, hipMemcpyHostToDevice, c->stream));
  p.forced_key[f][0] = K; p.forced_key[f][1] = F + 1;
  return LCS_OK;
}
// the rank tables of format 1C's 32 sizes, behind the others: built by the first call that follows 1C
int pdsch_tables_1c(lcs_ctx *c) {
  lcs_ctx::Pdsch &p = c->pdsch;
  if (p.tables_1c_ready) return LCS_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  PdsTabHead *heads = reinterpret_cast<PdsTabHead *>(p.h_heads.data());
  for (int i = 0; i < PDS_N_1C; ++i) {
    const int K = pds_k_at(pds_k_ceil_index(PDS_TBS_1C[i] + 24)), t = PDS_TABS + i;
    pds_rank_build(K, K - (PDS_TBS_1C[i] + 24), &heads[t], p.h_rank.data() + (size_t)t * 3 * PDS_MAX_D);
  }
  HIPCHK(c, hipMemcpyAsync(reinterpret_cast<PdsTabHead *>(p.heads.get()) + PDS_TABS, &heads[PDS_TABS], sizeof(PdsTabHead) * PDS_N_1C, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(p.rank.get() + (size_t)PDS_TABS * 3 * PDS_MAX_D, p.h_rank.data() + (size_t)PDS_TABS * 3 * PDS_MAX_D, sizeof(int16_t) * PDS_N_1C * 3 * PDS_MAX_D,
                           hipMemcpyHostToDevice, c->stream));
  p.tables_1c_ready = true;
  return LCS_OK;
}
}  // namespace

int lcs_launch_pdsch(lcs_ctx *c, const lcs_cell &cell, const int *rows4, const int *sfrow, int n_sf, int n_rb, int dl_mask, const PdcchPlan &plan, const PdschPlan &ps,
                     const PdschCombPlan *comb) {
  lcs_ctx::Pdsch &p = c->pdsch;
  lcs_ctx::MeasWide &w = c->meas_wide;
  int rc;
  if (n_sf <= 0 || n_sf > PCF_MAX_SF) { c->err = "pdsch: no such number of subframes"; return LCS_ERR_BAD_ARG; }
  if (comb && ((rc = p.cjob.reserve(c, (size_t)PDS_COMB_GROUPS * sizeof(PdsCombJob) / sizeof(int))) || (rc = p.cres.reserve(c, 2 * PDS_COMB_GROUPS)) ||
               (rc = p.chard.reserve(c, (size_t)PDS_COMB_GROUPS * PDS_MAX_K)) || (rc = p.cws.reserve(c, (size_t)PDS_COMB_GROUPS * PDS_WS_DOUBLES)) ||
               (rc = p.crec.reserve(c, 1)))) return rc;
  const int n_symb = cell.cp_type == LCS_CP_NORMAL ? 7 : 6, id = cell.n_id_2 + 3 * cell.n_id_1, ports = pcf_ports(cell.n_ports);
  if ((rc = pdsch_tables(c))) return rc;
  const PdsAllocIn al = {ps.alloc_flags, ps.sfn0, ps.si_window, 1 - ps.i_1a};
  if ((al.flags & 2) && (rc = pdsch_tables_1c(c))) return rc;
  if (al.flags && (rc = p.sets.reserve(c, (size_t)PDS_GRANTS * PDS_SET_WORDS * PCF_MAX_SF))) return rc;
  unsigned long long *sets = al.flags ? p.sets.get() : nullptr;
  PdsPlanIn in;
  in.n_rb = n_rb; in.ports = ports; in.n_symb = n_symb; in.id = id; in.tdd = ps.tdd; in.i_1a = ps.i_1a; in.rnti_mask = ps.rnti_mask; in.max_iter = ps.max_iter;
  in.n_forced = ps.n_forced;
  for (int f = 0; f < LCS_PDSCH_MAX_FORCED; ++f) {
    in.forced[f] = ps.forced[f];
    if (f >= ps.n_forced) continue;
    const int ki = pds_k_ceil_index(ps.forced[f].tbs + 24);
    if ((rc = pdsch_forced_table(c, f, pds_k_at(ki), pds_k_at(ki) - (ps.forced[f].tbs + 24)))) return rc;
  }
  const int n_slots = PDS_GRANTS * n_sf;
  const size_t llr_stride = (size_t)2 * 12 * n_rb * PDS_MAX_SYM;
  if ((rc = p.llr.reserve(c, llr_stride * n_slots)) || (rc = p.ws.reserve(c, (size_t)PDS_WS_DOUBLES * n_slots))) return rc;
  if (p.jump_rb != n_rb) {
    p.jump_rb = 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    lcs_tables::wide_jump_block(n_rb, p.h_jump);
    for (int b = 0; b < 8; ++b) lcs_tables::pn_jump_table((32 * PDS_SCR_CHUNK) << b, p.h_jump + 64 + 32 * b);
    HIPCHK(c, hipMemcpyAsync(p.jump, p.h_jump, sizeof(p.h_jump), hipMemcpyHostToDevice, c->stream));
    p.jump_rb = n_rb;
  }
  // pdcch.hip's kernels (and through them pcfich.hip's) on blocks of this stage's own: their code objects are those files'
  if ((rc = lcs_launch_pdcch_in(c, p.pdc, cell, rows4, n_sf, n_rb, dl_mask, plan))) return rc;
  for (int g = 0; g < n_sf; ++g) p.h_sfrow[g] = sfrow[g];
  HIPCHK(c, hipMemcpyAsync(p.sfrow, p.h_sfrow, sizeof(int) * n_sf, hipMemcpyHostToDevice, c->stream));
  PdsJob *jobs = reinterpret_cast<PdsJob *>(p.job.get());
  if (!sets) {
    hipLaunchKernelGGL(k_pdsch_plan, dim3((n_sf + 127) / 128), dim3(128), 0, c->stream, (const lcs_pdcch_info *)p.pdc.rec.get(), (const int *)p.sfrow.get(),
                       (const int *)p.tabs.get(), reinterpret_cast<const PdsTabHead *>(p.heads.get()), p.blk.get(), jobs, n_sf, in);
    HIPCHK(c, hipGetLastError());
  } else {
    hipLaunchKernelGGL(k_pdsch_plan_alloc, dim3((n_sf + 127) / 128), dim3(128), 0, c->stream, (const lcs_pdcch_info *)p.pdc.rec.get(), (const int *)p.sfrow.get(),
                       (const int *)p.tabs.get(), reinterpret_cast<const PdsTabHead *>(p.heads.get()), p.blk.get(), jobs, sets, n_sf, in, al);
    HIPCHK(c, hipGetLastError());
  }
  hipLaunchKernelGGL(k_pdsch_llr, dim3(n_slots), dim3(PDS_LLR_THREADS), 0, c->stream, (const double2 *)w.grid.get(), (const PdsJob *)jobs, (const uint32_t *)p.jump.get(),
                     (const uint32_t *)p.x1s.get(), p.llr.get(), llr_stride, id, (int)cell.cp_type, n_symb, ports, n_rb);
  HIPCHK(c, hipGetLastError());
  if (sets) {
    hipLaunchKernelGGL(k_pdsch_llr_set, dim3(n_slots), dim3(PDS_LLR_THREADS), 0, c->stream, (const double2 *)w.grid.get(), (const PdsJob *)jobs, (const uint32_t *)p.jump.get(),
                       (const uint32_t *)p.x1s.get(), p.llr.get(), llr_stride, id, (int)cell.cp_type, n_symb, ports, n_rb, (const unsigned long long *)sets);
    HIPCHK(c, hipGetLastError());
  }
  hipLaunchKernelGGL(k_pdsch_dec, dim3(n_slots), dim3(PDS_DEC_THREADS), 0, c->stream, (const PdsJob *)jobs, (const double *)p.llr.get(), llr_stride, (const double *)nullptr,
                     (const int16_t *)p.rank.get(), p.ws.get(), p.res.get(), p.hard.get());
  HIPCHK(c, hipGetLastError());
  p.last_stride = llr_stride; p.last_n_sf = n_sf; p.last_n_rb = n_rb;
  if (comb) {
    PdsCombJob *cjobs = reinterpret_cast<PdsCombJob *>(p.cjob.get());
    hipLaunchKernelGGL(k_pdsch_comb_group, dim3(1), dim3(64), 0, c->stream, (const lcs_pdsch_block *)p.blk.get(), (const PdsJob *)jobs, (const int *)p.res.get(), cjobs, n_sf,
                       comb->si_window, comb->no_sib1);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_pdsch_comb_dec, dim3(PDS_COMB_GROUPS), dim3(PDS_DEC_THREADS), 0, c->stream, (const PdsCombJob *)cjobs, (const PdsJob *)jobs, (const double *)p.llr.get(),
                       llr_stride, (const int16_t *)p.rank.get(), p.cws.get(), p.cres.get(), p.chard.get());
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_pdsch_comb_fin, dim3(1), dim3(256), 0, c->stream, (const PdsCombJob *)cjobs, (const int *)p.res.get(), (const uint8_t *)p.hard.get(),
                       (const int *)p.cres.get(), (const uint8_t *)p.chard.get(), p.crec.get());
    HIPCHK(c, hipGetLastError());
  }
  hipLaunchKernelGGL(k_pdsch_fin, dim3(1), dim3(256), 0, c->stream, (const lcs_pdsch_block *)p.blk.get(), (const PdsJob *)jobs, (const int *)p.res.get(),
                     (const uint8_t *)p.hard.get(), p.rec.get(), n_sf, dl_mask, n_rb, ports);
  HIPCHK(c, hipGetLastError());
  return LCS_OK;
}

// the turbo decoder alone on d [3][K + 4] from the host -> c->pdsch.res[0 .. 1], c->pdsch.hard[0 .. K - 1]
int lcs_launch_turbo(lcs_ctx *c, const double *h_d, int K, int F, int max_iter) {
  lcs_ctx::Pdsch &p = c->pdsch;
  int rc;
  if ((rc = pdsch_tables(c)) || (rc = p.ws.reserve(c, PDS_WS_DOUBLES))) return rc;
  const int ki = pds_k_index(K);
  HIPCHK(c, hipStreamSynchronize(c->stream));              // nothing reads the host blocks that are rewritten
  p.h_din.assign(h_d, h_d + 3 * (size_t)(K + 4));
  PdsJob j = {};
  j.status = LCS_PDSCH_FOLLOW; j.K = K; j.F = F; j.f1 = PDS_QPP[ki][0]; j.f2 = PDS_QPP[ki][1]; j.max_iter = max_iter; j.direct = 1;
  std::memcpy(p.h_job, &j, sizeof(j));
  p.last_n_sf = 0;                                         // (slot 0's job is this block's now: lcs_pdsch_last_soft has nothing to hand out)
  HIPCHK(c, hipMemcpyAsync(p.din, p.h_din.data(), sizeof(double) * 3 * (size_t)(K + 4), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(p.job, p.h_job, sizeof(j), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_pdsch_dec, dim3(1), dim3(PDS_DEC_THREADS), 0, c->stream, reinterpret_cast<const PdsJob *>(p.job.get()), (const double *)p.din.get(), (size_t)0,
                     (const double *)p.din.get(), (const int16_t *)p.rank.get(), p.ws.get(), p.res.get(), p.hard.get());
  HIPCHK(c, hipGetLastError());
  return LCS_OK;
}
