// pdsch_comb.h -- the redundancy versions of one SI transport block, combined: which blocks of the PDSCH record repeat a transport
// block, the sum of their de-rate-matched soft bits and the record of the groups (lcs_pdsch_comb_wide, lcs_pdsch_comb; the rule is
// stated in include/lcs.h: lcs_pdsch_comb_info).  Host and device: the kernels (pdsch.hip: k_pdsch_comb_group, k_pdsch_comb_dec,
// k_pdsch_comb_fin) and the host twin (tests/host/pdsch_comb_host.cpp) run the functions of this file, which stand on pdsch.h's.
//
// THE ORDER OF THE SUM IS FIXED HERE: 0 + member 0's value + member 1's + .., every member's value pds_derm_value's own sum.
#pragma once
#include "pdsch.h"

#define PDS_COMB_GROUPS LCS_PDSCH_COMB_MAX_GROUPS
#define PDS_COMB_MEMBERS LCS_PDSCH_COMB_MAX_MEMBERS
static_assert(sizeof(lcs_pdsch_comb_cfg) == 16 && sizeof(lcs_pdsch_comb_group) == 344 && sizeof(lcs_pdsch_comb_info) == 48 + PDS_COMB_GROUPS * 344,
              "include/lcs.h: lcs_pdsch_comb_info");

// what the grouping leaves per group slot.  status LCS_PDSCH_FOLLOW: the combine-and-decode kernel runs it; else the group's final
// status (0: no group).  slot[m]: the grant slot (of PdsJob, the soft bits and the decisions) of member m, block[m] its place in the
// record.  src: the grant slot whose decisions are the group's payload (the first OK member, a lone CRC member), -1: the group's own
struct PdsCombJob {
  int status, n_members, slot[PDS_COMB_MEMBERS], block[PDS_COMB_MEMBERS], rule, tbs, K, F, f1, f2, tab, N, max_iter, rv_mask, n_ok, src, n_overflow, reserved;
};
// a block of the record as the grouping sees it
struct PdsCombBlock { int kind, status, subframe, tbs, rv; };

__host__ __device__ __forceinline__ bool pds_comb_member(const PdsCombBlock &b) { return b.kind == 1 && (b.status == LCS_PDSCH_OK || b.status == LCS_PDSCH_CRC); }

// The groups of the n listed blocks, in the order of their first member: the first PDS_COMB_GROUPS into g[] (n_members, block[], rule,
// tbs, rv_mask, n_ok; the rest of a job is the caller's), the others counted.  si_window 0: rule 2 off.  work: room of the caller's
// (LDS on the device: nothing here is indexed out of registers).  -> the groups listed
#define PDS_COMB_WORK (5 * LCS_PDSCH_MAX_BLOCKS)
__host__ __device__ inline int pds_comb_groups(const PdsCombBlock *b, int n, int si_window, int no_sib1, int *work /*[PDS_COMB_WORK]*/,
                                               PdsCombJob *g /*[PDS_COMB_GROUPS]*/, int *n_overflow) {
  // every group there is (at most one per block): its rule, key and first subframe and how many members it has
  int *rule = work, *tbs = work + LCS_PDSCH_MAX_BLOCKS, *par = work + 2 * LCS_PDSCH_MAX_BLOCKS, *first_sf = work + 3 * LCS_PDSCH_MAX_BLOCKS,
      *cnt = work + 4 * LCS_PDSCH_MAX_BLOCKS;
  int n_all = 0;
  for (int i = 0; i < n && i < LCS_PDSCH_MAX_BLOCKS; ++i) {
    if (!pds_comb_member(b[i])) continue;
    const bool sib1 = !no_sib1 && b[i].subframe % 10 == 5;
    if (!sib1 && si_window <= 0) continue;
    const int r = sib1 ? 1 : 2, p = sib1 ? (b[i].subframe / 10) % 2 : 0;
    int open = -1;                                          // the latest group of the key
    for (int u = 0; u < n_all; ++u) if (rule[u] == r && tbs[u] == b[i].tbs && par[u] == p) open = u;
    if (open >= 0 && (cnt[open] >= PDS_COMB_MEMBERS || (r == 2 && b[i].subframe - first_sf[open] >= si_window))) open = -1;
    if (open < 0) {
      open = n_all++;
      rule[open] = r; tbs[open] = b[i].tbs; par[open] = p; first_sf[open] = b[i].subframe; cnt[open] = 0;
      if (open < PDS_COMB_GROUPS) {
        PdsCombJob &j = g[open];
        j.status = 0; j.n_members = 0; j.rule = r; j.tbs = b[i].tbs; j.rv_mask = 0; j.n_ok = 0; j.src = -1;
        for (int m = 0; m < PDS_COMB_MEMBERS; ++m) j.block[m] = j.slot[m] = -1;
      }
    }
    if (open < PDS_COMB_GROUPS) {
      PdsCombJob &j = g[open];
      j.block[j.n_members++] = i;
      j.rv_mask |= 1 << (b[i].rv & 3);
      j.n_ok += b[i].status == LCS_PDSCH_OK;
    }
    cnt[open] += 1;
  }
  *n_overflow = n_all > PDS_COMB_GROUPS ? n_all - PDS_COMB_GROUPS : 0;
  return n_all < PDS_COMB_GROUPS ? n_all : PDS_COMB_GROUPS;
}

// value k of stream s of a group: r0 its rank in the table of (K, F), N the table's non-nulls; per member the soft bits, their number
// and base(rv)
__host__ __device__ __forceinline__ double pds_comb_value(const double *const *llr, const int *G, const int *base, int n_members, int N, int r0) {
  double v = 0.0;
#pragma unroll
  for (int m = 0; m < PDS_COMB_MEMBERS; ++m) if (m < n_members) v = v + pds_derm_value(llr[m], G[m], N, base[m], r0);
  return v;
}

// the head of the record from its groups
__host__ __device__ inline void pds_comb_summary(lcs_pdsch_comb_info *o, int n_groups, int n_overflow) {
  int st[LCS_PDSCH_COMB_N_STATUS], members = 0, decoded = 0;
  for (int i = 0; i < LCS_PDSCH_COMB_N_STATUS; ++i) st[i] = 0;
  for (int i = 0; i < n_groups; ++i) {
    const lcs_pdsch_comb_group &g = o->group[i];
    if (g.status >= 0 && g.status < LCS_PDSCH_COMB_N_STATUS) st[g.status] += 1;
    members += g.n_members;
    decoded += (g.status == LCS_PDSCH_COMB_OK || g.status == LCS_PDSCH_COMB_CRC) && g.n_iter > 0;
  }
  o->n_groups = n_groups; o->n_overflow = n_overflow; o->n_members = members; o->n_decoded = decoded;
  for (int i = 0; i < LCS_PDSCH_COMB_N_STATUS; ++i) o->n_status[i] = st[i];
  o->reserved[0] = o->reserved[1] = o->reserved[2] = 0;
}
