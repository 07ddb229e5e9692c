// pdsch.h -- the PDSCH behind the format 1A grants of the PDCCH common search space: resource map, soft bits, turbo de-rate-matching
// and the turbo decoder (36.211 6.3, 6.4; 36.212 5.1.1, 5.1.3.2, 5.1.4.1; 36.213 7.1.7; lcs_pdsch_wide, lcs_pdsch, lcs_turbo_decode;
// the rule is stated in include/lcs.h: lcs_pdsch_info).  Host and device: the kernels (pdsch.hip: k_pdsch_plan, k_pdsch_llr,
// k_pdsch_dec, k_pdsch_fin) and the host twin (tests/host/pdsch_host.cpp) run the functions of this file, and the tables the kernels
// read are built on the host by its functions and from its tables (PDS_TBS, PDS_QPP, pds_rank_build, pds_x1_states).
//
// BOTH NUMBER TABLES OF THIS FILE (transport block sizes, QPP parameters) ARE WRITTEN FROM MEMORY OF THE STANDARD.  What pins them:
// every (f1, f2) gives a permutation, and every transport block size + 24 is a block size (tests/test_pdsch_ref.py).  A wrong entry
// shows as crc_ok = 0 on a real cell at that size only.
//
// THE ORDER OF EVERY SUM IS FIXED HERE.  The channel of port p at (l, k): pcfich.h's pcf_h_at on the two reference rows of the port
// that bracket symbol l inside the subframe, ha + (hb - ha) ((l - la) / (lb - la)); the nearest row's value outside them.  The symbol
// of an element: pcf_soft.  A circular-buffer position: 0 + its soft bits in ascending e.  A branch metric: 0.5 ((ls + la) su + lp sc);
// a forward metric: max over the two branches of alpha + g; a backward one: max of g + beta; a posterior: max over the input-0
// branches of alpha + (g + beta), minus the same over the input-1 branches; the extrinsic 0.75 ((L - ls) - la).  A maximum does not
// depend on the order it is taken in.  Plain fp64, -ffp-contract=off on both sides.
#pragma once
#include <math.h>
#include <vector>
#include "pdcch.h"

#define PDS_GRANTS 2                     // grants followed per subframe
#define PDS_WIN 32                       // steps of a trellis window
#define PDS_MAX_K 2240
#define PDS_MAX_D (PDS_MAX_K + 4)
#define PDS_MAX_WIN (PDS_MAX_K / PDS_WIN)
#define PDS_N_K 127                      // block sizes up to 2240
#define PDS_N_MCS 27
#define PDS_TABS (2 * PDS_N_MCS + LCS_PDSCH_MAX_FORCED)   // rank tables: [column][mcs], then one per forced grant
#define PDS_MAX_SYM 14
#define PDS_SCR_CHUNK 5                  // scrambling words a thread of k_pdsch_llr makes: 256 x 5 x 32 >= 2 x 12 x 100 x 14
#define PDS_SCR_WORDS (256 * PDS_SCR_CHUNK)
#define PDS_JUMP_WORDS (64 + 8 * 32)     // [32] to the reference sequence, [32] by 1600 clocks, [8][32] by 32 PDS_SCR_CHUNK 2^b clocks
static_assert(sizeof(lcs_pdsch_cfg) == 112 && sizeof(lcs_pdsch_block) == 336 && sizeof(lcs_pdsch_info) == 80 + LCS_PDSCH_MAX_BLOCKS * 336,
              "include/lcs.h: lcs_pdsch_info");
static_assert(2 * 12 * 100 * PDS_MAX_SYM <= 32 * PDS_SCR_WORDS, "the scrambling words cover the largest allocation");

// what the plan leaves per grant slot beside the public block; status LCS_PDSCH_FOLLOW: the soft-bit and decode kernels run it
struct PdsJob {
  int status, K, F, f1, f2, tab, G, N, base, max_iter, direct, c_init, row0, n_ctrl, k_lo, k_hi, sf, n_re, tdd, reserved;
};
#define LCS_PDSCH_FOLLOW (-1)
// PdsJob.reserved: how the grant's resource blocks are given
#define PDS_MODE_SET 1                   // by the grant slot's two sets (the side buffer), not by [k_lo, k_hi)
#define PDS_MODE_1C 2                    // a format 1C grant
#define PDS_MODE_GAP2 4                  // N_gap,2
#define PDS_MODE_UNREAD 8                // a distributed grant that the setting does not follow
#define PDS_N_1C 32                      // the transport block sizes of format 1C; their rank tables lie behind PDS_TABS
#define PDS_SET_RB 112                   // room of a slot's list of resource blocks
#define PDS_SET_WORDS 4                  // a grant slot's sets in the side buffer: [slot of the subframe][lo, hi] 64-bit masks of PRBs
struct PdsTabHead { int K, F, N, base[4]; };     // N non-nulls of the circular buffer, base[rv]: how many of them lie before k0(rv)
struct PdsGeom { int n_rb, ports, n_symb, id, sf, tdd, n_ctrl, k_lo, k_hi; };

// ------------------------------------------------------------------ block sizes and the interleaver
__host__ __device__ __forceinline__ int pds_k_at(int i) { return i < 60 ? 40 + 8 * i : i < 92 ? 512 + 16 * (i - 59) : i < 124 ? 1024 + 32 * (i - 91) : 2048 + 64 * (i - 123); }
// the index of the smallest block size >= B; -1 beyond 2240
__host__ __device__ __forceinline__ int pds_k_ceil_index(int B) {
  if (B > PDS_MAX_K) return -1;
  if (B <= 40) return 0;
  if (B <= 512) return (B - 40 + 7) / 8;
  if (B <= 1024) return 59 + (B - 512 + 15) / 16;
  if (B <= 2048) return 91 + (B - 1024 + 31) / 32;
  return 123 + (B - 2048 + 63) / 64;
}
__host__ __device__ __forceinline__ int pds_k_index(int K) { const int i = pds_k_ceil_index(K); return (i >= 0 && K >= 40 && pds_k_at(i) == K) ? i : -1; }
__host__ __device__ __forceinline__ int pds_qpp(int f1, int f2, int K, int i) {
  return (int)(((unsigned long long)f1 * (unsigned long long)i + (unsigned long long)f2 * (unsigned long long)i * (unsigned long long)i) % (unsigned long long)K);
}
__host__ __device__ __forceinline__ int pds_pad(int k) { return k + (k >> 5); }      // where step k lies in a stream in LDS: windows a bank apart
#define PDS_PAD_D (PDS_MAX_D + PDS_MAX_D / 32 + 2)

// ------------------------------------------------------------------ the grant
struct Pds1a { int flag, distributed, rb_start, n_prb, mcs, rv, tpc, ndi; };
// format 1A as it is sent with SI-, P- and RA-RNTI (36.212 5.3.3.1.3; capi.dci_1a_fields): bit t of `bits` = the t-th bit sent
__host__ __device__ __forceinline__ Pds1a pds_1a_fields(unsigned long long bits, int n_rb, int tdd) {
  int pos = 0;
  auto take = [&](int n) { int v = 0; for (int i = 0; i < n; ++i) v = (v << 1) | (int)((bits >> (pos + i)) & 1ull); pos += n; return v; };
  Pds1a f;
  f.flag = take(1); f.distributed = take(1);
  int nb = 0;
  while ((1 << nb) < n_rb * (n_rb + 1) / 2) nb += 1;
  const int riv = take(nb);
  int length = riv / n_rb + 1, start = riv % n_rb;
  if (length + start > n_rb) { length = n_rb - length + 2; start = n_rb - 1 - start; }
  f.rb_start = start; f.n_prb = length;
  f.mcs = take(5);
  take(tdd ? 4 : 3);
  f.ndi = take(1);
  f.rv = take(2);
  f.tpc = take(2);
  return f;
}

// ------------------------------------------------------------------ distributed allocations and format 1C (the rule: include/lcs.h,
// lcs_pdsch_alloc_cfg; 36.211 6.2.3.2, 36.212 5.3.3.1.4, 36.213 7.1.6.3 -- WRITTEN FROM MEMORY OF THE STANDARD.  What pins it:
// tests/test_pdsch_dvrb_host.py -- every slot's map is a permutation, a VRB's two PRBs lie N_gap apart, the 1C width is the PDCCH
// table's)
struct PdsDvrb { int n_gap, n_vrb, unit, n_row, n_null; };      // unit: the interleaving unit N~
// gap: 0 = N_gap,1; 1 = N_gap,2 (n_rb >= 50 only; n_vrb = 0 below that)
__host__ __device__ __forceinline__ PdsDvrb pds_dvrb(int n_rb, int gap) {
  PdsDvrb d;
  const int g1 = n_rb <= 10 ? (n_rb + 1) / 2 : n_rb == 11 ? 4 : n_rb <= 19 ? 8 : n_rb <= 26 ? 12 : n_rb <= 44 ? 18 : n_rb <= 63 ? 27 : n_rb <= 79 ? 32 : 48;
  const int g2 = n_rb < 50 ? 0 : n_rb <= 63 ? 9 : 16;
  const int P = n_rb <= 10 ? 1 : n_rb <= 26 ? 2 : n_rb <= 63 ? 3 : 4;
  if (gap == 0) { d.n_gap = g1; d.n_vrb = 2 * (g1 < n_rb - g1 ? g1 : n_rb - g1); d.unit = d.n_vrb; }
  else { d.n_gap = g2; d.n_vrb = g2 ? (n_rb / (2 * g2)) * 2 * g2 : 0; d.unit = 2 * g2; }
  d.n_row = d.unit ? ((d.unit + 4 * P - 1) / (4 * P)) * P : 0;
  d.n_null = 4 * d.n_row - d.unit;
  return d;
}
// the PRB of VRB v < n_vrb in a slot of parity `odd`
__host__ __device__ __forceinline__ int pds_dvrb_prb(const PdsDvrb &d, int v, int odd) {
  const int t = v % d.unit, o = d.unit * (v / d.unit);
  const int a = 2 * d.n_row * (t % 2) + t / 2, b = d.n_row * (t % 4) + t / 4;
  int r = b;
  if (d.n_null != 0) {
    if (t >= d.unit - d.n_null) r = (t % 2) ? a - d.n_row : a - d.n_row + d.n_null / 2;
    else if (t % 4 >= 2) r = b - d.n_null / 2;
  }
  if (odd) r = (r + d.unit / 2) % d.unit;
  return o + (r < d.unit / 2 ? r : r + d.n_gap - d.unit / 2);
}
struct Pds1c { int gap, riv, riv_ok, rb_start, n_prb, i_tbs, n_step; };
__host__ __device__ __forceinline__ int pds_1c_riv_bits(int n_rb) {
  const int v1 = pds_dvrb(n_rb, 0).n_vrb / (n_rb < 50 ? 2 : 4);
  int nb = 0;
  while ((1 << nb) < v1 * (v1 + 1) / 2) nb += 1;
  return nb;
}
// format 1C as it is sent (36.212 5.3.3.1.4): bit t of `bits` = the t-th bit sent
__host__ __device__ __forceinline__ Pds1c pds_1c_fields(unsigned long long bits, int n_rb) {
  int pos = 0;
  auto take = [&](int n) { int v = 0; for (int i = 0; i < n; ++i) v = (v << 1) | (int)((bits >> (pos + i)) & 1ull); pos += n; return v; };
  Pds1c f;
  f.gap = n_rb >= 50 ? take(1) : 0;
  f.n_step = n_rb < 50 ? 2 : 4;
  f.riv = take(pds_1c_riv_bits(n_rb));
  const int n = pds_dvrb(n_rb, f.gap).n_vrb / f.n_step;
  f.riv_ok = f.riv < n * (n + 1) / 2;
  int length = f.riv / n + 1, start = f.riv % n;
  if (length + start > n) { length = n - length + 2; start = n - 1 - start; }
  f.rb_start = f.n_step * start; f.n_prb = f.n_step * length;
  f.i_tbs = take(5);
  return f;
}
// the setting (lcs_pdsch_alloc_cfg resolved): flags bit 0 follows distributed 1A, bit 1 format 1C at size index i_1c
struct PdsAllocIn { int flags, sfn0, si_window, i_1c; };
// the redundancy version a 1C grant of `kind` in grid subframe g is assumed to have
__host__ __device__ __forceinline__ int pds_1c_rv(int kind, int g, const PdsAllocIn &a) {
  if (kind != 1 || a.sfn0 < 0) return 0;
  const int sfn = (a.sfn0 + g / 10) % 1024, sf = g % 10;
  int k;
  if (sf == 5 && sfn % 2 == 0) k = (sfn / 2) % 4;
  else if (a.si_window > 0 && a.si_window != 15) k = ((10 * sfn + sf) % a.si_window) % 4;
  else return 0;
  return ((3 * k + 1) / 2) % 4;
}
// the two sets of VRBs [v0, v0 + n) (inside n_vrb): m[2 slot], m[2 slot + 1] = PRBs 0 .. 63, 64 .. 127
__host__ __device__ __forceinline__ void pds_set_masks(const PdsDvrb &d, int v0, int n, unsigned long long (&m)[PDS_SET_WORDS]) {
  unsigned long long a0 = 0, a1 = 0, b0 = 0, b1 = 0;
  for (int v = v0; v < v0 + n; ++v) {
    const int p = pds_dvrb_prb(d, v, 0), q = pds_dvrb_prb(d, v, 1);
    if (p < 64) a0 |= 1ull << p; else a1 |= 1ull << (p - 64);
    if (q < 64) b0 |= 1ull << q; else b1 |= 1ull << (q - 64);
  }
  m[0] = a0; m[1] = a1; m[2] = b0; m[3] = b1;
}
__host__ __device__ __forceinline__ bool pds_set_has(unsigned long long lo, unsigned long long hi, int p) { return p < 64 ? (lo >> p) & 1ull : (hi >> (p - 64)) & 1ull; }
// cut[0]: the half blocks (six columns) of the set below the central 72 columns, cut[1]: those inside them
__host__ __device__ __forceinline__ void pds_set_cut(int n_rb, unsigned long long lo, unsigned long long hi, int *cut /*[2]*/) {
  int below = 0, inside = 0;
  for (int p = 0; p < n_rb; ++p) {
    if (!pds_set_has(lo, hi, p)) continue;
    for (int h = 2 * p; h < 2 * p + 2; ++h) { below += h < n_rb - 6; inside += h >= n_rb - 6 && h < n_rb + 6; }
  }
  cut[0] = below; cut[1] = inside;
}
// the set's resource blocks in ascending order -> prb[]; returns how many
__host__ __device__ __forceinline__ int pds_set_list(int n_rb, unsigned long long lo, unsigned long long hi, uint8_t *prb /*[PDS_SET_RB]*/) {
  int n = 0;
  for (int p = 0; p < n_rb; ++p) if (pds_set_has(lo, hi, p)) prb[n++] = (uint8_t)p;
  return n;
}

// ------------------------------------------------------------------ resource elements
// the reference elements that symbol l keeps free: columns = r (mod m); false: none
__host__ __device__ __forceinline__ bool pds_crs(const PdsGeom &q, int l, int *m, int *r) {
  const int ls = l % q.n_symb;
  const bool first = ls == 0, second = ls == q.n_symb - 3;
  if (!(first || second || (q.ports == 4 && ls == 1))) return false;
  if (q.ports == 1) { *m = 6; *r = ((second ? 3 : 0) + q.id) % 6; }
  else { *m = 3; *r = q.id % 3; }
  return true;
}
// is the central block of 72 columns left out in symbol l: PBCH, PSS, SSS
__host__ __device__ __forceinline__ bool pds_central(const PdsGeom &q, int l) {
  if (q.sf == 0 && l >= q.n_symb && l < q.n_symb + 4) return true;
  if (q.sf != 0 && q.sf != 5) return false;
  return q.tdd ? l == 2 * q.n_symb - 1 : (l == q.n_symb - 2 || l == q.n_symb - 1);
}
__host__ __device__ __forceinline__ int pds_res_below(int x, int m, int r) { return (x + m - 1 - r) / m; }      // columns < x that are = r (mod m)
// columns of [a, b) that symbol l's reference elements leave
__host__ __device__ __forceinline__ int pds_free(const PdsGeom &q, int l, int a, int b) {
  if (b <= a) return 0;
  int m, r;
  if (!pds_crs(q, l, &m, &r)) return b - a;
  return (b - a) - (pds_res_below(b, m, r) - pds_res_below(a, m, r));
}
// the elements of symbol l in columns [k_lo, k)
__host__ __device__ __forceinline__ int pds_count(const PdsGeom &q, int l, int k) {
  int n = pds_free(q, l, q.k_lo, k);
  if (pds_central(q, l)) {
    const int c0 = 6 * q.n_rb - 36, c1 = 6 * q.n_rb + 36;
    n -= pds_free(q, l, q.k_lo > c0 ? q.k_lo : c0, k < c1 ? k : c1);
  }
  return n;
}
// the column of the element of rank r in symbol l (r < pds_count(q, l, q.k_hi)): the lowest k with r + 1 elements in [k_lo, k]
__host__ __device__ __forceinline__ int pds_col_at(const PdsGeom &q, int l, int r) {
  int lo = q.k_lo, hi = q.k_hi - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (pds_count(q, l, mid + 1) >= r + 1) hi = mid; else lo = mid + 1;
  }
  return lo;
}
// base[l - n_ctrl]: elements before symbol l, l = n_ctrl .. 2 n_symb (the last entry is N_RE)
__host__ __device__ __forceinline__ int pds_bases(const PdsGeom &q, int *base /*[PDS_MAX_SYM + 1]*/) {
  int n = 0;
  for (int l = q.n_ctrl; l < 2 * q.n_symb; ++l) { base[l - q.n_ctrl] = n; n += pds_count(q, l, q.k_hi); }
  base[2 * q.n_symb - q.n_ctrl] = n;
  return n;
}
// element e -> (l, k)
__host__ __device__ __forceinline__ void pds_elem_at(const PdsGeom &q, const int *base, int e, int *l, int *k) {
  int i = 0;
  while (i + 1 < 2 * q.n_symb - q.n_ctrl && base[i + 1] <= e) i += 1;
  *l = q.n_ctrl + i;
  *k = pds_col_at(q, *l, e - base[i]);
}

// The same over a set of resource blocks per slot (q.k_lo, q.k_hi unused).  A half block of six columns lies whole inside or outside
// the central 72 columns (which cut a resource block in half when n_rb is odd) and keeps 6, 5 or 4 elements in every symbol, so a
// symbol holds that many times the slot's half blocks outside the cut.  cut [2][2]: pds_set_cut of slot 0, slot 1.
__host__ __device__ __forceinline__ int pds_set_per_half(const PdsGeom &q, int l) {
  int m, r;
  return pds_crs(q, l, &m, &r) ? 6 - 6 / m : 6;
}
__host__ __device__ __forceinline__ int pds_set_count(const PdsGeom &q, int n_prb, const int *cut, int l) {
  return pds_set_per_half(q, l) * (2 * n_prb - (pds_central(q, l) ? cut[2 * (l >= q.n_symb) + 1] : 0));
}
__host__ __device__ __forceinline__ int pds_set_bases(const PdsGeom &q, int n_prb, const int *cut, int *base /*[PDS_MAX_SYM + 1]*/) {
  int n = 0;
  for (int l = q.n_ctrl; l < 2 * q.n_symb; ++l) { base[l - q.n_ctrl] = n; n += pds_set_count(q, n_prb, cut, l); }
  base[2 * q.n_symb - q.n_ctrl] = n;
  return n;
}
// element e -> (l, k); prb [2][PDS_SET_RB]: pds_set_list of slot 0, slot 1
__host__ __device__ __forceinline__ void pds_set_elem_at(const PdsGeom &q, const uint8_t *prb, const int *cut, const int *base, int e, int *l, int *k) {
  int i = 0;
  while (i + 1 < 2 * q.n_symb - q.n_ctrl && base[i + 1] <= e) i += 1;
  const int ll = q.n_ctrl + i, si = ll >= q.n_symb, per = pds_set_per_half(q, ll), r = e - base[i];
  int h = r / per, j = r - h * per, m = 1, rr = -1;
  if (pds_central(q, ll) && h >= cut[2 * si]) h += cut[2 * si + 1];
  pds_crs(q, ll, &m, &rr);
  int col = 12 * (int)prb[PDS_SET_RB * si + (h >> 1)] + 6 * (h & 1);
  for (int c = 0; c < 6; ++c) {                // the j-th column of the half block that is no reference element
    const bool taken = rr >= 0 && (col % m) == rr;
    if (!taken && j == 0) break;
    if (!taken) j -= 1;
    col += 1;
  }
  *l = ll;
  *k = col;
}

// ------------------------------------------------------------------ channel and soft bits
// the six reference rows of a subframe: i < 4: symbols 0, n_symb - 3 of the two slots (ports 0, 1); 4, 5: symbol 1 of the two slots
__host__ __device__ __forceinline__ int pds_ref_sym(int i, int n_symb) { return i < 4 ? (i >> 1) * n_symb + (i & 1) * (n_symb - 3) : (i - 4) * n_symb + 1; }
// builds reference row i of subframe sf: its sequence and the shifts of its ports (shift6[i][port])
__host__ __device__ __forceinline__ void pds_ref_row(int i, int sf, int id, int cp_type, int n_symb, int n_rb, const uint32_t *__restrict__ jump,
                                                     uint32_t *bits, double *shift4) {
  const int slot = 2 * sf + (i < 4 ? (i >> 1) : (i - 4)), t = i < 4 ? ((i & 1) ? 2 : 0) : 1;
  rs_dl_row_wide(slot, t, id, cp_type, n_symb, n_rb, jump, bits, shift4);
}
// h of `port` at symbol l, column k.  sfrow: the subframe's symbol 0 in the grid, rows 12 n_rb (re, im) pairs apart
__host__ __device__ __forceinline__ cd2 pds_h(int port, int l, int k, int n_rb, int n_symb, const double *__restrict__ sfrow,
                                              const uint32_t (*bits)[RS_DL_WIDE_WORDS], const double (*shift)[4]) {
  const int i0 = port < 2 ? 0 : 4, n = port < 2 ? 4 : 2;
  int ia = 0, ib = n - 1;
  for (int i = 0; i < n; ++i) if (pds_ref_sym(i0 + i, n_symb) <= l) ia = i;
  for (int i = n - 1; i >= 0; --i) if (pds_ref_sym(i0 + i, n_symb) >= l) ib = i;
  if (ib < ia) ib = ia;                      // (cannot be: kept for the reader)
  const size_t stride = (size_t)24 * n_rb;
  const int la = pds_ref_sym(i0 + ia, n_symb), lb = pds_ref_sym(i0 + ib, n_symb);
  const cd2 ha = pcf_h_at(sfrow + stride * la, bits[i0 + ia], (int)shift[i0 + ia][port], k, n_rb);
  if (la == lb || l <= la) return ha;
  const cd2 hb = pcf_h_at(sfrow + stride * lb, bits[i0 + ib], (int)shift[i0 + ib][port], k, n_rb);
  if (l >= lb) return hb;
  const double t = (double)(l - la) / (double)(lb - la);
  return mk(ha.re + (hb.re - ha.re) * t, ha.im + (hb.im - ha.im) * t);
}
// what element e at (l, k) brings by itself (as pcf_elem)
__host__ __device__ __forceinline__ void pds_elem(int e, int l, int k, int n_rb, int ports, int n_symb, const double *__restrict__ sfrow,
                                                  const uint32_t (*bits)[RS_DL_WIDE_WORDS], const double (*shift)[4], cd2 *y, cd2 *ha, cd2 *hb) {
  int a, b;
  pcf_pair_ports(e, ports, &a, &b);
  const double *row = sfrow + (size_t)24 * n_rb * l;
  *y = mk(row[2 * k], row[2 * k + 1]);
  *ha = pds_h(a, l, k, n_rb, n_symb, sfrow, bits, shift);
  *hb = mk(0.0, 0.0);
  if (b >= 0) *hb = pds_h(b, l, k, n_rb, n_symb, sfrow, bits, shift);
}
// the Gold sequence's second register n clocks on: jump = the jump-ahead table for n clocks (its first 31 words)
__host__ __device__ __forceinline__ uint32_t pds_x2_jump(uint32_t x2, const uint32_t *__restrict__ jump) {
  uint32_t v = 0;
  for (int b = 0; b < 31; ++b) if ((x2 >> b) & 1u) v ^= jump[b];
  return v;
}
__host__ __device__ __forceinline__ uint32_t pds_c_init(int rnti, int sf, int id) { return (uint32_t)rnti * 16384u + (uint32_t)sf * 512u + (uint32_t)id; }
// PDS_SCR_CHUNK words of the scrambling sequence from the two registers as they stand before the chunk's first bit
__host__ __device__ __forceinline__ void pds_scr_chunk(uint32_t x1, uint32_t x2, uint32_t *words) {
  for (int w = 0; w < PDS_SCR_CHUNK; ++w) {
    uint32_t word = 0;
    for (int i = 0; i < 32; ++i) {
      word |= ((x1 ^ x2) & 1u) << i;
      const uint32_t n1 = ((x1 >> 3) ^ x1) & 1u;
      const uint32_t n2 = ((x2 >> 3) ^ (x2 >> 2) ^ (x2 >> 1) ^ x2) & 1u;
      x1 = (x1 >> 1) | (n1 << 30);
      x2 = (x2 >> 1) | (n2 << 30);
    }
    words[w] = word;
  }
}

// ------------------------------------------------------------------ the decoder
// state s = 4 r1 + 2 r2 + r3 of the register (r1 the newest); input u: a = u ^ r2 ^ r3 is fed back, z = a ^ r1 ^ r3 is the parity
__host__ __device__ __forceinline__ constexpr int pds_next(int s, int u) { return (((u ^ (s >> 1) ^ s) & 1) << 2) | (s >> 1); }
__host__ __device__ __forceinline__ constexpr int pds_parity(int s, int u) { return (u ^ (s >> 1) ^ s ^ (s >> 2) ^ s) & 1; }
__host__ __device__ __forceinline__ double pds_max(double a, double b) { return b > a ? b : a; }
__host__ __device__ __forceinline__ void pds_gamma(double ls, double la, double lp, double (&g)[4] /*[2 u + c]*/) {
  const double x = ls + la;
  g[0] = 0.5 * (x + lp); g[1] = 0.5 * (x - lp); g[2] = 0.5 * (-x + lp); g[3] = 0.5 * (-x - lp);
}
// the backward metrics at step K from the three tail steps, run back from state 0: x[t], z[t] the tail's systematic and parity values
__host__ __device__ __forceinline__ void pds_tail_beta(const double *x, const double *z, double (&b)[8]) {
#pragma unroll
  for (int s = 0; s < 8; ++s) b[s] = s == 0 ? 0.0 : -INFINITY;
#pragma unroll
  for (int t = 2; t >= 0; --t) {
    double n[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int u = ((s >> 1) ^ s) & 1, zz = ((s >> 2) ^ s) & 1;            // the input that feeds back 0, and its parity
      n[s] = 0.5 * ((u ? -x[t] : x[t]) + (zz ? -z[t] : z[t])) + b[s >> 1];
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) b[s] = n[s];
  }
}
// One window of one constituent decoder: steps k0 .. k0 + n - 1.  sys / ext are indexed by pds_pad(j), j = perm ? perm[k] : k (the
// second decoder reads and writes its systematic values and extrinsics through the interleaver); par by pds_pad(k).  a: the forward
// metrics at step k0 in, at step k0 + n out; b: the backward metrics at step k0 + n in, at step k0 out.  ws: room for the window's
// forward metrics, entry (8 t + s) stride apart.  hard (the second decoder only): the decision of bit j.  A step with j < F admits
// only input-0 branches and leaves its extrinsic and decision alone.
__host__ __device__ __forceinline__ void pds_window(const double *sys, const double *par, double *ext, const uint16_t *perm, uint8_t *hard, int F,
                                                    int k0, int n, double (&a)[8], double (&b)[8], double *ws, size_t stride) {
#pragma unroll 1
  for (int t = 0; t < n; ++t) {
    const int k = k0 + t, j = perm ? (int)perm[k] : k;
#pragma unroll
    for (int s = 0; s < 8; ++s) ws[(size_t)(8 * t + s) * stride] = a[s];
    double g[4];
    pds_gamma(sys[pds_pad(j)], ext[pds_pad(j)], par[pds_pad(k)], g);
    const bool filler = j < F;
    double nx[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) nx[s] = -INFINITY;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      nx[pds_next(s, 0)] = pds_max(nx[pds_next(s, 0)], a[s] + g[pds_parity(s, 0)]);
      if (!filler) nx[pds_next(s, 1)] = pds_max(nx[pds_next(s, 1)], a[s] + g[2 + pds_parity(s, 1)]);
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) a[s] = nx[s];
  }
  double bb[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) bb[s] = b[s];
#pragma unroll 1
  for (int t = n - 1; t >= 0; --t) {
    const int k = k0 + t, j = perm ? (int)perm[k] : k;
    const double ls = sys[pds_pad(j)], la = ext[pds_pad(j)];
    double g[4];
    pds_gamma(ls, la, par[pds_pad(k)], g);
    const bool filler = j < F;
    double m0 = -INFINITY, m1 = -INFINITY, nb[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const double al = ws[(size_t)(8 * t + s) * stride];
      const double t0 = g[pds_parity(s, 0)] + bb[pds_next(s, 0)], t1 = g[2 + pds_parity(s, 1)] + bb[pds_next(s, 1)];
      nb[s] = filler ? t0 : pds_max(t0, t1);
      m0 = pds_max(m0, al + t0);
      m1 = pds_max(m1, al + t1);
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) bb[s] = nb[s];
    if (!filler) {
      const double L = m0 - m1;
      ext[pds_pad(j)] = 0.75 * ((L - ls) - la);
      if (hard) hard[j] = L < 0.0 ? 1 : 0;
    }
  }
#pragma unroll
  for (int s = 0; s < 8; ++s) b[s] = bb[s];
}
// CRC24A (0x864CFB, zero initial state) of bits 0 .. K - 1, bit k = bit k & 31 of word k >> 5; the caller keeps the filler bits zero,
// which a zero initial state does not see
__host__ __device__ __forceinline__ uint32_t pds_crc24a(const uint32_t *words, int K) {
  uint32_t crc = 0;
  for (int k = 0; k < K; ++k) {
    const uint32_t msb = ((crc >> 23) & 1u) ^ ((words[k >> 5] >> (k & 31)) & 1u);
    crc = (crc << 1) & 0xffffffu;
    if (msb) crc ^= 0x864cfbu;
  }
  return crc;
}
// byte t of the transport block from the decisions: bits F + 8 t .. F + 8 t + 7, MSB first, zeros beyond tbs
__host__ __device__ __forceinline__ uint8_t pds_payload_byte(const uint8_t *hard, int F, int tbs, int t) {
  unsigned v = 0;
  for (int i = 0; i < 8; ++i) v = (v << 1) | ((8 * t + i < tbs) ? (unsigned)(hard[F + 8 * t + i] & 1) : 0u);
  return (uint8_t)v;
}

// ------------------------------------------------------------------ the plan of one subframe
struct PdsPlanIn {
  int n_rb, ports, n_symb, id, tdd, i_1a, rnti_mask, max_iter, n_forced;
  lcs_pdsch_grant forced[LCS_PDSCH_MAX_FORCED];
};
__host__ __device__ __forceinline__ void pds_block_zero(lcs_pdsch_block *b) {
  b->subframe = b->slot = b->rnti = b->kind = b->rb_start = b->n_prb = b->mcs = b->rv = b->tbs = b->n_re = b->K = b->F = b->n_iter = b->status = 0;
  for (int i = 0; i < LCS_PDSCH_PAYLOAD; ++i) b->payload[i] = 0;
}
// the grant's geometry, sizes and job once its fields stand in *b (rb_start, n_prb, rv, tbs, rnti); tab: its rank table.  mode: PDS_MODE_*;
// with PDS_MODE_SET rb_start and n_prb are VRBs and set [PDS_SET_WORDS] takes the two sets of PRBs.  ALLOC = false: the instantiation of
// the stage without the setting, in which nothing of the set-based geometry is compiled
template <bool ALLOC>
__host__ __device__ inline void pds_plan_grant(const PdsPlanIn &in, int g, int row0, int cfi, int tab, const int *__restrict__ qpp /*[127][2]*/,
                                               const PdsTabHead *__restrict__ heads, lcs_pdsch_block *b, PdsJob *j, int mode = 0,
                                               unsigned long long *set = nullptr) {
  const int sf = g % 10;
  j->status = 0; j->direct = 0; j->tdd = in.tdd; j->reserved = mode; j->tab = tab; j->max_iter = in.max_iter; j->sf = sf; j->row0 = row0;
  j->K = j->F = j->f1 = j->f2 = j->G = j->N = j->base = j->n_re = j->n_ctrl = j->k_lo = j->k_hi = 0; j->c_init = 0;
  if (b->status) { j->status = b->status; return; }
  const int n_limit = (ALLOC && (mode & PDS_MODE_SET)) ? pds_dvrb(in.n_rb, (mode & PDS_MODE_GAP2) ? 1 : 0).n_vrb : in.n_rb;
  if (b->rb_start < 0 || b->n_prb < 1 || b->rb_start + b->n_prb > n_limit) b->status = LCS_PDSCH_BAD_ALLOC;
  else if (in.tdd && (sf == 1 || sf == 6)) b->status = LCS_PDSCH_SPECIAL;
  else if (row0 < 0) b->status = LCS_PDSCH_ROWS;
  else if (cfi < 1 || cfi > 3) b->status = LCS_PDSCH_NO_CFI;
  const int ki = pds_k_ceil_index(b->tbs + 24);
  if (!b->status && (b->tbs < 1 || ki < 0)) b->status = LCS_PDSCH_BAD_ALLOC;
  if (b->status) { j->status = b->status; return; }
  PdsGeom q;
  q.n_rb = in.n_rb; q.ports = in.ports; q.n_symb = in.n_symb; q.id = in.id; q.sf = sf; q.tdd = in.tdd;
  q.n_ctrl = pdc_n_ctrl(cfi, in.n_rb); q.k_lo = 12 * b->rb_start; q.k_hi = 12 * (b->rb_start + b->n_prb);
  int base[PDS_MAX_SYM + 1];
  if (ALLOC && (mode & PDS_MODE_SET)) {
    unsigned long long m[PDS_SET_WORDS];
    int cut[4];
    pds_set_masks(pds_dvrb(in.n_rb, (mode & PDS_MODE_GAP2) ? 1 : 0), b->rb_start, b->n_prb, m);
    pds_set_cut(in.n_rb, m[0], m[1], cut);
    pds_set_cut(in.n_rb, m[2], m[3], cut + 2);
    for (int i = 0; i < PDS_SET_WORDS; ++i) set[i] = m[i];
    b->n_re = pds_set_bases(q, b->n_prb, cut, base);
    q.k_lo = q.k_hi = 0;
  } else b->n_re = pds_bases(q, base);
  b->K = pds_k_at(ki); b->F = b->K - (b->tbs + 24);
  j->status = LCS_PDSCH_FOLLOW;
  j->K = b->K; j->F = b->F; j->f1 = qpp[2 * ki]; j->f2 = qpp[2 * ki + 1];
  j->G = 2 * b->n_re; j->N = heads[tab].N; j->base = heads[tab].base[b->rv & 3];
  j->c_init = (int)pds_c_init(b->rnti, sf, in.id);
  j->n_ctrl = q.n_ctrl; j->k_lo = q.k_lo; j->k_hi = q.k_hi; j->n_re = b->n_re;
}
// the PDS_GRANTS grant slots of grid subframe g: from the forced list, or from the accepted entries of the PDCCH record -- format 1A
// at size index i_1a and, where the setting follows it, format 1C at i_1c; by ascending candidate slot, then size index.
// row0: the grid row of the subframe's symbol 0 when every row of the subframe is there, else -1.  tbs_tab [2][27]; tbs_1c [32] and
// sets [PDS_GRANTS][PDS_SET_WORDS] are read and written with a non-zero setting only.  ALLOC = false (al.flags = 0): format 1A's size alone is walked
template <bool ALLOC>
__host__ __device__ inline void pds_plan_sf_alloc(const PdsPlanIn &in, const PdsAllocIn &al, int g, int row0, const lcs_pdcch_info *__restrict__ pdc,
                                                  const int *__restrict__ tbs_tab, const int *__restrict__ tbs_1c, const int *__restrict__ qpp,
                                                  const PdsTabHead *__restrict__ heads, lcs_pdsch_block *blk /*[2]*/, PdsJob *job /*[2]*/, unsigned long long *sets) {
  int n = 0;
  const int cfi = pdc->cfi[g];
  for (int u = 0; u < PDS_GRANTS; ++u) pds_block_zero(&blk[u]);
  if (ALLOC && al.flags)
    for (int i = 0; i < PDS_GRANTS * PDS_SET_WORDS; ++i) sets[i] = 0ull;
  if (in.n_forced > 0) {
    for (int f = 0; f < in.n_forced && n < PDS_GRANTS; ++f) {
      const lcs_pdsch_grant &fg = in.forced[f];
      if (fg.subframe != g) continue;
      lcs_pdsch_block *b = &blk[n];
      b->subframe = g; b->slot = f; b->rnti = fg.rnti; b->kind = pdc_kind((uint32_t)fg.rnti); b->rb_start = fg.rb_start; b->n_prb = fg.n_prb;
      b->mcs = -1; b->rv = fg.rv & 3; b->tbs = fg.tbs;
      pds_plan_grant<ALLOC>(in, g, row0, cfi, 2 * PDS_N_MCS + f, qpp, heads, b, &job[n]);
      n += 1;
    }
  } else if (cfi) {
    unsigned long long seen_bits[PDS_GRANTS];
    uint32_t seen_rnti[PDS_GRANTS];
    int seen_size[PDS_GRANTS];
    for (int s = 0; s < PDC_SLOTS && n < PDS_GRANTS; ++s) {
      for (int i = ALLOC ? 0 : in.i_1a; i < (ALLOC ? PDC_SIZES : in.i_1a + 1) && n < PDS_GRANTS; ++i) {
        const bool is_1c = ALLOC && (al.flags & 2) && i == al.i_1c;
        if (i != in.i_1a && !is_1c) continue;
        const lcs_pdcch_dec &d = pdc->dec[g][s][i];
        if (!(d.flags & 2) || (!is_1c && !(d.bits & 1ull)) || !(pdc_kind(d.rnti_x) & in.rnti_mask)) continue;
        bool dup = false;
        for (int u = 0; u < n; ++u) dup = dup || (seen_bits[u] == d.bits && seen_rnti[u] == d.rnti_x && seen_size[u] == i);
        if (dup) continue;
        seen_bits[n] = d.bits; seen_rnti[n] = d.rnti_x; seen_size[n] = i;
        lcs_pdsch_block *b = &blk[n];
        b->subframe = g; b->slot = s; b->rnti = (int)d.rnti_x; b->kind = pdc_kind(d.rnti_x);
        int tab = 0, mode = 0;
        if (is_1c) {
          const Pds1c f = pds_1c_fields(d.bits, in.n_rb);
          b->rb_start = f.rb_start; b->n_prb = f.n_prb; b->mcs = f.i_tbs; b->rv = pds_1c_rv(b->kind, g, al);
          mode = PDS_MODE_SET | PDS_MODE_1C | (f.gap ? PDS_MODE_GAP2 : 0);
          if (!f.riv_ok) b->status = LCS_PDSCH_BAD_ALLOC;
          else b->tbs = tbs_1c[f.i_tbs];
          tab = PDS_TABS + f.i_tbs;
        } else {
          const Pds1a f = pds_1a_fields(d.bits, in.n_rb, in.tdd);
          b->rb_start = f.rb_start; b->n_prb = f.n_prb; b->mcs = f.mcs; b->rv = f.rv;
          if (f.distributed) mode = (ALLOC && (al.flags & 1)) ? PDS_MODE_SET | ((in.n_rb >= 50 && f.ndi) ? PDS_MODE_GAP2 : 0) : PDS_MODE_UNREAD;
          if (mode == PDS_MODE_UNREAD) b->status = LCS_PDSCH_DISTRIBUTED;
          else if (f.mcs > 26) b->status = LCS_PDSCH_MCS;
          else b->tbs = tbs_tab[PDS_N_MCS * (f.tpc & 1) + f.mcs];
          tab = PDS_N_MCS * (f.tpc & 1) + (f.mcs <= 26 ? f.mcs : 0);
        }
        pds_plan_grant<ALLOC>(in, g, row0, cfi, tab, qpp, heads, b, &job[n], mode, (ALLOC && al.flags) ? sets + PDS_SET_WORDS * n : nullptr);
        n += 1;
      }
    }
  }
  for (int u = n; u < PDS_GRANTS; ++u) { PdsJob z = {}; job[u] = z; }
}
// the same with the setting off: format 1A's localized grants alone
__host__ __device__ inline void pds_plan_sf(const PdsPlanIn &in, int g, int row0, const lcs_pdcch_info *__restrict__ pdc, const int *__restrict__ tbs_tab,
                                            const int *__restrict__ qpp, const PdsTabHead *__restrict__ heads, lcs_pdsch_block *blk /*[2]*/, PdsJob *job /*[2]*/) {
  const PdsAllocIn off = {0, -1, 0, 0};
  pds_plan_sf_alloc<false>(in, off, g, row0, pdc, tbs_tab, nullptr, qpp, heads, blk, job, nullptr);
}
// what lcs_pdsch_last_alloc says of a listed block: from its public fields and its job's mode
__host__ __device__ inline void pds_alloc_of(int n_rb, const lcs_pdsch_block &b, int mode, lcs_pdsch_alloc *o) {
  const bool set = (mode & PDS_MODE_SET) != 0;
  const PdsDvrb dv = pds_dvrb(n_rb, (mode & PDS_MODE_GAP2) ? 1 : 0);
  o->format = (mode & PDS_MODE_1C) ? 1 : 0; o->distributed = (set || (mode & PDS_MODE_UNREAD)) ? 1 : 0; o->gap = (mode & PDS_MODE_GAP2) ? 1 : 0;
  o->n_gap = o->distributed ? dv.n_gap : 0; o->n_vrb = o->distributed ? dv.n_vrb : n_rb; o->n_step = (mode & PDS_MODE_1C) ? (n_rb < 50 ? 2 : 4) : 1;
  o->reserved = 0;
  const bool inside = !(mode & PDS_MODE_UNREAD) && b.rb_start >= 0 && b.n_prb >= 1 && b.rb_start + b.n_prb <= o->n_vrb;
  o->n_prb = inside ? b.n_prb : 0;
  for (int s = 0; s < 2; ++s)
    for (int i = 0; i < LCS_PDSCH_ALLOC_RB; ++i) o->prb[s][i] = (uint8_t)(i >= o->n_prb ? 0 : set ? pds_dvrb_prb(dv, b.rb_start + i, s) : b.rb_start + i);
}
// the head of the record from its blocks, in order
__host__ __device__ inline void pds_summary(lcs_pdsch_info *o, int n_sf, int n_blocks, int n_overflow, int dl_mask, int n_rb, int ports) {
  int k[3] = {0, 0, 0}, st[LCS_PDSCH_N_STATUS];
  for (int i = 0; i < LCS_PDSCH_N_STATUS; ++i) st[i] = 0;
  for (int i = 0; i < n_blocks; ++i) {
    const lcs_pdsch_block &b = o->block[i];
    if (b.kind == 1) k[0] += 1; else if (b.kind == 2) k[1] += 1; else if (b.kind == 4) k[2] += 1;
    if (b.status >= 0 && b.status < LCS_PDSCH_N_STATUS) st[b.status] += 1;
  }
  o->n_sf = n_sf; o->n_blocks = n_blocks; o->n_ok = st[LCS_PDSCH_OK]; o->n_si = k[0]; o->n_paging = k[1]; o->n_ra = k[2];
  o->n_overflow = n_overflow; o->dl_mask = dl_mask; o->n_rb = n_rb; o->n_ports = ports;
  for (int i = 0; i < LCS_PDSCH_N_STATUS; ++i) o->n_status[i] = st[i];
}

// ------------------------------------------------------------------ the tables (host)
// 36.213 table 7.1.7.2.1-1, columns N_PRB = 2 and 3, I_TBS = 0 .. 26 (from memory: see the head of this file)
// 36.213 table 7.1.7.2.3-1: the transport block sizes of format 1C by I_TBS (from memory; every entry + 24 is a turbo block size)
static const int PDS_TBS_1C[PDS_N_1C] = {40, 56, 72, 120, 136, 144, 176, 208, 224, 256, 280, 296, 328, 336, 392, 488, 552, 600, 632, 696, 776, 840, 904, 1000, 1064, 1128,
                                         1224, 1288, 1384, 1480, 1608, 1736};
static const int PDS_TBS[2][PDS_N_MCS] = {
    {32, 56, 72, 104, 120, 144, 176, 208, 256, 296, 328, 376, 440, 488, 552, 600, 632, 696, 776, 840, 904, 1000, 1064, 1128, 1192, 1256, 1480},
    {56, 88, 144, 176, 208, 224, 256, 328, 392, 456, 504, 584, 680, 744, 840, 904, 968, 1064, 1160, 1288, 1384, 1480, 1608, 1736, 1800, 1864, 2216}};
// 36.212 table 5.1.3-3, (f1, f2) of the 127 block sizes up to 2240 in ascending size (from memory: see the head of this file)
static const int PDS_QPP[PDS_N_K][2] = {
    {3, 10}, {7, 12}, {19, 42}, {7, 16}, {7, 18}, {11, 20}, {5, 22}, {11, 24}, {7, 26}, {41, 84}, {103, 90}, {15, 32}, {9, 34}, {17, 108}, {9, 38}, {21, 120},
    {101, 84}, {21, 44}, {57, 46}, {23, 48}, {13, 50}, {27, 52}, {11, 36}, {27, 56}, {85, 58}, {29, 60}, {33, 62}, {15, 32}, {17, 198}, {33, 68}, {103, 210},
    {19, 36}, {19, 74}, {37, 76}, {19, 78}, {21, 120}, {21, 82}, {115, 84}, {193, 86}, {21, 44}, {133, 90}, {81, 46}, {45, 94}, {23, 48}, {243, 98}, {151, 40},
    {155, 102}, {25, 52}, {51, 106}, {47, 72}, {91, 110}, {29, 168}, {29, 114}, {247, 58}, {29, 118}, {89, 180}, {91, 122}, {157, 62}, {55, 84}, {31, 64},
    {17, 66}, {35, 68}, {227, 420}, {65, 96}, {19, 74}, {37, 76}, {41, 234}, {39, 80}, {185, 82}, {43, 252}, {21, 86}, {155, 44}, {79, 120}, {139, 92},
    {23, 94}, {217, 48}, {25, 98}, {17, 80}, {127, 102}, {25, 52}, {239, 106}, {17, 48}, {137, 110}, {215, 112}, {29, 114}, {15, 58}, {147, 118}, {29, 60},
    {59, 122}, {65, 124}, {55, 84}, {31, 64},
    {17, 66}, {171, 204}, {67, 140}, {35, 72}, {19, 74}, {39, 76}, {19, 78}, {199, 240}, {21, 82}, {211, 252}, {21, 86}, {43, 88}, {149, 60}, {45, 92},
    {49, 846}, {71, 48}, {13, 28}, {17, 80}, {25, 102}, {183, 104}, {55, 954}, {127, 96}, {27, 110}, {29, 112}, {29, 114}, {57, 116}, {45, 354}, {31, 120},
    {59, 610}, {185, 124}, {113, 420}, {31, 64},
    {17, 66}, {171, 136}, {209, 420}};
// the sub-block interleaver's column permutation (36.212 table 5.1.4-1: the turbo code's)
static const int PDS_PERM[32] = {0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30, 1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31};
// where value k of stream s (d0, d1, d2; D = K + 4 of them) lies in the circular buffer w of 3 K_PI positions
inline int pds_w_pos(int s, int k, int D) {
  const int R = (D + 31) / 32, KP = 32 * R, ND = KP - D;
  int inv[32];
  for (int c = 0; c < 32; ++c) inv[PDS_PERM[c]] = c;
  const int y = ND + k;
  if (s < 2) {
    const int v = inv[y % 32] * R + y / 32;
    return s == 0 ? v : KP + 2 * v;
  }
  const int m = (y - 1 + KP) % KP;           // pi(kk) = (P(kk / R) + 32 (kk mod R) + 1) mod K_PI = y
  return KP + 2 * (inv[m % 32] * R + m / 32) + 1;
}
inline int pds_k0(int D, int rv) { const int R = (D + 31) / 32, Kw = 96 * R; return R * (2 * ((Kw + 8 * R - 1) / (8 * R)) * rv + 2); }
// rank[s PDS_MAX_D + k]: how many non-nulls of the circular buffer lie before the position of value k of stream s, -1 for a null (a
// filler of d0 or d1); head: N and, per rv, how many lie before k0.  The position of rank r counted from k0 takes the soft bits
// e = r, r + N, r + 2 N, ..
inline void pds_rank_build(int K, int F, PdsTabHead *head, int16_t *rank /*[3][PDS_MAX_D]*/) {
  const int D = K + 4, R = (D + 31) / 32, Kw = 96 * R;
  std::vector<int> owner((size_t)Kw, -1);
  for (int i = 0; i < 3 * PDS_MAX_D; ++i) rank[i] = -1;
  for (int s = 0; s < 3; ++s)
    for (int k = 0; k < D; ++k)
      if (!(s < 2 && k < F)) owner[(size_t)pds_w_pos(s, k, D)] = s * PDS_MAX_D + k;
  std::vector<int> before((size_t)Kw + 1, 0);
  int n = 0;
  for (int j = 0; j < Kw; ++j) {
    before[(size_t)j] = n;
    if (owner[(size_t)j] >= 0) rank[owner[(size_t)j]] = (int16_t)n++;
  }
  before[(size_t)Kw] = n;
  head->K = K; head->F = F; head->N = n;
  for (int rv = 0; rv < 4; ++rv) head->base[rv] = before[(size_t)(pds_k0(D, rv) % Kw)];
}
// the first register of the Gold sequence 1600 + 32 PDS_SCR_CHUNK j clocks on, j < 256
inline void pds_x1_states(uint32_t *out /*[256]*/) {
  uint32_t x1 = 1u;
  for (int i = 0; i < 1600 + 32 * PDS_SCR_CHUNK * 256; ++i) {
    if (i >= 1600 && (i - 1600) % (32 * PDS_SCR_CHUNK) == 0) out[(i - 1600) / (32 * PDS_SCR_CHUNK)] = x1;
    x1 = (x1 >> 1) | ((((x1 >> 3) ^ x1) & 1u) << 30);
  }
}
// value k of stream s from the G soft bits e of a block
__host__ __device__ __forceinline__ double pds_derm_value(const double *__restrict__ llr, int G, int N, int base, int r0) {
  if (r0 < 0) return 0.0;
  int r = r0 - base;
  if (r < 0) r += N;
  double v = 0.0;
  for (int e = r; e < G; e += N) v = v + llr[e];
  return v;
}
