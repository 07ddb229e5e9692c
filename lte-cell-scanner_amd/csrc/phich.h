// phich.h -- the HARQ indicators of every downlink subframe of a full-bandwidth grid (36.211 6.9, 36.212 5.3.5; lcs_phich_wide,
// lcs_phich, lcs_phich_values; the rule is stated in include/lcs.h: lcs_phich_info).  Host and device: the kernels (phich.hip: k_phich,
// k_phich_fin) and the host twin (tests/host/phich_host.cpp) run the functions of this file, and the unit table the kernel reads is
// built on the host by phi_build_map from the PDCCH stage's own REG list (pdc_build_map_t: the REG rule is not restated here).
//
// TABLES.  A PhiMap is made for (n_rb, ports, CP, n_id_cell, PHICH duration and Ng) and every m_i: re[12 u + 4 i + j] is the resource
// element (l << 16 | k) of element j of quadruplet i of mapping unit u < n_unit; n_unit = -1 for a map that the rule refuses (the
// units do not fit their symbol), 0 for m_i = 0.
//
// LANES.  A unit has 12 lanes, lane e = 4 i + j; five units share a wave (lanes 60 .. 63 idle), so the partners of a pair (e ^ 1) and
// of a quadruplet (e ^ 2) are xor-neighbours.  THE ORDER OF EVERY SUM IS FIXED HERE.  A lane's symbol is pcfich.h's (pcf_h_at,
// pcf_soft) with the ports of phi_elem; its gain G = (|ha|^2) + (|hb of the pair's other lane|^2).  The butterfly (phi_bfly_*): stage
// 1, lane j holds t_j + t_(j^1) for even j and t_(j^1) - t_j for odd j; stage 2 (normal CP only), a_j + a_(j^2) for j < 2 and
// a_(j^2) - a_j above: lane j then holds the despread value of Walsh code j, and of the pair's code j & 1 with the extended CP.  The
// gains go through the same stages with + only.  phi_final adds the repetitions 0, 1, 2 in that order.  The subframe's noise:
// lane i < 64 adds S[i], S[i + 64], .. of the entries with a d sum above zero (0 + them in that order), then cell_meas.h's
// butterfly over the 64 lanes.  Plain fp64, -ffp-contract=off on both sides.
#pragma once
#include <math.h>
#include <vector>
#include "pdcch.h"

#define PHI_MAX_UNIT 50                  // 25 units x m_i 2
#define PHI_UNIT_RE 12
#define PHI_WAVE_UNITS 5                 // units of a wave: 60 of its 64 lanes
#define PHI_MAX_ENT LCS_PHICH_MAX_ENTRIES
#define PHI_ENT_PASSES ((PHI_MAX_ENT + 63) / 64)
#define PHI_MAX_HI LCS_PHICH_MAX_HI
static_assert(sizeof(lcs_phich_cfg) == 72 && sizeof(lcs_phich_sf) == 32 && sizeof(lcs_phich_hi) == 24 &&
              sizeof(lcs_phich_info) == 48 + PCF_MAX_SF * 32 + PHI_MAX_HI * 24, "include/lcs.h: lcs_phich_info");
static_assert(PHI_MAX_ENT == 8 * PHI_MAX_UNIT && LCS_PHICH_MAX_GROUP == 2 * PHI_MAX_UNIT, "include/lcs.h: the PHICH's limits");

struct PhiMap { int n_unit; int re[PHI_MAX_UNIT * PHI_UNIT_RE]; };
// one entry of the subframe's table, as k_phich leaves it for k_phich_fin
struct PhiEntry { double value, dsum, S; };

__host__ __device__ __forceinline__ int phi_n_seq(int cp_type) { return cp_type == LCS_CP_NORMAL ? 8 : 4; }
__host__ __device__ __forceinline__ int phi_n_group(int cp_type, int n_unit) { return n_unit <= 0 ? 0 : cp_type == LCS_CP_NORMAL ? n_unit : 2 * n_unit; }
// rows a subframe needs inside the grid, from its symbol 0 on
__host__ __device__ __forceinline__ int phi_rows_needed(int ports, int phich_duration) { return phich_duration == 2 ? 3 : ports == 4 ? 2 : 1; }
// is grid subframe g read, the map apart
__host__ __device__ __forceinline__ bool phi_sf_used(int g, int n_ofdm, int n_symb, int ports, int phich_duration, bool tdd, int dl_mask) {
  const int r0 = 2 * g * n_symb, sf = g % 10;
  if (!((dl_mask >> sf) & 1) || r0 + phi_rows_needed(ports, phich_duration) - 1 >= n_ofdm) return false;
  return !(tdd && phich_duration == 2 && (sf == 1 || sf == 6));
}
// index of the scrambling bit (and of d) of element e of its unit
__host__ __device__ __forceinline__ int phi_c_index(int e, int cp_type) { return cp_type == LCS_CP_NORMAL ? e : 2 * (e >> 2) + (e & 1); }
// the table index group * n_seq + seq of what lane j of a quadruplet of unit u holds: the real sequence (fam 0) or the one with j (fam 1)
__host__ __device__ __forceinline__ int phi_entry_index(int cp_type, int u, int j, int fam) {
  return cp_type == LCS_CP_NORMAL ? 8 * u + j + 4 * fam : 8 * u + 4 * (j >> 1) + (j & 1) + 2 * fam;
}
// what element e of unit u at resource element re brings by itself: pdc_elem with the PHICH's ports (the whole quadruplet i goes
// through ports (0, 2) when i + u is even, through (1, 3) when it is odd)
__host__ __device__ __forceinline__ void phi_elem(int e, int u, int k, int n_rb, int ports, const double *__restrict__ rowy, const double *__restrict__ row0,
                                                  const double *__restrict__ row1, const uint32_t *bits0, const uint32_t *bits1, const double *shift4,
                                                  cd2 *y, cd2 *ha, cd2 *hb) {
  const int q = ((e >> 2) + u) & 1;
  const int a = ports == 4 ? q : 0, b = ports == 4 ? q + 2 : ports == 2 ? 1 : -1;
  const int sa = (int)(a == 1 ? shift4[1] : shift4[0]);
  const int sb = (int)(b == 3 ? shift4[3] : b == 2 ? shift4[2] : shift4[1]);
  *y = mk(rowy[2 * k], rowy[2 * k + 1]);
  *ha = pcf_h_at(row0, bits0, sa, k, n_rb);
  *hb = mk(0.0, 0.0);
  if (ports == 4) *hb = pcf_h_at(row1, bits1, sb, k, n_rb);
  else if (ports == 2) *hb = pcf_h_at(row0, bits0, sb, k, n_rb);
}
__host__ __device__ __forceinline__ double phi_gain(cd2 ha, cd2 hb_pair) { return (ha.re * ha.re + ha.im * ha.im) + (hb_pair.re * hb_pair.re + hb_pair.im * hb_pair.im); }
__host__ __device__ __forceinline__ cd2 phi_descramble(cd2 s, uint32_t scr, int ci) { return ((scr >> ci) & 1u) ? mk(-s.re, -s.im) : s; }
// one stage of the butterfly on lane j with the partner's value p: bit = 1 or 2
__host__ __device__ __forceinline__ cd2 phi_bfly(cd2 mine, cd2 p, int j, int bit) { return (j & bit) ? csub(p, mine) : cadd(mine, p); }
// the projection onto the sequence's BPSK axis, with the rule's constant
__host__ __device__ __forceinline__ double phi_proj(cd2 X, int fam, int ports) {
  const double K = ports == 1 ? 0.70710678118654752440 : 1.0;
  return fam ? K * (X.im - X.re) : K * (X.re + X.im);
}
// an entry from its three repetitions
__host__ __device__ __forceinline__ PhiEntry phi_final(double a0, double a1, double a2, double d0, double d1, double d2) {
  PhiEntry z; z.value = 0.0; z.dsum = 0.0; z.S = 0.0;
  double ds = d0 + d1; ds = ds + d2;
  double as = a0 + a1; as = as + a2;
  if (!(ds > 0.0) || !isfinite(ds) || !isfinite(as)) return z;
  const double v = as / ds;
  double S = 0.0;
  if (d0 > 0.0) { const double x = a0 / d0 - v; S = S + d0 * (x * x); }
  if (d1 > 0.0) { const double x = a1 / d1 - v; S = S + d1 * (x * x); }
  if (d2 > 0.0) { const double x = a2 / d2 - v; S = S + d2 * (x * x); }
  if (!isfinite(v) || !isfinite(S)) return z;
  PhiEntry o; o.value = v; o.dsum = ds; o.S = S;
  return o;
}
// flags (1 present, 2 ack) and sigma of an entry under the subframe's noise
__host__ __device__ __forceinline__ int phi_decide(PhiEntry en, double noise, double min_amp, double min_sigma, double *sigma) {
  *sigma = 0.0;
  if (!(en.dsum > 0.0)) return 0;
  const double sg = sqrt(noise / (2.0 * en.dsum)), av = fabs(en.value);
  if (!isfinite(sg)) return 0;
  *sigma = sg;
  if (!(av >= min_amp) || !(av >= min_sigma * sg)) return 0;
  return en.value < 0.0 ? 3 : 1;
}
__host__ __device__ __forceinline__ lcs_phich_sf phi_sf_entry(int n_unit, int cp_type, int n_present, int n_ack, double noise) {
  lcs_phich_sf s;
  s.n_unit = n_unit; s.n_group = phi_n_group(cp_type, n_unit); s.n_present = n_present; s.n_ack = n_ack; s.n_nack = n_present - n_ack;
  s.reserved = 0; s.noise = noise;
  return s;
}
__host__ __device__ __forceinline__ lcs_phich_hi phi_hi_entry(int g, int idx, int cp_type, int flags, double value, double sigma) {
  lcs_phich_hi h;
  h.g = (int16_t)g; h.group = (uint8_t)(idx / phi_n_seq(cp_type)); h.seq = (uint8_t)(idx % phi_n_seq(cp_type)); h.flags = flags; h.value = value; h.sigma = sigma;
  return h;
}
__host__ __device__ __forceinline__ lcs_phich_hi phi_hi_zero() {
  lcs_phich_hi h;
  h.g = 0; h.group = 0; h.seq = 0; h.flags = 0; h.value = 0.0; h.sigma = 0.0;
  return h;
}
// the head of the record from the totals over its per-subframe entries g < n_sf (integer sums: their order does not matter)
__host__ __device__ inline void phi_head(lcs_phich_info *o, int n_sf, int n_read, int n_p, int n_a, int dl_mask, int n_rb, int ports) {
  o->n_sf = n_sf; o->n_read = n_read; o->n_present = n_p; o->n_ack = n_a; o->n_nack = n_p - n_a;
  o->n_hi = n_p < PHI_MAX_HI ? n_p : PHI_MAX_HI; o->n_dropped = n_p - o->n_hi;
  o->dl_mask = dl_mask; o->n_rb = n_rb; o->n_ports = ports; o->reserved[0] = o->reserved[1] = 0;
}
// the same with the totals taken from the entries themselves
__host__ __device__ inline void phi_summary(lcs_phich_info *o, int n_sf, int dl_mask, int n_rb, int ports) {
  int n_read = 0, n_p = 0, n_a = 0;
  for (int g = 0; g < n_sf; ++g) {
    if (o->sf[g].n_unit < 0) continue;
    n_read += 1; n_p += o->sf[g].n_present; n_a += o->sf[g].n_ack;
  }
  phi_head(o, n_sf, n_read, n_p, n_a, dl_mask, n_rb, ports);
}

// ------------------------------------------------------------------ the table (host)
// The units of m_i: the `phich` list of the PDCCH stage's map with three control symbols, which the list does not depend on beyond
// their being there.  n_unit = -1: refused
inline void phi_build_map(int n_rb, int ports, int cp_type, int id, int phich_duration, int phich_resource, int mi, PhiMap *m) {
  m->n_unit = 0;
  for (int i = 0; i < PHI_MAX_UNIT * PHI_UNIT_RE; ++i) m->re[i] = -1;
  if (mi <= 0) return;
  PdcMapT<1> unused;
  std::vector<int> phich;
  if (!pdc_build_map_t<1>(n_rb, ports, cp_type, id, phich_duration, phich_resource, mi, 3, &unused, nullptr, &phich) ||
      phich.size() % 3 != 0 || phich.size() > (size_t)3 * PHI_MAX_UNIT) { m->n_unit = -1; return; }
  m->n_unit = (int)phich.size() / 3;
  for (size_t r = 0; r < phich.size(); ++r) {
    const int kp = phich[r] >> 2, l = phich[r] & 3, per = pdc_regs_per_rb(l, ports, cp_type);
    for (int j = 0; j < 4; ++j) m->re[4 * r + j] = (l << 16) | pdc_reg_col(kp, per, j, id);
  }
}
// The maps of m_i = 0, 1, 2 together.  Unit m' of a map depends on m' alone, not on how many units follow it, so where the map of
// m_i = 2 is not refused that of m_i = 1 is its first half: one walk through the PDCCH stage's REG lists instead of two (they are
// the cost of a change of key).  tests/test_phich_host.py holds every map made this way to the generator's list for its own m_i.
inline void phi_build_maps(int n_rb, int ports, int cp_type, int id, int phich_duration, int phich_resource, PhiMap *maps /*[3]*/) {
  phi_build_map(n_rb, ports, cp_type, id, phich_duration, phich_resource, 0, &maps[0]);
  phi_build_map(n_rb, ports, cp_type, id, phich_duration, phich_resource, 2, &maps[2]);
  if (maps[2].n_unit < 0 || maps[2].n_unit % 2 != 0) { phi_build_map(n_rb, ports, cp_type, id, phich_duration, phich_resource, 1, &maps[1]); return; }
  maps[1] = maps[2];
  maps[1].n_unit = maps[2].n_unit / 2;
  for (int i = PHI_UNIT_RE * maps[1].n_unit; i < PHI_MAX_UNIT * PHI_UNIT_RE; ++i) maps[1].re[i] = -1;
}
