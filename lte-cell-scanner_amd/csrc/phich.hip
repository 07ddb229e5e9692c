// phich.hip -- the PHICH of a wide cell on the device (lcs_phich_wide, lcs_phich, lcs_phich_values; the rule: phich.h, include/lcs.h).
// A translation unit of its own, like pcfich.hip whose grid it reads: a context that never calls the stage runs no kernel of this file
// and allocates none of its buffers, and the code objects of the other stages are what they are without it.  No atomics, no scratch,
// every result written by exactly one lane, nothing depends on the order in which workgroups run; fp64 throughout and bit-equal to
// the host twin (tests/host/phich_host.cpp).
#include <cstring>
#include "lcs_internal.h"
#include "lte_device.h"
#include "phich.h"
#include "wide_call.h"

static_assert(sizeof(PhiEntry) == sizeof(lcs_ctx::PhichEntry), "lcs_internal.h: PhichEntry is phich.h's PhiEntry");
#define PHI_THREADS 256
#define PHI_FIN_WAVES 16

// ------------------------------------------------------------------ the table of a subframe: one workgroup per subframe
// Workgroup g takes grid subframe g: sf3[3 g + l] is the row of `grid` that holds its symbol l (-1 for a subframe that is not read, and
// for a symbol the rule does not need), sf3[3 n_sf + s] the m_i of subframe s.  Threads 0 and 1 build the reference sequences of
// symbols 0 and 1 (the second with four ports only), thread 64 the scrambling bits.  Then every wave takes blocks of five units: lane
// 12 uu + e holds element e of unit uu of the block -- its y at (l, k) of the map and the two channel values at column k --, the lanes
// of a pair trade hb and y (__shfl_xor 1), the descrambled symbols and the gains go through the Hadamard butterfly across the four
// lanes of a quadruplet (xor 1, xor 2; xor 1 alone with the extended CP), and the four lanes of quadruplet 0 fetch the other two
// repetitions from lanes + 4 and + 8 and write the unit's eight entries (value, d sum, S) of tab.  Thread 0 writes n_unit.
__global__ __launch_bounds__(PHI_THREADS) void k_phich(const double2 *__restrict__ grid, const int *__restrict__ sf3, const uint32_t *__restrict__ jump /*[2][32]*/,
                                                       const PhiMap *__restrict__ maps /*[3]*/, PhiEntry *__restrict__ tab /*[n_sf][PHI_MAX_ENT]*/,
                                                       int *__restrict__ sfu /*[n_sf]*/, int n_sf, int id, int cp_type, int n_symb, int ports, int n_rb) {
  const int g = blockIdx.x, tid = threadIdx.x;
  if (g >= n_sf) return;
  __shared__ uint32_t s_bits[2][RS_DL_WIDE_WORDS];
  __shared__ double s_shift[4];
  __shared__ uint32_t s_scr;
  const int r0 = sf3[3 * g];                                 // the same for the whole workgroup
  const int mi = sf3[3 * n_sf + g % 10];
  const PhiMap *map = maps + (mi < 0 ? 0 : mi > 2 ? 2 : mi);
  const int n_unit = r0 >= 0 ? map->n_unit : -1;
  if (tid == 0) sfu[g] = n_unit;
  if (n_unit <= 0 || n_unit > PHI_MAX_UNIT) return;
  const int sf = g % 10;
  if (tid < 4) s_shift[tid] = 0.0;
  __syncthreads();
  if (tid < (ports == 4 ? 2 : 1)) rs_dl_row_wide(2 * sf, tid, id, cp_type, n_symb, n_rb, jump, s_bits[tid], s_shift);
  if (tid == 64) s_scr = pcf_scramble(sf, id, jump + 32);
  __syncthreads();
  const size_t ncol = (size_t)12 * n_rb;
  const double *row0 = reinterpret_cast<const double *>(grid + (size_t)r0 * ncol);
  const double *row1 = reinterpret_cast<const double *>(grid + (size_t)(ports == 4 ? sf3[3 * g + 1] : r0) * ncol);
  const int wave = tid >> 6, lane = tid & 63;
  const int uu = lane / PHI_UNIT_RE, e = lane - PHI_UNIT_RE * uu, j = e & 3;
  const bool normal = cp_type == LCS_CP_NORMAL;
#pragma unroll 1
  for (int u0 = PHI_WAVE_UNITS * wave; u0 < n_unit; u0 += PHI_WAVE_UNITS * (PHI_THREADS / 64)) {
    const int u = u0 + uu;
    const bool live = uu < PHI_WAVE_UNITS && u < n_unit;
    const int re = live ? map->re[PHI_UNIT_RE * u + e] : -1;
    const int l = re >= 0 ? (re >> 16) : 0, k = re >= 0 ? (re & 0xffff) : 0;
    const int ry = sf3[3 * g + l];
    const double *rowy = reinterpret_cast<const double *>(grid + (size_t)(ry >= 0 ? ry : r0) * ncol);
    cd2 y, ha, hb;
    phi_elem(e, u, k, n_rb, ports, rowy, row0, row1, s_bits[0], s_bits[1], s_shift, &y, &ha, &hb);
    const cd2 hb_pair = mk(__shfl_xor(hb.re, 1), __shfl_xor(hb.im, 1)), y_pair = mk(__shfl_xor(y.re, 1), __shfl_xor(y.im, 1));
    const cd2 s = pcf_soft(e, ports, y, ha, hb_pair, y_pair);
    cd2 t = phi_descramble(s, s_scr, phi_c_index(e, cp_type));
    double G = phi_gain(ha, hb_pair);
    t = phi_bfly(t, mk(__shfl_xor(t.re, 1), __shfl_xor(t.im, 1)), j, 1);
    G = G + __shfl_xor(G, 1);
    if (normal) {
      t = phi_bfly(t, mk(__shfl_xor(t.re, 2), __shfl_xor(t.im, 2)), j, 2);
      G = G + __shfl_xor(G, 2);
    }
    const double a = phi_proj(t, 0, ports), b = phi_proj(t, 1, ports);
    // the repetitions: quadruplets 1 and 2 of the same unit sit 4 and 8 lanes up
    const int up1 = (lane + 4) & 63, up2 = (lane + 8) & 63;
    const double a1 = __shfl(a, up1), a2 = __shfl(a, up2), b1 = __shfl(b, up1), b2 = __shfl(b, up2), G1 = __shfl(G, up1), G2 = __shfl(G, up2);
    if (live && e < 4) {
      PhiEntry *row = tab + (size_t)g * PHI_MAX_ENT;
      row[phi_entry_index(cp_type, u, j, 0)] = phi_final(a, a1, a2, G, G1, G2);
      row[phi_entry_index(cp_type, u, j, 1)] = phi_final(b, b1, b2, G, G1, G2);
    }
  }
}

// ------------------------------------------------------------------ noise, decisions, the ordered list: one workgroup
// Wave w takes subframes w, w + 16, ..: lane i holds entries i, i + 64, ..; the noise is their S through the wave's butterfly, the
// decisions follow, and lane 0 writes the subframe's entry.  The counts meet in LDS; then every wave places the present entries of
// its subframes behind those of the subframes before them (ballots in entry order: ordered prefix sums, no atomics), the entries
// beyond the list are zeroed and thread 0 writes the head from the counts in LDS.
static __device__ __forceinline__ int phi_wave_sum_int(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__global__ __launch_bounds__(64 * PHI_FIN_WAVES) void k_phich_fin(const PhiEntry *__restrict__ tab, const int *__restrict__ sfu, lcs_phich_info *__restrict__ out,
                                                                  int n_sf, int cp_type, int dl_mask, int n_rb, int ports, double min_amp, double min_sigma) {
  __shared__ double s_noise[PCF_MAX_SF];
  __shared__ int s_cnt[PCF_MAX_SF], s_ack[PCF_MAX_SF], s_read[PCF_MAX_SF];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int g = wave; g < PCF_MAX_SF; g += PHI_FIN_WAVES) {
    const int n_unit = g < n_sf ? sfu[g] : 0;
    const int n_ent = n_unit > 0 ? 8 * n_unit : 0;
    const PhiEntry *row = tab + (size_t)g * PHI_MAX_ENT;
    double part = 0.0;
    int cnt = 0;
#pragma unroll 1
    for (int q = 0; 64 * q < n_ent; ++q) {                  // (n_ent <= 64 PHI_ENT_PASSES)
      const int i = lane + 64 * q;
      if (i < n_ent && row[i].dsum > 0.0) { part = part + row[i].S; cnt += 1; }
    }
    const double tot = meas_row_sum_lanes<64>(part);
    cnt = phi_wave_sum_int(cnt);
    const double noise = cnt > 0 ? tot / (double)cnt : 0.0;
    int n_p = 0, n_a = 0;
#pragma unroll 1
    for (int q = 0; 64 * q < n_ent; ++q) {                  // (n_ent <= 64 PHI_ENT_PASSES)
      const int i = lane + 64 * q;
      double sg;
      const int fl = i < n_ent ? phi_decide(row[i], noise, min_amp, min_sigma, &sg) : 0;
      n_p += fl & 1; n_a += (fl >> 1) & 1;
    }
    n_p = phi_wave_sum_int(n_p); n_a = phi_wave_sum_int(n_a);
    if (lane == 0) {
      out->sf[g] = g < n_sf ? phi_sf_entry(n_unit < 0 ? -1 : n_unit, cp_type, n_p, n_a, noise) : phi_sf_entry(0, cp_type, 0, 0, 0.0);
      s_noise[g] = noise; s_cnt[g] = n_p; s_ack[g] = n_a; s_read[g] = (g < n_sf && n_unit >= 0) ? 1 : 0;
    }
  }
  __syncthreads();
  for (int g = wave; g < n_sf; g += PHI_FIN_WAVES) {
    const int n_unit = sfu[g];
    const int n_ent = n_unit > 0 ? 8 * n_unit : 0;
    if (s_cnt[g] == 0) continue;
    int base = 0;
    for (int h = 0; h < g; ++h) base += s_cnt[h];
    const PhiEntry *row = tab + (size_t)g * PHI_MAX_ENT;
    const double noise = s_noise[g];
#pragma unroll 1
    for (int q = 0; 64 * q < n_ent; ++q) {                  // (n_ent <= 64 PHI_ENT_PASSES)
      const int i = lane + 64 * q;
      double sg = 0.0;
      const int fl = i < n_ent ? phi_decide(row[i], noise, min_amp, min_sigma, &sg) : 0;
      const unsigned long long m = __ballot(fl & 1);
      const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
      if ((fl & 1) && pos < PHI_MAX_HI) out->hi[pos] = phi_hi_entry(g, i, cp_type, fl, row[i].value, sg);
      base += __popcll(m);
    }
  }
  int total = 0, acks = 0, reads = 0;
  for (int h = 0; h < n_sf; ++h) { total += s_cnt[h]; acks += s_ack[h]; reads += s_read[h]; }
  for (int i = total + (int)threadIdx.x; i < PHI_MAX_HI; i += 64 * PHI_FIN_WAVES) out->hi[i] = phi_hi_zero();
  if (threadIdx.x == 0) phi_head(out, n_sf, reads, total, acks, dl_mask, n_rb, ports);
}

// ------------------------------------------------------------------ launchers
// the unit tables of the call's key, on the host (c->phich.h_map: what the entry points plan the subframes by) and on the device
int lcs_phich_tables(lcs_ctx *c, const lcs_cell &cell, int n_rb, const PhichPlan &plan) {
  lcs_ctx::Phich &p = c->phich;
  int rc;
  const int id = cell.n_id_2 + 3 * cell.n_id_1, ports = pcf_ports(cell.n_ports);
  const size_t map_ints = 3 * sizeof(PhiMap) / sizeof(int);
  if ((rc = p.map.reserve(c, map_ints)) || (rc = p.jump.reserve(c, 64)) || (rc = p.sf.reserve(c, sizeof(p.h_sf) / sizeof(int))) ||
      (rc = p.tab.reserve(c, (size_t)PCF_MAX_SF * PHI_MAX_ENT)) || (rc = p.sfu.reserve(c, PCF_MAX_SF)) || (rc = p.rec.reserve(c, 1))) return rc;
  const int key[6] = {n_rb, ports, (int)cell.cp_type, id, plan.sh.phich_duration, plan.sh.phich_resource};
  if (std::memcmp(key, p.key, sizeof(key)) != 0) {
    p.key[0] = 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));              // nothing reads the host block that is rewritten
    p.h_map.assign(map_ints, 0);
    PhiMap *maps = reinterpret_cast<PhiMap *>(p.h_map.data());
    phi_build_maps(n_rb, ports, (int)cell.cp_type, id, plan.sh.phich_duration, plan.sh.phich_resource, maps);
    HIPCHK(c, hipMemcpyAsync(p.map, p.h_map.data(), sizeof(int) * map_ints, hipMemcpyHostToDevice, c->stream));
    std::memcpy(p.key, key, sizeof(key));
  }
  if (p.jump_rb != n_rb) {
    p.jump_rb = 0;
    lcs_tables::wide_jump_block(n_rb, p.h_jump);
    HIPCHK(c, hipMemcpyAsync(p.jump, p.h_jump, sizeof(p.h_jump), hipMemcpyHostToDevice, c->stream));
    p.jump_rb = n_rb;
  }
  return LCS_OK;
}
int lcs_phich_map_units(const lcs_ctx *c, int mi) {
  return reinterpret_cast<const PhiMap *>(c->phich.h_map.data())[mi].n_unit;
}

int lcs_launch_phich(lcs_ctx *c, const lcs_cell &cell, const int *rows3, int n_sf, int n_rb, int dl_mask, const PhichPlan &plan) {
  lcs_ctx::Phich &p = c->phich;
  lcs_ctx::MeasWide &w = c->meas_wide;
  if (n_sf <= 0 || n_sf > PCF_MAX_SF) { c->err = "phich: no such number of subframes"; return LCS_ERR_BAD_ARG; }
  const int n_symb = cell.cp_type == LCS_CP_NORMAL ? 7 : 6, id = cell.n_id_2 + 3 * cell.n_id_1, ports = pcf_ports(cell.n_ports);
  for (int i = 0; i < 3 * n_sf; ++i) p.h_sf[i] = rows3[i];
  for (int i = 0; i < 10; ++i) p.h_sf[3 * n_sf + i] = plan.sh.mi[i];
  HIPCHK(c, hipMemcpyAsync(p.sf, p.h_sf, sizeof(int) * (3 * n_sf + 10), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_phich, dim3(n_sf), dim3(PHI_THREADS), 0, c->stream, (const double2 *)w.grid.get(), (const int *)p.sf.get(), (const uint32_t *)p.jump.get(),
                     reinterpret_cast<const PhiMap *>(p.map.get()), reinterpret_cast<PhiEntry *>(p.tab.get()), p.sfu.get(), n_sf, id, (int)cell.cp_type, n_symb, ports, n_rb);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_phich_fin, dim3(1), dim3(64 * PHI_FIN_WAVES), 0, c->stream, reinterpret_cast<const PhiEntry *>(p.tab.get()), (const int *)p.sfu.get(), p.rec.get(), n_sf,
                     (int)cell.cp_type, dl_mask, n_rb, ports, plan.min_amp, plan.min_sigma);
  HIPCHK(c, hipGetLastError());
  return LCS_OK;
}
