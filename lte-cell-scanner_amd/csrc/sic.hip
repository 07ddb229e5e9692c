// sic.hip -- the cancellation stage (lcs_sic_cancel_dev, lcs_search_*_sic; the rule: sic.h).  A translation unit of its own: a
// context that never calls the stage runs none of these kernels and allocates none of their buffers.
//
// One launch sequence serves a batch; a single capture is n_buf = 1 of the same path.  Per call:
//   k_sic_grid    (symbol tiles, cell)    the capture's grid over the WHOLE capture: eight symbols per wave through the register
//                                         transform of lte_device.h (fft128_x8), one per 8 lanes
//   k_sic_chan    (slot, cell)            least squares on the CRS, the +-4-slot mean per reference subcarrier, interpolation to 72
//   k_sic_gain    (cell)                  the sync gain from every SSS symbol
//   k_sic_synth   (symbol tiles, cell)    the known elements through the channel, the inverse transform, the table td[symbol][128]
//                                         in HBM, and the energy of each component per symbol
//   k_sic_sub     (sample tiles, buffer)  one thread per output sample, the buffer's cells in list order, each cell's owning symbol
//                                         in closed form (sic_owner): no atomics, the same bits every run
//   k_sic_grid    again, on the residual  ... and
//   k_sic_info    (cell)                  the record: the components' energies, the gain, the PSS subcarriers' energy before / after
// Every index below is bounded by the record's own t_lo .. t_hi (sic_geometry: the whole symbol, cyclic prefix and window, lies
// inside the capture) and the per-call offsets sym0 / slot0 the host computed from the same numbers.
#include <algorithm>
#include <vector>

#include "lcs_internal.h"
#include "lte_device.h"
#include "cell_meas.h"
#include "sic.h"

struct SicCell {
  SicGeom g;
  int id, n_id_1, n_id_2, n_ports, cp_type, dl_mask, special, duplex;
  int src_buf, res_buf;      // the capture it is cancelled from, and the residual slot
  int sym0, slot0;           // where its symbols / slots start in the per-symbol / per-slot arrays
};
#define SIC_PBCH_STRIDE 240

template <int FMT> __device__ __forceinline__ cd2 sic_load(const void *__restrict__ cap, size_t i);
template <> __device__ __forceinline__ cd2 sic_load<LCS_FMT_IQ_U8>(const void *__restrict__ cap, size_t i) {
  const unsigned p = reinterpret_cast<const uint16_t *>(cap)[i];      // src/capbuf.cpp:172-181
  return mk(((double)(p & 255u) - 127.0) / 128.0, ((double)(p >> 8) - 127.0) / 128.0);
}
template <> __device__ __forceinline__ cd2 sic_load<LCS_FMT_C64>(const void *__restrict__ cap, size_t i) {
  const float2 v = reinterpret_cast<const float2 *>(cap)[i];
  return mk((double)v.x, (double)v.y);
}
// cis(2 pi x) for x in cycles, any size: the whole cycles go first
__device__ __forceinline__ cd2 sic_cis_cycles(double x) {
  double s_, c_;
  sincospi(2.0 * (x - rint(x)), &s_, &c_);
  return mk(c_, s_);
}

// ------------------------------------------------------------------ the grid: [symbol][72], sic.h step 2
// use_res: the source is the residual array (slot res_buf) instead of the capture (slot src_buf)
template <int FMT>
__global__ __launch_bounds__(64) void k_sic_grid(const SicCell *__restrict__ cells, const void *__restrict__ cap, int use_res,
                                                 double2 *__restrict__ grid) {
  __shared__ cd2 tw[128];
  __shared__ cd2 tb[8 * FFT128_WSTRIDE];
  const int lane = threadIdx.x, w = lane >> 3, l = lane & 7;
  const SicCell &q = cells[blockIdx.y];
  const int n_sym = q.g.t_hi - q.g.t_lo + 1;
  if ((int)blockIdx.x * 8 >= n_sym) return;      // the whole workgroup
  fft128_twiddle_table(tw, lane, 64);
  __syncthreads();
  const int s = blockIdx.x * 8 + w;
  const bool valid = s < n_sym;
  cd2 x[16];
  double late = 0.0;
  if (valid) {
    const int t = q.g.t_lo + s;
    const double d = sic_d(q.g, t);
    const long wpos = (long)rint(d);
    late = (double)wpos - d;
    const size_t base = (size_t)(use_res ? q.res_buf : q.src_buf) * q.g.n_cap;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const long n = wpos + l + 8 * j;             // 0 <= a(t) <= wpos, wpos + 127 < n_cap
      x[j] = cmul(sic_load<FMT>(cap, base + (size_t)n), sic_cis_cycles(-q.g.rot * (double)n));
    }
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) x[j] = mk(0, 0);
  }
  fft128_x8(x, tb, tw, lane);
  if (!valid) return;
  double2 *out = grid + (size_t)(q.sym0 + s) * 72;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int c = e >> 3, k1 = e & 7;
    if (k1 == 3 || k1 == 4) continue;            // bins 48 .. 95: never kept
    const int i = sic_idx_of_bin((l + 8 * c) + 16 * k1);
    if (i < 0) continue;
    st(&out[i], cmul(x[e], sic_cis_cycles(-late * (double)sic_cn(i) / 128.0)));
  }
}

// ------------------------------------------------------------------ the channel: [slot][4][72], sic.h step 3
#define SIC_CH_THREADS 128
__global__ __launch_bounds__(SIC_CH_THREADS) void k_sic_chan(const SicCell *__restrict__ cells, const double2 *__restrict__ grid,
                                                             const uint32_t *__restrict__ pn_jump, double2 *__restrict__ chan) {
  __shared__ double rs[(2 * SIC_AVG_SLOTS + 1) * 3][24];
  __shared__ cd2 h[4][24];
  const SicCell &q = cells[blockIdx.y];
  const int js = blockIdx.x, tid = threadIdx.x;
  if (js >= q.g.n_slots) return;
  const int j = q.g.j_lo + js, n_symb = q.g.n_symb, c3 = q.id % 3;
  if (tid < (2 * SIC_AVG_SLOTS + 1) * 3) {
    double sh4[4];
    rs_dl_row(sic_mod(j + tid / 3 - SIC_AVG_SLOTS, 20), tid % 3, q.id, q.cp_type, n_symb, pn_jump, rs[tid], sh4);
  }
  __syncthreads();
  if (tid < 96) {
    const int p = tid / 24, m = tid % 24;
    cd2 acc = mk(0, 0);
    int cnt = 0;
    if (p < q.n_ports) {
      for (int dj = -SIC_AVG_SLOTS; dj <= SIC_AVG_SLOTS; ++dj) {
        const int jj = j + dj;
        if (jj < q.g.j_lo || jj >= q.g.j_lo + q.g.n_slots) continue;
        const int s = sic_mod(jj, 20);
        for (int row = 0; row < 3; ++row) {
          const int sh = sic_crs_shift(p, row, s, q.id);
          if (sh < 0) continue;
          const int t = jj * n_symb + (row == 2 ? n_symb - 3 : row);
          if (t < q.g.t_lo || t > q.g.t_hi || !sic_usable(q.g, t, q.dl_mask, q.special)) continue;
          const int mm = m - (sh - c3) / 3;
          if (mm < 0 || (mm & 1)) continue;
          const int i = mm >> 1;                 // <= 11, and sh + 6 i <= 71
          const double *r = rs[(dj + SIC_AVG_SLOTS) * 3 + row];
          acc = cadd(acc, cmul(ld(&grid[(size_t)(q.sym0 + t - q.g.t_lo) * 72 + sh + 6 * i]), mk(r[2 * i], -r[2 * i + 1])));
          ++cnt;
        }
      }
    }
    h[p][m] = cnt ? cdivr(acc, (double)cnt) : mk(0, 0);
  }
  __syncthreads();
  for (int e = tid; e < q.n_ports * 72; e += SIC_CH_THREADS) {
    const int p = e / 72, k = e % 72;
    int m0; double fr;
    sic_interp(k, c3, &m0, &fr);
    const cd2 a = h[p][m0], b = h[p][m0 + 1];
    st(&chan[((size_t)(q.slot0 + js) * 4 + p) * 72 + k], cadd(a, cscale(csub(b, a), fr)));
  }
}

// ------------------------------------------------------------------ the sync gain, sic.h step 4
__global__ __launch_bounds__(64) void k_sic_gain(const SicCell *__restrict__ cells, const double2 *__restrict__ grid,
                                                 const double2 *__restrict__ chan, const int8_t *__restrict__ sss_fd, double2 *__restrict__ gain) {
  __shared__ cd2 s_num[64];
  __shared__ double s_den[64];
  const SicCell &q = cells[blockIdx.x];
  const int k = threadIdx.x;
  cd2 num = mk(0, 0);
  double den = 0.0;
  for (int hf = sic_hf_lo(q.g); hf <= sic_hf_hi(q.g); ++hf) {
    const int t = sic_sss_symbol(q.g, hf, q.duplex);
    if (t < q.g.t_lo || t > q.g.t_hi || k >= 62) continue;
    const int js = sic_slot_of(q.g, t) - q.g.j_lo;
    const double sq = (double)sss_fd[(((size_t)q.n_id_1 * 3 + q.n_id_2) * 2 + (sic_mod(hf, 2))) * 62 + k];
    const cd2 ref = cscale(ld(&chan[((size_t)(q.slot0 + js) * 4 + 0) * 72 + 5 + k]), sq);
    num = cadd(num, cmul(ld(&grid[(size_t)(q.sym0 + t - q.g.t_lo) * 72 + 5 + k]), cconj(ref)));
    den = den + cabs2(ref);
  }
  s_num[k] = num; s_den[k] = den;
  __syncthreads();
  if (k == 0) {
    cd2 a = mk(0, 0);
    double b = 0.0;
    for (int i = 0; i < 62; ++i) { a = cadd(a, s_num[i]); b = b + s_den[i]; }
    st(&gain[blockIdx.x], b > 0.0 ? cdivr(a, b) : mk(0, 0));
  }
}

// ------------------------------------------------------------------ synthesis: td[symbol][128], sic.h steps 5 and 6
__global__ __launch_bounds__(64) void k_sic_synth(const SicCell *__restrict__ cells, const double2 *__restrict__ chan,
                                                  const double2 *__restrict__ gain, const float2 *__restrict__ pbch,
                                                  const double2 *__restrict__ pss_fd, const int8_t *__restrict__ sss_fd,
                                                  const uint32_t *__restrict__ pn_jump, int mask, float2 *__restrict__ td,
                                                  double *__restrict__ part) {
  __shared__ cd2 tw[128];
  __shared__ cd2 tb[8 * FFT128_WSTRIDE];
  __shared__ cd2 T[8][72];
  __shared__ double rsrow[8][24];
  __shared__ double pw[8][8][4];
  const int lane = threadIdx.x, w = lane >> 3, l = lane & 7;
  const int ci = blockIdx.y;
  const SicCell &q = cells[ci];
  const int n_sym = q.g.t_hi - q.g.t_lo + 1;
  if ((int)blockIdx.x * 8 >= n_sym) return;      // the whole workgroup
  fft128_twiddle_table(tw, lane, 64);
  __syncthreads();
  const int sidx = blockIdx.x * 8 + w;
  const bool valid = sidx < n_sym;
  const int t = q.g.t_lo + (valid ? sidx : 0), n_symb = q.g.n_symb;
  const int j = sic_slot_of(q.g, t), sym = sic_sym_of(q.g, t), s = sic_mod(j, 20), js = j - q.g.j_lo;
  int seq_slot;
  const int kind = sic_sync_kind(q.g, t, q.duplex, &seq_slot);
  const int row = sic_crs_row(sym, n_symb);
  const bool use = sic_usable(q.g, t, q.dl_mask, q.special);
  const bool crs_here = valid && row >= 0 && use && (mask & LCS_SIC_CRS);
  if (crs_here && l == 0) {
    double sh4[4];
    rs_dl_row(s, row, q.id, q.cp_type, n_symb, pn_jump, rsrow[w], sh4);
  }
  lcs_wave_sync();
  const double d = sic_d(q.g, t);
  const double late = rint(d) - d;
  const cd2 g = ld(&gain[ci]);
  const double2 *H = chan + (size_t)(q.slot0 + js) * 4 * 72;
  const float2 *pb = pbch + ((size_t)ci * SIC_MAX_FRAMES + (sic_floordiv(j, 20) - q.g.f_lo)) * SIC_PBCH_STRIDE;
  double e4[4] = {0.0, 0.0, 0.0, 0.0};
  for (int qk = 0; qk < 9; ++qk) {
    const int k = l + 8 * qk;
    cd2 v = mk(0, 0);
    int comp = -1;
    if (valid && kind) {
      if (k >= 5 && k < 67 && (mask & (kind == 1 ? LCS_SIC_PSS : LCS_SIC_SSS))) {
        const cd2 seq = kind == 1 ? ld(&pss_fd[q.n_id_2 * 62 + k - 5])
                                  : mk((double)sss_fd[(((size_t)q.n_id_1 * 3 + q.n_id_2) * 2 + seq_slot / 10) * 62 + k - 5], 0.0);
        v = cmul(g, cmul(ld(&H[k]), seq));
        comp = kind - 1;
      }
    } else if (valid && use) {
      if (crs_here) {
        for (int p = 0; p < q.n_ports; ++p) {
          const int sh = sic_crs_shift(p, row, s, q.id);
          if (sh < 0 || k < sh || (k - sh) % 6) continue;
          const int i = (k - sh) / 6;
          v = cadd(v, cmul(ld(&H[p * 72 + k]), mk(rsrow[w][2 * i], rsrow[w][2 * i + 1])));
          comp = 2;
        }
      }
      if (comp < 0 && s == 1 && (mask & LCS_SIC_PBCH)) {
        const int idx = sic_pbch_index(q.g.normal, sym, k, q.id);
        if (idx >= 0) {
          const float2 sv = pb[idx], mv = pb[idx ^ 1];      // idx < 240; the quarter's length is even, so idx ^ 1 is inside it
          for (int p = 0; p < q.n_ports; ++p) {
            double xr, xi;
            sic_pbch_port(q.n_ports, p, idx, (double)sv.x, (double)sv.y, (double)mv.x, (double)mv.y, &xr, &xi);
            v = cadd(v, cmul(ld(&H[p * 72 + k]), mk(xr, xi)));
          }
          comp = 3;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) e4[c] = e4[c] + (comp == c ? cabs2(v) : 0.0);
    T[w][k] = cmul(v, sic_cis_cycles(late * (double)sic_cn(k) / 128.0));
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) pw[w][l][c] = e4[c];
  lcs_wave_sync();
  if (valid && l == 0) {
    for (int c = 0; c < 4; ++c) {
      double a = 0.0;
      for (int i = 0; i < 8; ++i) a = a + pw[w][i][c];
      part[(size_t)(q.sym0 + sidx) * 4 + c] = a / 128.0;
    }
  }
  // inverse transform: conj(fft(conj(X))) / 128
  cd2 x[16];
#pragma unroll
  for (int jj = 0; jj < 16; ++jj) {
    const int i = sic_idx_of_bin(l + 8 * jj);
    x[jj] = i >= 0 ? cconj(T[w][i]) : mk(0, 0);
  }
  fft128_x8(x, tb, tw, lane);
  if (!valid) return;
  float2 *out = td + (size_t)(q.sym0 + sidx) * 128;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int n = (l + 8 * (e >> 3)) + 16 * (e & 7);
    out[n] = make_float2((float)(x[e].re / 128.0), (float)(-x[e].im / 128.0));
  }
}

// ------------------------------------------------------------------ subtraction: one thread per output sample, sic.h step 7
#define SIC_SUB_THREADS 256
template <int FMT>
__global__ __launch_bounds__(SIC_SUB_THREADS) void k_sic_sub(const SicCell *__restrict__ cells, const int *__restrict__ range /*[slots][3]: source buffer, first cell, cells*/,
                                                             const void *__restrict__ cap, const float2 *__restrict__ td, uint32_t n_cap,
                                                             float2 *__restrict__ res) {
  const int slot = blockIdx.y;
  const size_t n = (size_t)blockIdx.x * SIC_SUB_THREADS + threadIdx.x;
  if (n >= n_cap) return;
  const int src = range[3 * slot], first = range[3 * slot + 1], cnt = range[3 * slot + 2];
  cd2 v = sic_load<FMT>(cap, (size_t)src * n_cap + n);
  for (int ci = first; ci < first + cnt; ++ci) {
    const SicCell &q = cells[ci];
    int t, off;
    if (!sic_owner(q.g, (long)n, &t, &off)) continue;
    const float2 y = td[(size_t)(q.sym0 + t - q.g.t_lo) * 128 + off];
    v = csub(v, cmul(mk((double)y.x, (double)y.y), sic_cis_cycles(q.g.rot * (double)n)));
  }
  res[(size_t)slot * n_cap + n] = make_float2((float)v.re, (float)v.im);
}

// ------------------------------------------------------------------ the record
__global__ __launch_bounds__(64) void k_sic_info(const SicCell *__restrict__ cells, const double2 *__restrict__ grid,
                                                 const double2 *__restrict__ grid_res, const double *__restrict__ part,
                                                 const double2 *__restrict__ gain, lcs_sic_info *__restrict__ info) {
  __shared__ double red[64][6];
  const SicCell &q = cells[blockIdx.x];
  const int k = threadIdx.x, n_sym = q.g.t_hi - q.g.t_lo + 1;
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int n_pss = 0;
  for (int hf = sic_hf_lo(q.g); hf <= sic_hf_hi(q.g); ++hf) {
    const int t = sic_pss_symbol(q.g, hf, q.duplex);
    if (t < q.g.t_lo || t > q.g.t_hi) continue;
    ++n_pss;
    if (k >= 62) continue;
    const size_t at = (size_t)(q.sym0 + t - q.g.t_lo) * 72 + 5 + k;
    v[4] = v[4] + cabs2(ld(&grid[at]));
    v[5] = v[5] + cabs2(ld(&grid_res[at]));
  }
  for (int s = k; s < n_sym; s += 64)
    for (int c = 0; c < 4; ++c) v[c] = v[c] + part[(size_t)(q.sym0 + s) * 4 + c];
  for (int c = 0; c < 6; ++c) red[k][c] = v[c];
  __syncthreads();
  if (k == 0) {
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < 64; ++i)
      for (int c = 0; c < 6; ++c) a[c] = a[c] + red[i][c];
    lcs_sic_info o;
    for (int c = 0; c < 4; ++c) o.power[c] = a[c];
    const cd2 g = ld(&gain[blockIdx.x]);
    o.gain_re = g.re; o.gain_im = g.im;
    o.pss_before = a[4]; o.pss_after = a[5];
    o.n_sym = n_sym; o.n_pss = n_pss; o.n_dup = 0; o.ul_dl_config = LCS_TDD_NOT_ESTIMATED;
    info[blockIdx.x] = o;
  }
}

// ------------------------------------------------------------------ host side
static bool sic_record_ok(const lcs_cell &r) {
  const bool bw = r.n_rb_dl == 6 || r.n_rb_dl == 15 || r.n_rb_dl == 25 || r.n_rb_dl == 50 || r.n_rb_dl == 75 || r.n_rb_dl == 100;
  return bw && (r.n_ports == 1 || r.n_ports == 2 || r.n_ports == 4) && r.n_id_1 >= 0 && r.n_id_1 < 168 && r.n_id_2 >= 0 && r.n_id_2 < 3 &&
         (r.phich_duration == 1 || r.phich_duration == 2) && r.phich_resource >= 1 && r.phich_resource <= 4 && r.sfn >= 0 && r.sfn < 1024;
}

int lcs_launch_sic(lcs_ctx *c, const void *d_cap, int fmt, int n_buf, uint32_t n_cap, const lcs_cell *cells, const int *n_cells_per_buf,
                   int max_cells_per_buf, const double *fc_req, const double *fc_prog, double fs_prog, int mask, int duplex, const int *src_of,
                   const int32_t *ul_dl_config, float2 *d_res, lcs_sic_info *info) {
  lcs_ctx::Sic &w = c->sic;
  std::vector<SicCell> rec;
  std::vector<int> range(3 * (size_t)n_buf), where, cfg_used;      // where: the caller's index of every record that is cancelled
  std::vector<float2> pbch;
  std::vector<double> period(2 * 960);
  int n_sym_all = 0, n_slot_all = 0, max_sym = 0, max_slots = 0;
  for (int b = 0; b < n_buf; ++b) {
    range[3 * b] = src_of ? src_of[b] : b; range[3 * b + 1] = (int)rec.size();
    for (int i = 0; i < n_cells_per_buf[b]; ++i) {
      const lcs_cell &r = cells[(size_t)b * max_cells_per_buf + i];
      SicCell q{};
      if (!sic_record_ok(r) || !sic_geometry(r.frame_start, r.freq_fine, r.freq_superfine, r.cp_type, n_cap, fc_req[b], fc_prog[b], fs_prog, &q.g))
        continue;
      if (q.g.n_frames > SIC_MAX_FRAMES) { c->err = "lcs_sic: the capture spans more than 16 frames of a cell (the PBCH table's limit)"; return LCS_ERR_BAD_ARG; }
      q.id = r.n_id_2 + 3 * r.n_id_1; q.n_id_1 = r.n_id_1; q.n_id_2 = r.n_id_2; q.n_ports = r.n_ports; q.cp_type = r.cp_type;
      q.duplex = duplex; q.dl_mask = duplex == LCS_DUPLEX_TDD ? 0x021 : 0x3ff; q.special = 0;
      // a TDD cell whose uplink-downlink configuration is known: its downlink subframes, and symbol 0 of the special ones (sic.h step 5)
      const int cfg = (duplex == LCS_DUPLEX_TDD && ul_dl_config) ? ul_dl_config[(size_t)b * max_cells_per_buf + i] : LCS_TDD_NOT_ESTIMATED;
      if (cfg >= 0 && meas_mask_ok(meas_tdd_dl_mask(cfg))) { q.dl_mask = meas_tdd_dl_mask(cfg); q.special = 1; }
      cfg_used.push_back(q.special ? cfg : LCS_TDD_NOT_ESTIMATED);
      q.src_buf = range[3 * b]; q.res_buf = b;
      q.sym0 = n_sym_all; q.slot0 = n_slot_all;
      const int n_sym = q.g.t_hi - q.g.t_lo + 1;
      n_sym_all += n_sym; n_slot_all += q.g.n_slots;
      max_sym = std::max(max_sym, n_sym); max_slots = std::max(max_slots, q.g.n_slots);
      // the PBCH of every frame of the capture: frame f of the grid carries sfn + f (decode_mib's rule)
      const size_t at = pbch.size();
      pbch.resize(at + (size_t)SIC_MAX_FRAMES * SIC_PBCH_STRIDE, make_float2(0.f, 0.f));
      const int per = sic_pbch_per_frame(q.g.normal);
      int have = -1;
      for (int f = 0; f < q.g.n_frames; ++f) {
        const int sfn = sic_mod(r.sfn + q.g.f_lo + f, 1024);
        if ((sfn & ~3) != have) {
          have = sfn & ~3;
          if (!lcs_tables::pbch_encode(q.id, r.n_ports, r.n_rb_dl, r.phich_duration, r.phich_resource, have, r.cp_type, period.data())) { c->err = "lcs_sic: a record no MIB carries"; return LCS_ERR_BAD_ARG; }
        }
        for (int i2 = 0; i2 < per; ++i2)
          pbch[at + (size_t)f * SIC_PBCH_STRIDE + i2] = make_float2((float)period[2 * ((sfn & 3) * per + i2)], (float)period[2 * ((sfn & 3) * per + i2) + 1]);
      }
      rec.push_back(q);
      where.push_back(b * max_cells_per_buf + i);
    }
    range[3 * b + 2] = (int)rec.size() - range[3 * b + 1];
  }
  if (info) for (size_t i = 0; i < (size_t)n_buf * max_cells_per_buf; ++i) { info[i] = lcs_sic_info{}; info[i].ul_dl_config = LCS_TDD_NOT_ESTIMATED; }
  const int n = (int)rec.size();
  int rc;
  const size_t cell_bytes = (size_t)std::max(n, 1) * sizeof(SicCell), range_at = (cell_bytes + 15) & ~(size_t)15;
  if ((rc = w.cells.reserve(c, range_at + range.size() * sizeof(int)))) return rc;
  const SicCell *d_cells = reinterpret_cast<const SicCell *>(w.cells.get());
  const int *d_range = reinterpret_cast<const int *>(w.cells.get() + range_at);
  HIPCHK(c, hipMemcpyAsync(w.cells.get() + range_at, range.data(), range.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  const dim3 sub_grid((n_cap + SIC_SUB_THREADS - 1) / SIC_SUB_THREADS, n_buf);
  if (n) {
    if ((rc = w.pbch.reserve(c, pbch.size())) || (rc = w.grid.reserve(c, (size_t)n_sym_all * 72)) || (rc = w.grid_res.reserve(c, (size_t)n_sym_all * 72)) ||
        (rc = w.chan.reserve(c, (size_t)n_slot_all * 4 * 72)) || (rc = w.gain.reserve(c, n)) || (rc = w.td.reserve(c, (size_t)n_sym_all * 128)) ||
        (rc = w.part.reserve(c, (size_t)n_sym_all * 4)) || (rc = w.info.reserve(c, n)))
      return rc;
    HIPCHK(c, hipMemcpyAsync(w.cells.get(), rec.data(), (size_t)n * sizeof(SicCell), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(w.pbch.get(), pbch.data(), pbch.size() * sizeof(float2), hipMemcpyHostToDevice, c->stream));
    // ports beyond n_ports are never read; the estimate's block is cleared so that a stale value cannot be mistaken for one
    HIPCHK(c, hipMemsetAsync(w.chan.get(), 0, (size_t)n_slot_all * 4 * 72 * sizeof(double2), c->stream));
    const dim3 sym_grid((max_sym + 7) / 8, n);
    if (fmt == LCS_FMT_IQ_U8) k_sic_grid<LCS_FMT_IQ_U8><<<sym_grid, 64, 0, c->stream>>>(d_cells, d_cap, 0, w.grid);
    else k_sic_grid<LCS_FMT_C64><<<sym_grid, 64, 0, c->stream>>>(d_cells, d_cap, 0, w.grid);
    k_sic_chan<<<dim3(max_slots, n), SIC_CH_THREADS, 0, c->stream>>>(d_cells, w.grid, c->d_pn_jump, w.chan);
    k_sic_gain<<<n, 64, 0, c->stream>>>(d_cells, w.grid, w.chan, c->d_sss_fd, w.gain);
    k_sic_synth<<<sym_grid, 64, 0, c->stream>>>(d_cells, w.chan, w.gain, w.pbch, c->d_pss_fd, c->d_sss_fd, c->d_pn_jump, mask, w.td, w.part);
  }
  if (fmt == LCS_FMT_IQ_U8) k_sic_sub<LCS_FMT_IQ_U8><<<sub_grid, SIC_SUB_THREADS, 0, c->stream>>>(d_cells, d_range, d_cap, w.td, n_cap, d_res);
  else k_sic_sub<LCS_FMT_C64><<<sub_grid, SIC_SUB_THREADS, 0, c->stream>>>(d_cells, d_range, d_cap, w.td, n_cap, d_res);
  std::vector<lcs_sic_info> got(n);
  if (n) {
    k_sic_grid<LCS_FMT_C64><<<dim3((max_sym + 7) / 8, n), 64, 0, c->stream>>>(d_cells, d_res, 1, w.grid_res);
    k_sic_info<<<n, 64, 0, c->stream>>>(d_cells, w.grid, w.grid_res, w.part, w.gain, w.info);
    HIPCHK(c, hipMemcpyAsync(got.data(), w.info.get(), (size_t)n * sizeof(lcs_sic_info), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));      // the host blocks above are the sources of the copies
  if (info) for (int i = 0; i < n; ++i) { info[where[i]] = got[i]; info[where[i]].ul_dl_config = cfg_used[i]; }
  return LCS_OK;
}
