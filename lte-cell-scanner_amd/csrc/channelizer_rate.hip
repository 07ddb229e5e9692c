// channelizer_rate.hip -- the channelizer at a rational rate change: fs_out = fs_in * U / D, gcd(U, D) = 1, 1 < D / U <= 16
// (include/lcs.h, lcs_channelize_rational).  It is lcs_channelize applied to the capture zero-stuffed by U, with the
// low-pass g of 16 D taps at the fine rate U fs_in; of the U fine samples between two input samples only one is not zero:
//
//     y_k[m] = U sum_n g[m D + Tg-1 - n U] x[n] exp(-i w_k n),      Tg = 16 D,  0 <= m D + Tg-1 - n U < Tg
//
// Write m = q + U i, q = m mod U.  The first sample of output m's window is s_q + i D with s_q = ceil(q D / U), so all
// outputs of one residue q are an integer decimation by D with a filter of their own,
//
//     y_k[q + U i] = exp(-i w_k (s_q + i D)) * sum_j c_q[j] exp(-i w_k j) x[s_q + i D + j],
//     c_q[j] = U g[Tg-1 - ((s_q + j) U - q D)]   where that index is >= 0:  floor or ceil of 16 D / U taps,
//
// i.e. U strided-Toeplitz real GEMMs of the form channelizer.hip runs on the fp32 matrix cores, their outputs interleaved.
// The operand scheme is that kernel's: the (re, im) float stream of the capture is B (one k-step of v_mfma_f32_32x32x2_f32
// = one complex sample), a carrier is the two rows [g_re, -g_im] / [g_im, g_re] of A, a tile is 16 carriers x 32 outputs
// whose windows start D samples apart.  A workgroup (4 waves) owns 16 carriers x the 32 NI U consecutive outputs
// i0 U .. (i0 + 32 NI) U: NI U tiles (tile t: residue t % U, columns i0 + 32 (t / U) + 0..31) dealt to its waves in turn.
// NI is 1 from U = 8 on and grows for small U so that every wave has work.  The 32 NI D + 4 G samples the tiles span are
// converted to float once and staged in LDS as rows of D samples with the odd row stride 2 D + 1 floats -- 36 rows, 37 KB,
// at D = 128 -- so the 32 columns of a B operand fall into 32 banks for every D.  k_chan_rate_tables builds the filter
// rows per call into the context's table in the lane order of the A operand, G groups of four k-steps per residue
// (4 G >= ceil(16 D / U); the taps a residue does not have are zeros, and the samples they meet are staged like any
// other).  The carrier phase of output m is step_k * (s_q + i D) in 64-bit fixed point, wrapped exactly.
#include "channelizer.h"
#include <algorithm>

typedef float cr_f32x16 __attribute__((ext_vector_type(16)));
typedef float cr_f32x4 __attribute__((ext_vector_type(4)));

// the context's table in A-operand lane order (cr_table_value)
__global__ __launch_bounds__(256) void k_chan_rate_tables(const unsigned long long *__restrict__ step, const float *__restrict__ taps,
                                                          int n_ch, int U, int D, int G, int n_rb, float *__restrict__ tab) {
  const size_t total = (size_t)n_rb * U * G * 256;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x)
    tab[e] = cr_table_value(e, step, taps, n_ch, U, D, G);
}

// POW (the 8-bit form): as k_channelize<FMT, true> -- the sum of |y|^2 per carrier over the outputs the workgroup stored goes to
// part[carrier][blockIdx.x]: per lane over its wave's tiles in tile order, then cr_power_partials.
// STREAM (the continuous form): as k_channelize<FMT, POW, true> -- the workgroups start at column sa.i_base of the whole stream, the
// samples come from the history and the chunk (x, n_in), the outputs sa.m_first <= m < sa.m_end are stored at column m - sa.m_first
// of rows sa.row_stride apart; the up to U - 1 outputs of column i_base in front of m_first are computed and dropped.
template <int FMT, bool POW, bool STREAM = false>
__global__ __launch_bounds__(256) void k_channelize_rate(const void *__restrict__ x, unsigned long long n_in, int U, int D, int G, int NI,
                                                         int xrows, const float *__restrict__ tab,
                                                         const unsigned long long *__restrict__ step, int n_ch,
                                                         float2 *__restrict__ out, unsigned n_out, float *__restrict__ part, cs_args sa) {
  extern __shared__ float xs[];      // xrows rows of D samples, row stride 2 D + 1
  unsigned long long i0 = (unsigned long long)blockIdx.x * (32u * NI);
  if constexpr (STREAM) i0 += sa.i_base;
  const int rb = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the samples [i0 D, (i0 + xrows) D) as floats; beyond the capture's end zeros (only zero taps and outputs >= n_out read them)
  const unsigned long long n0 = i0 * (unsigned)D;
  for (int idx = tid; idx < xrows * D; idx += 256) {
    const int o = cr_stage_offset(idx, D);
    const unsigned long long n = n0 + (unsigned)idx;
    float2 v;
    if constexpr (STREAM) v = cs_sample<FMT>(sa.hist, x, cs_source(n, sa.i_base * (unsigned)D, sa.n_hist, n_in));
    else v = n < n_in ? chan_sample<FMT>(x, n) : make_float2(0.f, 0.f);
    xs[o] = v.x;
    xs[o + 1] = v.y;
  }
  __syncthreads();
  float pw[8];      // POW: |y|^2 of the lane's columns per carrier, index v / 2
  if constexpr (POW) {
#pragma unroll
    for (int i = 0; i < 8; ++i) pw[i] = 0.f;
  }
  for (int t = wave; t < U * NI; t += 4) {      // uniform per wave
    const cr_tile tl = cr_tile_of(t, U, D);
    cr_f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    const cr_f32x4 *ap = (const cr_f32x4 *)tab + cr_a_group(rb, tl.q, 0, lane, U, G);
    const float *b = xs + cr_b_base(tl, lane, D);
    cr_pos w = cr_b_first(tl, D);
    cr_f32x4 a_next = ap[0];
    for (int s4 = 0; s4 < G; ++s4) {
      const cr_f32x4 a = a_next;
      a_next = ap[(size_t)std::min(s4 + 1, G - 1) * 64];      // the next four k-steps' operands load under this step's MFMAs
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[cr_b_step(w, D)], acc, 0, 0, 0);
        cr_b_next(w, D);
      }
    }
    const cr_col col = cr_col_of(i0, tl, lane, U, D);
    if constexpr (STREAM) {
      if (col.m < sa.m_first || col.m >= sa.m_end) continue;
    } else if (col.m >= n_out) continue;
#pragma unroll
    for (int v = 0; v < 16; v += 2) {      // registers v, v + 1: (re, im) of one carrier (cr_acc_row)
      const int ch = cr_acc_carrier(rb, v, lane);
      if (ch >= n_ch) continue;
      const float2 y = cr_rotate(acc[v], acc[v + 1], step[ch], col.nd);
      if constexpr (STREAM) out[(size_t)ch * sa.row_stride + (col.m - sa.m_first)] = y;
      else out[(size_t)ch * n_out + col.m] = y;
      if constexpr (POW) pw[v >> 1] += y.x * y.x + y.y * y.y;
    }
  }
  if constexpr (POW) cr_power_partials(pw, rb, n_ch, part);
}

// The rational form's part of lcs_launch_channelize (channelizer.hip): a kernel is launched from the file that holds it
void lcs_chan_rate_enqueue(lcs_ctx *c, const ChanCall &a, const cr_geom &geo, dim3 tab_grid, dim3 grid, const unsigned long long *d_step,
                           const float *d_taps, float *d_part) {
  hipLaunchKernelGGL(k_chan_rate_tables, tab_grid, dim3(256), 0, c->stream, d_step, d_taps, a.n_ch, a.up, a.down, geo.G, (int)grid.y, c->chan_tab);
  chan_by_form(a.fmt, d_part != nullptr, [&](auto fmt, auto pow) {
    hipLaunchKernelGGL((k_channelize_rate<decltype(fmt)::value, decltype(pow)::value>), grid, dim3(256), geo.lds_bytes, c->stream, a.d_wide,
                       (unsigned long long)a.n_in, a.up, a.down, geo.G, geo.NI, geo.xrows, (const float *)c->chan_tab, d_step, a.n_ch, (float2 *)a.d_out,
                       (unsigned)a.n_out, d_part, cs_args{});
  });
}

// The continuous form's two launches of this file's kernels (channelizer.hip: lcs_chan_stream_start, lcs_chan_stream_enqueue)
void lcs_chan_rate_tables_enqueue(lcs_ctx *c, int n_ch, int up, int down, const cr_geom &geo, dim3 tab_grid, int n_rb, const unsigned long long *d_step,
                                  const float *d_taps, float *d_tab) {
  hipLaunchKernelGGL(k_chan_rate_tables, tab_grid, dim3(256), 0, c->stream, d_step, d_taps, n_ch, up, down, geo.G, n_rb, d_tab);
}
void lcs_chan_rate_stream_enqueue(lcs_ctx *c, int fmt, const void *d_chunk, uint64_t n_chunk, int up, int down, const cr_geom &geo, dim3 grid,
                                  const float *d_tab, const unsigned long long *d_step, int n_ch, float2 *d_out, const cs_args &sa) {
  chan_by_form(fmt, false, [&](auto f, auto) {
    hipLaunchKernelGGL((k_channelize_rate<decltype(f)::value, false, true>), grid, dim3(256), geo.lds_bytes, c->stream, d_chunk,
                       (unsigned long long)n_chunk, up, down, geo.G, geo.NI, geo.xrows, d_tab, d_step, n_ch, d_out, 0u, (float *)nullptr, sa);
  });
}
