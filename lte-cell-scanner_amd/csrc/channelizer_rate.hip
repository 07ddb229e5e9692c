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
// part[carrier][blockIdx.x]: per lane over its wave's tiles in tile order, over the 32 columns by lane exchanges, over the waves
// through LDS in wave order.
template <int FMT, bool POW>
__global__ __launch_bounds__(256) void k_channelize_rate(const void *__restrict__ x, unsigned long long n_in, int U, int D, int G, int NI,
                                                         int xrows, const float *__restrict__ tab,
                                                         const unsigned long long *__restrict__ step, int n_ch,
                                                         float2 *__restrict__ out, unsigned n_out, float *__restrict__ part) {
  extern __shared__ float xs[];      // xrows rows of D samples, row stride 2 D + 1
  const unsigned long long i0 = (unsigned long long)blockIdx.x * (32u * NI);
  const int rb = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the samples [i0 D, (i0 + xrows) D) as floats; beyond the capture's end zeros (only zero taps and outputs >= n_out read them)
  const unsigned long long n0 = i0 * (unsigned)D;
  for (int idx = tid; idx < xrows * D; idx += 256) {
    const int o = cr_stage_offset(idx, D);
    const unsigned long long n = n0 + (unsigned)idx;
    const float2 v = n < n_in ? chan_sample<FMT>(x, n) : make_float2(0.f, 0.f);
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
    if (col.m >= n_out) continue;
#pragma unroll
    for (int v = 0; v < 16; v += 2) {      // registers v, v + 1: (re, im) of one carrier (cr_acc_row)
      const int ch = cr_acc_carrier(rb, v, lane);
      if (ch >= n_ch) continue;
      const float2 y = cr_rotate(acc[v], acc[v + 1], step[ch], col.nd);
      out[(size_t)ch * n_out + col.m] = y;
      if constexpr (POW) pw[v >> 1] += y.x * y.x + y.y * y.y;
    }
  }
  if constexpr (POW) {
    __shared__ float red[4][CR_CARRIERS];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float v = pw[i];
#pragma unroll
      for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o);      // within the lane's half: the 32 columns of its carriers
      if ((lane & 31) == 0) red[wave][cr_acc_row(2 * i, lane) >> 1] = v;
    }
    __syncthreads();
    const int ch = rb * CR_CARRIERS + tid;
    if (tid < CR_CARRIERS && ch < n_ch) part[(size_t)ch * gridDim.x + blockIdx.x] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  }
}

unsigned lcs_chan_rate_blocks(uint32_t n_out, int up, int down) { return cr_grid_x(n_out, up, cr_geometry(up, down).NI); }

template <int FMT>
static void chan_rate_launch(lcs_ctx *c, dim3 grid, size_t lds_bytes, const void *d_wide, unsigned long long n_in, int up, int down, const cr_geom &geo,
                             const unsigned long long *d_step, int n_ch, void *d_out, unsigned n_out, float *d_part) {
  if (d_part)
    hipLaunchKernelGGL((k_channelize_rate<FMT, true>), grid, dim3(256), lds_bytes, c->stream, d_wide, n_in, up, down, geo.G, geo.NI, geo.xrows,
                       (const float *)c->chan_tab, d_step, n_ch, (float2 *)d_out, n_out, d_part);
  else
    hipLaunchKernelGGL((k_channelize_rate<FMT, false>), grid, dim3(256), lds_bytes, c->stream, d_wide, n_in, up, down, geo.G, geo.NI, geo.xrows,
                       (const float *)c->chan_tab, d_step, n_ch, (float2 *)d_out, n_out, d_part);
}

int lcs_launch_channelize_rational(lcs_ctx *c, const void *d_wide, int fmt, uint64_t n_in, double fs_in, int up, int down,
                                   const double *f_shift, int n_ch, void *d_out, uint32_t n_out, float *d_part) {
  const int Tg = 16 * down, n_rb = (n_ch + CR_CARRIERS - 1) / CR_CARRIERS;
  const cr_geom geo = cr_geometry(up, down);
  const int G = geo.G, ni = geo.NI;
  const size_t lds_bytes = geo.lds_bytes;
  const size_t par_bytes = (size_t)n_ch * sizeof(unsigned long long) + 16 * 128 * sizeof(float);
  const size_t tab_floats = (size_t)n_rb * up * G * 256;
  int k = 0, rc;
  if (par_bytes > c->chan_par.capacity() || tab_floats > c->chan_tab.capacity())      // grown on demand (earlier calls may still read the old ones)
    HIPCHK(c, hipStreamSynchronize(c->stream));
  if ((rc = c->chan_par.reserve(c, par_bytes)) || (rc = c->chan_tab.reserve(c, tab_floats))) return rc;
  if (!c->ev_chan0) {
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_chan0, LCS_EVENT_NOFENCE));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_chan1, LCS_EVENT_NOFENCE));
  }
  if ((rc = lcs_chan_slot(c, par_bytes, &k))) return rc;
  unsigned long long *h_step = reinterpret_cast<unsigned long long *>(c->chan_hpin[k].get());
  float *h_taps = (float *)(h_step + n_ch);
  for (int i = 0; i < n_ch; ++i) h_step[i] = lcs_chan_step(f_shift[i], fs_in);
  double taps[16 * 128];
  lcs_chan_taps(down, taps);
  for (int t = 0; t < Tg; ++t) h_taps[t] = (float)taps[t];
  const size_t upl = (size_t)n_ch * sizeof(unsigned long long) + Tg * sizeof(float);
  HIPCHK(c, hipMemcpyAsync(c->chan_par, h_step, upl, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(c->ev_chan_slot[k], c->stream));
  const unsigned long long *d_step = reinterpret_cast<const unsigned long long *>(c->chan_par.get());
  const float *d_taps = (const float *)(d_step + n_ch);
  HIPCHK(c, hipEventRecord(c->ev_chan0, c->stream));
  const int tab_grid = (int)std::min<size_t>((tab_floats + 255) / 256, 2048);
  hipLaunchKernelGGL(k_chan_rate_tables, dim3(tab_grid), dim3(256), 0, c->stream, d_step, d_taps, n_ch, up, down, G, n_rb, c->chan_tab);
  const dim3 grid(cr_grid_x(n_out, up, ni), n_rb);
  if (fmt == LCS_FMT_C64) chan_rate_launch<LCS_FMT_C64>(c, grid, lds_bytes, d_wide, n_in, up, down, geo, d_step, n_ch, d_out, n_out, d_part);
  else if (fmt == LCS_FMT_IQ_S16) chan_rate_launch<LCS_FMT_IQ_S16>(c, grid, lds_bytes, d_wide, n_in, up, down, geo, d_step, n_ch, d_out, n_out, d_part);
  else chan_rate_launch<LCS_FMT_IQ_S8>(c, grid, lds_bytes, d_wide, n_in, up, down, geo, d_step, n_ch, d_out, n_out, d_part);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev_chan1, c->stream));
  c->chan_timed = true;
  return LCS_OK;
}
