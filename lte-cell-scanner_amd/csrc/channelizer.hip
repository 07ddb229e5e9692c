// channelizer.hip -- wideband channelizer: one wideband capture in HBM -> n_ch narrowband buffers at fs_in / D, each the
// input mixed down by its carrier's shift, low-passed by the fixed T = 16 D tap filter and decimated (include/lcs.h,
// lcs_channelize).  Output k, sample m:
//
//     y_k[m] = sum_t h[t] x[mD + T-1-t] exp(-i w_k (mD + T-1-t))
//            = exp(-i w_k mD) * sum_j g_k[j] x[mD + j],          g_k[j] = h[T-1-j] exp(-i w_k j),  j = T-1-t
//
// The sum is a strided-Toeplitz GEMM and runs on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 products, a
// k-ordered fma chain).  As a REAL product: the interleaved (re, im) float stream xf of the capture is the B operand as it
// stands -- B[kk][m] = xf[2 D m + kk], kk = 2 j + c -- and a carrier is two rows of A over kk:
//     row (k, re): [ g_re(j), -g_im(j) ]      row (k, im): [ g_im(j),  g_re(j) ]
// A tile of A is 32 rows = 16 carriers; a workgroup (4 waves) owns 16 carriers x 256 outputs, each wave two 32 x 32 tiles
// that share one A operand.  The (256 + 15) D input samples the workgroup's windows span are converted to float once and
// staged in LDS as rows of D samples with an odd row stride (2 D + 1 floats): lane (m, c) of a B operand reads row
// m + j / D, column 2 (j % D) + c, so the 32 columns of a tile fall into different banks for every D.  The filter bank
// k_chan_tables builds per call sits in the context's table in the lane order of the A operand, four k-steps to a
// 16-byte load, and is read through the caches (64 KB per 16 carriers at D = 16, the same for every workgroup of a row
// block).  The carrier phase of output m is step_k * (m D) in 64-bit fixed point (2^64 = one turn), wrapped exactly; its
// top 32 bits feed sinpif / cospif.  The per-tap phases of g_k come from the same accumulator through double sinpi / cospi.
#include "channelizer.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

typedef float ch_f32x16 __attribute__((ext_vector_type(16)));
typedef float ch_f32x4 __attribute__((ext_vector_type(4)));

#define CH_SMAX (2 * 16 + 1)           // row stride in floats at D = 16

// Kaiser window's I0 by its power series (x <= 7.75: 40 terms reach 1e-17 relative)
static double chan_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 64; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

// h[t] = sinc((t - (T-1)/2) / D) * kaiser(T, 7.75)[t], normalised to sum 1 (include/lcs.h)
void lcs_chan_taps(int decim, double *taps) {
  const int T = 16 * decim;
  const double alpha = 0.5 * (T - 1), beta = 7.75, i0b = chan_i0(beta);
  double sum = 0;
  for (int t = 0; t < T; ++t) {
    const double y = M_PI * ((t - alpha) / decim);      // never 0: T is even
    const double r = (t - alpha) / alpha;
    taps[t] = std::sin(y) / y * (chan_i0(beta * std::sqrt(1.0 - r * r)) / i0b);
    sum += taps[t];
  }
  for (int t = 0; t < T; ++t) taps[t] /= sum;
}

// 2^64 x frac(df / fs_in), |df / fs_in| <= 1/2 (two's complement: a negative shift is its own wrap-around)
unsigned long long lcs_chan_step(double f_shift, double fs_in) {
  const double v = std::ldexp(f_shift / fs_in, 64);
  if (v >= 0x1p63) return 1ull << 63;
  return (unsigned long long)(long long)std::llrint(v);
}

// The filter bank in A-operand order: tab[((rb * T/4 + s4) * 64 + lane) * 4 + i] = A[row lane & 31 of block rb][kk = 2 (4 s4 + i) + (lane >> 5)]
__global__ __launch_bounds__(256) void k_chan_tables(const unsigned long long *__restrict__ step, const float *__restrict__ taps,
                                                     int n_ch, int D, int n_rb, float *__restrict__ tab) {
  const int T = 16 * D, q4 = T / 4;
  const size_t total = (size_t)n_rb * T * 64;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(e & 3), l = (int)((e >> 2) & 63);
    const size_t rest = e >> 8;
    const int s4 = (int)(rest % q4), rb = (int)(rest / q4);
    const int s = 4 * s4 + i, r = l & 31, c = l >> 5;
    const int ch = rb * CR_CARRIERS + (r >> 1), ri = r & 1;
    float v = 0.f;
    if (ch < n_ch) {
      const unsigned long long ph = step[ch] * (unsigned long long)s;
      const double ht = 2.0 * ((double)(long long)ph * 0x1p-64);      // half-turns, [-1, 1)
      const double h = (double)taps[T - 1 - s];
      const double g_re = h * cospi(ht), g_im = -h * sinpi(ht);
      v = (float)(ri == 0 ? (c == 0 ? g_re : -g_im) : (c == 0 ? g_im : g_re));
    }
    tab[e] = v;
  }
}

// POW (the 8-bit form, lcs_channelize_u8): the workgroup also leaves, per carrier, the sum of |y|^2 over the outputs it stored in
// part[carrier][blockIdx.x] -- per lane over its two tiles, then cr_power_partials.
// STREAM (the continuous form, lcs_chan_stream_push): a push's launch.  Every index is one of the whole stream: the workgroups start
// at output sa.i_base (the stream's m_first at up == 1), the staged samples come from the stream's history and the chunk behind it
// (x, n_in: the chunk and its length; cs_source), and only the outputs sa.m_first <= m < sa.m_end are stored, at column
// m - sa.m_first of rows sa.row_stride apart.  A column's A rows, its samples and its k order are those of the one-shot launch,
// wherever in a workgroup it sits.  The one-shot instantiations read nothing of sa.
template <int FMT, bool POW, bool STREAM = false>
__global__ __launch_bounds__(256) void k_channelize(const void *__restrict__ x, unsigned long long n_in, int D,
                                                    const float *__restrict__ tab, const unsigned long long *__restrict__ step,
                                                    int n_ch, float2 *__restrict__ out, unsigned n_out, float *__restrict__ part, cs_args sa) {
  __shared__ float xs[CH_XROWS * CH_SMAX];
  const int S = 2 * D + 1, T = 16 * D;
  using index_t = std::conditional_t<STREAM, unsigned long long, unsigned>;
  index_t m0 = blockIdx.x * CH_NT;
  if constexpr (STREAM) m0 += sa.i_base;
  const int rb = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the samples [m0 D, (m0 + CH_XROWS) D) as floats; beyond the capture's end zeros (only outputs >= n_out read them)
  const unsigned long long n0 = (unsigned long long)m0 * D;
  for (int idx = tid; idx < CH_XROWS * D; idx += 256) {
    const int o = cr_stage_offset(idx, D);
    const unsigned long long n = n0 + (unsigned)idx;
    float2 v;
    if constexpr (STREAM) v = cs_sample<FMT>(sa.hist, x, cs_source(n, sa.i_base * (unsigned)D, sa.n_hist, n_in));
    else v = n < n_in ? chan_sample<FMT>(x, n) : make_float2(0.f, 0.f);
    xs[o] = v.x;
    xs[o + 1] = v.y;
  }
  __syncthreads();
  ch_f32x16 acc0, acc1;
#pragma unroll
  for (int v = 0; v < 16; ++v) { acc0[v] = 0.f; acc1[v] = 0.f; }
  const ch_f32x4 *ap = (const ch_f32x4 *)tab + (size_t)rb * (T / 4) * 64 + lane;
  const float *b0 = xs + (wave * 64 + (lane & 31)) * S + (lane >> 5);
  const float *b1 = b0 + 32 * S;
  int q = 0, p = 0;      // k-step s = q D + p (uniform)
  ch_f32x4 a_next = ap[0];
  for (int s4 = 0; s4 < T / 4; ++s4) {
    const ch_f32x4 a = a_next;
    a_next = ap[(size_t)std::min(s4 + 1, T / 4 - 1) * 64];      // the next four k-steps' operands load under this step's MFMAs
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int off = q * S + 2 * p;
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b0[off], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b1[off], acc1, 0, 0, 0);
      if (++p == D) { p = 0; ++q; }
    }
  }
  float pw[8];      // POW: |y|^2 of the lane's columns per carrier, index v / 2
  if constexpr (POW) {
#pragma unroll
    for (int i = 0; i < 8; ++i) pw[i] = 0.f;
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const index_t m = m0 + wave * 64 + t * 32 + (lane & 31);
    if constexpr (STREAM) {
      if (m < sa.m_first || m >= sa.m_end) continue;
    } else if (m >= n_out) continue;
    const unsigned long long nd = (unsigned long long)m * (unsigned)D;
#pragma unroll
    for (int v = 0; v < 16; v += 2) {      // registers v, v + 1: (re, im) of one carrier (cr_acc_row)
      const int ch = cr_acc_carrier(rb, v, lane);
      if (ch >= n_ch) continue;
      const float2 y = cr_rotate(t ? acc1[v] : acc0[v], t ? acc1[v + 1] : acc0[v + 1], step[ch], nd);
      if constexpr (STREAM) out[(size_t)ch * sa.row_stride + (m - sa.m_first)] = y;
      else out[(size_t)ch * n_out + m] = y;
      if constexpr (POW) pw[v >> 1] += y.x * y.x + y.y * y.y;
    }
  }
  if constexpr (POW) cr_power_partials(pw, rb, n_ch, part);
}

// The continuous form's history: behind a push's main kernel, the n_keep samples from the next aligned base on (sample `skip` of
// [history ++ chunk]) go into the OTHER history slot -- a short chunk leaves part of the old history needed, so the two never
// alias.  Samples travel as the w 16-bit units they are made of (1, 2, 4: s8, s16, c64); one workgroup, at most cs_keep_max samples.
__global__ __launch_bounds__(256) void k_chan_keep(const uint16_t *__restrict__ hist, const uint16_t *__restrict__ chunk, unsigned n_hist,
                                                   unsigned long long n_chunk, unsigned long long skip, unsigned n_keep, unsigned w,
                                                   uint16_t *__restrict__ dst) {
  for (unsigned e = threadIdx.x; e < n_keep * w; e += 256) {
    const unsigned s = e / w, u = e - s * w;
    const cs_where from = cs_source(skip + s, 0, n_hist, n_chunk);
    dst[e] = from.part == CS_ZERO ? (uint16_t)0 : (from.part == CS_HIST ? hist : chunk)[from.off * w + u];
  }
}

// The 8-bit output (include/lcs.h, lcs_channelize_u8): carrier ch's floats y[ch][n_out] -> bytes out[ch][n_out][2].  Every workgroup
// sums its carrier's power partials in double in index order (one lane; the same bits in every workgroup of the carrier), takes the
// exponent and hands the gain 2^e round through LDS.  A row of bytes starts 2 n_out bytes behind the last, at any even address: its
// interior is cut into groups of 8 samples from the first 16-byte boundary on -- a lane reads a group as four 16-byte loads (the
// floats are 8-byte aligned) and stores it as one 16-byte store -- and the up to 7 samples in front of the first and behind the last
// whole group go out as 2-byte stores from the row's first workgroup.  Memory-bound: 8 bytes in, 2 out per sample.
#define CQ_GROUPS 2048                 // groups of 8 samples per workgroup: 8 per lane
typedef float cq_f32x4 __attribute__((ext_vector_type(4), aligned(8)));

__global__ __launch_bounds__(256) void k_chan_quant_u8(const float2 *__restrict__ y, const float *__restrict__ part, int n_blocks, unsigned n_out,
                                                       unsigned n_xb, uint8_t *__restrict__ out, float *__restrict__ gain) {
  __shared__ float s_gain;
  const unsigned ch = blockIdx.x / n_xb, xb = blockIdx.x - ch * n_xb;
  const int tid = threadIdx.x;
  if (tid == 0) {
    const float *p = part + (size_t)ch * n_blocks;
    double P = 0.0;
    for (int i = 0; i < n_blocks; ++i) P += (double)p[i];
    const float g = ldexpf(1.f, chan_u8_exponent(P / (double)n_out));
    s_gain = g;
    if (gain && xb == 0) gain[ch] = g;
  }
  __syncthreads();
  const float g = s_gain;
  const float2 *row = y + (size_t)ch * n_out;
  uint8_t *orow = out + (size_t)ch * n_out * 2;
  const unsigned to_16 = (unsigned)((16u - (unsigned)(reinterpret_cast<uintptr_t>(orow) & 15u)) & 15u) >> 1;      // samples up to the boundary
  const unsigned head = to_16 < n_out ? to_16 : n_out;
  const unsigned n_g = (n_out - head) >> 3, tail = head + 8u * n_g;
  const unsigned g_end = (xb + 1u) * CQ_GROUPS < n_g ? (xb + 1u) * CQ_GROUPS : n_g;
  for (unsigned gi = xb * CQ_GROUPS + tid; gi < g_end; gi += 256) {
    const unsigned s0 = head + 8u * gi;      // s0 + 7 < tail <= n_out
    const cq_f32x4 *src = reinterpret_cast<const cq_f32x4 *>(row + s0);
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const cq_f32x4 f = src[j];
      w[j] = chan_u8_code(g * f[0]) | (chan_u8_code(g * f[1]) << 8) | (chan_u8_code(g * f[2]) << 16) | (chan_u8_code(g * f[3]) << 24);
    }
    *reinterpret_cast<uint4 *>(orow + 2 * (size_t)s0) = make_uint4(w[0], w[1], w[2], w[3]);
  }
  if (xb == 0 && tid < 16) {      // lanes 0..7: the samples in front of the first group; 8..15: those behind the last
    const unsigned s = tid < 8 ? (unsigned)tid : tail + (unsigned)(tid - 8);
    if (tid < 8 ? s < head : s < n_out) {
      const float2 f = row[s];
      *reinterpret_cast<uint16_t *>(orow + 2 * (size_t)s) = (uint16_t)(chan_u8_code(g * f.x) | (chan_u8_code(g * f.y) << 8));
    }
  }
}

// floats y[n_ch][n_out] and their power partials part[n_ch][n_blocks] -> bytes and gains
static int chan_quant_enqueue(lcs_ctx *c, const float2 *y, const float *part, unsigned n_blocks, int n_ch, unsigned n_out, void *d_out, float *d_gain) {
  const unsigned n_xb = std::max(1u, (n_out / 8 + CQ_GROUPS - 1) / CQ_GROUPS);
  hipLaunchKernelGGL(k_chan_quant_u8, dim3((unsigned)n_ch * n_xb), dim3(256), 0, c->stream, y, part, (int)n_blocks, n_out, n_xb, (uint8_t *)d_out, d_gain);
  HIPCHK(c, hipGetLastError());
  return LCS_OK;
}

// The power of a finished capture of the stream (include/lcs.h, lcs_chan_stream_push_u8): part[ch][block] = the sum of |y|^2 over block
// `block` of row ch of y[n_ch][n_out], for k_chan_quant_u8 to add up.  A block is CP_PAIRS pairs of samples from the row's start on,
// whatever launch computed them, so the sum's order depends on n_out alone: lane t takes the pairs t, t + 256, t + 512, t + 768 of its
// block -- four 16-byte loads in flight (a row starts at any 8-byte address) -- squares and adds them in that order in fp32, the wave
// adds its lanes by a butterfly of lane exchanges, the four waves meet in LDS in wave order.  The odd last sample of a row counts as
// the pair behind the last whole one.  No atomics; 8 bytes in per sample.  y holds one more sample than its rows (see the loads).
#define CP_ILP 4
#define CP_PAIRS (256 * CP_ILP)
static unsigned cap_power_blocks(unsigned n_out) { return ((n_out + 1) / 2 + CP_PAIRS - 1) / CP_PAIRS; }

__global__ __launch_bounds__(256) void k_chan_cap_power(const float2 *__restrict__ y, unsigned n_out, float *__restrict__ part) {
  __shared__ float red[4];
  const float2 *row = y + (size_t)blockIdx.y * n_out;
  const cq_f32x4 *row4 = reinterpret_cast<const cq_f32x4 *>(row);
  const unsigned n2 = n_out >> 1, i0 = blockIdx.x * CP_PAIRS + threadIdx.x, last = n2 ? n2 - 1 : 0;
  cq_f32x4 v[CP_ILP];
#pragma unroll
  for (int k = 0; k < CP_ILP; ++k) v[k] = row4[std::min(i0 + 256u * k, last)];      // unconditional (a branch per load would serialise them): the
  // tail reads the last pair again, and a row of ONE sample reads 8 bytes behind itself -- y has one sample of padding behind its last row
  const float2 f = row[n_out - 1];
  const float tail = (n_out & 1u) ? f.x * f.x + f.y * f.y : 0.f;      // the odd last sample: pair n2
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < CP_ILP; ++k) {
    const unsigned i = i0 + 256u * k;
    const float pair = (v[k][0] * v[k][0] + v[k][1] * v[k][1]) + (v[k][2] * v[k][2] + v[k][3] * v[k][3]);
    s += i < n2 ? pair : (i == n2 ? tail : 0.f);      // selected, not multiplied: what a lane beyond the row's end loaded may be anything
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// One call's parameters on their way to the device: [n_ch] phase steps, then T taps as float.  Two page-locked slots used in
// turn, each guarded by the event behind its copy, so a call never waits for the GPU unless three calls are in flight.
int lcs_chan_slot(lcs_ctx *c, size_t bytes, int *slot) {
  const int k = c->chan_slot ^= 1;
  if (!c->ev_chan_slot[k]) HIPCHK(c, hipEventCreateWithFlags(&c->ev_chan_slot[k], hipEventDisableTiming));
  else HIPCHK(c, hipEventSynchronize(c->ev_chan_slot[k]));
  *slot = k;
  return c->chan_hpin[k].reserve(c, bytes);
}

// workgroups along the outputs
unsigned lcs_chan_blocks(const ChanCall &a) {
  return a.up == 1 ? (a.n_out + CH_NT - 1) / CH_NT : cr_grid_x(a.n_out, a.up, cr_geometry(a.up, a.down).NI);
}

void lcs_chan_rate_enqueue(lcs_ctx *c, const ChanCall &a, const cr_geom &geo, dim3 tab_grid, dim3 grid, const unsigned long long *d_step,
                           const float *d_taps, float *d_part);      // channelizer_rate.hip

// Every form's launch: parameters up, the form's table kernel, its main kernel, the two events the call's time is taken between.
// The filter bank has 256 up G floats per row block in both forms (G = 4 down at up == 1: the 16 down taps).
int lcs_launch_channelize(lcs_ctx *c, const ChanCall &a, float *d_part) {
  const int T = 16 * a.down, n_ch = a.n_ch, n_rb = (n_ch + CR_CARRIERS - 1) / CR_CARRIERS;
  const cr_geom geo = cr_geometry(a.up, a.down);
  const size_t par_bytes = (size_t)n_ch * sizeof(unsigned long long) + 16 * 128 * sizeof(float);
  const size_t tab_floats = (size_t)n_rb * a.up * geo.G * 256;
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
  for (int i = 0; i < n_ch; ++i) h_step[i] = lcs_chan_step(a.f_shift[i], a.fs_in);
  double taps[16 * 128];
  lcs_chan_taps(a.down, taps);
  for (int t = 0; t < T; ++t) h_taps[t] = (float)taps[t];
  const size_t upl = (size_t)n_ch * sizeof(unsigned long long) + T * sizeof(float);
  HIPCHK(c, hipMemcpyAsync(c->chan_par, h_step, upl, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(c->ev_chan_slot[k], c->stream));
  const unsigned long long *d_step = reinterpret_cast<const unsigned long long *>(c->chan_par.get());
  const float *d_taps = (const float *)(d_step + n_ch);
  HIPCHK(c, hipEventRecord(c->ev_chan0, c->stream));
  const dim3 tab_grid((unsigned)std::min<size_t>((tab_floats + 255) / 256, 2048)), grid(lcs_chan_blocks(a), n_rb);
  if (a.up == 1) {
    hipLaunchKernelGGL(k_chan_tables, tab_grid, dim3(256), 0, c->stream, d_step, d_taps, n_ch, a.down, n_rb, c->chan_tab);
    chan_by_form(a.fmt, d_part != nullptr, [&](auto fmt, auto pow) {
      hipLaunchKernelGGL((k_channelize<decltype(fmt)::value, decltype(pow)::value>), grid, dim3(256), 0, c->stream, a.d_wide,
                         (unsigned long long)a.n_in, a.down, (const float *)c->chan_tab, d_step, n_ch, (float2 *)a.d_out, (unsigned)a.n_out, d_part,
                         cs_args{});
    });
  } else {
    lcs_chan_rate_enqueue(c, a, geo, tab_grid, grid, d_step, d_taps, d_part);
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev_chan1, c->stream));
  c->chan_timed = true;
  return LCS_OK;
}

// The 8-bit form: the float form writes the context's scratch and the power partials, and k_chan_quant_u8 turns the scratch into
// the caller's bytes.  The scratch grows on demand like the filter bank: one stream synchronisation, because an earlier call's
// kernels may still read the old block.
int lcs_launch_channelize_u8(lcs_ctx *c, const ChanCall &a, float *d_gain) {
  const unsigned n_blocks = lcs_chan_blocks(a), n_out = a.n_out;
  const size_t y_elems = (size_t)a.n_ch * n_out, part_elems = (size_t)a.n_ch * n_blocks;
  int rc;
  if (y_elems > c->chan_y.capacity() || part_elems > c->chan_part.capacity()) HIPCHK(c, hipStreamSynchronize(c->stream));
  if ((rc = c->chan_y.reserve(c, y_elems)) || (rc = c->chan_part.reserve(c, part_elems))) return rc;
  ChanCall y = a;
  y.d_out = c->chan_y;
  if ((rc = lcs_launch_channelize(c, y, c->chan_part))) return rc;
  if ((rc = chan_quant_enqueue(c, c->chan_y, c->chan_part, n_blocks, a.n_ch, n_out, a.d_out, d_gain))) return rc;
  HIPCHK(c, hipEventRecord(c->ev_chan1, c->stream));      // the call's time runs through its last kernel
  return LCS_OK;
}

// ---- the continuous form (include/lcs.h, lcs_chan_stream_open).  open builds what depends on the carriers and the rate only --
// steps, taps, the A-operand table -- once, into buffers of the stream's own; a push launches its main kernel over the columns
// that hold its outputs and the history append, and carries its scalars as kernel arguments.
void lcs_chan_rate_tables_enqueue(lcs_ctx *c, int n_ch, int up, int down, const cr_geom &geo, dim3 tab_grid, int n_rb, const unsigned long long *d_step,
                                  const float *d_taps, float *d_tab);      // channelizer_rate.hip
void lcs_chan_rate_stream_enqueue(lcs_ctx *c, int fmt, const void *d_chunk, uint64_t n_chunk, int up, int down, const cr_geom &geo, dim3 grid,
                                  const float *d_tab, const unsigned long long *d_step, int n_ch, float2 *d_out, const cs_args &sa);

static void chan_stream_drop(lcs_ctx *c) {
  lcs_ctx::ChanStream &st = c->chan_stream;
  st.par.reset(), st.tab.reset(), st.hist[0].reset(), st.hist[1].reset(), st.cap.reset(), st.cap_part.reset();
  st.open = st.u8 = false;
}

int lcs_chan_stream_start(lcs_ctx *c, int fmt, double fs_in, int up, int down, const double *f_shift, int n_ch) {
  lcs_ctx::ChanStream &st = c->chan_stream;
  const int T = 16 * down, n_rb = (n_ch + CR_CARRIERS - 1) / CR_CARRIERS;
  const cr_geom geo = cr_geometry(up, down);
  const size_t par_bytes = (size_t)n_ch * sizeof(unsigned long long) + (size_t)T * sizeof(float);
  const size_t tab_floats = (size_t)n_rb * up * geo.G * 256, hist_bytes = (size_t)cs_keep_max(up, down) * chan_sample_bytes(fmt);
  int rc;
  if ((rc = st.par.alloc(c, par_bytes)) || (rc = st.tab.alloc(c, tab_floats)) || (rc = st.hist[0].alloc(c, hist_bytes)) ||
      (rc = st.hist[1].alloc(c, hist_bytes))) {
    chan_stream_drop(c);
    return rc;
  }
  std::vector<char> h(par_bytes);
  unsigned long long *h_step = reinterpret_cast<unsigned long long *>(h.data());
  float *h_taps = reinterpret_cast<float *>(h_step + n_ch);
  for (int i = 0; i < n_ch; ++i) h_step[i] = lcs_chan_step(f_shift[i], fs_in);
  double taps[16 * 128];
  lcs_chan_taps(down, taps);
  for (int t = 0; t < T; ++t) h_taps[t] = (float)taps[t];
  const unsigned long long *d_step = reinterpret_cast<const unsigned long long *>(st.par.get());
  const float *d_taps = reinterpret_cast<const float *>(d_step + n_ch);
  const dim3 tab_grid((unsigned)std::min<size_t>((tab_floats + 255) / 256, 2048));
  hipError_t e = hipMemcpyAsync(st.par, h.data(), par_bytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    if (up == 1) hipLaunchKernelGGL(k_chan_tables, tab_grid, dim3(256), 0, c->stream, d_step, d_taps, n_ch, down, n_rb, st.tab.get());
    else lcs_chan_rate_tables_enqueue(c, n_ch, up, down, geo, tab_grid, n_rb, d_step, d_taps, st.tab);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);      // h is ordinary memory that goes with this call; once per stream
  if (e != hipSuccess) {
    chan_stream_drop(c);
    return lcs_hip_error(c, "lcs_chan_stream_open", e);
  }
  st.fmt = fmt, st.up = up, st.down = down, st.n_ch = n_ch;
  st.cur = 0, st.n_hist = 0, st.n_total = 0;
  st.u8 = false, st.n_cap = 0, st.filled = 0;
  st.open = true;
  return LCS_OK;
}

// The stream of 8-bit captures: the float stream plus the capture in hand.  A failed allocation drops the whole stream.
int lcs_chan_stream_start_u8(lcs_ctx *c, int fmt, double fs_in, int up, int down, const double *f_shift, int n_ch, uint32_t n_cap) {
  lcs_ctx::ChanStream &st = c->chan_stream;
  int rc;
  if ((rc = lcs_chan_stream_start(c, fmt, fs_in, up, down, f_shift, n_ch))) return rc;
  if ((rc = st.cap.alloc(c, (size_t)n_ch * n_cap + 1)) || (rc = st.cap_part.alloc(c, (size_t)n_ch * cap_power_blocks(n_cap)))) {
    chan_stream_drop(c);
    return rc;
  }
  st.u8 = true, st.n_cap = n_cap;
  return LCS_OK;
}

// One push, already found acceptable: nothing here can refuse.  The stream moves on only when both launches were taken.
int lcs_chan_stream_enqueue(lcs_ctx *c, const void *d_chunk, uint64_t n_chunk, void *d_out, uint32_t row_stride) {
  lcs_ctx::ChanStream &st = c->chan_stream;
  if (!n_chunk) return LCS_OK;      // nothing new: the outputs, the base and the history stay what they are
  const cr_geom geo = cr_geometry(st.up, st.down);
  const cs_plan p = cs_plan_push(st.n_total, n_chunk, st.up, st.down, st.up == 1 ? CH_NT : 32 * geo.NI);
  const int n_rb = (st.n_ch + CR_CARRIERS - 1) / CR_CARRIERS;
  const unsigned long long *d_step = reinterpret_cast<const unsigned long long *>(st.par.get());
  const void *hist = st.hist[st.cur].get();
  if (p.grid_x) {
    const cs_args sa = {hist, p.i_base, st.n_hist, p.m_first, p.m_end, row_stride};
    const dim3 grid(p.grid_x, n_rb);
    if (st.up == 1) {
      chan_by_form(st.fmt, false, [&](auto fmt, auto) {
        hipLaunchKernelGGL((k_channelize<decltype(fmt)::value, false, true>), grid, dim3(256), 0, c->stream, d_chunk, (unsigned long long)n_chunk,
                           st.down, (const float *)st.tab, d_step, st.n_ch, (float2 *)d_out, 0u, (float *)nullptr, sa);
      });
    } else {
      lcs_chan_rate_stream_enqueue(c, st.fmt, d_chunk, n_chunk, st.up, st.down, geo, grid, st.tab, d_step, st.n_ch, (float2 *)d_out, sa);
    }
    HIPCHK(c, hipGetLastError());
  }
  const unsigned long long n_base = p.i_base * (unsigned)st.down;      // == st.n_total - st.n_hist
  hipLaunchKernelGGL(k_chan_keep, dim3(1), dim3(256), 0, c->stream, (const uint16_t *)hist, (const uint16_t *)d_chunk, st.n_hist,
                     (unsigned long long)n_chunk, p.n_base_next - n_base, p.n_keep, chan_sample_bytes(st.fmt) / 2u, (uint16_t *)st.hist[st.cur ^ 1].get());
  HIPCHK(c, hipGetLastError());
  st.cur ^= 1;
  st.n_hist = p.n_keep;
  st.n_total += n_chunk;
  return LCS_OK;
}

// One push of the stream of 8-bit captures, already found acceptable.  A push cut in two is bit for bit the push uncut, so it is cut
// where captures fill: every piece goes into the float capture at column `filled`, and a capture that fills leaves for its slot of
// d_out / d_gain before the next piece overwrites it -- everything in order on the context's stream, so one float capture is enough.
int lcs_chan_stream_enqueue_u8(lcs_ctx *c, const void *d_chunk, uint64_t n_chunk, void *d_out, float *d_gain) {
  lcs_ctx::ChanStream &st = c->chan_stream;
  const size_t sample = chan_sample_bytes(st.fmt), cap_bytes = 2 * (size_t)st.n_ch * st.n_cap;
  const unsigned n_pb = cap_power_blocks(st.n_cap);
  const char *chunk = static_cast<const char *>(d_chunk);
  unsigned slot = 0;
  return cs_cap_plan(st.n_total, n_chunk, st.filled, st.n_cap, st.up, st.down, [&](const cs_seg &s) -> int {
    if (int rc = lcs_chan_stream_enqueue(c, chunk, s.n, st.cap.get() + st.filled, st.n_cap)) return rc;
    chunk += s.n * sample;
    st.filled += s.n_emit;
    if (!s.fills) return LCS_OK;
    st.filled = 0;
    hipLaunchKernelGGL(k_chan_cap_power, dim3(n_pb, (unsigned)st.n_ch), dim3(256), 0, c->stream, (const float2 *)st.cap, st.n_cap, st.cap_part.get());
    HIPCHK(c, hipGetLastError());
    const unsigned k = slot++;
    return chan_quant_enqueue(c, st.cap, st.cap_part, n_pb, st.n_ch, st.n_cap, static_cast<char *>(d_out) + k * cap_bytes,
                              d_gain ? d_gain + (size_t)k * st.n_ch : nullptr);
  });
}

// the queued pushes may still read the stream's buffers
int lcs_chan_stream_end(lcs_ctx *c) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  chan_stream_drop(c);
  return LCS_OK;
}

int lcs_chan_last_ms(lcs_ctx *c, float *ms) {
  if (!c->chan_timed) { c->err = "lcs_last_channelize_ms: no lcs_channelize call on this context yet"; return LCS_ERR_BAD_ARG; }
  HIPCHK(c, hipEventSynchronize(c->ev_chan1));
  HIPCHK(c, hipEventElapsedTime(ms, c->ev_chan0, c->ev_chan1));
  return LCS_OK;
}
