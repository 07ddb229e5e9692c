// tfg_wide.hip -- the time-frequency grid of a cell at DFT lengths 128 .. 2048 from wide samples on the device, and the cell
// measurement over its 12 n_rb columns (lcs_extract_tfg_wide, lcs_cell_meas_wide; the rule: cell_meas_wide.h, include/lcs.h).  A
// translation unit of its own: a context that never calls the stage runs no kernel of this file and allocates none of its buffers,
// and the per-cell chain's code objects (tfg_mib.hip, cell_meas.hip) are what they are without it.
#include <vector>
#include "lcs_internal.h"
#include "tfg_layout.h"
#include "lte_device.h"
#include "cell_meas_wide.h"

// exp(j pi u), out of line (lte_device.h says why): the frequency correction's phase is a product kk i with i up to 2.4 M, which
// sincospi reduces exactly where sincos(pi kk i) would lose eleven digits first
__device__ __attribute__((noinline)) static cd2 cispi_call(double u) { double s_, c_; sincospi(u, &s_, &c_); return mk(c_, s_); }

// ------------------------------------------------------------------ one row of the grid per workgroup
// The row's n_fft samples are widened, turned by the frequency correction (absolute sample index, phase in double) and laid into
// LDS as fp64 complex, 16 bytes an element: 32 KiB at 2048 points.  The transform is decimation in frequency, radix 2 in place
// while a butterfly's two inputs are 16 or more elements apart (log2(n_fft) - 4 stages, twiddles from the host's table), which
// leaves n_fft / 16 contiguous blocks of 16; block t then goes into the registers of thread t, through fft16 (lte_device.h), and out
// to the grid: its sixteen results are the bins bitrev(t) + (n_fft / 16) k2, of which the 12 n_rb kept ones are scaled, late-compensated
// and stored.  No bit-reversal pass, and nothing but the kept columns is written.
// LDS banking (MI355X: a 16-byte access sees 16 slots of 16 bytes per bank row; reads conflict inside four 16-lane groups
// {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, .. and writes inside groups of 8 contiguous lanes).  In a radix-2 stage consecutive lanes take
// consecutive elements, which is conflict-free as it stands.  The last step is the one a plain layout breaks: thread t reads
// elements 16 t + e, a stride of one whole bank row, every lane of a group on the same slot, 16 ways.  Hence element i lives at
// i ^ ((i >> 4) & 15): thread t's element e sits on slot e ^ (t & 15), and the sixteen lanes of a read group have sixteen different
// t & 15.  The radix-2 stages keep their property under the swizzle as long as a read group's lanes lie in the 16-element blocks
// 2 u and 2 u + 1 (they differ in bit 0 of the XOR, which maps {4 .. 11} and {0 .. 3, 12 .. 15} onto themselves): every stage
// with butterflies 32 or more apart.  The one stage at distance 16 takes blocks 2 u and 2 u + 2 and is two-way conflicted in half
// of its groups; it is one of up to seven, and the kernel's time goes to the sample loads and the sincospi, not to LDS.
__host__ __device__ constexpr int tw_threads(int n_fft) { return n_fft / 8 < 64 ? 64 : n_fft / 8; }
__host__ __device__ constexpr int tw_log2(int n) { return n <= 1 ? 0 : 1 + tw_log2(n / 2); }
__device__ __forceinline__ int tw_sw(int i) { return i ^ ((i >> 4) & 15); }

template <int N_FFT>
__global__ __launch_bounds__(tw_threads(N_FFT)) void k_tfg_wide(const float2 *__restrict__ cap, uint32_t n_cap, const double *__restrict__ ideal,
                                                                 const double2 *__restrict__ tw, double2 *__restrict__ grid, double kk, int n_rb) {
  constexpr int T = tw_threads(N_FFT), BLOCKS = N_FFT / 16, LB = tw_log2(BLOCKS);
  __shared__ cd2 s[N_FFT];
  const int tid = threadIdx.x;
  const double loc_ideal = ideal[blockIdx.x];
  const long loc = (long)d_round_i(loc_ideal);
  for (int n = tid; n < N_FFT; n += T) {
    const long i = loc + n;
    const bool in = i >= 0 && (uint64_t)i < n_cap;       // (the entry points refuse a row outside the buffer; nothing is read there)
    const float2 v = cap[in ? (size_t)i : 0];
    const cd2 rot = cispi_call(kk * (double)i);
    s[tw_sw(n)] = in ? cmul(mk((double)v.x, (double)v.y), rot) : mk(0, 0);
  }
  __syncthreads();
  // x[n] + x[n + half] -> the even bins' half, (x[n] - x[n + half]) W^(n step) -> the odd bins' half; W = exp(-2 pi j / N_FFT)
  for (int half = N_FFT / 2, step = 1; half >= 16; half >>= 1, step <<= 1) {
    for (int j = tid; j < N_FFT / 2; j += T) {
      const int k = j & (half - 1), i0 = ((j - k) << 1) + k, i1 = i0 + half;
      const cd2 a = s[tw_sw(i0)], b = s[tw_sw(i1)], w = ld(&tw[k * step]);
      s[tw_sw(i0)] = cadd(a, b);
      s[tw_sw(i1)] = cmul(csub(a, b), w);
    }
    __syncthreads();
  }
  if (tid < BLOCKS) {
    cd2 x[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) x[e] = s[tw_sw(16 * tid + e)];
    fft16(x);
    const int r = (int)(__brev((unsigned)tid) >> (32 - LB));      // the block's bins are r + BLOCKS k2
    const double late = (double)loc - loc_ideal;                   // |late| <= 1/2
    double2 *out = grid + (size_t)blockIdx.x * 12 * n_rb;
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) {
      int cn;
      const int col = measw_col_of_bin(r + BLOCKS * k2, N_FFT, n_rb, &cn);
      if (col < 0) continue;
      // exp(-j 2 pi late / n_fft cn) as exp(j pi u), u = -2 late cn / n_fft (the division is by a power of two)
      const cd2 ph = cispi_call(-2.0 * late * (double)cn / (double)N_FFT);
      st(&out[col], cmul(cdivr(fft16_out(x, k2), sqrt((double)N_FFT)), ph));
    }
  }
}

// ------------------------------------------------------------------ the measurement: one wave per bin of reference rows
// k_cell_meas's lane-per-entry pattern from 12 entries a row to 2 n_rb <= 200: workgroup b (one wave) takes bin b's rows
// q = b, b + 40, .. in row order, each in measw_passes(n_rb) passes of 64 entries, lane l holding entry l + 64 t.  A lane loads its
// entry's six subcarriers and, instead of shuffling h in from the lane beside it (which is another PASS for lane 63), the right
// neighbour's two reference elements: tdd_h of the same operands gives the same bits.  The rows of a bin share (slot, symbol), so
// the wave builds its RS sequence once (rs_dl_row_wide, as bits).  Per row the seven lane sums go through the wave's butterfly to
// rowv[value][q]; the per-RB values stay in the registers of the even lanes across the bin's rows -- they are indexed by the
// unrolled pass, never by a run-time value (cell_meas.h's note on scratch) -- and leave as binrb[b][value][rb].
// k_cell_meas_wide_fin then adds bins in row order, the bins of the mask in increasing order, and finishes the record.
__global__ __launch_bounds__(MEASW_LANES) void k_cell_meas_wide(const double2 *__restrict__ grid, const uint32_t *__restrict__ pn_jump,
                                                                double *__restrict__ rowv, double *__restrict__ binrb, int n_q, int id,
                                                                int cp_type, int n_symb, int ports, int n_rb, int dl_mask) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= n_q || !meas_bin_used(b, dl_mask)) return;       // the same for the whole workgroup
  __shared__ uint32_t s_bits[RS_DL_WIDE_WORDS];
  __shared__ double s_shift[4];
  if (lane == 0) {
    for (int p = 0; p < 4; ++p) s_shift[p] = -1.0;
    rs_dl_row_wide(b >> 1, (b & 1) ? 2 : 0, id, cp_type, n_symb, n_rb, pn_jump, s_bits, s_shift);
  }
  __syncthreads();
  const int shift0 = (int)s_shift[0], shift1 = (int)s_shift[1];
  const int n_ent = 2 * n_rb, n_pass = measw_passes(n_rb);
  const size_t ncol = (size_t)12 * n_rb;
  double acc[MEASW_MAX_PASSES][MEASW_NRB];
#pragma unroll
  for (int t = 0; t < MEASW_MAX_PASSES; ++t)
#pragma unroll
    for (int k = 0; k < MEASW_NRB; ++k) acc[t][k] = 0.0;
  bool first = true;
  for (int q = b; q < n_q; q += TDD_BINS) {
    const double2 *src = grid + (size_t)q * ncol;
    double lv[MEAS_NV];
#pragma unroll
    for (int i = 0; i < MEAS_NV; ++i) lv[i] = 0.0;
#pragma unroll
    for (int t = 0; t < MEASW_MAX_PASSES; ++t) {
      if (t >= n_pass) continue;                             // wave-uniform
      const int m = lane + MEASW_LANES * t;
      const bool live = m < n_ent, nb = m + 1 < n_ent;
      double2 x[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) x[k] = live ? src[6 * m + k] : make_double2(0, 0);
      const double2 y0 = nb ? src[6 * (m + 1) + shift0] : make_double2(0, 0), y1 = nb ? src[6 * (m + 1) + shift1] : make_double2(0, 0);
      const cd2 rs = rs_dl_wide_value(s_bits, live ? m : 0), rsn = rs_dl_wide_value(s_bits, nb ? m + 1 : 0);
      const meas_x6 xs = {mk(x[0].x, x[0].y), mk(x[1].x, x[1].y), mk(x[2].x, x[2].y), mk(x[3].x, x[3].y), mk(x[4].x, x[4].y), mk(x[5].x, x[5].y)};
      const cd2 h0 = meas_h(xs, shift0, rs), h1 = meas_h(xs, shift1, rs);
      const cd2 h0n = tdd_h(mk(y0.x, y0.y), rsn), h1n = tdd_h(mk(y1.x, y1.y), rsn);
      double v[MEAS_NV];
      meas_entry(xs, m, ports, h0, h0n, h1, h1n, v, n_ent);
#pragma unroll
      for (int i = 0; i < MEAS_NV; ++i) {
        v[i] = live ? v[i] : 0.0;
        lv[i] = measw_acc(t == 0, lv[i], v[i]);
      }
      const double w_next = __shfl_down(v[MEAS_W], 1);       // entry m + 1's w: the same pass, since 64 is even and m is (where it counts)
      double r[MEASW_NRB];
      measw_rb_values(v, w_next, r);
#pragma unroll
      for (int k = 0; k < MEASW_NRB; ++k) acc[t][k] = measw_acc(first, acc[t][k], r[k]);
    }
#pragma unroll
    for (int i = 0; i < MEAS_NV; ++i) {
      const double sum = meas_row_sum_lanes<MEASW_LANES>(lv[i]);
      if (lane == 0) rowv[(size_t)i * TC_MAX_Q + q] = sum;
    }
    first = false;
  }
#pragma unroll
  for (int t = 0; t < MEASW_MAX_PASSES; ++t) {
    const int m = lane + MEASW_LANES * t;
    if (t < n_pass && !(lane & 1) && m < n_ent) {
#pragma unroll
      for (int k = 0; k < MEASW_NRB; ++k) binrb[((size_t)b * MEASW_NRB + k) * MEASW_MAX_RB + (m >> 1)] = acc[t][k];
    }
  }
}

#define MWF_THREADS 512
static_assert(MEAS_NV * TDD_BINS <= MWF_THREADS && MEASW_MAX_RB <= MWF_THREADS && sizeof(lcs_meas_wide_info) % sizeof(double) == 0, "k_cell_meas_wide_fin's split");
__global__ __launch_bounds__(MWF_THREADS) void k_cell_meas_wide_fin(const double *__restrict__ rowv, const double *__restrict__ binrb,
                                                                    lcs_meas_wide_info *__restrict__ out, int n_q, int ports, int n_rb, int n_fft,
                                                                    int dl_mask) {
  __shared__ double s_bin[MEAS_NV][TDD_BINS];
  __shared__ double s_tot[MEAS_NV];
  __shared__ lcs_meas_wide_info s_info;
  __shared__ int s_ok;
  const int tid = threadIdx.x, n_rows = meas_n_rows(n_q, dl_mask);
  if (tid < MEAS_NV * TDD_BINS) {
    const int i = tid / TDD_BINS, b = tid % TDD_BINS;
    s_bin[i][b] = meas_bin_used(b, dl_mask) ? meas_bin_sum(rowv + (size_t)i * TC_MAX_Q, b, n_q) : 0.0;     // (nobody wrote the other bins' rows)
  }
  __syncthreads();
  if (tid < MEAS_NV) s_tot[tid] = meas_total(s_bin[tid], dl_mask);
  __syncthreads();
  if (tid == 0) s_ok = measw_finish_head(s_tot, n_rows, ports, dl_mask, n_rb, n_fft, &s_info) ? 1 : 0;
  __syncthreads();
  if (tid < MEASW_MAX_RB) {
    double t[MEASW_NRB] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const bool ok = s_ok && tid < n_rb;
    if (ok) {
#pragma unroll
      for (int k = 0; k < MEASW_NRB; ++k) t[k] = measw_total_strided(binrb + (size_t)k * MEASW_MAX_RB + tid, (size_t)MEASW_NRB * MEASW_MAX_RB, n_q, dl_mask);
    }
    measw_finish_rb(t, ok, n_rows, tid, &s_info);
  }
  __syncthreads();
  for (int i = tid; i < (int)(sizeof(lcs_meas_wide_info) / sizeof(double)); i += MWF_THREADS)
    reinterpret_cast<double *>(out)[i] = reinterpret_cast<const double *>(&s_info)[i];
}

// ------------------------------------------------------------------ launchers
template <int N_FFT>
static void tfg_wide_launch(lcs_ctx *c, const float2 *d_cap, uint32_t n_cap, const double2 *tw, int n_rows, double kk, int n_rb) {
  hipLaunchKernelGGL(k_tfg_wide<N_FFT>, dim3(n_rows), dim3(tw_threads(N_FFT)), 0, c->stream, d_cap, n_cap, c->meas_wide.ideal.get(), tw,
                     c->meas_wide.grid.get(), kk, n_rb);
}

int lcs_launch_tfg_wide(lcs_ctx *c, const float2 *d_cap, uint32_t n_cap, const double *h_ideal, int n_rows, double kk, int n_fft, int n_rb) {
  lcs_ctx::MeasWide &w = c->meas_wide;
  const int li = measw_log2r(n_fft);
  if (li < 0 || n_rows <= 0) { c->err = "tfg_wide: no such transform length"; return LCS_ERR_BAD_ARG; }
  int rc;
  if (!w.tw[li]) {
    // W^t = exp(-2 pi j t / n_fft), t < n_fft / 2, in double on the host: once per context and length
    std::vector<double2> h((size_t)n_fft / 2);
    for (int t = 0; t < n_fft / 2; ++t) h[t] = make_double2(cos(2.0 * M_PI * (double)t / (double)n_fft), -sin(2.0 * M_PI * (double)t / (double)n_fft));
    if ((rc = w.tw[li].alloc(c, h.size()))) return rc;
    HIPCHK(c, hipMemcpy(w.tw[li], h.data(), h.size() * sizeof(double2), hipMemcpyHostToDevice));
  }
  const size_t need = (size_t)n_rows * 12 * n_rb;
  if (need > w.grid.capacity() || (size_t)n_rows > w.ideal.capacity()) {
    HIPCHK(c, hipStreamSynchronize(c->stream));            // nothing reads the blocks that go
    if ((rc = w.grid.reserve(c, need)) || (rc = w.ideal.reserve(c, (size_t)n_rows))) return rc;
  }
  HIPCHK(c, hipMemcpyAsync(w.ideal, h_ideal, sizeof(double) * n_rows, hipMemcpyHostToDevice, c->stream));
  switch (n_fft) {
    case 128: tfg_wide_launch<128>(c, d_cap, n_cap, w.tw[li], n_rows, kk, n_rb); break;
    case 256: tfg_wide_launch<256>(c, d_cap, n_cap, w.tw[li], n_rows, kk, n_rb); break;
    case 512: tfg_wide_launch<512>(c, d_cap, n_cap, w.tw[li], n_rows, kk, n_rb); break;
    case 1024: tfg_wide_launch<1024>(c, d_cap, n_cap, w.tw[li], n_rows, kk, n_rb); break;
    default: tfg_wide_launch<2048>(c, d_cap, n_cap, w.tw[li], n_rows, kk, n_rb); break;
  }
  HIPCHK(c, hipGetLastError());
  return LCS_OK;
}

int lcs_launch_cell_meas_wide(lcs_ctx *c, const lcs_cell &cell, int n_q, int n_fft, int n_rb, int dl_mask) {
  lcs_ctx::MeasWide &w = c->meas_wide;
  int rc;
  if ((rc = w.rowv.reserve(c, (size_t)MEAS_NV * TC_MAX_Q)) || (rc = w.binrb.reserve(c, (size_t)TDD_BINS * MEASW_NRB * MEASW_MAX_RB)) ||
      (rc = w.pn_jump.reserve(c, 32)) || (rc = w.rec.reserve(c, 1)))
    return rc;
  lcs_tables::pn_jump_table(1600 + 2 * (110 - n_rb), w.h_pn_jump);
  HIPCHK(c, hipMemcpyAsync(w.pn_jump, w.h_pn_jump, sizeof(w.h_pn_jump), hipMemcpyHostToDevice, c->stream));
  const int n_symb = cell.cp_type == LCS_CP_NORMAL ? 7 : 6, id = cell.n_id_2 + 3 * cell.n_id_1;
  hipLaunchKernelGGL(k_cell_meas_wide, dim3(TDD_BINS), dim3(MEASW_LANES), 0, c->stream, (const double2 *)w.grid.get(), (const uint32_t *)w.pn_jump.get(),
                     w.rowv.get(), w.binrb.get(), n_q, id, (int)cell.cp_type, n_symb, meas_ports(cell.n_ports), n_rb, dl_mask);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_cell_meas_wide_fin, dim3(1), dim3(MWF_THREADS), 0, c->stream, (const double *)w.rowv.get(), (const double *)w.binrb.get(),
                     w.rec.get(), n_q, meas_ports(cell.n_ports), n_rb, n_fft, dl_mask);
  HIPCHK(c, hipGetLastError());
  return LCS_OK;
}
