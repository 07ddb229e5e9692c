// channelizer.h -- the wideband channelizer: what its entry points (lcs_api.hip) hand down as one ChanCall, the rules a call
// is refused by, the one launcher (channelizer.hip: the integer form up == 1, the 8-bit output stage; channelizer_rate.hip: the
// rational form's kernels) and the index arithmetic both forms' kernels share with the host twins under tests/host.  The
// per-context state (parameter and filter-bank buffers, page-locked slots, events, the float scratch of the 8-bit form) are the
// chan_* / ev_chan* members of the context, shared by all forms.
#pragma once
#include "lcs_internal.h"
#include <cmath>

// One call as every layer below the entry points sees it: fs_out = fs_in * up / down, and lcs_channelize is up = 1, down = decim
struct ChanCall {
  const void *d_wide;
  int fmt;
  uint64_t n_in;
  double fs_in;
  int up, down;
  const double *f_shift;
  int n_ch;
  void *d_out;
  uint32_t n_out;
};

// What the entry points refuse, in the order they look: the text of the first rule a call breaks, nullptr for a call that may be
// launched.  CHAN_DECIM: the rate rule of lcs_channelize; CHAN_RATE: those of lcs_channelize_rational and lcs_channelize_u8;
// CHAN_RATE_ONLY stops behind them (lcs_channelize_rational hands a call with up == 1 to lcs_channelize there).
enum ChanRules { CHAN_DECIM, CHAN_RATE, CHAN_RATE_ONLY };
static inline const char *chan_refusal(const ChanCall &a, ChanRules rules) {
  if (!a.d_wide || !a.f_shift || !a.d_out) return "null pointer";
  if (rules == CHAN_DECIM) {
    if (a.down < 2 || a.down > 16) return "decim outside 2..16";
  } else {
    if (a.down < 2 || a.down > 128) return "down outside 2..128";
    if (a.up < 1 || a.up > 127) return "up outside 1..127";
    if (a.up >= a.down) return "up >= down: interpolation is not supported";
    if (a.down > 16 * a.up) return "down / up > 16";
    for (int p = a.up, q = a.down; q;) {
      const int r = p % q;
      p = q, q = r;
      if (!q && p != 1) return "up and down have a common factor";
    }
    if (rules == CHAN_RATE_ONLY) return nullptr;
  }
  if (a.n_ch < 1) return "n_ch < 1";
  if (a.n_out < 1) return "n_out < 1";
  if (!(a.fs_in > 0) || !std::isfinite(a.fs_in)) return "fs_in is not a positive rate";
  // the last output's window ends at sample floor(((n_out-1) down + 16 down - 1) / up): at up == 1 the bound is (n_out-1) decim + 16 decim
  if (a.n_in < (((uint64_t)a.n_out - 1) * a.down + 16ull * a.down - 1) / a.up + 1)
    return a.up == 1 ? "n_in < (n_out-1)*decim + 16*decim: the capture is too short for n_out outputs"
                     : "n_in < floor(((n_out-1)*down + 16*down - 1) / up) + 1: the capture is too short for n_out outputs";
  if (a.fmt != LCS_FMT_C64 && a.fmt != LCS_FMT_IQ_S8 && a.fmt != LCS_FMT_IQ_S16) return "unknown sample format";
  for (int k = 0; k < a.n_ch; ++k)
    if (!(std::fabs(a.f_shift[k]) <= 0.5 * a.fs_in)) return "|f_shift| > fs_in/2";
  if (reinterpret_cast<uintptr_t>(a.d_out) & 15) return "d_out is not 16-byte aligned";
  const uintptr_t in_align = a.fmt == LCS_FMT_C64 ? 7 : a.fmt == LCS_FMT_IQ_S16 ? 3 : 1;
  if (reinterpret_cast<uintptr_t>(a.d_wide) & in_align) return "d_wide is not aligned to its sample size";
  return nullptr;
}

// The continuous form (include/lcs.h, lcs_chan_stream_open): what its four entry points refuse beyond chan_refusal, in the order they
// look.  open hands its rate, format, shifts and n_ch to chan_refusal first (CHAN_RATE; the rules for n_in, n_out and d_out have
// nothing to look at there) and then asks here; count looks at the first two rules, close at the first.  count and close take either
// kind of stream; a push on a stream of 8-bit captures is refused behind the first rule.
enum ChanStreamEntry { CHAN_STREAM_OPEN, CHAN_STREAM_COUNT, CHAN_STREAM_PUSH, CHAN_STREAM_CLOSE };
struct ChanPush {
  bool is_open;              // the context has a stream
  int fmt;                   // the stream's format
  const void *d_chunk;
  uint64_t n_chunk;
  void *d_out;
  uint32_t row_stride, out_cap;
  uint64_t n_emit;           // what the push would hand out (cs_count)
  bool is_u8 = false;        // the stream hands out 8-bit captures (lcs_chan_stream_open_u8): its pushes are lcs_chan_stream_push_u8's
};
static inline const char *chan_stream_refusal(const ChanPush &a, ChanStreamEntry entry) {
  if (entry == CHAN_STREAM_OPEN) return a.is_open ? "a channelizer stream is already open on this context" : nullptr;
  if (!a.is_open) return "no channelizer stream is open on this context";
  if (entry == CHAN_STREAM_CLOSE) return nullptr;
  if (entry == CHAN_STREAM_PUSH && a.is_u8) return "the stream hands out 8-bit captures: push with lcs_chan_stream_push_u8";
  if (a.n_chunk > (1ull << 31)) return "n_chunk > 2^31";
  if (entry == CHAN_STREAM_COUNT) return nullptr;
  if (!a.d_chunk && a.n_chunk) return "null chunk with n_chunk > 0";
  const uintptr_t in_align = a.fmt == LCS_FMT_C64 ? 7 : a.fmt == LCS_FMT_IQ_S16 ? 3 : 1;
  if (reinterpret_cast<uintptr_t>(a.d_chunk) & in_align) return "d_chunk is not aligned to its sample size";
  if (!a.d_out && a.n_emit) return "null d_out with outputs to hand out";
  if (reinterpret_cast<uintptr_t>(a.d_out) & 7) return "d_out is not 8-byte aligned";
  if (a.row_stride < a.out_cap) return "row_stride < out_cap";
  if (a.out_cap < a.n_emit) return "out_cap < n_emit: size or split the chunk by lcs_chan_stream_count";
  return nullptr;
}

// The stream of 8-bit captures (include/lcs.h, lcs_chan_stream_open_u8): what open_u8 (behind chan_refusal, as open), count_u8 and
// push_u8 refuse, in the order they look; count_u8 stops behind the chunk's length.  Where a rule is one of chan_stream_refusal's it
// has that rule's text.
struct ChanPushU8 {
  bool is_open, is_u8;       // the context has a stream; it hands out 8-bit captures
  int fmt;
  const void *d_chunk;
  uint64_t n_chunk;
  void *d_out;
  const float *d_gain;
  uint32_t cap_room, n_cap;  // capture slots behind d_out; open_u8: the capture's length
  uint64_t n_done;           // the captures the push would hand out (cs_cap_done)
};
static inline const char *chan_stream_u8_refusal(const ChanPushU8 &a, ChanStreamEntry entry) {
  if (entry == CHAN_STREAM_OPEN) {
    if (a.n_cap < 1) return "n_cap < 1";
    return a.is_open ? "a channelizer stream is already open on this context" : nullptr;
  }
  if (!a.is_open) return "no channelizer stream is open on this context";
  if (!a.is_u8) return "the stream hands out floats: 8-bit captures need lcs_chan_stream_open_u8";
  if (a.n_chunk > (1ull << 31)) return "n_chunk > 2^31";
  if (entry == CHAN_STREAM_COUNT) return nullptr;
  if (!a.d_chunk && a.n_chunk) return "null chunk with n_chunk > 0";
  const uintptr_t in_align = a.fmt == LCS_FMT_C64 ? 7 : a.fmt == LCS_FMT_IQ_S16 ? 3 : 1;
  if (reinterpret_cast<uintptr_t>(a.d_chunk) & in_align) return "d_chunk is not aligned to its sample size";
  if (!a.d_out && a.n_done) return "null d_out with captures to hand out";
  if (reinterpret_cast<uintptr_t>(a.d_out) & 15) return "d_out is not 16-byte aligned";
  if (reinterpret_cast<uintptr_t>(a.d_gain) & 3) return "d_gain is not aligned to a float";
  if (a.cap_room < a.n_done) return "cap_room < n_done: size d_out or split the chunk by lcs_chan_stream_count_u8";
  return nullptr;
}

void lcs_chan_taps(int decim, double *taps /*[16*decim]*/);      // any decim >= 2
unsigned long long lcs_chan_step(double f_shift, double fs_in);
// d_part == nullptr: the float forms.  Otherwise [n_ch][lcs_chan_blocks(call)] floats: every workgroup along the outputs leaves
// the sum of |y|^2 of its outputs per carrier there.
int lcs_launch_channelize(lcs_ctx *c, const ChanCall &a, float *d_part);
unsigned lcs_chan_blocks(const ChanCall &a);
// lcs_channelize_u8: the float form into the context's scratch with the power partials, then k_chan_quant_u8 (channelizer.hip)
int lcs_launch_channelize_u8(lcs_ctx *c, const ChanCall &a, float *d_gain);
int lcs_chan_last_ms(lcs_ctx *c, float *ms);   // HIP-event time of the context's last channelizer launch (any form)
// the continuous form: the stream's own steps, taps, table and history (ChanStream, lcs_internal.h); channelizer.hip
int lcs_chan_stream_start(lcs_ctx *c, int fmt, double fs_in, int up, int down, const double *f_shift, int n_ch);
int lcs_chan_stream_enqueue(lcs_ctx *c, const void *d_chunk, uint64_t n_chunk, void *d_out, uint32_t row_stride);
int lcs_chan_stream_end(lcs_ctx *c);
// the stream of 8-bit captures: start as above plus the float capture [n_ch][n_cap] and its power partials; a push is cut where
// captures fill (cs_cap_segment), every piece is enqueued as above into the float capture, and a full capture goes through
// k_chan_cap_power and k_chan_quant_u8 into its slot of d_out / d_gain
int lcs_chan_stream_start_u8(lcs_ctx *c, int fmt, double fs_in, int up, int down, const double *f_shift, int n_ch, uint32_t n_cap);
int lcs_chan_stream_enqueue_u8(lcs_ctx *c, const void *d_chunk, uint64_t n_chunk, void *d_out, float *d_gain);

// The kernels are templates over the capture's format and POW (the power partials of the 8-bit form):
// chan_by_form(fmt, pow, [&](auto fmt, auto pow) { launch k<decltype(fmt)::value, decltype(pow)::value> }) picks the instantiation.
template <class F> inline void chan_by_form(int fmt, bool pow, F &&launch) {
  auto by_pow = [&](auto f) {
    if (pow) launch(f, std::true_type{});
    else launch(f, std::false_type{});
  };
  if (fmt == LCS_FMT_C64) by_pow(std::integral_constant<int, LCS_FMT_C64>{});
  else if (fmt == LCS_FMT_IQ_S16) by_pow(std::integral_constant<int, LCS_FMT_IQ_S16>{});
  else by_pow(std::integral_constant<int, LCS_FMT_IQ_S8>{});
}

// ---- the 8-bit output's rule (include/lcs.h, lcs_channelize_u8): k_chan_quant_u8 and tests/host/chan_u8_host.cpp call these two.
// The exponent e of a carrier of mean power P = mean |y|^2: the integer with 16^2 < 4^e P / 2 <= 32^2, i.e. 2^9 < 4^e P <= 2^11;
// 0 for a power that is zero or not finite.  P = m 2^x, 1/2 <= m < 1: 2 e is the even number in [10 - x, 11 - x], and in
// (10 - x, 12 - x] when m is 1/2 exactly (a power of two sits on the closed end).
__host__ __device__ __forceinline__ int chan_u8_exponent(double P) {
  if (!(P > 0.0) || !std::isfinite(P)) return 0;
  int x;
  const double m = frexp(P, &x);
  const int t = 11 - x + (m == 0.5 ? 1 : 0);
  return (t - (t & 1)) / 2;      // floor(t / 2): t - (t & 1) is even for either sign
}
// The code of a scaled component z = 2^e * component: clamp(127 + rint(z), 0, 255), ties to even; 127 for a z that is not finite
__host__ __device__ __forceinline__ unsigned chan_u8_code(float z) {
  if (!std::isfinite(z)) return 127u;
  return (unsigned)fminf(fmaxf(127.f + rintf(z), 0.f), 255.f);
}

// sample n of a capture of format FMT as (re, im) floats
template <int FMT>
__host__ __device__ __forceinline__ float2 chan_sample(const void *x, unsigned long long n) {
  if (FMT == LCS_FMT_C64) return ((const float2 *)x)[n];
  if (FMT == LCS_FMT_IQ_S16) {
    const uint32_t p = ((const uint32_t *)x)[n];
    return make_float2((float)(int)(int16_t)(p & 0xFFFFu) * (1.f / 32768.f), (float)(int)(int16_t)(p >> 16) * (1.f / 32768.f));
  }
  const uint32_t p = ((const uint16_t *)x)[n];
  return make_float2((float)(int)(int8_t)(p & 255u) * (1.f / 128.f), (float)(int)(int8_t)(p >> 8) * (1.f / 128.f));
}

// ---- the continuous form's bookkeeping (include/lcs.h, lcs_chan_stream_push).  N samples pushed so far, Tg = 16 D.  Everything is
// an ABSOLUTE index of the whole stream.  The launcher and the kernels go by these, and tests/host/chan_stream_host.cpp walks them.
// M(N): the outputs N samples give -- the largest n_out chan_refusal takes for n_in = N: (n_out - 1) D + Tg - 1 < N U
static inline unsigned long long cs_count(unsigned long long N, int U, int D) {
  const unsigned __int128 fine = (unsigned __int128)N * (unsigned)U;      // no limit on N below 2^64
  const unsigned Tg = 16u * (unsigned)D;
  return fine < Tg ? 0ull : (unsigned long long)((fine - Tg) / (unsigned)D) + 1ull;
}
// The aligned base behind M outputs: the first sample of column floor(M / U), the column (outputs i U .. i U + U - 1) that holds
// output M.  Output M's own window starts at ceil(M D / U) >= floor(M / U) D, and every later window starts later still.
static inline unsigned long long cs_base(unsigned long long M, int U, int D) { return M / (unsigned)U * (unsigned)D; }
// Samples kept behind a push: kept = N - cs_base(M(N)).  M > (N U - Tg) / D gives N < (M D + Tg) / U, and floor(M / U) >=
// (M - U + 1) / U, so kept < (Tg + (U - 1) D) / U = 16 D / U + D - D / U (with M = 0: kept = N < Tg / U).  kept is an integer:
// kept <= ceil((Tg + (U - 1) D) / U) - 1 = floor((Tg + (U - 1) D - 1) / U), the size of a history slot in samples (365 at 8/127)
static inline unsigned cs_keep_max(int U, int D) { return (unsigned)((16 * D + (U - 1) * D - 1) / U); }
// One push: N_prev samples before it, n_chunk new ones
struct cs_plan {
  unsigned long long m_first, m_end;      // the outputs handed out: m_first <= m < m_end
  unsigned long long i_base;              // the first column launched, floor(m_first / U); the history starts at sample i_base D
  unsigned long long n_base_next;         // where the history behind the push starts: cs_base(m_end)
  unsigned n_keep;                        // ... and how many samples it holds: N_prev + n_chunk - n_base_next
  unsigned cols, grid_x;                  // columns i_base .. floor((m_end - 1) / U) and the workgroups along them (0: nothing to hand out)
};
static inline cs_plan cs_plan_push(unsigned long long N_prev, unsigned long long n_chunk, int U, int D, int cols_per_block) {
  cs_plan p;
  p.m_first = cs_count(N_prev, U, D);
  p.m_end = cs_count(N_prev + n_chunk, U, D);
  p.i_base = p.m_first / (unsigned)U;
  p.n_base_next = cs_base(p.m_end, U, D);
  p.n_keep = (unsigned)(N_prev + n_chunk - p.n_base_next);
  p.cols = p.m_end > p.m_first ? (unsigned)((p.m_end - 1) / (unsigned)U - p.i_base) + 1u : 0u;
  p.grid_x = (p.cols + (unsigned)cols_per_block - 1) / (unsigned)cols_per_block;
  return p;
}
// ---- captures of n_cap outputs from the stream (include/lcs.h, lcs_chan_stream_push_u8): capture c is the outputs c n_cap ..
// (c + 1) n_cap - 1 of every carrier.  The launcher cuts a push by these, and tests/host/chan_stream_u8_host.cpp walks them.
// The inverse of cs_count: the smallest N with M(N) >= t, t >= 1: N U >= (t - 1) D + Tg.  M grows by at most one per sample
// (U < D), so M(cs_need(t)) == t and M(cs_need(t) - 1) == t - 1.
static inline unsigned long long cs_need(unsigned long long t, int U, int D) {
  const unsigned __int128 fine = (unsigned __int128)(t - 1) * (unsigned)D + 16u * (unsigned)D;
  return (unsigned long long)((fine + (unsigned)U - 1) / (unsigned)U);
}
// the captures complete behind N samples, and those a push of n_chunk samples completes
static inline unsigned long long cs_cap_count(unsigned long long N, unsigned n_cap, int U, int D) { return cs_count(N, U, D) / n_cap; }
static inline unsigned long long cs_cap_done(unsigned long long N_prev, unsigned long long n_chunk, unsigned n_cap, int U, int D) {
  return cs_cap_count(N_prev + n_chunk, n_cap, U, D) - cs_cap_count(N_prev, n_cap, U, D);
}
// One piece of a push: the next n samples hand out n_emit outputs, all of the capture being filled, and `fills` says that they
// complete it.  N_prev samples before the piece, n_left > 0 in the push from it on, `filled` outputs of the capture in hand
// (filled == M(N_prev) mod n_cap): the piece ends with the sample that completes the capture, cs_need of the capture's end, or with
// the push.
struct cs_seg { unsigned long long n; unsigned n_emit; bool fills; };
static inline cs_seg cs_cap_segment(unsigned long long N_prev, unsigned long long n_left, unsigned filled, unsigned n_cap, int U, int D) {
  const unsigned long long m = cs_count(N_prev, U, D), t = m - filled + n_cap;      // the capture's end
  const unsigned long long to_fill = cs_need(t, U, D) - N_prev;                      // > 0: M(N_prev) < t
  cs_seg s;
  s.fills = to_fill <= n_left;
  s.n = s.fills ? to_fill : n_left;
  s.n_emit = (unsigned)(cs_count(N_prev + s.n, U, D) - m);
  return s;
}
// A push as its pieces, in order: each(piece) -> 0 to go on; returns the first other value.  The pieces add up to n_chunk; nothing for n_chunk == 0.
template <class F>
static inline int cs_cap_plan(unsigned long long N_prev, unsigned long long n_chunk, unsigned filled, unsigned n_cap, int U, int D, F &&each) {
  for (unsigned long long done = 0; done < n_chunk;) {
    const cs_seg s = cs_cap_segment(N_prev + done, n_chunk - done, filled, n_cap, U, D);
    if (const int rc = each(s)) return rc;
    done += s.n;
    filled = s.fills ? 0u : filled + s.n_emit;
  }
  return 0;
}
// What a push's kernels know of the stream.  Sample n >= n_base of the stream is one of: history (samples [n_base, n_base + n_hist)
// in the input's format), the chunk behind it, or -- behind the chunk's end -- a zero
struct cs_args {
  const void *hist;
  unsigned long long i_base;              // n_base = i_base D
  unsigned n_hist;
  unsigned long long m_first, m_end;
  unsigned row_stride;
};
enum { CS_HIST = 0, CS_CHUNK = 1, CS_ZERO = 2 };
struct cs_where { int part; unsigned long long off; };
__host__ __device__ __forceinline__ cs_where cs_source(unsigned long long n, unsigned long long n_base, unsigned n_hist, unsigned long long n_chunk) {
  cs_where w;
  w.off = n - n_base;                     // n >= n_base: no workgroup of a push starts in front of column i_base
  w.part = CS_HIST;
  if (w.off >= n_hist) {
    w.off -= n_hist;
    w.part = w.off < n_chunk ? CS_CHUNK : CS_ZERO;
  }
  return w;
}
template <int FMT>
__host__ __device__ __forceinline__ float2 cs_sample(const void *hist, const void *chunk, const cs_where &w) {
  if (w.part == CS_ZERO) return make_float2(0.f, 0.f);
  return chan_sample<FMT>(w.part == CS_HIST ? hist : chunk, w.off);
}
// bytes of one sample of a format
__host__ __device__ __forceinline__ unsigned chan_sample_bytes(int fmt) { return fmt == LCS_FMT_C64 ? 8u : fmt == LCS_FMT_IQ_S16 ? 4u : 2u; }

// ---- the kernels' bookkeeping: where every tap, sample and output goes for a rate U / D.  The kernels and the launcher decide by
// these -- the rational form by all of them, k_channelize (U = 1, two tiles per wave) by its staging offset, its accumulator map,
// its rotation and its power partials -- and tests/host/chan_rate_host.cpp walks a workgroup on the CPU with the same ones (a
// host build supplies sinpi / cospi / sinpif / cospif itself where its libm has none).
#define CR_CARRIERS 16                 // carriers per A tile (32 rows)
#define CR_LDS_MAX (48 * 1024)         // NI grows only while the staged samples stay below this
// k_channelize (up == 1)
#define CH_NT 256                      // outputs per workgroup: 4 waves x 2 tiles x 32 columns
#define CH_XROWS (CH_NT + 15)          // LDS rows of D samples: the windows of CH_NT outputs span (CH_NT + 15) D samples

struct cr_geom { int G, NI, xrows; size_t lds_bytes; };
struct cr_tile { int q, it, sq; };                 // residue, column block of the workgroup, s_q = ceil(q D / U)
struct cr_pos { int rr, p; };                      // window position s_q + j = rr D + p
struct cr_col { unsigned long long m, nd; };       // output index, first sample of its window (the sample its phase is taken at)

// floats of LDS a workgroup with NI column tiles per residue stages, and its rows
static inline size_t cr_lds_floats(int D, int G, int ni, int *rows) {
  *rows = (32 * ni * D + 4 * G + D - 1) / D;
  return (size_t)*rows * (2 * D + 1);
}
static inline cr_geom cr_geometry(int up, int down) {
  cr_geom g;
  g.G = ((16 * down + up - 1) / up + 3) / 4;      // k-step groups per residue: ceil(16 D / U) taps, padded to fours
  // column tiles per residue: at least two tiles for every wave, and a whole number per wave where LDS allows
  int ni = 1, rows_next = 0;
  while ((up * ni < 8 || ((up * ni) & 3)) && up * ni < 32 && cr_lds_floats(down, g.G, ni + 1, &rows_next) * sizeof(float) <= CR_LDS_MAX) ++ni;
  g.NI = ni;
  g.lds_bytes = cr_lds_floats(down, g.G, ni, &g.xrows) * sizeof(float);
  return g;
}
// workgroups along the outputs: each owns 32 NI columns of every residue
static inline unsigned cr_grid_x(unsigned n_out, int up, int ni) {
  const unsigned n_i = (n_out + up - 1) / up;      // columns of residue 0, the longest
  return (n_i + 32 * ni - 1) / (32 * ni);
}

__host__ __device__ __forceinline__ int cr_sq(int q, int U, int D) { return (q * D + U - 1) / U; }

// tab[((((rb * U + q) * G + s4) * 64 + lane) * 4 + i] = A[row lane & 31 of block rb][kk = 2 (4 s4 + i) + (lane >> 5)] of residue q
__host__ __device__ __forceinline__ float cr_table_value(size_t e, const unsigned long long *__restrict__ step, const float *__restrict__ taps,
                                                         int n_ch, int U, int D, int G) {
  const int Tg = 16 * D;
  const int i = (int)(e & 3), l = (int)((e >> 2) & 63);
  size_t rest = e >> 8;
  const int s4 = (int)(rest % G);
  rest /= G;
  const int q = (int)(rest % U), rb = (int)(rest / U);
  const int j = 4 * s4 + i, r = l & 31, c = l >> 5;
  const int ch = rb * CR_CARRIERS + (r >> 1), ri = r & 1;
  const int sq = cr_sq(q, U, D);
  const int t = Tg - 1 - ((sq + j) * U - q * D);      // <= Tg - 1 by the choice of s_q
  float v = 0.f;
  if (ch < n_ch && t >= 0) {
    const unsigned long long ph = step[ch] * (unsigned long long)j;
    const double ht = 2.0 * ((double)(long long)ph * 0x1p-64);      // half-turns, [-1, 1)
    const double h = (double)U * (double)taps[t];
    const double g_re = h * cospi(ht), g_im = -h * sinpi(ht);
    v = (float)(ri == 0 ? (c == 0 ? g_re : -g_im) : (c == 0 ? g_im : g_re));
  }
  return v;
}

// the 16-byte group of four k-steps 4 s4 .. 4 s4 + 3 a lane loads as its A operands, in float4 units of the table
__host__ __device__ __forceinline__ size_t cr_a_group(int rb, int q, int s4, int lane, int U, int G) {
  return (((size_t)rb * U + q) * G + s4) * 64 + lane;
}
// staged sample idx (capture sample i0 D + idx) -> its float offset in LDS: rows of D samples, odd row stride 2 D + 1
__host__ __device__ __forceinline__ int cr_stage_offset(int idx, int D) {
  const int row = idx / D, p = idx - row * D;
  return row * (2 * D + 1) + 2 * p;
}
// tile t of a workgroup: residue t % U, columns i0 + 32 (t / U) + 0..31
__host__ __device__ __forceinline__ cr_tile cr_tile_of(int t, int U, int D) {
  cr_tile r;
  r.it = t / U;
  r.q = t - r.it * U;
  r.sq = cr_sq(r.q, U, D);
  return r;
}
// a lane's B operand at k-step j of a tile is xs[cr_b_base + cr_b_step]: column lane & 31, (re | im) = lane >> 5; the window walks on
__host__ __device__ __forceinline__ int cr_b_base(const cr_tile &t, int lane, int D) { return (t.it * 32 + (lane & 31)) * (2 * D + 1) + (lane >> 5); }
__host__ __device__ __forceinline__ cr_pos cr_b_first(const cr_tile &t, int D) {
  cr_pos w;
  w.rr = t.sq / D;
  w.p = t.sq - w.rr * D;
  return w;
}
__host__ __device__ __forceinline__ int cr_b_step(const cr_pos &w, int D) { return w.rr * (2 * D + 1) + 2 * w.p; }
__host__ __device__ __forceinline__ void cr_b_next(cr_pos &w, int D) {
  if (++w.p == D) { w.p = 0; ++w.rr; }
}
// the tile's column of a lane: output m = i U + q of column i = i0 + 32 it + (lane & 31), its window starts at sample i D + s_q
__host__ __device__ __forceinline__ cr_col cr_col_of(unsigned long long i0, const cr_tile &t, int lane, int U, int D) {
  const unsigned long long i = i0 + (unsigned)(t.it * 32 + (lane & 31));
  cr_col r;
  r.m = i * (unsigned)U + (unsigned)t.q;
  r.nd = i * (unsigned)D + (unsigned)t.sq;
  return r;
}
// accumulator register v of a lane: row (v & 3) + 8 (v >> 2) + 4 (lane >> 5) of the tile, column lane & 31; row = 2 carrier + (re | im)
__host__ __device__ __forceinline__ int cr_acc_row(int v, int lane) { return (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5); }
__host__ __device__ __forceinline__ int cr_acc_carrier(int rb, int v, int lane) { return rb * CR_CARRIERS + (cr_acc_row(v, lane) >> 1); }
// (re, im) of a carrier's sum, turned by the carrier phase at sample nd (64-bit fixed point, wrapped exactly)
__host__ __device__ __forceinline__ float2 cr_rotate(float re, float im, unsigned long long step, unsigned long long nd) {
  const unsigned long long ph = step * nd;
  const float ht = (float)(int)(unsigned)(ph >> 32) * 0x1p-31f;      // half-turns of the carrier phase at sample s_q + i D
  const float sn = sinpif(ht), cs = cospif(ht);
  return make_float2(re * cs + im * sn, im * cs - re * sn);
}
// POW (the 8-bit form): pw[i] is the lane's sum of |y|^2 over the outputs it stored for the carrier of its registers 2 i, 2 i + 1.
// The workgroup's sum per carrier goes to part[carrier][blockIdx.x]: over the 32 columns by a butterfly of lane exchanges, over
// the four waves through LDS in wave order -- one fixed order, no atomics, so two runs give the same bits.
__device__ __forceinline__ void cr_power_partials(const float (&pw)[8], int rb, int n_ch, float *__restrict__ part) {
  __shared__ float red[4][CR_CARRIERS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
