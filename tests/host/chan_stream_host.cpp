// Host-side twin of the channelizer's continuous form (channelizer.h: cs_count, cs_base, cs_keep_max, cs_plan_push, cs_source,
// chan_stream_refusal): the launcher's bookkeeping of a stream walked push by push, and a push walked workgroup by workgroup on the
// CPU -- staging from the two-part source, tiles, k-steps, one v_mfma_f32_32x32x2_f32 as a 64-lane loop, guards, rotation, stores
// -- with every index taken from the helpers the kernels and the launcher call.  tests/test_channelizer_stream_host.py drives it
// as a library; built with -DCS_HOST_MAIN it is a program of its own that runs the counting and source-map cases over the whole
// rate domain (the form a sanitizer build takes).  Test infrastructure.
#include <cmath>
#if !(defined(__GLIBC__) && defined(__GLIBC_PREREQ))
#define CR_HOST_OWN_PI 1
#elif !__GLIBC_PREREQ(2, 41)
#define CR_HOST_OWN_PI 1
#endif
#ifdef CR_HOST_OWN_PI
// sin / cos of x half-turns; exact at every multiple of a quarter turn (tests/host/chan_rate_host.cpp)
static void cr_host_sincospi(double x, double *s, double *c) {
  const double r = x - 2.0 * std::nearbyint(0.5 * x);
  const double k = std::nearbyint(2.0 * r);
  const double f = r - 0.5 * k;
  const double sf = std::sin(M_PI * f), cf = std::cos(M_PI * f);
  switch ((int)k & 3) {
    case 0: *s = sf, *c = cf; break;
    case 1: *s = cf, *c = -sf; break;
    case 2: *s = -sf, *c = -cf; break;
    default: *s = -cf, *c = sf; break;
  }
}
static double sinpi(double x) { double s, c; cr_host_sincospi(x, &s, &c); return s; }
static double cospi(double x) { double s, c; cr_host_sincospi(x, &s, &c); return c; }
static float sinpif(float x) { return (float)sinpi((double)x); }
static float cospif(float x) { return (float)cospi((double)x); }
#endif
#include "../../lte-cell-scanner_amd/csrc/channelizer.h"
#include <cstdio>
#include <cstring>
#include <vector>

typedef unsigned long long ull;

// the launch shape of a form: columns a workgroup owns, rows of D samples it stages (k_channelize at up == 1, k_channelize_rate otherwise)
struct shape { int cols, xrows, G; };
static shape shape_of(int U, int D) {
  const cr_geom g = cr_geometry(U, D);
  shape s;
  s.cols = U == 1 ? CH_NT : 32 * g.NI;
  s.xrows = U == 1 ? CH_XROWS : g.xrows;
  s.G = g.G;
  return s;
}

extern "C" ull cs_host_count(ull N, int U, int D) { return cs_count(N, U, D); }
extern "C" unsigned cs_host_keep_max(int U, int D) { return cs_keep_max(U, D); }

// ---- counting.  M(N) against chan_refusal: n_out = M(N) is taken (M >= 1), n_out = M(N) + 1 is refused as too short; M grows by 0
// or 1 per sample.  N: every value up to 2 Tg / U + 6 D, then around multiples of D further out and below 2^31.  Returns the
// number of N checked, or -(1 + the first N that fails).
extern "C" long long cs_host_check_counts(int U, int D) {
  alignas(16) static char any[16];
  const double f0 = 0.0;
  const ChanRules rules = U == 1 ? CHAN_DECIM : CHAN_RATE;
  std::vector<ull> ns;
  const ull dense = 2ull * 16 * D / U + 6ull * D;
  for (ull n = 0; n <= dense; ++n) ns.push_back(n);
  for (ull k : {100ull, 1000ull, 65536ull, 1ull << 20, (1ull << 31) / (ull)D - 2})
    for (int d = -3; d <= 3; ++d) ns.push_back(k * D + d);
  long long checked = 0;
  ull prev_n = 0, prev_m = 0;
  for (ull N : ns) {
    const ull M = cs_count(N, U, D);
    if (N == prev_n + 1 && !(M == prev_m || M == prev_m + 1)) return -(long long)(1 + N);
    if (N > prev_n && M < prev_m) return -(long long)(1 + N);
    prev_n = N, prev_m = M;
    ChanCall a = {any, LCS_FMT_IQ_S16, N, 1.0, U, D, &f0, 1, any, (uint32_t)M};
    if (M >= 1 && chan_refusal(a, rules)) return -(long long)(1 + N);
    a.n_out = (uint32_t)M + 1;
    const char *what = chan_refusal(a, rules);
    if (!what || !std::strstr(what, "the capture is too short")) return -(long long)(1 + N);
    ++checked;
  }
  return checked;
}

// ---- a stream's bookkeeping, push by push, as lcs_chan_stream_enqueue keeps it
struct stream_state { ull n_total; unsigned n_hist; };
enum {
  CS_OK = 0, CS_KEEP_ABOVE_SLOT = 1, CS_BASE_MOVED_BACK = 2, CS_BASE_BEHIND_NEXT_WINDOW = 3, CS_BASE_NOT_HISTORY = 4, CS_READ_BEFORE_BASE = 5,
  CS_HIST_OUTSIDE = 6, CS_CHUNK_OUTSIDE = 7, CS_ZERO_INSIDE = 8, CS_WINDOW_NOT_ARRIVED = 9, CS_KEEP_SOURCE = 10, CS_OUTPUT_NOT_LAUNCHED = 11,
  CS_COUNT_MISMATCH = 12
};
// one push: every premise of the kernels, then the state moves on.  Returns the first premise broken.
static int check_push(stream_state &st, ull n_chunk, int U, int D) {
  const shape sh = shape_of(U, D);
  const unsigned Tg = 16u * D;
  const cs_plan p = cs_plan_push(st.n_total, n_chunk, U, D, sh.cols);
  const ull n_base = p.i_base * (unsigned)D, N = st.n_total + n_chunk;
  if (n_base != st.n_total - st.n_hist) return CS_BASE_NOT_HISTORY;                     // the history starts at the first launched column
  if (p.n_keep > cs_keep_max(U, D)) return CS_KEEP_ABOVE_SLOT;
  if (p.n_base_next < n_base) return CS_BASE_MOVED_BACK;                                // ... so the next push never reads in front of it
  if (p.n_base_next > (p.m_end * (unsigned)D + U - 1) / U) return CS_BASE_BEHIND_NEXT_WINDOW;   // output M's window starts at ceil(M D / U)
  if (p.n_base_next + p.n_keep != N) return CS_COUNT_MISMATCH;
  // every stored output lies in a launched column, and its taps meet samples that have arrived
  for (ull m = p.m_first; m < p.m_end; ++m) {
    const ull i = m / U;
    if (i < p.i_base || i >= p.i_base + (ull)p.grid_x * sh.cols) return CS_OUTPUT_NOT_LAUNCHED;
    if ((m * (unsigned)D + Tg - 1) / U >= N) return CS_WINDOW_NOT_ARRIVED;
  }
  // every staged index of every launched workgroup: a real sample of the history or the chunk, or a zero behind the chunk's end
  for (unsigned bx = 0; bx < p.grid_x; ++bx) {
    const ull n0 = (p.i_base + (ull)bx * sh.cols) * (unsigned)D;
    for (int idx = 0; idx < sh.xrows * D; ++idx) {
      const ull n = n0 + (unsigned)idx;
      if (n < n_base) return CS_READ_BEFORE_BASE;
      const cs_where w = cs_source(n, n_base, st.n_hist, n_chunk);
      if (w.part == CS_HIST && !(w.off < st.n_hist && n_base + w.off == n)) return CS_HIST_OUTSIDE;
      if (w.part == CS_CHUNK && !(w.off < n_chunk && st.n_total + w.off == n)) return CS_CHUNK_OUTSIDE;
      if (w.part == CS_ZERO && n < N) return CS_ZERO_INSIDE;
    }
  }
  // k_chan_keep: n_keep real samples from the next base on
  for (unsigned s = 0; s < p.n_keep; ++s) {
    const cs_where w = cs_source(p.n_base_next - n_base + s, 0, st.n_hist, n_chunk);
    if (w.part == CS_ZERO || (w.part == CS_HIST ? w.off >= st.n_hist : w.off >= n_chunk)) return CS_KEEP_SOURCE;
  }
  st.n_hist = p.n_keep;
  st.n_total = N;
  return CS_OK;
}

static ull rnd(ull &s) {      // xorshift64*
  s ^= s >> 12, s ^= s << 25, s ^= s >> 27;
  return s * 2685821657736338717ull;
}
// a seeded chunk length: runs of 0, 1 and 2, lengths up to 3 D, now and then several workgroups' worth
static ull chunk_len(ull &s, int &run, int U, int D, int cols) {
  if (run > 0) { --run; return rnd(s) % 3; }
  const ull r = rnd(s) % 16;
  if (r == 0) { run = 1 + (int)(rnd(s) % 40); return rnd(s) % 3; }
  if (r == 1) return 1 + rnd(s) % ((ull)3 * cols * D);
  if (r == 2) return 16ull * D / U + rnd(s) % 3;
  return 1 + rnd(s) % (3ull * D);
}
// n_push seeded pushes of a fresh stream.  Returns 0, or 100 * (1 + index of the push) + the premise it broke.
extern "C" long long cs_host_check_stream(int U, int D, ull seed, int n_push) {
  stream_state st = {0, 0};
  ull s = seed * 0x9E3779B97F4A7C15ull + 88172645463325252ull;
  int run = seed % 3 == 0 ? 25 : 0;      // a third of the streams open with a run of tiny chunks
  const int cols = shape_of(U, D).cols;
  for (int k = 0; k < n_push; ++k)
    if (const int rc = check_push(st, chunk_len(s, run, U, D, cols), U, D)) return 100ll * (1 + k) + rc;
  return 0;
}
// the same with given chunk lengths (the tests' own sequences)
extern "C" long long cs_host_check_chunks(int U, int D, const ull *chunks, int n_push) {
  stream_state st = {0, 0};
  for (int k = 0; k < n_push; ++k)
    if (const int rc = check_push(st, chunks[k], U, D)) return 100ll * (1 + k) + rc;
  return 0;
}

// ---- refusals: chan_stream_refusal, and open's use of chan_refusal
extern "C" const char *cs_host_refusal(int entry, int is_open, int fmt, ull d_chunk, ull n_chunk, ull d_out, unsigned row_stride, unsigned out_cap,
                                       ull n_emit) {
  const ChanPush a = {is_open != 0, fmt, reinterpret_cast<const void *>(d_chunk), n_chunk, reinterpret_cast<void *>(d_out), row_stride, out_cap, n_emit};
  return chan_stream_refusal(a, (ChanStreamEntry)entry);
}
extern "C" const char *cs_host_open_refusal(int is_open, int fmt, double fs_in, int up, int down, const double *f_shift, int n_ch) {
  alignas(16) static char any[16];
  const ChanCall a = {any, fmt, ~0ull, fs_in, up, down, f_shift, n_ch, any, 1};
  const char *what = chan_refusal(a, CHAN_RATE);
  return what ? what : chan_stream_refusal(ChanPush{is_open != 0}, CHAN_STREAM_OPEN);
}

#ifndef CS_HOST_MAIN
// ---- the walk.  D += A B of one v_mfma_f32_32x32x2_f32 (tests/host/chan_rate_host.cpp): fp32, one fma per k.  acc[v][l].
static void mfma(const float *a, const float *b, float (*acc)[64]) {
  for (int v = 0; v < 16; ++v)
    for (int h = 0; h < 2; ++h) {
      const int row = cr_acc_row(v, 32 * h);
      const float a0 = a[row], a1 = a[32 + row];
      float *d = acc[v] + 32 * h;
      for (int c = 0; c < 32; ++c) d[c] = __builtin_fmaf(a1, b[32 + c], __builtin_fmaf(a0, b[c], d[c]));
    }
}

// One launch of either form's kernel on the CPU.  stream == false: the one-shot launch (x: the capture of n_in samples, outputs m <
// m_end to out[ch * row_stride + m]).  stream == true: a push (x: the chunk, sa as the launcher fills it).  A column tile is 32
// columns of one residue; which wave runs it changes nothing.
template <int FMT>
static long long launch(bool stream, const void *x, ull n_in, int U, int D, const float *tab, const ull *step, int n_ch, float2 *out, size_t out_elems,
                        unsigned grid_x, const cs_args &sa) {
  const shape sh = shape_of(U, D);
  const int n_rb = (n_ch + CR_CARRIERS - 1) / CR_CARRIERS;
  std::vector<float> xs((size_t)sh.xrows * (2 * D + 1));
  long long outside = 0;
  for (int rb = 0; rb < n_rb; ++rb)
    for (unsigned bx = 0; bx < grid_x; ++bx) {
      std::fill(xs.begin(), xs.end(), NAN);      // LDS is not initialised
      const ull i0 = (stream ? sa.i_base : 0ull) + (ull)bx * sh.cols;
      const ull n0 = i0 * (unsigned)D;
      for (int idx = 0; idx < sh.xrows * D; ++idx) {
        const int o = cr_stage_offset(idx, D);
        const ull n = n0 + (unsigned)idx;
        float2 v;
        if (stream) v = cs_sample<FMT>(sa.hist, x, cs_source(n, sa.i_base * (unsigned)D, sa.n_hist, n_in));
        else v = n < n_in ? chan_sample<FMT>(x, n) : make_float2(0.f, 0.f);
        xs[o] = v.x;
        xs[o + 1] = v.y;
      }
      for (int t = 0; t < U * (sh.cols / 32); ++t) {
        const cr_tile tl = cr_tile_of(t, U, D);
        // a tile none of whose columns is stored leaves no trace (the kernel computes it and drops it): not walked
        if (cr_col_of(i0, tl, 31, U, D).m < sa.m_first || cr_col_of(i0, tl, 0, U, D).m >= sa.m_end) continue;
        float acc[16][64] = {};
        float a[64], b[64];
        cr_pos w = cr_b_first(tl, D);
        for (int s4 = 0; s4 < sh.G; ++s4)
          for (int i = 0; i < 4; ++i) {
            for (int lane = 0; lane < 64; ++lane) {
              a[lane] = tab[cr_a_group(rb, tl.q, s4, lane, U, sh.G) * 4 + i];
              b[lane] = xs[cr_b_base(tl, lane, D) + cr_b_step(w, D)];
            }
            mfma(a, b, acc);
            cr_b_next(w, D);
          }
        for (int lane = 0; lane < 64; ++lane) {
          const cr_col col = cr_col_of(i0, tl, lane, U, D);
          if (col.m < sa.m_first || col.m >= sa.m_end) continue;
          for (int v = 0; v < 16; v += 2) {
            const int ch = cr_acc_carrier(rb, v, lane);
            if (ch >= n_ch) continue;
            const size_t o = (size_t)ch * sa.row_stride + (size_t)(col.m - sa.m_first);
            if (o >= out_elems) { ++outside; continue; }
            out[o] = cr_rotate(acc[v][lane], acc[v + 1][lane], step[ch], col.nd);
          }
        }
      }
    }
  return outside;
}

// A whole stream on the CPU: the capture x of n_in samples pushed as the given chunks (their sum is n_in), every push written
// behind the last into out[n_ch][M(n_in)]; n_push == 0: ONE one-shot launch instead.  taps: any 16 D floats.  Returns the stores that
// fell outside out, -1 for a chunk sequence of the wrong length, -2 for a push whose (m_first, n_emit) is not M(N)'s.
template <int FMT>
static long long run(const char *x, ull n_in, int U, int D, const ull *step, const float *taps, int n_ch, float2 *out, const ull *chunks, int n_push) {
  const shape sh = shape_of(U, D);
  const int n_rb = (n_ch + CR_CARRIERS - 1) / CR_CARRIERS;
  const unsigned sb = chan_sample_bytes(FMT);
  const ull n_out = cs_count(n_in, U, D);
  std::vector<float> tab((size_t)n_rb * U * sh.G * 256);
  for (size_t e = 0; e < tab.size(); ++e) tab[e] = cr_table_value(e, step, taps, n_ch, U, D, sh.G);
  if (!n_push) {
    const cs_args whole = {nullptr, 0, 0, 0, n_out, (unsigned)n_out};
    const unsigned grid_x = (unsigned)(((n_out + U - 1) / U + sh.cols - 1) / sh.cols);
    return launch<FMT>(false, x, n_in, U, D, tab.data(), step, n_ch, out, (size_t)n_ch * n_out, grid_x, whole);
  }
  std::vector<char> hist[2] = {std::vector<char>((size_t)cs_keep_max(U, D) * sb), std::vector<char>((size_t)cs_keep_max(U, D) * sb)};
  int cur = 0;
  unsigned n_hist = 0;
  ull n_total = 0, filled = 0;
  long long outside = 0;
  for (int k = 0; k < n_push; ++k) {
    const ull n_chunk = chunks[k];
    if (n_total + n_chunk > n_in) return -1;
    if (!n_chunk) continue;
    const char *chunk = x + n_total * sb;
    const cs_plan p = cs_plan_push(n_total, n_chunk, U, D, sh.cols);
    if (p.m_first != filled) return -2;
    if (p.grid_x) {
      const cs_args sa = {hist[cur].data(), p.i_base, n_hist, p.m_first, p.m_end, (unsigned)n_out};
      outside += launch<FMT>(true, chunk, n_chunk, U, D, tab.data(), step, n_ch, out + filled, (size_t)n_ch * n_out - filled, p.grid_x, sa);
    }
    // k_chan_keep
    const unsigned w = sb / 2;
    const uint16_t *h16 = (const uint16_t *)hist[cur].data(), *c16 = (const uint16_t *)chunk;
    uint16_t *dst = (uint16_t *)hist[cur ^ 1].data();
    if (p.n_keep > cs_keep_max(U, D)) return -3;
    for (unsigned e = 0; e < p.n_keep * w; ++e) {
      const unsigned s = e / w, u = e - s * w;
      const cs_where from = cs_source(p.n_base_next - p.i_base * (unsigned)D + s, 0, n_hist, n_chunk);
      dst[e] = from.part == CS_ZERO ? (uint16_t)0 : (from.part == CS_HIST ? h16 : c16)[from.off * w + u];
    }
    cur ^= 1;
    n_hist = p.n_keep;
    n_total += n_chunk;
    filled = p.m_end;
  }
  return n_total == n_in && filled == n_out ? outside : -1;
}

extern "C" long long cs_host_run(int fmt, const void *x, ull n_in, int U, int D, const ull *step, const float *taps, int n_ch, float *out,
                                 const ull *chunks, int n_push) {
  if (fmt == LCS_FMT_C64) return run<LCS_FMT_C64>((const char *)x, n_in, U, D, step, taps, n_ch, (float2 *)out, chunks, n_push);
  if (fmt == LCS_FMT_IQ_S16) return run<LCS_FMT_IQ_S16>((const char *)x, n_in, U, D, step, taps, n_ch, (float2 *)out, chunks, n_push);
  if (fmt == LCS_FMT_IQ_S8) return run<LCS_FMT_IQ_S8>((const char *)x, n_in, U, D, step, taps, n_ch, (float2 *)out, chunks, n_push);
  return -4;
}
#else
// The stand-alone form: counting and source map over every rate of the domain, a few seeded streams each.  Prints one line, exits
// with 1 at the first premise broken.
static int gcd(int a, int b) { return b ? gcd(b, a % b) : a; }
int main() {
  long long pairs = 0, counted = 0, pushes = 0;
  for (int U = 1; U < 128; ++U)
    for (int D = U + 1; D <= 128; ++D) {
      if (D > 16 * U || gcd(U, D) != 1) continue;
      const long long n = cs_host_check_counts(U, D);
      if (n < 0) { std::printf("counting fails at %d/%d, N = %lld\n", U, D, -n - 1); return 1; }
      for (ull seed = 0; seed < 3; ++seed) {
        const long long rc = cs_host_check_stream(U, D, seed + 7ull * U + 1000ull * D, 60);
        if (rc) { std::printf("stream %d/%d seed %llu: push %lld breaks premise %lld\n", U, D, seed, rc / 100 - 1, rc % 100); return 1; }
        pushes += 60;
      }
      ++pairs, counted += n;
    }
  // the refusal routine reads nothing through its pointers
  if (!cs_host_refusal(CHAN_STREAM_PUSH, 1, LCS_FMT_IQ_S16, 0x10002, 5, 0x20008, 4, 8, 1)) { std::printf("refusal\n"); return 1; }
  std::printf("%lld rates, %lld counts, %lld pushes: ok\n", pairs, counted, pushes);
  return 0;
}
#endif
