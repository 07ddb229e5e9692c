// Host-side twin of the channelizer stream's 8-bit captures (channelizer.h: cs_need, cs_cap_count, cs_cap_done, cs_cap_segment,
// cs_cap_plan, chan_stream_u8_refusal): the inverse of the output count over the rate domain, the launcher's cut of a push where
// captures fill walked push by push, and the refusal rules.  tests/test_channelizer_stream_u8_host.py drives it as a library; built
// with -DCSU_HOST_MAIN it is a program of its own that runs the counting and plan cases over the whole rate domain (the form a
// sanitizer build takes).  Test infrastructure.
#include <cmath>
#if !(defined(__GLIBC__) && defined(__GLIBC_PREREQ))
#define CR_HOST_OWN_PI 1
#elif !__GLIBC_PREREQ(2, 41)
#define CR_HOST_OWN_PI 1
#endif
#ifdef CR_HOST_OWN_PI
// channelizer.h's table helpers name these; nothing here calls them (tests/host/chan_stream_host.cpp has the exact ones)
static double sinpi(double x) { return std::sin(M_PI * x); }
static double cospi(double x) { return std::cos(M_PI * x); }
static float sinpif(float x) { return (float)sinpi((double)x); }
static float cospif(float x) { return (float)cospi((double)x); }
#endif
#include "../../lte-cell-scanner_amd/csrc/channelizer.h"
#include <cstdio>
#include <vector>

typedef unsigned long long ull;

extern "C" ull csu_host_need(ull t, int U, int D) { return cs_need(t, U, D); }
extern "C" ull csu_host_count(ull N, int U, int D) { return cs_count(N, U, D); }
extern "C" ull csu_host_cap_done(ull N_prev, ull n_chunk, unsigned n_cap, int U, int D) { return cs_cap_done(N_prev, n_chunk, n_cap, U, D); }

// ---- cs_need against cs_count: M(need(t)) == t (U < D: the count grows by at most one per sample) and M(need(t) - 1) == t - 1, for t
// around 1, around multiples of U and out to 2^40.  Returns the number of t checked, or -(the first t that fails).
extern "C" long long csu_host_check_need(int U, int D) {
  std::vector<ull> ts;
  for (ull t = 1; t <= 3ull * U + 40; ++t) ts.push_back(t);
  for (ull k : {7ull, 100ull, 1000ull, 65536ull, 153600ull, 1ull << 20, 1ull << 31, (1ull << 40) / (ull)U})
    for (int d = -2; d <= 2; ++d) ts.push_back(k * U + d);
  for (int d = -3; d <= 0; ++d) ts.push_back((1ull << 40) + d);
  long long checked = 0;
  for (ull t : ts) {
    const ull N = cs_need(t, U, D);
    if (N < 1 || cs_count(N, U, D) != t || cs_count(N - 1, U, D) != t - 1) return -(long long)t;
    ++checked;
  }
  return checked;
}

// ---- a push's plan, as lcs_chan_stream_enqueue_u8 walks it
enum {
  CSU_OK = 0, CSU_SUM = 1, CSU_EMPTY_PIECE = 2, CSU_CROSSES = 3, CSU_EMIT = 4, CSU_FILLS_FLAG = 5, CSU_COMPLETE_INSIDE = 6, CSU_DONE = 7,
  CSU_FILLED = 8, CSU_NOT_LAST = 9
};
struct cap_state { ull n_total; unsigned filled; ull caps; };
// one push: every premise of the launcher, then the state moves on.  Returns the first premise broken; *n_done: the captures completed.
static int check_push(cap_state &st, ull n_chunk, unsigned n_cap, int U, int D, ull *n_done) {
  ull N = st.n_total, sum = 0, done = 0;
  unsigned filled = st.filled;
  int bad = CSU_OK;
  bool ended = false;
  cs_cap_plan(st.n_total, n_chunk, st.filled, n_cap, U, D, [&](const cs_seg &s) -> int {
    if (ended) return bad = CSU_NOT_LAST;                                               // only the last piece may leave its capture open
    if (!s.n) return bad = CSU_EMPTY_PIECE;
    const ull m0 = cs_count(N, U, D), m1 = cs_count(N + s.n, U, D);
    if (m0 % n_cap != filled) return bad = CSU_FILLED;                                  // the fill count is M(N) mod n_cap
    if (m1 - m0 != s.n_emit) return bad = CSU_EMIT;
    if ((ull)filled + s.n_emit > n_cap) return bad = CSU_CROSSES;                       // no piece's outputs cross a capture's end
    if (s.fills != (filled + s.n_emit == n_cap)) return bad = CSU_FILLS_FLAG;
    // a capture is complete exactly at a piece's end: never one sample earlier, and then exactly one
    if (cs_cap_count(N + s.n - 1, n_cap, U, D) != cs_cap_count(N, n_cap, U, D)) return bad = CSU_COMPLETE_INSIDE;
    if (cs_cap_count(N + s.n, n_cap, U, D) != cs_cap_count(N, n_cap, U, D) + (s.fills ? 1 : 0)) return bad = CSU_COMPLETE_INSIDE;
    N += s.n, sum += s.n;
    filled = s.fills ? 0u : filled + s.n_emit;
    done += s.fills ? 1 : 0;
    ended = !s.fills;
    return 0;
  });
  if (bad) return bad;
  if (sum != n_chunk) return CSU_SUM;
  if (done != cs_cap_done(st.n_total, n_chunk, n_cap, U, D)) return CSU_DONE;
  if (done != cs_count(st.n_total + n_chunk, U, D) / n_cap - cs_count(st.n_total, U, D) / n_cap) return CSU_DONE;
  st.n_total = N, st.filled = filled, st.caps += done;
  *n_done = done;
  return CSU_OK;
}

static ull rnd(ull &s) {      // xorshift64*
  s ^= s >> 12, s ^= s << 25, s ^= s >> 27;
  return s * 2685821657736338717ull;
}
// a seeded chunk length: runs of 0, 1 and 2, lengths up to 3 D, now and then up to 8 D, the filter's length or about half a capture
static ull chunk_len(ull &s, int &run, unsigned n_cap, int U, int D) {
  if (run > 0) { --run; return rnd(s) % 3; }
  const ull r = rnd(s) % 16;
  if (r == 0) { run = 1 + (int)(rnd(s) % 40); return rnd(s) % 3; }
  if (r == 1) return 1 + rnd(s) % (8ull * D);
  if (r == 2) return 16ull * D / U + rnd(s) % 3;
  if (r == 3) return cs_need(n_cap, U, D) / 2 + rnd(s) % (2ull * D);      // about half a capture
  return 1 + rnd(s) % (3ull * D);
}
// n_push seeded pushes of a fresh stream, push number n_push / 2 one chunk that completes exactly 9 captures; every chunk is also cut
// in two at a seeded place: the two parts complete, together, what the chunk completes.  Returns 0, or 100 * (1 + index of the push) +
// the premise it broke (90: the nine captures, 91: the cut).
extern "C" long long csu_host_check_stream(int U, int D, unsigned n_cap, ull seed, int n_push) {
  cap_state st = {0, 0, 0};
  ull s = seed * 0x9E3779B97F4A7C15ull + 88172645463325252ull;
  int run = seed % 3 == 0 ? 25 : 0;
  for (int k = 0; k < n_push; ++k) {
    ull n = chunk_len(s, run, n_cap, U, D), done = 0;
    const bool nine = k == n_push / 2;
    if (nine) n = cs_need((st.caps + 9) * n_cap, U, D) - st.n_total;      // up to the sample that completes the ninth capture from here
    if (n) {
      cap_state a = st;
      ull d0 = 0, d1 = 0;
      const ull cut = rnd(s) % (n + 1);
      if (check_push(a, cut, n_cap, U, D, &d0) || check_push(a, n - cut, n_cap, U, D, &d1)) return 100ll * (1 + k) + 91;
      if (const int rc = check_push(st, n, n_cap, U, D, &done)) return 100ll * (1 + k) + rc;
      if (d0 + d1 != done || a.n_total != st.n_total || a.filled != st.filled) return 100ll * (1 + k) + 91;
    } else if (const int rc = check_push(st, 0, n_cap, U, D, &done)) return 100ll * (1 + k) + rc;
    if (nine && (done != 9 || st.filled != 0)) return 100ll * (1 + k) + 90;
  }
  return 0;
}
// the same with given chunk lengths; done[k]: the captures push k completes
extern "C" long long csu_host_check_chunks(int U, int D, unsigned n_cap, const ull *chunks, int n_push, ull *done) {
  cap_state st = {0, 0, 0};
  for (int k = 0; k < n_push; ++k)
    if (const int rc = check_push(st, chunks[k], n_cap, U, D, done + k)) return 100ll * (1 + k) + rc;
  return 0;
}
// the pieces of one push: (n, n_emit, fills) triples into out[3 * cap]; returns their number
extern "C" long long csu_host_plan(ull N_prev, ull n_chunk, unsigned filled, unsigned n_cap, int U, int D, ull *out, long long cap) {
  long long k = 0;
  cs_cap_plan(N_prev, n_chunk, filled, n_cap, U, D, [&](const cs_seg &s) -> int {
    if (k < cap) out[3 * k] = s.n, out[3 * k + 1] = s.n_emit, out[3 * k + 2] = s.fills;
    ++k;
    return 0;
  });
  return k;
}

// ---- refusals: chan_stream_u8_refusal, open_u8's use of chan_refusal, and the float push on a stream of 8-bit captures
extern "C" const char *csu_host_refusal(int entry, int is_open, int is_u8, int fmt, ull d_chunk, ull n_chunk, ull d_out, ull d_gain, unsigned cap_room,
                                        unsigned n_cap, ull n_done) {
  const ChanPushU8 a = {is_open != 0, is_u8 != 0, fmt, reinterpret_cast<const void *>(d_chunk), n_chunk, reinterpret_cast<void *>(d_out),
                        reinterpret_cast<const float *>(d_gain), cap_room, n_cap, n_done};
  return chan_stream_u8_refusal(a, (ChanStreamEntry)entry);
}
extern "C" const char *csu_host_open_refusal(int is_open, int fmt, double fs_in, int up, int down, const double *f_shift, int n_ch, unsigned n_cap) {
  alignas(16) static char any[16];
  const ChanCall a = {any, fmt, ~0ull, fs_in, up, down, f_shift, n_ch, any, 1};
  const char *what = chan_refusal(a, CHAN_RATE);
  ChanPushU8 u = {is_open != 0};
  u.n_cap = n_cap;
  return what ? what : chan_stream_u8_refusal(u, CHAN_STREAM_OPEN);
}
extern "C" const char *csu_host_float_refusal(int entry, int is_open, int is_u8, ull n_chunk) {
  alignas(16) static char any[16];
  ChanPush a = {is_open != 0, LCS_FMT_IQ_S16, any, n_chunk, any, 8, 8, 1};
  a.is_u8 = is_u8 != 0;
  return chan_stream_refusal(a, (ChanStreamEntry)entry);
}

#ifdef CSU_HOST_MAIN
// The stand-alone form: cs_need and seeded plans over every rate of the domain at the four capture lengths.  Prints one line, exits
// with 1 at the first premise broken.
static int gcd(int a, int b) { return b ? gcd(b, a % b) : a; }
int main() {
  long long pairs = 0, needs = 0, pushes = 0;
  for (int U = 1; U < 128; ++U)
    for (int D = U + 1; D <= 128; ++D) {
      if (D > 16 * U || gcd(U, D) != 1) continue;
      const long long n = csu_host_check_need(U, D);
      if (n < 0) { std::printf("cs_need fails at %d/%d, t = %lld\n", U, D, -n); return 1; }
      for (unsigned n_cap : {1u, 5u, 257u, 153600u}) {
        const long long rc = csu_host_check_stream(U, D, n_cap, 3ull * U + 1000ull * D + n_cap, 30);
        if (rc) { std::printf("plan %d/%d n_cap %u: push %lld breaks premise %lld\n", U, D, n_cap, rc / 100 - 1, rc % 100); return 1; }
        pushes += 30;
      }
      ++pairs, needs += n;
    }
  // the refusal routine reads nothing through its pointers
  if (!csu_host_refusal(CHAN_STREAM_PUSH, 1, 1, LCS_FMT_IQ_S16, 0x10002, 5, 0x20010, 0, 4, 8, 1)) { std::printf("refusal\n"); return 1; }
  std::printf("%lld rates, %lld needs, %lld pushes: ok\n", pairs, needs, pushes);
  return 0;
}
#endif
