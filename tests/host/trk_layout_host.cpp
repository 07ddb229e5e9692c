// Host-side harness for trk_layout.h, the tracker's buffer layouts and the continuous form's integer rules (nothing else is
// included): tests/test_trk_layout_host.py walks every shape of its domain through the functions below.  With
// -DTRK_LAYOUT_HOST_MAIN the file is a stand-alone program that walks the same domain by itself and checks what can be checked
// without a reference: the form that is built with -fsanitize=address,undefined.  Test infrastructure.
#include "../../lte-cell-scanner_amd/csrc/trk_layout.h"

extern "C" void trk_host_table(int *n_arr, int *n_buf, int *buf, int *elem, int *align) {
  *n_arr = TA_N;
  *n_buf = TB_N;
  for (int a = 0; a < TA_N; ++a) { buf[a] = TRK_ROWS[a].buf; elem[a] = TRK_ROWS[a].elem; align[a] = TRK_ROWS[a].align; }
}
extern "C" void trk_host_caps(int n_sym, int *out /*rs_cap, n_off, hf_cap*/) { out[0] = trk_rs_cap(n_sym); out[1] = trk_n_off(n_sym); out[2] = trk_hf_cap(n_sym); }
extern "C" void trk_host_grow(int cap_cells, int cap_sym, int n_cells, int n_sym, int *out /*fits, cells, symbols*/) {
  TrkShape cap, s;
  cap.n_cells = cap_cells; cap.n_sym = cap_sym; s.n_cells = n_cells; s.n_sym = n_sym;
  const TrkShape g = trk_grow(cap, s);
  out[0] = trk_fits(cap, s) ? 1 : 0; out[1] = g.n_cells; out[2] = g.n_sym;
}
static void put(const TrkLay &l, uint64_t *off, uint64_t *len, uint64_t *bytes) {
  for (int a = 0; a < TA_N; ++a) { off[a] = l.off[a]; len[a] = l.n[a]; }
  for (int b = 0; b < TB_N; ++b) bytes[b] = l.bytes[b];
}
// off, len [n][TA_N] (bytes, elements), bytes [n][TB_N]: the layout of n shapes / of n capacities of the cutter
extern "C" void trk_host_layouts(int n, const int *n_cells, const int *n_sym, uint64_t *off, uint64_t *len, uint64_t *bytes) {
  for (int i = 0; i < n; ++i) {
    TrkShape s;
    s.n_cells = n_cells[i]; s.n_sym = n_sym[i];
    put(trk_layout(s), off + (size_t)i * TA_N, len + (size_t)i * TA_N, bytes + (size_t)i * TB_N);
  }
}
extern "C" void trk_host_cut_layouts(int n, const uint64_t *cells_cap, const uint64_t *n_cap, uint64_t *off, uint64_t *len, uint64_t *bytes) {
  for (int i = 0; i < n; ++i) put(trk_layout(trk_cut_dims(cells_cap[i], n_cap[i])), off + (size_t)i * TA_N, len + (size_t)i * TA_N, bytes + (size_t)i * TB_N);
}
extern "C" void trk_host_stream_step(long long n_seen, long long tail_start, int n_sym, int F, long long *out /*n_tail, L, n_after, T_next, keep_from, n_keep*/) {
  const TrkStreamStep s = trk_stream_step(n_seen, tail_start, n_sym, F);
  out[0] = s.n_tail; out[1] = s.L; out[2] = s.n_after; out[3] = s.T_next; out[4] = (long long)s.keep_from; out[5] = (long long)s.n_keep;
}
extern "C" int trk_host_mib_first(long long mib_next, long long T, int F) { return trk_mib_first(mib_next, T, F); }

#ifdef TRK_LAYOUT_HOST_MAIN
#include <cstdio>
#include <vector>
static const int SYMS[17] = {1, 6, 7, 119, 120, 121, 139, 140, 141, 479, 480, 500, 839, 840, 980, 1260, 2000};
static long fails = 0;
#define REQUIRE(x) do { if (!(x)) { if (++fails < 10) std::fprintf(stderr, "line %d: %s\n", __LINE__, #x); } } while (0)

// the arrays of buffers first .. last - 1 of layout `l`: aligned, behind each other, within what `cap` gives their buffer
static void check(const TrkLay &l, const TrkLay &cap, int first, int last) {
  size_t end[TB_N] = {};
  for (int a = 0; a < TA_N; ++a) {
    const TrkRow &r = TRK_ROWS[a];
    if (r.buf < first || r.buf >= last) continue;
    REQUIRE(l.off[a] % r.align == 0 && l.off[a] >= end[r.buf]);
    end[r.buf] = l.off[a] + l.size(a);
    REQUIRE(end[r.buf] <= cap.bytes[r.buf] && end[r.buf] <= l.bytes[r.buf]);
  }
}
int main() {
  long n_pairs = 0;
  for (int cc = 1; cc <= 64; ++cc)
    for (int is = 0; is < 17; ++is) {
      TrkShape none, first;
      first.n_cells = cc; first.n_sym = SYMS[is];
      const TrkShape cap = trk_grow(none, first);             // every capacity the growth rule gives: these cells, a symbol count with its head room
      REQUIRE(trk_fits(cap, first) && cap.n_cells == cc && cap.n_sym >= SYMS[is]);
      const TrkLay lc = trk_layout(cap);
      for (int c = 1; c <= cc; ++c)
        for (int js = 0; js < 17 && SYMS[js] <= cap.n_sym; ++js) {
          TrkShape s;
          s.n_cells = c; s.n_sym = SYMS[js];
          REQUIRE(trk_fits(cap, s));
          const TrkLay l = trk_layout(s);
          check(l, lc, TB_TD, TB_STAGE);
          check(l, l, TB_STAGE, TB_ACFD);                     // the staging block is reserved for the block's own shape
          check(l, lc, TB_ACFD, TB_CUT_HIT);
          ++n_pairs;
        }
      for (int c = 1; c <= cc; ++c) {                          // the cutter: capacities (cc cells, c x symbols samples) a sequence of calls can reach
        const size_t n_cap = (size_t)c * SYMS[is];
        if (n_cap < (size_t)cc) continue;
        const TrkLay l = trk_layout(trk_cut_dims((size_t)cc, n_cap));
        check(l, l, TB_CUT_HIT, TB_N);
        REQUIRE(l.n[TA_CUT_HIT] == n_cap && l.n[TA_CUT_LATE] == n_cap && l.n[TA_CUT_N] == (size_t)cc && l.n[TA_CUT_FLAGS] == (size_t)cc && l.n[TA_CUT_POS] == (size_t)cc);
      }
    }
  // the stream rules: 200 cut sequences per frame length from a linear congruential generator
  unsigned long long x = 12345;
  auto rnd = [&](int n) { x = x * 6364136223846793005ull + 1442695040888963407ull; return (int)((x >> 33) % (unsigned)n); };
  for (int F = 120; F <= 140; F += 20)
    for (int seq = 0; seq < 200; ++seq) {
      long long n_seen = 0, tail = 0;
      const int calls = 1 + rnd(40);
      for (int k = 0; k < calls; ++k) {
        const int n_sym = 1 + rnd(1500);
        const TrkStreamStep s = trk_stream_step(n_seen, tail, n_sym, F);
        REQUIRE(s.T_next % F == 0 && s.T_next >= tail && s.keep_from + s.n_keep == (size_t)s.L && s.n_after == n_seen + n_sym);
        if (s.n_after < 3 * F) REQUIRE(s.n_keep == (size_t)s.n_after); else REQUIRE(s.n_keep >= (size_t)(3 * F) && s.n_keep < (size_t)(4 * F));
        REQUIRE(trk_mib_first(tail / F + rnd(6) - 2, tail, F) >= 0);
        n_seen = s.n_after; tail = s.T_next;
      }
    }
  std::printf("%ld pairs, %ld failures\n", n_pairs, fails);
  return fails ? 1 : 0;
}
#endif
