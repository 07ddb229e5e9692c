// Host-side harness for the dongle-data predicate of lte_device.h (dongle_component_f32 / _f64: the same __host__ __device__
// code k_c64_probe_u8 and k_ingest_c128 decide by): tests/test_probe_host.py runs the float flavour over all 2^32 bit patterns
// against a table built without it, and the double flavour over the edges.  Test infrastructure.
#include "../../lte-cell-scanner_amd/csrc/lte_device.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

// the expression the float probe used before (one fma, then the test for integrality on the ROUNDED sum): kept here so that the
// test can show it fails the specification
static bool old_sum_expression(float x, unsigned char *byte) {
  const float v = std::fma(x, 128.0f, 127.0f);
  const float r = rintf(v);
  const bool ok = v == r && r >= 0.0f && r <= 255.0f;
  *byte = (unsigned char)(int)fminf(fmaxf(r, 0.0f), 255.0f);
  return ok;
}

// Reference that shares no code with the predicate: the 256 values by integer arithmetic and one division in double ((b - 127) / 128
// is exact in double, and exact as a float: at most 8 significant bits), their bit patterns sorted, a pattern looked up by
// bisection.  -0.0 is the one extra pattern that compares equal to a table value.
struct Ref {
  uint32_t bits[257];
  unsigned char byte[257];
  Ref() {
    std::pair<uint32_t, unsigned char> e[257];
    for (int b = 0; b < 256; ++b) {
      const float f = (float)((double)(b - 127) / 128.0);
      std::memcpy(&e[b].first, &f, 4);
      e[b].second = (unsigned char)b;
    }
    e[256] = {0x80000000u, (unsigned char)127};      // -0.0
    std::sort(e, e + 257);
    for (int i = 0; i < 257; ++i) { bits[i] = e[i].first; byte[i] = e[i].second; }
  }
  bool lookup(uint32_t u, unsigned char *b) const {
    const uint32_t *p = std::lower_bound(bits, bits + 257, u);
    if (p == bits + 257 || *p != u) return false;
    *b = byte[p - bits];
    return true;
  }
};

// All 2^32 float bit patterns through the predicate (which = 0) or the old expression (which = 1), n_threads threads.
// out[0] = patterns accepted, out[1] = patterns where (ok, byte) differs from the reference, out[2] = accepted by the reference,
// out[3] = the first differing pattern (if any).
extern "C" void probe_host_sweep_f32(int which, int n_threads, unsigned long long *out) {
  const Ref ref;
  std::atomic<unsigned long long> n_acc{0}, n_bad{0}, n_ref{0}, first_bad{~0ull};
  std::vector<std::thread> th;
  n_threads = std::max(1, std::min(n_threads, 64));
  for (int w = 0; w < n_threads; ++w)
    th.emplace_back([&, w] {
      const unsigned long long lo = (1ull << 32) * w / n_threads, hi = (1ull << 32) * (w + 1) / n_threads;
      unsigned long long acc = 0, bad = 0, nref = 0, fb = ~0ull;
      for (unsigned long long u = lo; u < hi; ++u) {
        const uint32_t u32 = (uint32_t)u;
        float x;
        std::memcpy(&x, &u32, 4);
        unsigned char b = 0, rb = 0;
        const bool ok = which ? old_sum_expression(x, &b) : dongle_component_f32(x, &b);
        // cheap pre-filter for the reference: every table value has 16 zero low bits (8 significant bits at most)
        const bool rok = (u32 & 0xFFFFu) == 0 && ref.lookup(u32, &rb);
        acc += ok;
        nref += rok;
        if (ok != rok || (ok && b != rb)) { ++bad; if (fb == ~0ull) fb = u; }
      }
      n_acc += acc; n_bad += bad; n_ref += nref;
      unsigned long long cur = first_bad.load();
      while (fb < cur && !first_bad.compare_exchange_weak(cur, fb)) {}
    });
  for (auto &t : th) t.join();
  out[0] = n_acc; out[1] = n_bad; out[2] = n_ref; out[3] = first_bad;
}

extern "C" int probe_host_f32(float x, unsigned char *byte) { return dongle_component_f32(x, byte) ? 1 : 0; }
extern "C" int probe_host_f64(double x, unsigned char *byte) { return dongle_component_f64(x, byte) ? 1 : 0; }
extern "C" int probe_host_old_f32(float x, unsigned char *byte) { return old_sum_expression(x, byte) ? 1 : 0; }
