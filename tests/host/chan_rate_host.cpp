// Host-side twin of the rational channelizer (channelizer_rate.hip): a workgroup walked on the CPU -- staging, waves, tiles,
// k-steps, one v_mfma_f32_32x32x2_f32 as a 64-lane loop, guards, phase rotation, stores -- with every index taken from the
// __host__ __device__ helpers of channelizer.h the kernels and the launcher call.  tests/test_channelizer_rate_twin_host.py
// compares it with the contract over the whole rate domain.  Test infrastructure.
#include <cmath>
#if !(defined(__GLIBC__) && defined(__GLIBC_PREREQ))
#define CR_HOST_OWN_PI 1
#elif !__GLIBC_PREREQ(2, 41)
#define CR_HOST_OWN_PI 1
#endif
#ifdef CR_HOST_OWN_PI
// sin / cos of x half-turns; exact at every multiple of a quarter turn: x = k / 2 + f with |f| <= 1/4 exactly, and f = 0 gives (0, 1)
static void cr_host_sincospi(double x, double *s, double *c) {
  const double r = x - 2.0 * std::nearbyint(0.5 * x);      // [-1, 1], exact
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
#include <vector>

extern "C" void cr_host_geometry(int U, int D, long long *out /*G, NI, xrows, lds_bytes*/) {
  const cr_geom g = cr_geometry(U, D);
  out[0] = g.G, out[1] = g.NI, out[2] = g.xrows, out[3] = (long long)g.lds_bytes;
}

extern "C" void cr_host_table(const unsigned long long *step, const float *taps, int n_ch, int U, int D, float *tab /*[n_rb U G 256]*/) {
  const int G = cr_geometry(U, D).G, n_rb = (n_ch + CR_CARRIERS - 1) / CR_CARRIERS;
  const size_t total = (size_t)n_rb * U * G * 256;
  for (size_t e = 0; e < total; ++e) tab[e] = cr_table_value(e, step, taps, n_ch, U, D, G);
}

// the LDS float offset every lane reads at every k-step of every tile of a workgroup: out[U NI][4 G][64]
extern "C" void cr_host_read_offsets(int U, int D, int *out) {
  const cr_geom g = cr_geometry(U, D);
  for (int wave = 0; wave < 4; ++wave)
    for (int t = wave; t < U * g.NI; t += 4) {
      const cr_tile tl = cr_tile_of(t, U, D);
      cr_pos w = cr_b_first(tl, D);
      for (int j = 0; j < 4 * g.G; ++j) {
        for (int l = 0; l < 64; ++l) out[((size_t)t * 4 * g.G + j) * 64 + l] = cr_b_base(tl, l, D) + cr_b_step(w, D);
        cr_b_next(w, D);
      }
    }
}

// the LDS float offset of the real part of every staged sample: out[xrows D]
extern "C" void cr_host_stage_offsets(int U, int D, int *out) {
  const cr_geom g = cr_geometry(U, D);
  for (int idx = 0; idx < g.xrows * D; ++idx) out[idx] = cr_stage_offset(idx, D);
}

// how often a launch stores every (ch, m): count[n_ch][n_out]; returns the stores that fall outside that array
extern "C" long long cr_host_store_census(int U, int D, int n_ch, unsigned n_out, int *count) {
  const cr_geom g = cr_geometry(U, D);
  const int n_rb = (n_ch + CR_CARRIERS - 1) / CR_CARRIERS;
  long long outside = 0;
  for (int rb = 0; rb < n_rb; ++rb)
    for (unsigned bx = 0; bx < cr_grid_x(n_out, U, g.NI); ++bx) {
      const unsigned long long i0 = (unsigned long long)bx * (32u * g.NI);
      for (int wave = 0; wave < 4; ++wave)
        for (int t = wave; t < U * g.NI; t += 4) {
          const cr_tile tl = cr_tile_of(t, U, D);
          for (int lane = 0; lane < 64; ++lane) {
            const cr_col col = cr_col_of(i0, tl, lane, U, D);
            if (col.m >= n_out) continue;
            for (int v = 0; v < 16; v += 2) {
              const int ch = cr_acc_carrier(rb, v, lane);
              if (ch >= n_ch) continue;
              const unsigned long long o = (unsigned long long)ch * n_out + col.m;
              if (ch < 0 || o >= (unsigned long long)n_ch * n_out) ++outside;
              else ++count[o];
            }
          }
        }
    }
  return outside;
}

// D += A B of one v_mfma_f32_32x32x2_f32: lane l holds A[row l & 31][k l >> 5] and B[k l >> 5][col l & 31]; register v of lane l is
// D[row cr_acc_row(v, l)][col l & 31]; fp32, one fma per k.  acc[v][l].
static inline __attribute__((always_inline)) void mfma_body(const float *a, const float *b, float (*acc)[64]) {
  for (int v = 0; v < 16; ++v)
    for (int h = 0; h < 2; ++h) {
      const int row = cr_acc_row(v, 32 * h);
      const float a0 = a[row], a1 = a[32 + row];
      float *d = acc[v] + 32 * h;
      for (int c = 0; c < 32; ++c) d[c] = __builtin_fmaf(a1, b[32 + c], __builtin_fmaf(a0, b[c], d[c]));
    }
}
#if defined(__x86_64__)
__attribute__((target("avx2,fma"))) static void mfma_hw(const float *a, const float *b, float (*acc)[64]) { mfma_body(a, b, acc); }
#endif
static void mfma_sw(const float *a, const float *b, float (*acc)[64]) { mfma_body(a, b, acc); }

template <int FMT>
static long long run(const void *x, unsigned long long n_in, int U, int D, const unsigned long long *step, const float *taps, int n_ch, float2 *out,
                     unsigned n_out) {
  const cr_geom g = cr_geometry(U, D);
  const int G = g.G, NI = g.NI, xrows = g.xrows, n_rb = (n_ch + CR_CARRIERS - 1) / CR_CARRIERS;
  void (*mfma)(const float *, const float *, float (*)[64]) = mfma_sw;
#if defined(__x86_64__)
  if (__builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma")) mfma = mfma_hw;
#endif
  std::vector<float> tab((size_t)n_rb * U * G * 256);
  cr_host_table(step, taps, n_ch, U, D, tab.data());
  std::vector<float> xs(g.lds_bytes / sizeof(float));
  long long outside = 0;
  for (int rb = 0; rb < n_rb; ++rb)
    for (unsigned bx = 0; bx < cr_grid_x(n_out, U, NI); ++bx) {
      // LDS is not initialised: what the staging loop leaves unwritten (the pad float of every row) poisons a sum that reads it
      std::fill(xs.begin(), xs.end(), NAN);
      const unsigned long long i0 = (unsigned long long)bx * (32u * NI);
      const unsigned long long n0 = i0 * (unsigned)D;
      for (int idx = 0; idx < xrows * D; ++idx) {
        const int o = cr_stage_offset(idx, D);
        const unsigned long long n = n0 + (unsigned)idx;
        const float2 v = n < n_in ? chan_sample<FMT>(x, n) : make_float2(0.f, 0.f);
        xs[o] = v.x;
        xs[o + 1] = v.y;
      }
      for (int wave = 0; wave < 4; ++wave)
        for (int t = wave; t < U * NI; t += 4) {
          const cr_tile tl = cr_tile_of(t, U, D);
          float acc[16][64] = {};
          float a[64], b[64];
          cr_pos w = cr_b_first(tl, D);
          for (int s4 = 0; s4 < G; ++s4)
            for (int i = 0; i < 4; ++i) {
              for (int lane = 0; lane < 64; ++lane) {
                a[lane] = tab[cr_a_group(rb, tl.q, s4, lane, U, G) * 4 + i];
                b[lane] = xs[cr_b_base(tl, lane, D) + cr_b_step(w, D)];
              }
              mfma(a, b, acc);
              cr_b_next(w, D);
            }
          for (int lane = 0; lane < 64; ++lane) {
            const cr_col col = cr_col_of(i0, tl, lane, U, D);
            if (col.m >= n_out) continue;
            for (int v = 0; v < 16; v += 2) {
              const int ch = cr_acc_carrier(rb, v, lane);
              if (ch >= n_ch) continue;
              const unsigned long long o = (unsigned long long)ch * n_out + col.m;
              if (o >= (unsigned long long)n_ch * n_out) { ++outside; continue; }
              out[o] = cr_rotate(acc[v][lane], acc[v + 1][lane], step[ch], col.nd);
            }
          }
        }
    }
  return outside;
}

// the rational form's launch (lcs_launch_channelize, up > 1) on the CPU; out[n_ch][n_out] (re, im) floats.  Returns the number of stores that
// fell outside out (none were made), -1 for an unknown format.
extern "C" long long cr_host_run(int fmt, const void *x, unsigned long long n_in, int U, int D, const unsigned long long *step, const float *taps,
                                 int n_ch, float *out, unsigned n_out) {
  if (fmt == LCS_FMT_C64) return run<LCS_FMT_C64>(x, n_in, U, D, step, taps, n_ch, (float2 *)out, n_out);
  if (fmt == LCS_FMT_IQ_S16) return run<LCS_FMT_IQ_S16>(x, n_in, U, D, step, taps, n_ch, (float2 *)out, n_out);
  if (fmt == LCS_FMT_IQ_S8) return run<LCS_FMT_IQ_S8>(x, n_in, U, D, step, taps, n_ch, (float2 *)out, n_out);
  return -1;
}
