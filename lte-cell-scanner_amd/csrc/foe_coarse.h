// foe_coarse.h -- the PSS-only coarse frequency estimate and the rule that unwraps pss_sss_foe with it (lcs_set_foe_unwrap).
//
// pss_sss_foe measures ONE phase over pss_sss_dist samples: its estimate is the true offset modulo period = fs / pss_sss_dist
// (FDD 14 / 12 kHz, TDD 4660 / 4000 Hz).  The PSS alone gives an estimate that is coarse but has a range of +- fs / 128 = 15 kHz:
// the phase between the two halves of its time-domain symbol, 64 samples apart.  Per occurrence k, with P_k the first sample of
// the PSS's useful part, p the 128 samples of the template behind its cyclic prefix and f the hypothesis the peak was found at:
//   z_k[t] = capbuf[P_k + t] cis(-2 pi f / fs t) conj(p[t]),  A_k = sum_{t < 64} z_k[t],  B_k = sum_{t >= 64} z_k[t]
//   C = sum_k conj(A_k) B_k,  f_coarse = atan2(C.im, C.re) / (2 pi) fs / 64          (relative to f)
// and the integer number of periods the native estimate is off by is n = clamp(rint((f_coarse - (native - f)) / period), -1, 1).
// Everything here is plain fp64 and compiles for the host as well (tests/host/foe_coarse_host.cpp pins it to numpy);
// sss_foe.hip is the only device user: k_foe_fin_unwrap.
#pragma once
#include <math.h>
#include "lte_device.h"

#define FOE_HALF 64      // samples per half of the PSS's useful part, and the distance between the halves

// one sample of z: x cis(k t) conj(p), with rot = cis(k t) from the caller (the kernel has one per lane, the host twin one per sample)
__host__ __device__ __forceinline__ cd2 foe_halves_z(cd2 x, cd2 rot, cd2 p) {
  const cd2 xr = mk(x.re * rot.re - x.im * rot.im, x.re * rot.im + x.im * rot.re);
  return mk(xr.re * p.re + xr.im * p.im, xr.im * p.re - xr.re * p.im);
}
// A or B: one half of a window's z, summed in the order of a butterfly over 64 lanes -- v[i] += v[i ^ off] for off = 32, 16, .. 1,
// after which every entry holds the same sum (IEEE addition commutes, so both partners of a pair form the same double).  The host
// form works on an array, the device form on one value per lane; the same additions in the same order, bit for bit.
__host__ __device__ inline cd2 foe_half_sum(const cd2 *z) {
  cd2 v[FOE_HALF], w[FOE_HALF];
  for (int i = 0; i < FOE_HALF; ++i) v[i] = z[i];
  for (int off = FOE_HALF / 2; off >= 1; off >>= 1) {
    for (int i = 0; i < FOE_HALF; ++i) w[i] = mk(v[i].re + v[i ^ off].re, v[i].im + v[i ^ off].im);
    for (int i = 0; i < FOE_HALF; ++i) v[i] = w[i];
  }
  return v[0];
}
#ifdef __HIPCC__
__device__ __forceinline__ cd2 foe_half_sum_wave(cd2 v) {
#pragma unroll
  for (int off = FOE_HALF / 2; off >= 1; off >>= 1) v = mk(v.re + __shfl_xor(v.re, off), v.im + __shfl_xor(v.im, off));
  return v;
}
#endif
// conj(A) B: what one occurrence adds to C
__host__ __device__ __forceinline__ cd2 foe_halves_term(cd2 a, cd2 b) { return mk(a.re * b.re + a.im * b.im, a.re * b.im - a.im * b.re); }
// f_coarse of C in Hz, relative to the hypothesis
__host__ __device__ __forceinline__ double foe_coarse_hz(cd2 C, double fs) { return atan2(C.im, C.re) / (2 * M_PI) * fs / FOE_HALF; }
// no decision is taken on a sum of nothing, a zero or a non-finite one
__host__ __device__ __forceinline__ bool foe_coarse_usable(cd2 C, int n_occ) {
  return n_occ > 0 && isfinite(C.re) && isfinite(C.im) && (C.re != 0 || C.im != 0);
}
// periods to add to the native estimate: the nearest whole number, at most one either way (a NaN anywhere decides nothing)
__host__ __device__ __forceinline__ int foe_unwrap_n(double native, double freq, double f_coarse, double fs, int dist, bool usable) {
  const double period = fs / dist, res = native - freq;
  const double q = rint((f_coarse - res) / period);
  if (!usable || !(q == q)) return 0;
  return q > 1 ? 1 : (q < -1 ? -1 : (int)q);
}
// freq_fine: the native double itself when n = 0 -- no arithmetic touches it
__host__ __device__ __forceinline__ double foe_unwrap(double native, double freq, double f_coarse, double fs, int dist, bool usable) {
  const int n = foe_unwrap_n(native, freq, f_coarse, fs, dist, usable);
  return n == 0 ? native : native + n * (fs / dist);
}
