// sic.h -- the successive-cancellation rule: what of a decoded cell is known, where it lies in the capture, and how it is
// rebuilt.  __host__ __device__, shared by the kernels (sic.hip), the host twin (tests/host/sic_host.cpp) and, restated in
// numpy, tests/sic_ref.py.
//
// 1. Symbol geometry.  With k = (fc_requested - freq_fine) / fc_programmed and step = 16 / FS_LTE * fs_programmed * k (receiver
//    samples per nominal 1.92 MHz sample) extract_tfg puts the transform window of grid row t at round(d(t)),
//      d(t) = d0 + N(t) step,   d0 = frame_start + cp0 step (- .01 fs k when that stays above -0.5),
//      N(t) = 960 floor(t / 7) + 137 (t mod 7)  (normal CP, cp0 = 10)   |   160 t  (extended CP, cp0 = 32)
//    (extract_tfg adds the increments one by one; the product differs from its running sum by the rounding of the additions,
//    ~1e-10 samples).  Here t runs over every integer, backwards and forwards, for which the whole symbol (cyclic prefix + 128)
//    lies inside the capture: t_lo .. t_hi.  frame_start lies SIC_WIN_IN_CP = 2 samples before the frame boundary (measured
//    against synth's t0: 14198.0 for a boundary at 14199.99), so the window w(t) = round(d(t)) starts 2 samples inside the
//    cyclic prefix and the symbol begins at a(t) = w(t) - cp(t) + 2, cp(t) = 10 for the first symbol of a slot, else 9 (32).
//    Symbol t owns the samples [a(t), a(t + 1)): where rounding leaves a sample between two nominal symbols, or takes one
//    away, the EARLIER symbol's tail stretches or shrinks -- the periodic extension of its window covers either.  The last
//    symbol owns up to the end of its window.
// 2. Grid.  The window's samples times cis(-2 pi rot n), rot = freq_superfine / (fs k) cycles per sample at ABSOLUTE sample n,
//    the unscaled 128-point transform, the 72 occupied bins, and extract_tfg's phase cis(-2 pi late cn / 128), late = w - d.
// 3. Channel, from the CRS alone (never the PSS: a hidden cell with the same n_id_2 sends the same sequence).  Least squares
//    h = Y conj(rs) on every usable reference element of ports 0 .. n_ports - 1; per slot j, port and reference subcarrier
//    q_m = (id mod 3) + 3 m (m < 24) the MEAN of the usable values at that subcarrier in slots j - 4 .. j + 4 (0 where there is
//    none); between reference subcarriers linear interpolation over the true subcarrier number cn (the DC gap counts), beyond
//    the outermost ones the linear continuation; the same estimate for every symbol of slot j.
// 4. Sync gain: g = sum Y conj(H_0 s) / sum |H_0 s|^2 over the 62 SSS elements of every SSS symbol of the capture.  It scales
//    PSS and SSS alike (they leave port 0 at a gain of their own: sqrt(n_ports) in synth, vendor specific in the field).
// 5. Known elements: PSS / SSS at the duplex mode's positions in every half frame; CRS and PBCH in the `usable` symbols --
//    those of the subframes in dl_mask (FDD: all; TDD: 0 and 5, or the downlink subframes of the configuration found) and,
//    with `special`, symbol 0 of subframes 1 and 6.  The PBCH of frame f of the grid carries sfn + f (decode_mib's rule: the
//    record's sfn is that of the grid's first frame, pinned by synth's sfn0).
// 6. Synthesis: sum_p H_p X_p, times cis(+2 pi late cn / 128), inverse transform (1 / 128), periodic over [a(t), a(t + 1)),
//    times cis(+2 pi rot n).
// 7. Subtraction: per output sample, the cells of its buffer in list order, each cell's owning symbol by sic_owner.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/lcs.h"

#ifndef FS_LTE
#define FS_LTE 30720000.0
#endif
#define SIC_WIN_IN_CP 2
#define SIC_AVG_SLOTS 4
#define SIC_MAX_FRAMES 16      // frames of one capture a PBCH table holds (the launcher refuses a capture that spans more: LCS_ERR_BAD_ARG)

struct SicGeom {
  double d0, step, rot;
  int normal, n_symb;
  int t_lo, t_hi;              // first and last symbol wholly inside the capture
  int j_lo, n_slots;           // the slots they belong to
  int f_lo, n_frames;          // ... and the frames
  uint32_t n_cap;
};

__host__ __device__ inline int sic_floordiv(int a, int b) { const int q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }
__host__ __device__ inline int sic_mod(int a, int b) { return a - b * sic_floordiv(a, b); }
__host__ __device__ inline int sic_slot_of(const SicGeom &g, int t) { return sic_floordiv(t, g.n_symb); }
__host__ __device__ inline int sic_sym_of(const SicGeom &g, int t) { return sic_mod(t, g.n_symb); }
__host__ __device__ inline double sic_nominal(const SicGeom &g, int t) {
  return g.normal ? (double)(960 * sic_floordiv(t, 7) + 137 * sic_mod(t, 7)) : (double)(160 * t);
}
__host__ __device__ inline int sic_cp(const SicGeom &g, int t) { return g.normal ? (sic_mod(t, 7) == 0 ? 10 : 9) : 32; }
__host__ __device__ inline double sic_d(const SicGeom &g, int t) { return g.d0 + sic_nominal(g, t) * g.step; }
__host__ __device__ inline long sic_w(const SicGeom &g, int t) { return (long)rint(sic_d(g, t)); }
__host__ __device__ inline long sic_a(const SicGeom &g, int t) { return sic_w(g, t) - sic_cp(g, t) + SIC_WIN_IN_CP; }

// The symbol whose nominal stretch holds sample n, corrected by at most one symbol to the rounded boundaries.
__host__ __device__ inline int sic_symbol_at(const SicGeom &g, long n) {
  const double r = ((double)n - g.d0) / g.step + (double)((g.normal ? 10 : 32) - SIC_WIN_IN_CP);
  int t;
  if (g.normal) {
    const double slot = floor(r / 960.0), rr = r - 960.0 * slot;
    const double sym = rr < 138.0 ? 0.0 : fmin(6.0, 1.0 + floor((rr - 138.0) / 137.0));
    t = (int)(7.0 * slot + sym);
  } else {
    t = (int)floor(r / 160.0);
  }
  if (n < sic_a(g, t)) return t - 1;
  if (n >= sic_a(g, t + 1)) return t + 1;
  return t;
}
// sample n -> its owning symbol and the offset into the periodic extension of that symbol's window; false: no symbol owns it
__host__ __device__ inline bool sic_owner(const SicGeom &g, long n, int *t_out, int *off_out) {
  const int t = sic_symbol_at(g, n);
  if (t < g.t_lo || t > g.t_hi) return false;
  const long w = sic_w(g, t);
  if (t == g.t_hi && n >= w + 128) return false;
  *t_out = t;
  *off_out = (int)((n - w) & 127);      // two's complement: the periodic extension backwards into the cyclic prefix too
  return true;
}

// false: the record carries no usable timing (or the capture holds no whole symbol)
__host__ __device__ inline bool sic_geometry(double frame_start, double freq_fine, double freq_superfine, int cp_type, uint32_t n_cap,
                                             double fc_requested, double fc_programmed, double fs_programmed, SicGeom *g) {
  if (cp_type != LCS_CP_NORMAL && cp_type != LCS_CP_EXTENDED) return false;
  if (!(frame_start == frame_start) || !(freq_fine == freq_fine) || !(freq_superfine == freq_superfine)) return false;
  g->normal = cp_type == LCS_CP_NORMAL;
  g->n_symb = g->normal ? 7 : 6;
  g->n_cap = n_cap;
  const double k = (fc_requested - freq_fine) / fc_programmed;
  g->step = 16 / FS_LTE * fs_programmed * k;
  if (!(g->step > 0.5 && g->step < 2.0) || !(fabs(frame_start) < 1e6) || n_cap < 512) return false;
  g->d0 = frame_start + (g->normal ? 10 : 32) * g->step;
  if (g->d0 - .01 * fs_programmed * k > -0.5) g->d0 = g->d0 - .01 * fs_programmed * k;
  g->rot = freq_superfine / (fs_programmed * k);
  int lo = sic_symbol_at(*g, 0) - 1, hi = sic_symbol_at(*g, (long)n_cap - 1) + 1;
  while (sic_a(*g, lo) < 0) ++lo;
  while (hi >= lo && sic_w(*g, hi) + 128 > (long)n_cap) --hi;
  if (hi < lo) return false;
  g->t_lo = lo; g->t_hi = hi;
  g->j_lo = sic_slot_of(*g, lo);
  g->n_slots = sic_slot_of(*g, hi) - g->j_lo + 1;
  g->f_lo = sic_floordiv(g->j_lo, 20);
  g->n_frames = sic_floordiv(sic_slot_of(*g, hi), 20) - g->f_lo + 1;
  return true;
}

// grid index 0..71 <-> transform bin and true subcarrier number
__host__ __device__ inline int sic_bin_of(int i) { return i < 36 ? 92 + i : i - 35; }
__host__ __device__ inline int sic_idx_of_bin(int bin) { return bin >= 92 ? bin - 92 : ((bin >= 1 && bin <= 36) ? bin + 35 : -1); }
__host__ __device__ inline int sic_cn(int i) { return i < 36 ? i - 36 : i - 35; }

// whether the CRS and PBCH of symbol t are cancelled, and its CRS feed the channel estimate
__host__ __device__ inline bool sic_usable(const SicGeom &g, int t, int dl_mask, int special) {
  const int s = sic_mod(sic_slot_of(g, t), 20), sf = s >> 1;
  if ((dl_mask >> sf) & 1) return true;
  return special && (sf == 1 || sf == 6) && (s & 1) == 0 && sic_sym_of(g, t) == 0;
}
// which row of rs_dl_row (0, 1, 2 -> symbol 0, 1, n_symb - 3) symbol `sym` of a slot is, -1: it carries no CRS
__host__ __device__ inline int sic_crs_row(int sym, int n_symb) { return sym == 0 ? 0 : (sym == 1 ? 1 : (sym == n_symb - 3 ? 2 : -1)); }
// first subcarrier of port p's CRS in that symbol of slot-in-frame s, -1: the port has none there (36.211 6.10.1.2)
__host__ __device__ inline int sic_crs_shift(int port, int row, int s, int id) {
  int v = -1;
  if (row == 0) v = port == 0 ? 0 : (port == 1 ? 3 : -1);
  else if (row == 2) v = port == 0 ? 3 : (port == 1 ? 0 : -1);
  else if (row == 1) v = port == 2 ? 3 * (s & 1) : (port == 3 ? 3 + 3 * (s & 1) : -1);
  return v < 0 ? -1 : (v + id) % 6;
}
// 0: no sync signal in symbol t, 1: the PSS, 2: the SSS (*seq_slot: 0 or 10, the half frame whose SSS sequence it is)
__host__ __device__ inline int sic_sync_kind(const SicGeom &g, int t, int duplex, int *seq_slot) {
  const int s = sic_mod(sic_slot_of(g, t), 20), sym = sic_sym_of(g, t), h = s % 10;
  *seq_slot = s - h;
  if (duplex == LCS_DUPLEX_TDD) {
    if (h == 2 && sym == 2) return 1;
    if (h == 1 && sym == g.n_symb - 1) return 2;
    return 0;
  }
  if (h == 0 && sym == g.n_symb - 1) return 1;
  if (h == 0 && sym == g.n_symb - 2) return 2;
  return 0;
}
// the PSS / SSS symbol of half frame hf (slots 10 hf .. 10 hf + 9 of the grid); the caller checks it against t_lo .. t_hi
__host__ __device__ inline int sic_pss_symbol(const SicGeom &g, int hf, int duplex) {
  return duplex == LCS_DUPLEX_TDD ? (10 * hf + 2) * g.n_symb + 2 : 10 * hf * g.n_symb + g.n_symb - 1;
}
__host__ __device__ inline int sic_sss_symbol(const SicGeom &g, int hf, int duplex) {
  return duplex == LCS_DUPLEX_TDD ? (10 * hf + 1) * g.n_symb + g.n_symb - 1 : 10 * hf * g.n_symb + g.n_symb - 2;
}
__host__ __device__ inline int sic_hf_lo(const SicGeom &g) { return sic_floordiv(g.j_lo, 10); }
__host__ __device__ inline int sic_hf_hi(const SicGeom &g) { return sic_floordiv(g.j_lo + g.n_slots - 1, 10); }
// linear interpolation between the reference subcarriers q_m = c3 + 3 m: H[k] = h[m0] + fr (h[m0 + 1] - h[m0])
__host__ __device__ inline void sic_interp(int k, int c3, int *m0_out, double *fr_out) {
  int m0 = sic_floordiv(k - c3, 3);
  m0 = m0 < 0 ? 0 : (m0 > 22 ? 22 : m0);
  const double c0 = (double)sic_cn(c3 + 3 * m0), c1 = (double)sic_cn(c3 + 3 * m0 + 3);
  *m0_out = m0;
  *fr_out = ((double)sic_cn(k) - c0) / (c1 - c0);
}
// PBCH (36.211 6.6.4): symbols 0..3 of slot 1; where CRS of any of four ports may lie (k mod 3 == id mod 3 in symbols 0, 1 and,
// with the extended CP, 3) no PBCH is mapped.  -> index of element (sym, k) within the frame's quarter, -1: not a PBCH element
__host__ __device__ inline int sic_pbch_index(int normal, int sym, int k, int id) {
  if (sym < 0 || sym > 3) return -1;
  const bool skip = sym <= 1 || (sym == 3 && !normal);
  const int c3 = id % 3;
  if (skip && k % 3 == c3) return -1;
  const int first = sym == 0 ? 0 : (sym == 1 ? 48 : (sym == 2 ? 96 : 168));
  return first + (skip ? k - (k + 2 - c3) / 3 : k);
}
__host__ __device__ inline int sic_pbch_per_frame(int normal) { return normal ? 240 : 216; }
// What port p sends on PBCH element i, given s = symbol i and mate = symbol i ^ 1 (36.211 6.3.4.3: SFBC, SFBC-FSTD); re/im pairs
__host__ __device__ inline void sic_pbch_port(int n_ports, int p, int i, double s_re, double s_im, double m_re, double m_im, double *re, double *im) {
  *re = 0.0; *im = 0.0;
  if (n_ports == 1) { if (p == 0) { *re = s_re; *im = s_im; } return; }
  const double r2 = 0.70710678118654752440;
  int role;      // 0: the plain stream, 1: the conjugated one, -1: silent
  if (n_ports == 2) role = p;
  else role = (((i >> 1) & 1) == (p & 1)) ? (p >> 1) : -1;
  if (role == 0) { *re = s_re * r2; *im = s_im * r2; }
  else if (role == 1) {
    if (i & 1) { *re = m_re * r2; *im = -m_im * r2; }      // conj(s_{i-1})
    else { *re = -m_re * r2; *im = m_im * r2; }            // -conj(s_{i+1})
  }
}
