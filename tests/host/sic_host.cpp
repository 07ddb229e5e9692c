// Host-side harness for the cancellation rule (csrc/sic.h) and the PBCH encoder (csrc/lte_pbch_enc.cpp) -- the very text the kernels
// of sic.hip and lcs_launch_sic compile: tests/test_sic_host.py pins the encoder to synth.pbch_symbols, the symbol intervals to a
// sample-by-sample walk and the element maps to tests/sic_ref.py.  With -DSIC_HOST_MAIN it is a program of its own (sanitizer runs).
// Test infrastructure.
#include "../../lte-cell-scanner_amd/csrc/lte_tables.cpp"
#include "../../lte-cell-scanner_amd/csrc/lte_pbch_enc.cpp"
#include "../../lte-cell-scanner_amd/csrc/sic.h"

extern "C" int sic_host_pbch(int id, int n_ports, int n_rb_dl, int phich_duration, int phich_resource, int sfn, int cp_type, double *out) {
  return lcs_tables::pbch_encode(id, n_ports, n_rb_dl, phich_duration, phich_resource, sfn, cp_type, out) ? 1 : 0;
}

// out: t_lo, t_hi, j_lo, n_slots, f_lo, n_frames
extern "C" int sic_host_geometry(double frame_start, double freq_fine, int cp_type, uint32_t n_cap, double fc_req, double fc_prog, double fs, int *out) {
  SicGeom g;
  if (!sic_geometry(frame_start, freq_fine, freq_fine, cp_type, n_cap, fc_req, fc_prog, fs, &g)) return 0;
  out[0] = g.t_lo; out[1] = g.t_hi; out[2] = g.j_lo; out[3] = g.n_slots; out[4] = g.f_lo; out[5] = g.n_frames;
  return 1;
}

// The intervals of one cell against a walk over the samples.  -> 0: they tile [a(t_lo), w(t_hi) + 128) without gap or overlap, every
// boundary differs from the nominal one by at most a sample, t_lo / t_hi are the outermost whole symbols, and sic_owner names the
// walk's symbol and offset for EVERY sample of the capture; otherwise the number of the first check that failed.
extern "C" int sic_host_tiles(double frame_start, double freq_fine, int cp_type, uint32_t n_cap, double fc_req, double fc_prog, double fs) {
  SicGeom g;
  if (!sic_geometry(frame_start, freq_fine, freq_fine, cp_type, n_cap, fc_req, fc_prog, fs, &g)) return 1;
  if (sic_a(g, g.t_lo) < 0 || sic_a(g, g.t_lo - 1) >= 0) return 2;
  if (sic_w(g, g.t_hi) + 128 > (long)n_cap || sic_w(g, g.t_hi + 1) + 128 <= (long)n_cap) return 3;
  long n = 0;
  int t, off;
  for (; n < sic_a(g, g.t_lo); ++n) if (sic_owner(g, n, &t, &off)) return 4;
  for (int s = g.t_lo; s <= g.t_hi; ++s) {
    const long a = sic_a(g, s), e = s == g.t_hi ? sic_w(g, s) + 128 : sic_a(g, s + 1), w = sic_w(g, s);
    if (a != n) return 5;                                  // a gap or an overlap
    const long len = e - a, nominal = 128 + sic_cp(g, s);
    if (s < g.t_hi && (len < nominal - 1 || len > nominal + 1)) return 6;
    if (w - a != sic_cp(g, s) - SIC_WIN_IN_CP) return 7;
    for (; n < e; ++n) {
      if (!sic_owner(g, n, &t, &off) || t != s) return 8;
      long o = (n - w) % 128; if (o < 0) o += 128;
      if (off != (int)o) return 9;
    }
  }
  for (; n < (long)n_cap; ++n) if (sic_owner(g, n, &t, &off)) return 10;
  return 0;
}

// sic_host_tiles for frame_start = first + i step, i < count: -> -1 when all pass, else the first i that fails (*why: its check)
extern "C" long sic_host_tiles_raster(double first, double step, long count, double freq_fine, int cp_type, uint32_t n_cap, double fc_req,
                                      double fc_prog, double fs, int *why) {
  for (long i = 0; i < count; ++i) {
    const int r = sic_host_tiles(first + (double)i * step, freq_fine, cp_type, n_cap, fc_req, fc_prog, fs);
    if (r) { *why = r; return i; }
  }
  return -1;
}

// What the ports send in symbol `sym` (0..3) of slot 1 given the frame's PBCH quarter q (re, im pairs): out [4][72][2], zero elsewhere
extern "C" void sic_host_pbch_map(int normal, int n_ports, int id, int sym, const double *q, double *out) {
  for (int i = 0; i < 4 * 72 * 2; ++i) out[i] = 0.0;
  for (int k = 0; k < 72; ++k) {
    const int idx = sic_pbch_index(normal, sym, k, id);
    if (idx < 0) continue;
    for (int p = 0; p < n_ports; ++p)
      sic_pbch_port(n_ports, p, idx, q[2 * idx], q[2 * idx + 1], q[2 * (idx ^ 1)], q[2 * (idx ^ 1) + 1], &out[(p * 72 + k) * 2], &out[(p * 72 + k) * 2 + 1]);
  }
}

// interpolation weights and CRS positions as the kernels take them
extern "C" void sic_host_interp(int k, int c3, int *m0, double *fr) { sic_interp(k, c3, m0, fr); }
extern "C" int sic_host_crs_shift(int port, int row, int s, int id) { return sic_crs_shift(port, row, s, id); }
extern "C" int sic_host_sync_kind(int cp_type, int t, int duplex, int *seq_slot) {
  SicGeom g{};
  g.normal = cp_type == LCS_CP_NORMAL; g.n_symb = g.normal ? 7 : 6;
  return sic_sync_kind(g, t, duplex, seq_slot);
}

#ifdef SIC_HOST_MAIN
#include <cstdio>
int main() {
  int bad = 0;
  static double sym[2 * 960], map[4 * 72 * 2];
  for (int cp = 1; cp <= 2; ++cp)
    for (int ports = 1; ports <= 4; ports *= 2) {
      bad += !sic_host_pbch(301, ports, 50, 1, 2, 77, cp, sym);
      for (int s = 0; s < 4; ++s) sic_host_pbch_map(cp == 1, ports, 301, s, sym, map);
    }
  const double fc = 739e6;
  for (int cp = 1; cp <= 2; ++cp)
    for (double ppm = -120.0; ppm <= 120.0; ppm += 120.0)
      for (double fs0 = 0.0; fs0 < 19200.0; fs0 += 1371.3) bad += sic_host_tiles(fs0, -ppm * 1e-6 * fc, cp, 153600, fc, fc, 1.92e6) != 0;
  // off-nominal rates: fs_programmed +- 3e-4, fc_programmed 40 kHz below fc_requested, on the shortest and the longest capture
  for (int cp = 1; cp <= 2; ++cp)
    for (double rate = -3e-4; rate <= 3e-4; rate += 6e-4)
      for (double fs0 = -2.5; fs0 < 19200.0; fs0 += 2371.3) {
        bad += sic_host_tiles(fs0, rate > 0 ? 5000.0 : -5000.0, cp, 9600, fc, fc - 40e3, 1.92e6 * (1.0 + rate)) != 0;
        bad += sic_host_tiles(fs0, rate > 0 ? 5000.0 : -5000.0, cp, 268800, fc, fc - 40e3, 1.92e6 * (1.0 + rate)) != 0;
      }
  std::printf("sic_host: %d failures\n", bad);
  return bad != 0;
}
#endif
