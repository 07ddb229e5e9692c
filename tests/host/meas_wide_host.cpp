// Host-side harness for cell_meas_wide.h (the same __host__ __device__ code k_cell_meas_wide / k_cell_meas_wide_fin run; the wave's
// 64 lanes and passes reduce in measw_row_sum's order): the totals of a grid [n_ofdm][12 n_rb] under a mask and the record from
// them.  tests/test_meas_wide_host.py compares them with the numpy reference (tests/meas_wide_ref.py), tests/test_gpu_meas_wide.py
// holds the device's record to it bit for bit.  With -DMEAS_WIDE_HOST_MAIN the same source is a stand-alone program that reads one
// grid from a file and prints its record: the form that is built with -fsanitize=address,undefined.  Test infrastructure.
#include <cstdio>
#include <vector>
#include "../../lte-cell-scanner_amd/csrc/cell_meas_wide.h"

// tfg [n_ofdm][12 n_rb] complex; rs [40][2 n_rb] complex and shift [40][2] by bin b = 2 slot + (sym != 0).
// -> tot [7] (A_0 re im, A_1 re im, E_0, E_1, W), the record
extern "C" void meas_wide_host(const double *tfg, int n_ofdm, int n_symb, int n_rb, int n_fft, const double *rs, const int *shift, int n_ports,
                               int dl_mask, double *tot, lcs_meas_wide_info *out) {
  const int n_q = tdd_n_ref_rows(n_ofdm, n_symb), ports = meas_ports(n_ports);
  const int n_ent = 2 * n_rb, n_pass = measw_passes(n_rb), n_slots = n_pass * MEASW_LANES;
  const size_t ncol = (size_t)12 * n_rb;
  std::vector<double> row[MEAS_NV];
  for (int i = 0; i < MEAS_NV; ++i) row[i].assign((size_t)(n_q > 0 ? n_q : 1), 0.0);
  std::vector<double> binrb((size_t)TDD_BINS * MEASW_NRB * MEASW_MAX_RB, 0.0);
  std::vector<double> e[MEAS_NV];
  for (int i = 0; i < MEAS_NV; ++i) e[i].assign((size_t)n_slots, 0.0);
  std::vector<cd2> h[2];
  h[0].assign((size_t)n_ent + 1, mk(0, 0));
  h[1].assign((size_t)n_ent + 1, mk(0, 0));
  std::vector<meas_x6> x((size_t)n_ent);
  for (int q = 0; q < n_q; ++q) {
    const int b = q % TDD_BINS, r = tdd_grid_row(q, n_symb);
    if (!meas_bin_used(b, dl_mask)) continue;
    for (int m = 0; m < n_ent; ++m) {
      const double *g = tfg + ((size_t)r * ncol + 6 * m) * 2;
      x[m] = meas_x6{mk(g[0], g[1]), mk(g[2], g[3]), mk(g[4], g[5]), mk(g[6], g[7]), mk(g[8], g[9]), mk(g[10], g[11])};
      const cd2 s = mk(rs[((size_t)b * n_ent + m) * 2], rs[((size_t)b * n_ent + m) * 2 + 1]);
      h[0][m] = meas_h(x[m], shift[2 * b], s);
      h[1][m] = meas_h(x[m], shift[2 * b + 1], s);
    }
    for (int m = 0; m < n_slots; ++m) {
      double v[MEAS_NV] = {0, 0, 0, 0, 0, 0, 0};
      if (m < n_ent) measw_entry(x[m], m, n_ent, ports, h[0][m], h[0][m + 1], h[1][m], h[1][m + 1], v);
      for (int i = 0; i < MEAS_NV; ++i) e[i][m] = v[i];
    }
    for (int i = 0; i < MEAS_NV; ++i) row[i][q] = measw_row_sum(e[i].data(), n_pass);
    for (int rb = 0; rb < n_rb; ++rb) {
      double v[MEAS_NV], rv[MEASW_NRB];
      for (int i = 0; i < MEAS_NV; ++i) v[i] = e[i][2 * rb];
      measw_rb_values(v, e[MEAS_W][2 * rb + 1], rv);
      for (int k = 0; k < MEASW_NRB; ++k) {
        double &a = binrb[((size_t)b * MEASW_NRB + k) * MEASW_MAX_RB + rb];
        a = measw_acc(q < TDD_BINS, a, rv[k]);
      }
    }
  }
  for (int i = 0; i < MEAS_NV; ++i) {
    double bin[TDD_BINS];
    for (int b = 0; b < TDD_BINS; ++b) bin[b] = meas_bin_used(b, dl_mask) ? meas_bin_sum(row[i].data(), b, n_q) : 0.0;
    tot[i] = meas_total(bin, dl_mask);
  }
  const int n_rows = meas_n_rows(n_q, dl_mask);
  const bool ok = measw_finish_head(tot, n_rows, ports, dl_mask, n_rb, n_fft, out);
  for (int rb = 0; rb < MEASW_MAX_RB; ++rb) {
    double t[MEASW_NRB] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const bool have = ok && rb < n_rb;
    if (have)
      for (int k = 0; k < MEASW_NRB; ++k) t[k] = measw_total_strided(binrb.data() + (size_t)k * MEASW_MAX_RB + rb, (size_t)MEASW_NRB * MEASW_MAX_RB, n_q, dl_mask);
    measw_finish_rb(t, have, n_rows, rb, out);
  }
}
extern "C" int meas_wide_host_max_rb(int n_fft) { return measw_max_rb(n_fft); }
extern "C" int meas_wide_host_col_of_bin(int k, int n_fft, int n_rb, int *cn) { return measw_col_of_bin(k, n_fft, n_rb, cn); }
extern "C" int meas_wide_host_record_bytes() { return (int)sizeof(lcs_meas_wide_info); }
// one row of the generalised RS_DL (lte_device.h: rs_dl_row_wide) -> rs [2 n_rb] complex, shift [4] (untouched entries stay -1)
extern "C" void meas_wide_host_rs_row(int slot, int t, int id, int cp_type, int n_symb, int n_rb, const uint32_t *pn_jump, double *rs, double *shift4) {
  uint32_t bits[RS_DL_WIDE_WORDS];
  for (int p = 0; p < 4; ++p) shift4[p] = -1.0;
  rs_dl_row_wide(slot, t, id, cp_type, n_symb, n_rb, pn_jump, bits, shift4);
  for (int m = 0; m < 2 * n_rb; ++m) { const cd2 v = rs_dl_wide_value(bits, m); rs[2 * m] = v.re; rs[2 * m + 1] = v.im; }
}

#ifdef MEAS_WIDE_HOST_MAIN
// file: int32 n_ofdm, n_symb, n_rb, n_fft, n_ports, dl_mask, shift[40][2]; double rs[40][2 n_rb][2], tfg[n_ofdm][12 n_rb][2]
int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int hdr[6], shift[2 * TDD_BINS];
  bool ok = std::fread(hdr, sizeof(int), 6, f) == 6 && std::fread(shift, sizeof(int), 2 * TDD_BINS, f) == 2 * TDD_BINS;
  ok = ok && hdr[0] > 0 && hdr[0] <= 854 && measw_rb_ok(hdr[3], hdr[2]);
  std::vector<double> rs(ok ? (size_t)TDD_BINS * 2 * hdr[2] * 2 : 0), tfg(ok ? (size_t)hdr[0] * 12 * hdr[2] * 2 : 0);
  ok = ok && std::fread(rs.data(), sizeof(double), rs.size(), f) == rs.size() && std::fread(tfg.data(), sizeof(double), tfg.size(), f) == tfg.size();
  std::fclose(f);
  if (!ok) return 2;
  double tot[MEAS_NV];
  lcs_meas_wide_info o;
  meas_wide_host(tfg.data(), hdr[0], hdr[1], hdr[2], hdr[3], rs.data(), shift, hdr[4], hdr[5], tot, &o);
  std::printf("%d %d %d %d %d %d", o.status, o.n_rows, o.n_ports, o.dl_mask, o.n_rb, o.n_fft);
  const double d[10] = {o.rsrp[0], o.rsrp[1], o.noise[0], o.noise[1], o.rssi, o.rsrq, o.a_re_im[0], o.a_re_im[1], o.a_re_im[2], o.a_re_im[3]};
  for (int i = 0; i < 10; ++i) std::printf(" %.17g", d[i]);
  for (int i = 0; i < o.n_rb; ++i) std::printf(" %.17g %.17g %.17g", o.rsrp_rb[0][i], o.rsrp_rb[1][i], o.rssi_rb[i]);
  std::printf("\n");
  return 0;
}
#endif
