// Host-side harness for cell_meas.h (the same __host__ __device__ code k_cell_meas runs; its 16 lanes per row reduce in
// meas_row_sum's order): the seven totals of a grid under a mask and the record from them.  tests/test_cell_meas_host.py compares
// them with the numpy reference (tests/cell_meas_ref.py).  With -DMEAS_HOST_MAIN the same source is a stand-alone program that reads
// one grid from a file and prints its record: the form that is built with -fsanitize=address,undefined.  Test infrastructure.
#include <cstdio>
#include <vector>
#include "../../lte-cell-scanner_amd/csrc/cell_meas.h"

// tfg [n_ofdm][72] complex; rs [40][12] complex and shift [40][2]: RS_DL by bin b = 2 slot + (sym != 0), the shifts of ports 0 and 1.
// -> tot [7] (A_0 re im, A_1 re im, E_0, E_1, W), scale [7] (sum |h_m| |h_{m+1}| per port for both parts of A_p; E_p and W are
// sums of non-negative terms and their own scale), the record
extern "C" void meas_host(const double *tfg, int n_ofdm, int n_symb, const double *rs, const int *shift, int n_ports, int dl_mask,
                          double *tot, double *scale, lcs_meas_info *out) {
  const int n_q = tdd_n_ref_rows(n_ofdm, n_symb), ports = meas_ports(n_ports);
  std::vector<double> row[MEAS_NV];
  for (int i = 0; i < MEAS_NV; ++i) row[i].assign((size_t)(n_q > 0 ? n_q : 1), 0.0);
  double sc[2] = {0.0, 0.0};
  for (int q = 0; q < n_q; ++q) {
    const int b = q % TDD_BINS, r = tdd_grid_row(q, n_symb);
    if (!meas_bin_used(b, dl_mask)) continue;
    double e[MEAS_NV][TDD_ROW_LANES];
    cd2 h[2][TDD_ROW_LANES + 1];
    meas_x6 x[TDD_ROW_LANES];
    for (int m = 0; m <= TDD_ROW_LANES; ++m) h[0][m] = h[1][m] = mk(0, 0);
    for (int m = 0; m < 12; ++m) {
      const double *g = tfg + ((size_t)r * 72 + 6 * m) * 2;
      x[m] = meas_x6{mk(g[0], g[1]), mk(g[2], g[3]), mk(g[4], g[5]), mk(g[6], g[7]), mk(g[8], g[9]), mk(g[10], g[11])};
      const cd2 s = mk(rs[(b * 12 + m) * 2], rs[(b * 12 + m) * 2 + 1]);
      h[0][m] = meas_h(x[m], shift[2 * b], s);
      h[1][m] = meas_h(x[m], shift[2 * b + 1], s);
    }
    for (int m = 0; m < TDD_ROW_LANES; ++m) {
      double v[MEAS_NV] = {0, 0, 0, 0, 0, 0, 0};
      if (m < 12) meas_entry(x[m], m, ports, h[0][m], h[0][m + 1], h[1][m], h[1][m + 1], v);
      for (int i = 0; i < MEAS_NV; ++i) e[i][m] = v[i];
      if (m < 11)
        for (int p = 0; p < ports; ++p) sc[p] += sqrt(cabs2(h[p][m])) * sqrt(cabs2(h[p][m + 1]));
    }
    for (int i = 0; i < MEAS_NV; ++i) row[i][q] = meas_row_sum(e[i]);
  }
  for (int i = 0; i < MEAS_NV; ++i) {
    double bin[TDD_BINS];
    for (int b = 0; b < TDD_BINS; ++b) bin[b] = meas_bin_sum(row[i].data(), b, n_q);
    tot[i] = meas_total(bin, dl_mask);
  }
  scale[MEAS_A0_RE] = scale[MEAS_A0_IM] = sc[0];
  scale[MEAS_A1_RE] = scale[MEAS_A1_IM] = sc[1];
  scale[MEAS_E0] = tot[MEAS_E0]; scale[MEAS_E1] = tot[MEAS_E1]; scale[MEAS_W] = tot[MEAS_W];
  meas_finish(tot, meas_n_rows(n_q, dl_mask), ports, dl_mask, out);
}
extern "C" int meas_host_tdd_dl_mask(int ul_dl_config) { return meas_tdd_dl_mask(ul_dl_config); }
extern "C" int meas_host_n_rows(int n_ofdm, int n_symb, int dl_mask) { return meas_n_rows(tdd_n_ref_rows(n_ofdm, n_symb), dl_mask); }

#ifdef MEAS_HOST_MAIN
// file: int32 n_ofdm, n_symb, n_ports, dl_mask, shift[40][2]; double rs[40][12][2], tfg[n_ofdm][72][2]
int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int hdr[4], shift[2 * TDD_BINS];
  std::vector<double> rs(TDD_BINS * 12 * 2);
  bool ok = std::fread(hdr, sizeof(int), 4, f) == 4 && std::fread(shift, sizeof(int), 2 * TDD_BINS, f) == 2 * TDD_BINS &&
            std::fread(rs.data(), sizeof(double), rs.size(), f) == rs.size();
  std::vector<double> tfg(ok && hdr[0] > 0 ? (size_t)hdr[0] * 72 * 2 : 0);
  ok = ok && std::fread(tfg.data(), sizeof(double), tfg.size(), f) == tfg.size();
  std::fclose(f);
  if (!ok) return 2;
  double tot[MEAS_NV], scale[MEAS_NV];
  lcs_meas_info o;
  meas_host(tfg.data(), hdr[0], hdr[1], rs.data(), shift, hdr[2], hdr[3], tot, scale, &o);
  std::printf("%d %d %d %d", o.status, o.n_rows, o.n_ports, o.dl_mask);
  const double d[10] = {o.rsrp[0], o.rsrp[1], o.noise[0], o.noise[1], o.rssi, o.rsrq, o.a_re_im[0], o.a_re_im[1], o.a_re_im[2], o.a_re_im[3]};
  for (int i = 0; i < 10; ++i) std::printf(" %.17g", d[i]);
  std::printf("\n");
  return 0;
}
#endif
