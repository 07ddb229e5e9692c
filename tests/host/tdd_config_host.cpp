// Host-side harness for tdd_config.h (the same __host__ __device__ code k_tdd_config runs; its 16 lanes per row reduce in
// tdd_row_sum's order): the bins of a grid and the decision from them.  tests/test_tdd_config_host.py compares them with the numpy
// reference (tests/tdd_config_ref.py).  With -DTDD_HOST_MAIN the same source is a stand-alone program that reads one grid from a
// file and prints its record: the form that is built with -fsanitize=address,undefined.  Test infrastructure.
#include <cstdio>
#include <vector>
#include "../../lte-cell-scanner_amd/csrc/tdd_config.h"

// tfg [n_ofdm][72] complex; rs [40][12] complex and shift [40]: RS_DL of port 0 by bin b = 2 slot + (sym != 0).
// -> C [40] complex, N [40], scale [40] = sum over the bin's rows of sum_m |h_m| |h_{m+1}|
extern "C" void tdd_host_bins(const double *tfg, int n_ofdm, int n_symb, const double *rs, const int *shift, double *C, int *N, double *scale) {
  const int n_q = tdd_n_ref_rows(n_ofdm, n_symb);
  std::vector<cd2> c((size_t)n_q > 0 ? n_q : 1);
  for (int b = 0; b < TDD_BINS; ++b) scale[b] = 0.0;
  for (int q = 0; q < n_q; ++q) {
    const int b = q % TDD_BINS, row = tdd_grid_row(q, n_symb);
    cd2 h[TDD_ROW_LANES], p[TDD_ROW_LANES];
    for (int m = 0; m < TDD_ROW_LANES; ++m) {
      h[m] = mk(0, 0);
      if (m < 12) {
        const double *x = tfg + ((size_t)row * 72 + shift[b] + 6 * m) * 2;
        h[m] = tdd_h(mk(x[0], x[1]), mk(rs[(b * 12 + m) * 2], rs[(b * 12 + m) * 2 + 1]));
      }
    }
    for (int m = 0; m < TDD_ROW_LANES; ++m) {
      p[m] = m < 11 ? tdd_pair(h[m], h[m + 1]) : mk(0, 0);
      if (m < 11) scale[b] += sqrt(h[m].re * h[m].re + h[m].im * h[m].im) * sqrt(h[m + 1].re * h[m + 1].re + h[m + 1].im * h[m + 1].im);
    }
    c[q] = tdd_row_sum(p);
  }
  for (int b = 0; b < TDD_BINS; ++b) {
    const cd2 s = tdd_bin_sum(c.data(), b, n_q);
    C[2 * b] = s.re; C[2 * b + 1] = s.im;
    N[b] = tdd_bin_count(b, n_q);
  }
}
extern "C" void tdd_host_decide(const double *C, const int *N, lcs_tdd_info *out) {
  cd2 c[TDD_BINS];
  for (int b = 0; b < TDD_BINS; ++b) c[b] = mk(C[2 * b], C[2 * b + 1]);
  tdd_decide(c, N, out);
}
extern "C" int tdd_host_n_ref_rows(int n_ofdm, int n_symb) { return tdd_n_ref_rows(n_ofdm, n_symb); }
extern "C" int tdd_host_config_of_pattern(int pat) { return tdd_config_of_pattern(pat); }

#ifdef TDD_HOST_MAIN
// file: int32 n_ofdm, n_symb, shift[40]; double rs[40][12][2], tfg[n_ofdm][72][2]
int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int hdr[2], shift[TDD_BINS];
  std::vector<double> rs(TDD_BINS * 12 * 2);
  bool ok = std::fread(hdr, sizeof(int), 2, f) == 2 && std::fread(shift, sizeof(int), TDD_BINS, f) == TDD_BINS &&
            std::fread(rs.data(), sizeof(double), rs.size(), f) == rs.size();
  std::vector<double> tfg(ok && hdr[0] > 0 ? (size_t)hdr[0] * 72 * 2 : 0);
  ok = ok && std::fread(tfg.data(), sizeof(double), tfg.size(), f) == tfg.size();
  std::fclose(f);
  if (!ok) return 2;
  double C[2 * TDD_BINS], scale[TDD_BINS];
  int N[TDD_BINS];
  lcs_tdd_info o;
  tdd_host_bins(tfg.data(), hdr[0], hdr[1], rs.data(), shift, C, N, scale);
  tdd_host_decide(C, N, &o);
  std::printf("%d %d %.17g", o.ul_dl_config, o.dwpts_rs_rows, o.margin);
  for (int s = 0; s < 10; ++s) std::printf(" %.17g", o.T[s]);
  for (int j = 0; j < 4; ++j) std::printf(" %.17g", o.R[j]);
  std::printf("\n");
  return 0;
}
#endif
