// Host-side harness for pcfich.h (the same __host__ __device__ code k_pcfich / k_pcfich_fin run; the wave's 64 lanes reduce in
// meas_row_sum's order): the record of a grid [n_ofdm][12 n_rb] under a mask.  tests/test_pcfich_host.py compares it with the numpy
// statement of the rule (tests/pcfich_ref.py), tests/test_gpu_pcfich.py holds the device's record to it bit for bit.  With
// -DPCFICH_HOST_MAIN the same source is a stand-alone program that reads one grid from a file and prints its record: the form that
// is built with -fsanitize=address,undefined.  Test infrastructure.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../lte-cell-scanner_amd/csrc/pcfich.h"

// tfg [n_ofdm][12 n_rb] complex; jump [2][32]: the jump-ahead tables for 1600 + 2 (110 - n_rb) and for 1600 clocks -> the record
extern "C" void pcfich_host(const double *tfg, int n_ofdm, int n_symb, int n_rb, int id, int cp_type, int n_ports, int dl_mask,
                            const uint32_t *jump, lcs_pcfich_info *out) {
  const int ports = pcf_ports(n_ports), n_sf = pcf_n_sf(n_ofdm, n_symb);
  const size_t ncol = (size_t)12 * n_rb;
  std::memset(out, 0, sizeof(*out));
  for (int g = 0; g < n_sf && g < PCF_MAX_SF; ++g) {
    if (!pcf_sf_used(g, n_ofdm, n_symb, ports, dl_mask)) continue;
    const int sf = g % 10;
    uint32_t bits[2][RS_DL_WIDE_WORDS] = {};
    double shift[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t = 0; t < (ports == 4 ? 2 : 1); ++t) rs_dl_row_wide(2 * sf, t, id, cp_type, n_symb, n_rb, jump, bits[t], shift);
    const uint32_t scr = pcf_scramble(sf, id, jump + 32);
    const double *row0 = tfg + (size_t)(2 * g * n_symb) * ncol * 2;
    const double *row1 = ports == 4 ? row0 + ncol * 2 : row0;
    cd2 y[16], ha[16], hb[16];
    for (int e = 0; e < 16; ++e) pcf_elem(e, id, n_rb, ports, row0, row1, bits[0], bits[1], shift, &y[e], &ha[e], &hb[e]);
    double lanes[PCF_NV][PCF_LANES] = {};
    for (int e = 0; e < 16; ++e) {
      double v[PCF_NV];
      pcf_lane_values(e, scr, pcf_soft(e, ports, y[e], ha[e], hb[e ^ 1], y[e ^ 1]), v);
      for (int i = 0; i < PCF_NV; ++i) lanes[i][e] = v[i];
    }
    double tot[PCF_NV], corr[3], margin;
    for (int i = 0; i < PCF_NV; ++i) tot[i] = meas_row_sum<PCF_LANES>(lanes[i]);
    out->cfi[g] = pcf_decide(tot, corr, &margin);
    for (int k = 0; k < 3; ++k) out->corr[g][k] = corr[k];
    out->margin[g] = margin;
  }
  pcf_summary(out, n_sf, dl_mask, n_rb, ports);
}
extern "C" int pcfich_host_record_bytes() { return (int)sizeof(lcs_pcfich_info); }
extern "C" int pcfich_host_max_sf() { return PCF_MAX_SF; }
extern "C" unsigned pcfich_host_scramble(int sf, int id, const uint32_t *jump1600) { return pcf_scramble(sf, id, jump1600); }

#ifdef PCFICH_HOST_MAIN
// file: int32 n_ofdm, n_symb, n_rb, id, cp_type, n_ports, dl_mask, 0; uint32 jump[64]; double tfg[n_ofdm][12 n_rb][2]
int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int hdr[8];
  uint32_t jump[64];
  bool ok = std::fread(hdr, sizeof(int), 8, f) == 8 && std::fread(jump, sizeof(uint32_t), 64, f) == 64;
  ok = ok && hdr[0] > 0 && hdr[0] <= LCS_TFG_MAX_OFDM && (hdr[1] == 6 || hdr[1] == 7) && pcf_rb_ok(hdr[2]) && hdr[3] >= 0 && hdr[3] < 504;
  std::vector<double> tfg(ok ? (size_t)hdr[0] * 12 * hdr[2] * 2 : 0);
  ok = ok && std::fread(tfg.data(), sizeof(double), tfg.size(), f) == tfg.size();
  std::fclose(f);
  if (!ok) return 2;
  lcs_pcfich_info o;
  pcfich_host(tfg.data(), hdr[0], hdr[1], hdr[2], hdr[3], hdr[4], hdr[5], hdr[6], jump, &o);
  std::printf("%d %d %d %d %d %d %d %d %.17g %.17g", o.n_sf, o.n_decoded, o.n_cfi[0], o.n_cfi[1], o.n_cfi[2], o.dl_mask, o.n_rb, o.n_ports,
              o.mean_n_ctrl_sym, o.min_margin);
  for (int g = 0; g < o.n_sf; ++g) std::printf(" %d %.17g %.17g %.17g %.17g", o.cfi[g], o.corr[g][0], o.corr[g][1], o.corr[g][2], o.margin[g]);
  std::printf("\n");
  return 0;
}
#endif
