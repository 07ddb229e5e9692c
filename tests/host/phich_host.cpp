// Host-side harness for phich.h (the same __host__ __device__ code k_phich / k_phich_fin run, with the lanes' shuffles spelled as
// array accesses in the same order): the record and the per-subframe tables of a grid [n_ofdm][12 n_rb] under a mask.
// tests/test_phich_host.py compares it with the numpy statement of the rule (tests/phich_ref.py), tests/test_gpu_phich.py holds the
// device's record and values to it bit for bit.  With -DPHICH_HOST_MAIN the same source is a stand-alone program that reads one
// grid from a file and prints its record: the form that is built with -fsanitize=address,undefined.  Test infrastructure.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../lte-cell-scanner_amd/csrc/phich.h"

// the unit table of m_i: re [PHI_MAX_UNIT * 12] as PhiMap's -> n_unit (-1: refused)
extern "C" int phich_host_map(int n_rb, int n_ports, int cp_type, int id, int phich_duration, int phich_resource, int mi, int *re) {
  std::vector<PhiMap> maps(3);
  phi_build_maps(n_rb, pcf_ports(n_ports), cp_type, id, phich_duration, phich_resource, maps.data());
  const PhiMap &m = maps[mi < 0 ? 0 : mi > 2 ? 2 : mi];
  std::memcpy(re, m.re, sizeof(m.re));
  return m.n_unit;
}

// tfg [n_ofdm][12 n_rb] complex; mi [10]: the resolved m_i (0 .. 2); tdd: a TDD call; jump [2][32]: the jump-ahead tables for
// 1600 + 2 (110 - n_rb) and for 1600 clocks -> the record, and (each may be null) values / sigma [n_sf][PHI_MAX_ENT]
extern "C" void phich_host(const double *tfg, int n_ofdm, int n_symb, int n_rb, int id, int cp_type, int n_ports, int dl_mask, int phich_duration,
                           int phich_resource, const int *mi, int tdd, double min_amp, double min_sigma, const uint32_t *jump, lcs_phich_info *out,
                           double *values, double *sigma) {
  const int ports = pcf_ports(n_ports), n_sf = pcf_n_sf(n_ofdm, n_symb);
  const size_t ncol = (size_t)12 * n_rb;
  const bool normal = cp_type == LCS_CP_NORMAL;
  std::memset(out, 0, sizeof(*out));
  std::vector<PhiMap> maps(3);
  phi_build_maps(n_rb, ports, cp_type, id, phich_duration, phich_resource, maps.data());
  std::vector<PhiEntry> tab((size_t)PHI_MAX_ENT);
  int n_listed = 0;
  for (int g = 0; g < n_sf && g < PCF_MAX_SF; ++g) {
    const int sf = g % 10;
    const PhiMap &map = maps[mi[sf]];
    if (!phi_sf_used(g, n_ofdm, n_symb, ports, phich_duration, tdd != 0, dl_mask) || map.n_unit < 0) {
      out->sf[g] = phi_sf_entry(-1, cp_type, 0, 0, 0.0);
      continue;
    }
    const int n_unit = map.n_unit, n_ent = 8 * n_unit;
    uint32_t bits[2][RS_DL_WIDE_WORDS] = {};
    double shift[4] = {0.0, 0.0, 0.0, 0.0};
    if (n_unit > 0) for (int t = 0; t < (ports == 4 ? 2 : 1); ++t) rs_dl_row_wide(2 * sf, t, id, cp_type, n_symb, n_rb, jump, bits[t], shift);
    const uint32_t scr = n_unit > 0 ? pcf_scramble(sf, id, jump + 32) : 0u;
    const double *row0 = tfg + (size_t)(2 * g * n_symb) * ncol * 2;
    const double *row1 = ports == 4 ? row0 + ncol * 2 : row0;
    for (int u = 0; u < n_unit; ++u) {
      cd2 y[12], ha[12], hb[12], t[12];
      double G[12];
      for (int e = 0; e < 12; ++e) {
        const int re = map.re[12 * u + e];
        phi_elem(e, u, re & 0xffff, n_rb, ports, row0 + (size_t)(re >> 16) * ncol * 2, row0, row1, bits[0], bits[1], shift, &y[e], &ha[e], &hb[e]);
      }
      for (int e = 0; e < 12; ++e) {
        t[e] = phi_descramble(pcf_soft(e, ports, y[e], ha[e], hb[e ^ 1], y[e ^ 1]), scr, phi_c_index(e, cp_type));
        G[e] = phi_gain(ha[e], hb[e ^ 1]);
      }
      for (int stage = 1; stage <= (normal ? 2 : 1); stage <<= 1) {
        cd2 t2[12];
        double G2[12];
        for (int e = 0; e < 12; ++e) { t2[e] = phi_bfly(t[e], t[e ^ stage], e & 3, stage); G2[e] = G[e] + G[e ^ stage]; }
        for (int e = 0; e < 12; ++e) { t[e] = t2[e]; G[e] = G2[e]; }
      }
      for (int j = 0; j < 4; ++j)
        for (int fam = 0; fam < 2; ++fam)
          tab[(size_t)phi_entry_index(cp_type, u, j, fam)] =
              phi_final(phi_proj(t[j], fam, ports), phi_proj(t[j + 4], fam, ports), phi_proj(t[j + 8], fam, ports), G[j], G[j + 4], G[j + 8]);
    }
    // the subframe's noise: lane i adds its entries in ascending order, then the butterfly
    double lanes[64] = {};
    int cnt = 0;
    for (int i = 0; i < 64; ++i)
      for (int q = 0; q < PHI_ENT_PASSES; ++q) {
        const int k = i + 64 * q;
        if (k < n_ent && tab[(size_t)k].dsum > 0.0) { lanes[i] = lanes[i] + tab[(size_t)k].S; cnt += 1; }
      }
    const double noise = cnt > 0 ? meas_row_sum<64>(lanes) / (double)cnt : 0.0;
    int n_p = 0, n_a = 0;
    for (int k = 0; k < n_ent; ++k) {
      double sg;
      const int fl = phi_decide(tab[(size_t)k], noise, min_amp, min_sigma, &sg);
      if (values) values[(size_t)g * PHI_MAX_ENT + k] = tab[(size_t)k].value;
      if (sigma) sigma[(size_t)g * PHI_MAX_ENT + k] = sg;
      if (fl & 1) {
        if (n_listed < PHI_MAX_HI) out->hi[n_listed] = phi_hi_entry(g, k, cp_type, fl, tab[(size_t)k].value, sg);
        n_listed += 1; n_p += 1; n_a += (fl >> 1) & 1;
      }
    }
    out->sf[g] = phi_sf_entry(n_unit, cp_type, n_p, n_a, noise);
  }
  phi_summary(out, n_sf, dl_mask, n_rb, ports);
}
// sizes and offsets of the records, for the bindings' check: cfg, sf, hi, info; info.sf, info.hi; hi.value; cfg.min_amp
extern "C" void phich_host_layout(int *o) {
  o[0] = (int)sizeof(lcs_phich_cfg); o[1] = (int)sizeof(lcs_phich_sf); o[2] = (int)sizeof(lcs_phich_hi); o[3] = (int)sizeof(lcs_phich_info);
  o[4] = (int)offsetof(lcs_phich_info, sf); o[5] = (int)offsetof(lcs_phich_info, hi); o[6] = (int)offsetof(lcs_phich_hi, value);
  o[7] = (int)offsetof(lcs_phich_cfg, min_amp); o[8] = (int)offsetof(lcs_phich_sf, noise); o[9] = (int)offsetof(lcs_phich_info, dl_mask);
  o[10] = PHI_MAX_ENT; o[11] = PHI_MAX_HI;
}
extern "C" double phich_host_default(int which) { return which ? LCS_PHICH_MIN_SIGMA : LCS_PHICH_MIN_AMP; }

#ifdef PHICH_HOST_MAIN
// file: int32 n_ofdm, n_symb, n_rb, id, cp_type, n_ports, dl_mask, phich_duration, phich_resource, tdd, mi[10]; uint32 jump[64];
// double tfg[n_ofdm][12 n_rb][2]
int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int hdr[20];
  uint32_t jump[64];
  bool ok = std::fread(hdr, sizeof(int), 20, f) == 20 && std::fread(jump, sizeof(uint32_t), 64, f) == 64;
  ok = ok && hdr[0] > 0 && hdr[0] <= LCS_TFG_MAX_OFDM && (hdr[1] == 6 || hdr[1] == 7) && pcf_rb_ok(hdr[2]) && hdr[3] >= 0 && hdr[3] < 504 &&
       (hdr[7] == 1 || hdr[7] == 2) && hdr[8] >= 1 && hdr[8] <= 4;
  for (int i = 0; i < 10; ++i) ok = ok && hdr[10 + i] >= 0 && hdr[10 + i] <= 2;
  std::vector<double> tfg(ok ? (size_t)hdr[0] * 12 * hdr[2] * 2 : 0);
  ok = ok && std::fread(tfg.data(), sizeof(double), tfg.size(), f) == tfg.size();
  std::fclose(f);
  if (!ok) return 2;
  std::vector<lcs_phich_info> o(1);
  std::vector<double> values((size_t)PCF_MAX_SF * PHI_MAX_ENT, 0.0);
  phich_host(tfg.data(), hdr[0], hdr[1], hdr[2], hdr[3], hdr[4], hdr[5], hdr[6], hdr[7], hdr[8], hdr + 10, hdr[9], LCS_PHICH_MIN_AMP, LCS_PHICH_MIN_SIGMA, jump,
             o.data(), values.data(), nullptr);
  std::printf("%d %d %d %d %d %d %d", o[0].n_sf, o[0].n_read, o[0].n_present, o[0].n_ack, o[0].n_nack, o[0].n_hi, o[0].n_dropped);
  for (int g = 0; g < o[0].n_sf; ++g) std::printf(" %d %d %.17g", o[0].sf[g].n_unit, o[0].sf[g].n_present, o[0].sf[g].noise);
  std::printf("\n");
  return 0;
}
#endif
