// Host-side harness for pdcch.h and the length-n tail-biting decoder of lte_device.h (the same __host__ __device__ code k_pdcch_llr,
// k_pdcch_dec and k_pdcch_fin run; the tables the kernels read are built by the very functions called here).  tests/test_pdcch_host.py
// compares it with the numpy statement of the rule (tests/pdcch_ref.py), tests/test_gpu_pdcch.py holds the device's record to it bit
// for bit.  With -DPDCCH_HOST_MAIN the same source is a stand-alone program that reads one grid from a file and prints its record:
// the form that is built with -fsanitize=address,undefined.  Test infrastructure.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../lte-cell-scanner_amd/csrc/pdcch.h"

extern "C" int pdcch_host_record_bytes() { return (int)sizeof(lcs_pdcch_info); }
extern "C" int pdcch_host_cfg_bytes() { return (int)sizeof(lcs_pdcch_cfg); }

// one map with its three REG lists (k' << 2 | l'); the lists' lengths in n_lists[3] (pcfich, phich, order); returns 0 when refused
extern "C" int pdcch_host_map(int n_rb, int ports, int cp_type, int id, int dur, int res, int mi, int cfi, int *n_reg, int *n_cce, int *re /*[576]*/,
                              int *pcfich /*[4]*/, int *phich /*[cap]*/, int *order /*[cap]*/, int cap, int *n_lists) {
  PdcMap m;
  std::vector<int> a, b, o;
  const bool ok = pdc_build_map(n_rb, ports, cp_type, id, dur, res, mi, cfi, &m, &a, &b, &o);
  *n_reg = m.n_reg; *n_cce = m.n_cce;
  std::memcpy(re, m.re, sizeof(m.re));
  n_lists[0] = (int)a.size(); n_lists[1] = (int)b.size(); n_lists[2] = (int)o.size();
  for (size_t i = 0; i < a.size() && i < 4; ++i) pcfich[i] = a[i];
  for (size_t i = 0; i < b.size() && (int)i < cap; ++i) phich[i] = b[i];
  for (size_t i = 0; i < o.size() && (int)i < cap; ++i) order[i] = o[i];
  return ok ? 1 : 0;
}
extern "C" void pdcch_host_interleave(int n, int *w) {
  const std::vector<int> v = pdc_interleave(n);
  for (int i = 0; i < n; ++i) w[i] = v[(size_t)i];
}
extern "C" int pdcch_host_derm(int K, int E, int width, int16_t *out /*[3 K][width]*/) { return pdc_derm_build(K, E, width, out) ? 1 : 0; }
extern "C" void pdcch_host_scramble(int sf, int id, const uint32_t *jump1600, uint32_t *words /*[36]*/) {
  for (int w = 0; w < PDC_SCR_WORDS; ++w) words[w] = pdc_scramble_word(sf, id, w, jump1600);
}
extern "C" int pdcch_host_slot(int s, int n_cce, int *L, int *cce) { return pdc_slot(s, n_cce, L, cce) ? 1 : 0; }
extern "C" unsigned pdcch_host_rnti_x(unsigned long long bits, int A) { return pdc_rnti_x(bits, A); }

// The decoder on 3 n values d[s n + t].  form 0: the length-n forms; form 1 (n == 40 only): the PBCH's.  -> the 64 end metrics of pass
// 1, the winner (the lowest start state among the best, -1 without a finite one), its bits and its end metric from pass 2
extern "C" int pdcch_host_vit(const double *d, int n, int form, double *end64, unsigned long long *bits, double *end_pass2) {
  const double *d0 = d, *d1 = d + n, *d2 = d + 2 * n;
  double best = INFINITY;
  int ss = -1;
  for (int s = 0; s < 64; ++s) {
    const double fin = form ? vit_end_metric<false>(d0, d1, d2, s) : vit_end_metric_n<false>(d0, d1, d2, n, s);
    end64[s] = fin;
    if (fin < best) { best = fin; ss = s; }
  }
  *bits = 0ull; *end_pass2 = 0.0;
  if (ss >= 0) *bits = form ? vit_retrace_host(d0, d1, d2, ss, end_pass2) : vit_retrace_host_n(d0, d1, d2, n, ss, end_pass2);
  return ss;
}

// one candidate from the subframe's soft bits, as a wave of k_pdcch_dec
static lcs_pdcch_dec decode_candidate(const double *llr_sf, int cce, const int16_t *lst, int A, int rnti_mask) {
  const int K = A + 16;
  double d[PDC_MAX_CODED] = {}, lanes[64];
  bool finite = true;
  for (int lane = 0; lane < 64; ++lane) {
    double part = 0.0;
    for (int q = 0; q < 3; ++q) {
      const int b = lane + 64 * q;
      double v = 0.0;
      if (b < 3 * K) {
        v = pdc_coded_bit(llr_sf + 72 * cce, lst + b * PDC_DERM_W);
        d[b] = v;
        finite = finite && vit_finite(v);
      }
      part = part + fabs(v);
    }
    lanes[lane] = part;
  }
  const double den = meas_row_sum<64>(lanes);
  if (!finite) return pdc_entry_zero();
  double best = INFINITY;
  int ss = -1;
  for (int s = 0; s < 64; ++s) {
    const double fin = vit_end_metric_n<false>(d, d + K, d + 2 * K, K, s);
    if (fin < best) { best = fin; ss = s; }
  }
  if (ss < 0) return pdc_entry_zero();
  const unsigned long long bits = vit_retrace_host_n(d, d + K, d + 2 * K, K, ss, nullptr);
  return pdc_entry(bits, A, best, den, rnti_mask);
}

// tfg [n_ofdm][12 n_rb] complex; jump [2][32] as pcfich_host's; cfg with every field resolved (PHICH configuration, sizes) except
// phich_mi's -1 and rnti_mask's 0; cfi_in [n_sf]: the PCFICH's decision per subframe (read when cfg->cfi_force is 0);
// llr_out [n_sf][1152] or null (rows of subframes that are not read stay as they were) -> the record
extern "C" void pdcch_host(const double *tfg, int n_ofdm, int n_symb, int n_rb, int id, int cp_type, int n_ports, int dl_mask, const uint32_t *jump,
                           const lcs_pdcch_cfg *cfg, const int *cfi_in, double *llr_out, lcs_pdcch_info *out) {
  const int ports = pcf_ports(n_ports), n_sf = pcf_n_sf(n_ofdm, n_symb), n_max = pdc_n_ctrl_max(n_rb);
  const size_t ncol = (size_t)12 * n_rb;
  std::memset(out, 0, sizeof(*out));
  std::vector<PdcMap> maps(9);
  for (int mi = 0; mi < 3; ++mi)
    for (int cfi = 1; cfi <= 3; ++cfi) pdc_build_map(n_rb, ports, cp_type, id, cfg->phich_duration, cfg->phich_resource, mi, cfi, &maps[(size_t)(3 * mi + cfi - 1)]);
  std::vector<int16_t> derm((size_t)PDC_SIZES * 2 * PDC_MAX_CODED * PDC_DERM_W, (int16_t)-1);
  for (int si = 0; si < cfg->n_sizes; ++si)
    for (int lv = 0; lv < 2; ++lv) pdc_derm_build(cfg->size[si] + 16, lv ? 576 : 288, PDC_DERM_W, derm.data() + (size_t)(2 * si + lv) * PDC_MAX_CODED * PDC_DERM_W);
  bool tdd = false;
  for (int i = 0; i < 10; ++i) tdd = tdd || cfg->phich_mi[i] >= 0;
  const int rnti_mask = cfg->rnti_mask ? cfg->rnti_mask : 7;
  std::vector<double> llr((size_t)PDC_NLLR);
  for (int g = 0; g < n_sf && g < PCF_MAX_SF; ++g) {
    const int sf = g % 10, r0 = 2 * g * n_symb;
    if (!((dl_mask >> sf) & 1) || r0 + n_max - 1 >= n_ofdm) continue;
    if (tdd && cfg->phich_duration == 2 && (sf == 1 || sf == 6)) continue;
    const int cfi = cfg->cfi_force ? cfg->cfi_force : cfi_in[g];
    if (cfi < 1 || cfi > 3) continue;
    const int mi = cfg->phich_mi[sf] < 0 ? 1 : cfg->phich_mi[sf];
    const PdcMap &map = maps[(size_t)(3 * mi + cfi - 1)];
    if (map.n_cce == 0) continue;
    out->cfi[g] = cfi; out->n_reg[g] = map.n_reg; out->n_cce[g] = map.n_cce;
    uint32_t bits[2][RS_DL_WIDE_WORDS] = {}, scr[PDC_SCR_WORDS];
    double shift[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t = 0; t < (ports == 4 ? 2 : 1); ++t) rs_dl_row_wide(2 * sf, t, id, cp_type, n_symb, n_rb, jump, bits[t], shift);
    for (int w = 0; w < PDC_SCR_WORDS; ++w) scr[w] = pdc_scramble_word(sf, id, w, jump + 32);
    const double *row0 = tfg + (size_t)r0 * ncol * 2;
    const double *row1 = ports == 4 ? row0 + ncol * 2 : row0;
    for (int e = 0; e < PDC_NRE; e += 2) {
      double *l = llr.data() + 2 * e;
      l[0] = l[1] = l[2] = l[3] = 0.0;
      if (map.re[e] < 0) continue;
      cd2 y[2], ha[2], hb[2];
      for (int u = 0; u < 2; ++u) {
        const int re = map.re[e + u];
        pdc_elem(e + u, re & 0xffff, n_rb, ports, row0 + (size_t)(re >> 16) * ncol * 2, row0, row1, bits[0], bits[1], shift, &y[u], &ha[u], &hb[u]);
      }
      for (int u = 0; u < 2; ++u)
        pdc_llr(e + u, scr[(2 * (e + u)) >> 5], pcf_soft(e + u, ports, y[u], ha[u], hb[u ^ 1], y[u ^ 1]), &l[2 * u], &l[2 * u + 1]);
    }
    if (llr_out) std::memcpy(llr_out + (size_t)g * PDC_NLLR, llr.data(), sizeof(double) * PDC_NLLR);
    for (int s = 0; s < PDC_SLOTS; ++s) {
      int L, cce;
      if (!pdc_slot(s, map.n_cce, &L, &cce)) continue;
      for (int si = 0; si < cfg->n_sizes; ++si)
        out->dec[g][s][si] = decode_candidate(llr.data(), cce, derm.data() + (size_t)(2 * si + (L == 8 ? 1 : 0)) * PDC_MAX_CODED * PDC_DERM_W, cfg->size[si], rnti_mask);
    }
  }
  pdc_summary(out, n_sf, dl_mask, n_rb, ports);
}

#ifdef PDCCH_HOST_MAIN
// file: int32 n_ofdm, n_symb, n_rb, id, cp_type, n_ports, dl_mask, 0; uint32 jump[64]; lcs_pdcch_cfg; int32 cfi_in[72];
// double tfg[n_ofdm][12 n_rb][2]
int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int hdr[8], cfi_in[PCF_MAX_SF];
  uint32_t jump[64];
  lcs_pdcch_cfg cfg;
  bool ok = std::fread(hdr, sizeof(int), 8, f) == 8 && std::fread(jump, sizeof(uint32_t), 64, f) == 64 && std::fread(&cfg, sizeof(cfg), 1, f) == 1 &&
            std::fread(cfi_in, sizeof(int), PCF_MAX_SF, f) == PCF_MAX_SF;
  ok = ok && hdr[0] > 0 && hdr[0] <= LCS_TFG_MAX_OFDM && (hdr[1] == 6 || hdr[1] == 7) && pcf_rb_ok(hdr[2]) && hdr[3] >= 0 && hdr[3] < 504;
  ok = ok && cfg.n_sizes >= 1 && cfg.n_sizes <= 2 && cfg.phich_duration >= 1 && cfg.phich_duration <= 2 && cfg.phich_resource >= 1 && cfg.phich_resource <= 4;
  std::vector<double> tfg(ok ? (size_t)hdr[0] * 12 * hdr[2] * 2 : 0);
  ok = ok && std::fread(tfg.data(), sizeof(double), tfg.size(), f) == tfg.size();
  std::fclose(f);
  if (!ok) return 2;
  std::vector<lcs_pdcch_info> o(1);
  pdcch_host(tfg.data(), hdr[0], hdr[1], hdr[2], hdr[3], hdr[4], hdr[5], hdr[6], jump, &cfg, cfi_in, nullptr, &o[0]);
  std::printf("%d %d %d %d %d %d", o[0].n_sf, o[0].n_read, o[0].n_accepted, o[0].n_si, o[0].n_paging, o[0].n_ra);
  for (int g = 0; g < o[0].n_sf; ++g)
    for (int s = 0; s < PDC_SLOTS; ++s)
      for (int i = 0; i < PDC_SIZES; ++i) {
        const lcs_pdcch_dec &d = o[0].dec[g][s][i];
        std::printf(" %llu %u %d %.17g", (unsigned long long)d.bits, d.rnti_x, d.flags, d.quality);
      }
  std::printf("\n");
  return 0;
}
#endif
