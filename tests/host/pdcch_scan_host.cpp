// Host-side harness for pdcch_scan.h (the same __host__ __device__ code k_pscan_llr, k_pscan_dec, k_pscan_acc and k_pscan_fin run; the tables
// the kernels read are built by the very functions called here).  tests/test_pdcch_scan_host.py compares it with the numpy statement
// of the rule (tests/pdcch_scan_ref.py), tests/test_gpu_pdcch_scan.py holds the device's record and decode tables to it byte for
// byte.  With -DPDCCH_SCAN_HOST_MAIN the same source is a stand-alone program that reads one grid from a file and prints its record:
// the form that is built with -fsanitize=address,undefined.  Test infrastructure.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../lte-cell-scanner_amd/csrc/pdcch_scan.h"

extern "C" int pscan_host_record_bytes() { return (int)sizeof(lcs_pdcch_scan_info); }
extern "C" int pscan_host_cfg_bytes() { return (int)sizeof(lcs_pdcch_scan_cfg); }

// the map at the larger cap and, for comparison, the PDCCH stage's own
extern "C" int pscan_host_map(int n_rb, int ports, int cp_type, int id, int dur, int res, int mi, int cfi, int *n_reg, int *n_cce, int *re /*[3168]*/, int *re144 /*[576]*/) {
  std::vector<PscMap> m(1);
  PdcMap small;
  const bool ok = pdc_build_map_t<PSC_MAX_QUAD>(n_rb, ports, cp_type, id, dur, res, mi, cfi, &m[0]);
  const bool ok2 = pdc_build_map(n_rb, ports, cp_type, id, dur, res, mi, cfi, &small);
  *n_reg = m[0].n_reg; *n_cce = m[0].n_cce;
  std::memcpy(re, m[0].re, sizeof(m[0].re));
  std::memcpy(re144, small.re, sizeof(small.re));
  return (ok ? 1 : 0) | (ok2 ? 2 : 0) | ((small.n_reg == m[0].n_reg && small.n_cce == m[0].n_cce) ? 4 : 0);
}
// the 198 words by jumps and, for the first 36, by clocking from zero (pdc_scramble_word)
extern "C" void pscan_host_scramble(int sf, int id, uint32_t *words /*[198]*/, uint32_t *words36 /*[36]*/) {
  uint32_t jump[PSC_JUMP_WORDS];
  psc_build_jump(jump);
  for (int w = 0; w < PSC_SCR_WORDS; ++w) words[w] = psc_scramble_word(sf, id, w, jump);
  for (int w = 0; w < PDC_SCR_WORDS; ++w) words36[w] = pdc_scramble_word(sf, id, w, jump);
}
extern "C" int pscan_host_cand(int i, int n_cce, int *L, int *cce) {
  int lv;
  const bool ok = psc_cand(i, n_cce, &lv, cce);
  *L = 1 << lv;
  return ok ? 1 : 0;
}
extern "C" int pscan_host_n_cand(int n_cce) { return psc_n_cand(n_cce); }
// the distinct starts of the RNTIs' search spaces, ascending, -1 padded: out[r][sf][n_cce - 1][lv][6] for n_cce = 1 .. 88
extern "C" void pscan_host_spaces(const uint32_t *rnti, int n_rnti, signed char *out) {
  size_t o = 0;
  for (int r = 0; r < n_rnti; ++r)
    for (int sf = 0; sf < 10; ++sf)
      for (int n = 1; n <= PSC_MAX_CCE; ++n)
        for (int lv = 0; lv < 4; ++lv, o += 6) {
          int cnt = 0;
          for (int k = 0; k < 6; ++k) out[o + k] = -1;
          for (int c = 0; c + (1 << lv) <= n; c += 1 << lv)
            if (psc_in_space(rnti[r], sf, n, 1 << lv, c) && cnt < 6) out[o + cnt++] = (signed char)c;
        }
}
extern "C" unsigned pscan_host_rnti_x(unsigned long long lo, unsigned long long hi, int A, unsigned *narrow) {
  *narrow = A + 16 <= 64 ? pdc_rnti_x(lo, A) : 0u;
  return psc_rnti_x(lo, hi, A);
}

// one candidate at one size from its 72 L soft bits, as a wave of k_pscan_dec does; q_out [3 K] (or null): the quantised coded bits
static lcs_pdcch_scan_dec decode_one(const double *cl, int L, int lv, const int16_t *lst, int A, int sf, int n_cce, int cce, int rnti_mask, int *q_out, int *states) {
  const int K = A + 16;
  if (!psc_rate_ok(K, L)) return psc_entry_zero();
  double d[PSC_MAX_CODED], mx = 0.0;
  bool finite = true;
  for (int b = 0; b < 3 * K; ++b) {
    d[b] = pdc_coded_bit(cl, lst + b * PDC_DERM_W);
    finite = finite && vit_finite(d[b]);
    mx = fmax(mx, fabs(d[b]));
  }
  (void)lv;
  if (!finite) return psc_entry_zero();
  unsigned long long lo = 0ull, hi = 0ull;
  int n_obs = 0, n_err = 0, num = 0, den = 0, es = 0, ss = -1, q[PSC_MAX_CODED];
  if (mx > 0.0) {
    for (int b = 0; b < 3 * K; ++b) q[b] = psc_quant(d[b], mx);
    if (q_out) std::memcpy(q_out, q, sizeof(int) * 3 * K);
    psc_wava_host(q, K, &lo, &hi, &es, &ss);
    psc_score_host(q, K, lo, hi, &n_obs, &n_err, &num, &den);
  }
  if (states) { states[0] = es; states[1] = ss; }
  return psc_entry(lo, hi, A, es == ss, n_obs, n_err, num, den, sf, n_cce, L, cce, rnti_mask);
}
// the same for a test: the soft bits of one candidate alone (it sits at CCE `cce` of a subframe with n_cce CCEs)
extern "C" int pscan_host_decode(const double *cl, int L, int A, int sf, int n_cce, int cce, int rnti_mask, lcs_pdcch_scan_dec *out, int *q_out, int *states) {
  const int K = A + 16, lv = L == 1 ? 0 : L == 2 ? 1 : L == 4 ? 2 : 3;
  std::vector<int16_t> lst((size_t)PSC_MAX_CODED * PDC_DERM_W, (int16_t)-1);
  if (psc_rate_ok(K, L) && !pdc_derm_build(K, 72 * L, PDC_DERM_W, lst.data())) return 0;
  *out = decode_one(cl, L, lv, lst.data(), A, sf, n_cce, cce, rnti_mask, q_out, states);
  return 1;
}

// tfg [n_ofdm][12 n_rb] complex; jump [32]: the jump-ahead table of the reference sequence (pcfich_host's first); cfg with every
// field resolved except phich_mi's -1 and rnti_mask's 0; cfi_in [n_sf]: the PCFICH's decision per subframe (read when cfg->cfi_force
// is 0); msg_cap: LCS_PDCCH_SCAN_MAX_MSG, or less (the test hook for n_dropped); llr_out [n_sf][6336] or null; tab_out
// [n_sf][165][6] or null -> the record
extern "C" void pscan_host(const double *tfg, int n_ofdm, int n_symb, int n_rb, int id, int cp_type, int n_ports, int dl_mask, const uint32_t *jump,
                           const lcs_pdcch_scan_cfg *cfg, const int *cfi_in, int msg_cap, double *llr_out, lcs_pdcch_scan_dec *tab_out, lcs_pdcch_scan_info *out) {
  const int ports = pcf_ports(n_ports), n_sf_all = pcf_n_sf(n_ofdm, n_symb), n_sf = n_sf_all < PCF_MAX_SF ? n_sf_all : PCF_MAX_SF, n_max = pdc_n_ctrl_max(n_rb);
  const size_t ncol = (size_t)12 * n_rb;
  std::memset(out, 0, sizeof(*out));
  std::vector<PscMap> maps(9);
  for (int mi = 0; mi < 3; ++mi)
    for (int cfi = 1; cfi <= 3; ++cfi) pdc_build_map_t<PSC_MAX_QUAD>(n_rb, ports, cp_type, id, cfg->phich_duration, cfg->phich_resource, mi, cfi, &maps[(size_t)(3 * mi + cfi - 1)]);
  std::vector<int16_t> derm((size_t)PSC_SIZES * 4 * PSC_MAX_CODED * PDC_DERM_W, (int16_t)-1);
  for (int si = 0; si < cfg->n_sizes; ++si)
    for (int lv = 0; lv < 4; ++lv)
      if (psc_rate_ok(cfg->size[si] + 16, 1 << lv)) pdc_derm_build(cfg->size[si] + 16, 72 << lv, PDC_DERM_W, derm.data() + (size_t)(4 * si + lv) * PSC_MAX_CODED * PDC_DERM_W);
  uint32_t sj[PSC_JUMP_WORDS];
  psc_build_jump(sj);
  bool tdd = false;
  for (int i = 0; i < 10; ++i) tdd = tdd || cfg->phich_mi[i] >= 0;
  const int rnti_mask = cfg->rnti_mask ? cfg->rnti_mask : 7;
  std::vector<double> llr((size_t)PSC_NLLR);
  std::vector<lcs_pdcch_scan_dec> tab((size_t)PCF_MAX_SF * PSC_MAX_CAND * PSC_SIZES, psc_entry_zero());
  for (int g = 0; g < n_sf; ++g) {
    const int sf = g % 10, r0 = 2 * g * n_symb;
    if (!((dl_mask >> sf) & 1) || r0 + n_max - 1 >= n_ofdm) continue;
    if (tdd && cfg->phich_duration == 2 && (sf == 1 || sf == 6)) continue;
    const int cfi = cfg->cfi_force ? cfg->cfi_force : cfi_in[g];
    if (cfi < 1 || cfi > 3) continue;
    const int mi = cfg->phich_mi[sf] < 0 ? 1 : cfg->phich_mi[sf];
    const PscMap &map = maps[(size_t)(3 * mi + cfi - 1)];
    if (map.n_cce == 0 || map.n_cce > PSC_MAX_CCE) continue;
    out->sf[g].cfi = cfi; out->sf[g].n_reg = map.n_reg; out->sf[g].n_cce = map.n_cce;
    uint32_t bits[2][RS_DL_WIDE_WORDS] = {}, scr[PSC_SCR_WORDS];
    double shift[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t = 0; t < (ports == 4 ? 2 : 1); ++t) rs_dl_row_wide(2 * sf, t, id, cp_type, n_symb, n_rb, jump, bits[t], shift);
    for (int w = 0; w < PSC_SCR_WORDS; ++w) scr[w] = psc_scramble_word(sf, id, w, sj);
    const double *row0 = tfg + (size_t)r0 * ncol * 2;
    const double *row1 = ports == 4 ? row0 + ncol * 2 : row0;
    for (int e = 0; e < PSC_NRE; e += 2) {
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
    if (llr_out) std::memcpy(llr_out + (size_t)g * PSC_NLLR, llr.data(), sizeof(double) * PSC_NLLR);
    for (int i = 0; i < psc_n_cand(map.n_cce); ++i) {
      int lv, cce;
      psc_cand(i, map.n_cce, &lv, &cce);
      for (int si = 0; si < cfg->n_sizes; ++si)
        tab[((size_t)g * PSC_MAX_CAND + i) * PSC_SIZES + si] = decode_one(llr.data() + 72 * cce, 1 << lv, lv, derm.data() + (size_t)(4 * si + lv) * PSC_MAX_CODED * PDC_DERM_W,
                                                                          cfg->size[si], sf, map.n_cce, cce, rnti_mask, nullptr, nullptr);
    }
  }
  psc_finish_host(out, tab.data(), n_sf, cfg->n_sizes, cfg->min_quality, cfg->min_repeat, msg_cap < PSC_MAX_MSG ? msg_cap : PSC_MAX_MSG, dl_mask, n_rb, ports);
  if (tab_out) std::memcpy(tab_out, tab.data(), sizeof(lcs_pdcch_scan_dec) * (size_t)n_sf * PSC_MAX_CAND * PSC_SIZES);
}

#ifdef PDCCH_SCAN_HOST_MAIN
// file: int32 n_ofdm, n_symb, n_rb, id, cp_type, n_ports, dl_mask, 0; uint32 jump[32]; lcs_pdcch_scan_cfg; int32 cfi_in[72];
// double tfg[n_ofdm][12 n_rb][2]
int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int hdr[8], cfi_in[PCF_MAX_SF];
  uint32_t jump[32];
  lcs_pdcch_scan_cfg cfg;
  bool ok = std::fread(hdr, sizeof(int), 8, f) == 8 && std::fread(jump, sizeof(uint32_t), 32, f) == 32 && std::fread(&cfg, sizeof(cfg), 1, f) == 1 &&
            std::fread(cfi_in, sizeof(int), PCF_MAX_SF, f) == PCF_MAX_SF;
  ok = ok && hdr[0] > 0 && hdr[0] <= LCS_TFG_MAX_OFDM && (hdr[1] == 6 || hdr[1] == 7) && pcf_rb_ok(hdr[2]) && hdr[3] >= 0 && hdr[3] < 504;
  ok = ok && cfg.n_sizes >= 1 && cfg.n_sizes <= PSC_SIZES && cfg.phich_duration >= 1 && cfg.phich_duration <= 2 && cfg.phich_resource >= 1 && cfg.phich_resource <= 4;
  for (int i = 0; ok && i < cfg.n_sizes; ++i) ok = cfg.size[i] >= 8 && cfg.size[i] <= 64;
  std::vector<double> tfg(ok ? (size_t)hdr[0] * 12 * hdr[2] * 2 : 0);
  ok = ok && std::fread(tfg.data(), sizeof(double), tfg.size(), f) == tfg.size();
  std::fclose(f);
  if (!ok) return 2;
  std::vector<lcs_pdcch_scan_info> o(1);
  pscan_host(tfg.data(), hdr[0], hdr[1], hdr[2], hdr[3], hdr[4], hdr[5], hdr[6], jump, &cfg, cfi_in, PSC_MAX_MSG, nullptr, nullptr, &o[0]);
  std::printf("%d %d %d %d %d %d %d %d %d %d", o[0].n_sf, o[0].n_read, o[0].n_accepted, o[0].n_si, o[0].n_paging, o[0].n_ra, o[0].n_ue, o[0].n_rnti, o[0].n_msg, o[0].n_dropped);
  for (int i = 0; i < o[0].n_msg; ++i) {
    const lcs_pdcch_scan_msg &m = o[0].msg[i];
    std::printf(" %d %d %d %d %llu %u %d %d %d %d %.17g", m.g, m.L, m.cce, m.size_index, (unsigned long long)m.d.bits, m.d.rnti_x, m.d.flags, m.d.n_repeat, m.d.n_err, m.d.n_obs,
                m.d.quality);
  }
  std::printf("\n");
  return 0;
}
#endif
