// Host-side harness for pdsch.h (the same __host__ __device__ code k_pdsch_plan, k_pdsch_llr, k_pdsch_dec and k_pdsch_fin run; the
// tables the kernels read are built by the very functions called here).  tests/test_pdsch_host.py compares it with the numpy
// statement of the rule (tests/pdsch_ref.py), tests/test_gpu_pdsch.py holds the device's record to it byte for byte.  The windows of
// an iteration run one after the other here, each from the boundary metrics as they stood before the half iteration: what the
// kernel's lanes read before any of them writes.  With -DPDSCH_HOST_MAIN the same source is a stand-alone program that decodes
// blocks from a file: the form that is built with -fsanitize=address,undefined.  Test infrastructure.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../lte-cell-scanner_amd/csrc/pdsch.h"

extern "C" int pdsch_host_record_bytes() { return (int)sizeof(lcs_pdsch_info); }
extern "C" int pdsch_host_cfg_bytes() { return (int)sizeof(lcs_pdsch_cfg); }
extern "C" int pdsch_host_block_bytes() { return (int)sizeof(lcs_pdsch_block); }
extern "C" int pdsch_host_tbs(int col, int mcs) { return PDS_TBS[col][mcs]; }
extern "C" int pdsch_host_k_at(int i) { return pds_k_at(i); }
extern "C" int pdsch_host_k_ceil_index(int B) { return pds_k_ceil_index(B); }
extern "C" int pdsch_host_k_index(int K) { return pds_k_index(K); }
extern "C" void pdsch_host_qpp(int i, int *f) { f[0] = PDS_QPP[i][0]; f[1] = PDS_QPP[i][1]; }
extern "C" void pdsch_host_perm(int K, int *out) {
  const int i = pds_k_index(K);
  for (int k = 0; k < K; ++k) out[k] = pds_qpp(PDS_QPP[i][0], PDS_QPP[i][1], K, k);
}
extern "C" int pdsch_host_crc24a(const uint8_t *bits, int n) {
  std::vector<uint32_t> w((size_t)(n + 31) / 32, 0u);
  for (int k = 0; k < n; ++k) w[(size_t)k >> 5] |= (uint32_t)(bits[k] & 1) << (k & 31);
  return (int)pds_crc24a(w.data(), n);
}
// the scrambling words of a block as k_pdsch_llr makes them: chunk t of PDS_SCR_CHUNK words from the registers 1600 + 160 t clocks on,
// the second register jumped there bit by bit of t.  jump [320] as pdsch_host's; words [PDS_SCR_CHUNK n_chunk]
extern "C" void pdsch_host_scramble(unsigned c_init, int n_chunk, const uint32_t *jump, uint32_t *words) {
  uint32_t x1s[256];
  pds_x1_states(x1s);
  for (int t = 0; t < n_chunk && t < 256; ++t) {
    uint32_t x2 = pds_x2_jump(c_init, jump + 32);
    for (int b = 0; b < 8; ++b) if ((t >> b) & 1) x2 = pds_x2_jump(x2, jump + 64 + 32 * b);
    pds_scr_chunk(x1s[t], x2, words + PDS_SCR_CHUNK * t);
  }
}
extern "C" unsigned pdsch_host_c_init(int rnti, int sf, int id) { return pds_c_init(rnti, sf, id); }
// the elements of a grant as the kernel walks them: lk[2 e], lk[2 e + 1] = (l, k); returns N_RE
extern "C" int pdsch_host_elements(int n_rb, int ports, int n_symb, int id, int sf, int tdd, int n_ctrl, int rb_start, int n_prb, int *lk, int cap) {
  PdsGeom q;
  q.n_rb = n_rb; q.ports = ports; q.n_symb = n_symb; q.id = id; q.sf = sf; q.tdd = tdd; q.n_ctrl = n_ctrl; q.k_lo = 12 * rb_start; q.k_hi = 12 * (rb_start + n_prb);
  int base[PDS_MAX_SYM + 1];
  const int n = pds_bases(q, base);
  for (int e = 0; e < n && e < cap; ++e) pds_elem_at(q, base, e, &lk[2 * e], &lk[2 * e + 1]);
  return n;
}
// the fields of a format 1A payload: out = flag, distributed, rb_start, n_prb, mcs, rv, tpc
extern "C" void pdsch_host_1a(unsigned long long bits, int n_rb, int tdd, int *out) {
  const Pds1a f = pds_1a_fields(bits, n_rb, tdd);
  out[0] = f.flag; out[1] = f.distributed; out[2] = f.rb_start; out[3] = f.n_prb; out[4] = f.mcs; out[5] = f.rv; out[6] = f.tpc;
}
// the three streams of a block from its G soft bits, d [3][K + 4]
extern "C" void pdsch_host_derm(const double *llr, int G, int K, int F, int rv, double *d) {
  PdsTabHead h;
  std::vector<int16_t> rank((size_t)3 * PDS_MAX_D);
  pds_rank_build(K, F, &h, rank.data());
  for (int s = 0; s < 3; ++s)
    for (int k = 0; k < K + 4; ++k) d[s * (K + 4) + k] = pds_derm_value(llr, G, h.N, h.base[rv & 3], rank[(size_t)s * PDS_MAX_D + k]);
}

// the decoder as one workgroup of k_pdsch_dec runs it: d [3][K + 4] -> the decisions [K], the iterations, the status
static int decode_block(const double *dv, int K, int F, int f1, int f2, int max_iter, uint8_t *hard_out, int *n_iter) {
  const int D = K + 4, n_win = (K + PDS_WIN - 1) / PDS_WIN;
  std::vector<double> d[3], ext((size_t)PDS_PAD_D, 0.0);
  bool any = false, bad = false;
  for (int s = 0; s < 3; ++s) {
    d[s].assign((size_t)PDS_PAD_D, 0.0);
    for (int k = 0; k < D; ++k) {
      const double v = dv[s * D + k];
      d[s][(size_t)pds_pad(k)] = v;
      any = any || v != 0.0;
      bad = bad || !vit_finite(v);
    }
  }
  *n_iter = 0;
  for (int k = 0; k < K; ++k) hard_out[k] = 0;
  if (!any || bad) return LCS_PDSCH_SILENT;
  std::vector<uint16_t> perm((size_t)K);
  std::vector<uint8_t> hard((size_t)K, 0);
  for (int i = 0; i < K; ++i) perm[(size_t)i] = (uint16_t)pds_qpp(f1, f2, K, i);
  typedef double Metric[8];
  std::vector<double> ab_store((size_t)2 * 2 * (PDS_MAX_WIN + 1) * 8, 0.0);
  auto ab = [&](int dec, int fb, int w) -> double * { return ab_store.data() + (size_t)(((dec * 2 + fb) * (PDS_MAX_WIN + 1)) + w) * 8; };
  for (int dec = 0; dec < 2; ++dec) {
    for (int s = 1; s < 8; ++s) ab(dec, 0, 0)[s] = -INFINITY;
    const int o = K + 2 * dec;
    const double x[3] = {d[0][(size_t)pds_pad(o)], d[2][(size_t)pds_pad(o)], d[1][(size_t)pds_pad(o + 1)]};
    const double z[3] = {d[1][(size_t)pds_pad(o)], d[0][(size_t)pds_pad(o + 1)], d[2][(size_t)pds_pad(o + 1)]};
    Metric b;
    pds_tail_beta(x, z, b);
    for (int s = 0; s < 8; ++s) ab(dec, 1, n_win)[s] = b[s];
  }
  double ws[PDS_WIN * 8];
  std::vector<uint32_t> word((size_t)PDS_MAX_WIN, 0u);
  bool ok = false;
  for (int it = 1; it <= max_iter && !ok; ++it) {
    for (int dec = 0; dec < 2; ++dec) {
      const std::vector<double> old(ab_store);              // every lane reads before any lane writes
      for (int w = 0; w < n_win; ++w) {
        Metric a, b;
        const double *oa = old.data() + (size_t)(((dec * 2 + 0) * (PDS_MAX_WIN + 1)) + w) * 8, *ob = old.data() + (size_t)(((dec * 2 + 1) * (PDS_MAX_WIN + 1)) + w + 1) * 8;
        for (int s = 0; s < 8; ++s) { a[s] = oa[s]; b[s] = ob[s]; }
        const int k0 = PDS_WIN * w, n = K - k0 < PDS_WIN ? K - k0 : PDS_WIN;
        pds_window(d[0].data(), d[1 + dec].data(), ext.data(), dec ? perm.data() : nullptr, dec ? hard.data() : nullptr, F, k0, n, a, b, ws, 1);
        if (w + 1 < n_win) for (int s = 0; s < 8; ++s) ab(dec, 0, w + 1)[s] = a[s];
        if (w > 0) for (int s = 0; s < 8; ++s) ab(dec, 1, w)[s] = b[s];
      }
    }
    for (int w = 0; w < n_win; ++w) {
      uint32_t v = 0;
      for (int t = 0; t < PDS_WIN && PDS_WIN * w + t < K; ++t) v |= (uint32_t)((PDS_WIN * w + t >= F) ? (hard[(size_t)PDS_WIN * w + t] & 1) : 0) << t;
      word[(size_t)w] = v;
    }
    ok = pds_crc24a(word.data(), K) == 0u;
    *n_iter = it;
  }
  for (int k = 0; k < K; ++k) hard_out[k] = k >= F ? (hard[(size_t)k] & 1) : 0;
  return ok ? LCS_PDSCH_OK : LCS_PDSCH_CRC;
}
// lcs_turbo_decode's twin; returns the status
extern "C" int pdsch_host_turbo(const double *d, int K, int F, int max_iter, uint8_t *bits, int *n_iter) {
  const int ki = pds_k_index(K);
  if (ki < 0 || F < 0 || F >= K) return -1;
  return decode_block(d, K, F, PDS_QPP[ki][0], PDS_QPP[ki][1], max_iter, bits, n_iter);
}

// tfg [n_ofdm][12 n_rb] complex; jump [320]: to the reference sequence, by 1600 clocks, by 160 2^b clocks (b < 8); phich_duration and
// tdd as the PDCCH call resolved them; pdc: the PDCCH record the grants are read from; cfg with every field resolved (max_iter,
// rnti_mask); llr_out [n_sf][2][llr_stride] or null, d_out [n_sf][2][3][2244] or null (rows of slots that are not followed stay as
// they were) -> the record
extern "C" void pdsch_host(const double *tfg, int n_ofdm, int n_symb, int n_rb, int id, int cp_type, int n_ports, int dl_mask, const uint32_t *jump,
                           int phich_duration, int tdd, const lcs_pdcch_info *pdc, const lcs_pdsch_cfg *cfg, double *llr_out, int llr_stride, double *d_out,
                           lcs_pdsch_info *out) {
  const int ports = pcf_ports(n_ports), n_sf = pcf_n_sf(n_ofdm, n_symb), n_max = pdc_n_ctrl_max(n_rb);
  std::memset(out, 0, sizeof(*out));
  std::vector<int> tabs((size_t)2 * PDS_N_MCS + 2 * PDS_N_K);
  for (int i = 0; i < 2 * PDS_N_MCS; ++i) tabs[(size_t)i] = PDS_TBS[i / PDS_N_MCS][i % PDS_N_MCS];
  for (int i = 0; i < 2 * PDS_N_K; ++i) tabs[(size_t)(2 * PDS_N_MCS + i)] = PDS_QPP[i / 2][i % 2];
  std::vector<PdsTabHead> heads((size_t)PDS_TABS);
  std::vector<int16_t> rank((size_t)PDS_TABS * 3 * PDS_MAX_D, (int16_t)-1);
  for (int t = 0; t < 2 * PDS_N_MCS; ++t) {
    const int B = PDS_TBS[t / PDS_N_MCS][t % PDS_N_MCS] + 24, K = pds_k_at(pds_k_ceil_index(B));
    pds_rank_build(K, K - B, &heads[(size_t)t], rank.data() + (size_t)t * 3 * PDS_MAX_D);
  }
  PdsPlanIn in;
  in.n_rb = n_rb; in.ports = ports; in.n_symb = n_symb; in.id = id; in.tdd = tdd; in.i_1a = cfg->i_1a; in.rnti_mask = cfg->rnti_mask; in.max_iter = cfg->max_iter;
  in.n_forced = cfg->n_forced;
  for (int f = 0; f < LCS_PDSCH_MAX_FORCED; ++f) {
    in.forced[f] = cfg->forced[f];
    if (f >= cfg->n_forced) continue;
    const int B = cfg->forced[f].tbs + 24, K = pds_k_at(pds_k_ceil_index(B)), t = 2 * PDS_N_MCS + f;
    pds_rank_build(K, K - B, &heads[(size_t)t], rank.data() + (size_t)t * 3 * PDS_MAX_D);
  }
  uint32_t x1s[256];
  pds_x1_states(x1s);
  std::vector<lcs_pdsch_block> blk((size_t)PDS_GRANTS * n_sf);
  std::vector<PdsJob> job((size_t)PDS_GRANTS * n_sf);
  std::vector<int> res((size_t)2 * PDS_GRANTS * n_sf, 0);
  std::vector<uint8_t> hard((size_t)PDS_GRANTS * n_sf * PDS_MAX_K, 0);
  for (int g = 0; g < n_sf; ++g) {
    const int r0 = 2 * g * n_symb, sf = g % 10;
    int row0 = -1;
    if (((dl_mask >> sf) & 1) && r0 + n_max - 1 < n_ofdm && !(tdd && phich_duration == 2 && (sf == 1 || sf == 6)) && r0 + 2 * n_symb <= n_ofdm &&
        !(tdd && (sf == 1 || sf == 6))) row0 = r0;
    pds_plan_sf(in, g, row0, pdc, tabs.data(), tabs.data() + 2 * PDS_N_MCS, heads.data(), &blk[(size_t)PDS_GRANTS * g], &job[(size_t)PDS_GRANTS * g]);
  }
  std::vector<double> llr((size_t)2 * 12 * n_rb * PDS_MAX_SYM), dv((size_t)3 * PDS_MAX_D);
  for (int slot = 0; slot < PDS_GRANTS * n_sf; ++slot) {
    const PdsJob &j = job[(size_t)slot];
    res[(size_t)2 * slot] = 0; res[(size_t)2 * slot + 1] = j.status;
    if (j.status != LCS_PDSCH_FOLLOW) continue;
    PdsGeom q;
    q.n_rb = n_rb; q.ports = ports; q.n_symb = n_symb; q.id = id; q.sf = j.sf; q.tdd = j.tdd; q.n_ctrl = j.n_ctrl; q.k_lo = j.k_lo; q.k_hi = j.k_hi;
    uint32_t bits[6][RS_DL_WIDE_WORDS] = {};
    double shift[6][4] = {};
    for (int i = 0; i < (ports == 4 ? 6 : 4); ++i) pds_ref_row(i, j.sf, id, cp_type, n_symb, n_rb, jump, bits[i], shift[i]);
    int base[PDS_MAX_SYM + 1];
    pds_bases(q, base);
    std::vector<uint32_t> scr((size_t)PDS_SCR_WORDS, 0u);
    const int n_chunk = (2 * j.n_re + 32 * PDS_SCR_CHUNK - 1) / (32 * PDS_SCR_CHUNK);
    for (int t = 0; t < n_chunk; ++t) {
      uint32_t x2 = pds_x2_jump((uint32_t)j.c_init, jump + 32);
      for (int b = 0; b < 8; ++b) if ((t >> b) & 1) x2 = pds_x2_jump(x2, jump + 64 + 32 * b);
      pds_scr_chunk(x1s[t], x2, scr.data() + (size_t)PDS_SCR_CHUNK * t);
    }
    const double *sfrow = tfg + (size_t)j.row0 * 24 * n_rb;
    for (int e = 0; e < j.n_re; e += 2) {
      cd2 y[2], ha[2], hb[2];
      for (int u = 0; u < 2; ++u) {
        const bool live = e + u < j.n_re;
        int l = q.n_ctrl, k = q.k_lo;
        if (live) pds_elem_at(q, base, e + u, &l, &k);
        pds_elem(e + u, l, k, n_rb, ports, n_symb, sfrow, bits, shift, &y[u], &ha[u], &hb[u]);
        if (!live) { y[u] = mk(0.0, 0.0); hb[u] = mk(0.0, 0.0); }
      }
      for (int u = 0; u < 2 && e + u < j.n_re; ++u)
        pdc_llr(e + u, scr[(size_t)(2 * (e + u)) >> 5], pcf_soft(e + u, ports, y[u], ha[u], hb[u ^ 1], y[u ^ 1]), &llr[(size_t)2 * (e + u)], &llr[(size_t)2 * (e + u) + 1]);
    }
    if (llr_out) std::memcpy(llr_out + (size_t)slot * llr_stride, llr.data(), sizeof(double) * (size_t)j.G);
    const int16_t *rk = rank.data() + (size_t)j.tab * 3 * PDS_MAX_D;
    const int D = j.K + 4;
    for (int s = 0; s < 3; ++s)
      for (int k = 0; k < D; ++k) dv[(size_t)s * D + k] = pds_derm_value(llr.data(), j.G, j.N, j.base, rk[s * PDS_MAX_D + k]);
    if (d_out)
      for (int s = 0; s < 3; ++s) std::memcpy(d_out + ((size_t)slot * 3 + s) * PDS_MAX_D, dv.data() + (size_t)s * D, sizeof(double) * D);
    res[(size_t)2 * slot + 1] = decode_block(dv.data(), j.K, j.F, j.f1, j.f2, j.max_iter, hard.data() + (size_t)slot * PDS_MAX_K, &res[(size_t)2 * slot]);
  }
  int n = 0, over = 0, map[LCS_PDSCH_MAX_BLOCKS];
  for (int i = 0; i < PDS_GRANTS * n_sf; ++i) {
    if (job[(size_t)i].status == 0) continue;
    if (n < LCS_PDSCH_MAX_BLOCKS) map[n++] = i; else over += 1;
  }
  for (int i = 0; i < n; ++i) {
    const int sl = map[i], st = res[(size_t)2 * sl + 1];
    lcs_pdsch_block &o = out->block[i];
    o = blk[(size_t)sl];
    o.n_iter = res[(size_t)2 * sl]; o.status = st;
    for (int t = 0; t < LCS_PDSCH_PAYLOAD; ++t)
      o.payload[t] = (st == LCS_PDSCH_OK || st == LCS_PDSCH_CRC) ? pds_payload_byte(hard.data() + (size_t)sl * PDS_MAX_K, o.F, o.tbs, t) : 0;
  }
  pds_summary(out, n_sf, n, over, dl_mask, n_rb, ports);
}

#ifdef PDSCH_HOST_MAIN
// file: int32 n_ofdm, n_symb, n_rb, id, cp_type, n_ports, dl_mask, phich_duration, tdd, n_blocks; uint32 jump[320]; lcs_pdsch_cfg;
// lcs_pdcch_info; double tfg[n_ofdm][12 n_rb][2]; then per block int32 K, F, max_iter, 0 and double d[3][K + 4].  Prints the record's
// head and per block subframe, slot, status, iterations, n_re, K and the sum of the payload bytes; then per decoder block status,
// iterations and the CRC of the decisions.
int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int hdr[10];
  std::vector<uint32_t> jump(PDS_JUMP_WORDS);
  std::vector<lcs_pdcch_info> pdc(1);
  std::vector<lcs_pdsch_info> o(1);
  lcs_pdsch_cfg cfg;
  bool ok = std::fread(hdr, sizeof(int), 10, f) == 10 && std::fread(jump.data(), sizeof(uint32_t), jump.size(), f) == jump.size() &&
            std::fread(&cfg, sizeof(cfg), 1, f) == 1 && std::fread(&pdc[0], sizeof(lcs_pdcch_info), 1, f) == 1;
  ok = ok && hdr[0] > 0 && hdr[0] <= LCS_TFG_MAX_OFDM && (hdr[1] == 6 || hdr[1] == 7) && pcf_rb_ok(hdr[2]) && hdr[3] >= 0 && hdr[3] < 504 && hdr[9] >= 0 && hdr[9] <= 64;
  ok = ok && cfg.max_iter >= 1 && cfg.max_iter <= 16 && cfg.i_1a >= 0 && cfg.i_1a < PDC_SIZES && cfg.n_forced >= 0 && cfg.n_forced <= LCS_PDSCH_MAX_FORCED;
  std::vector<double> tfg(ok ? (size_t)hdr[0] * 12 * hdr[2] * 2 : 0);
  ok = ok && std::fread(tfg.data(), sizeof(double), tfg.size(), f) == tfg.size();
  if (ok) {
    pdsch_host(tfg.data(), hdr[0], hdr[1], hdr[2], hdr[3], hdr[4], hdr[5], hdr[6], jump.data(), hdr[7], hdr[8], &pdc[0], &cfg, nullptr, 0, nullptr, &o[0]);
    std::printf("%d %d %d %d %d %d %d\n", o[0].n_sf, o[0].n_blocks, o[0].n_ok, o[0].n_si, o[0].n_paging, o[0].n_ra, o[0].n_overflow);
    for (int i = 0; i < o[0].n_blocks; ++i) {
      const lcs_pdsch_block &b = o[0].block[i];
      int sum = 0;
      for (int t = 0; t < LCS_PDSCH_PAYLOAD; ++t) sum += b.payload[t];
      std::printf("%d %d %d %d %d %d %d\n", b.subframe, b.slot, b.status, b.n_iter, b.n_re, b.K, sum);
    }
  }
  for (int i = 0; ok && i < hdr[9]; ++i) {
    int bh[4];
    ok = std::fread(bh, sizeof(int), 4, f) == 4 && pds_k_index(bh[0]) >= 0 && bh[1] >= 0 && bh[1] < bh[0] && bh[2] >= 1 && bh[2] <= 16;
    if (!ok) break;
    std::vector<double> d((size_t)3 * (bh[0] + 4));
    ok = std::fread(d.data(), sizeof(double), d.size(), f) == d.size();
    if (!ok) break;
    std::vector<uint8_t> bits((size_t)bh[0]);
    int n_iter = 0;
    const int st = pdsch_host_turbo(d.data(), bh[0], bh[1], bh[2], bits.data(), &n_iter);
    std::printf("%d %d %d\n", st, n_iter, pdsch_host_crc24a(bits.data(), bh[0]));
  }
  std::fclose(f);
  return ok ? 0 : 2;
}
#endif
