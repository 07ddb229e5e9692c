// Host-side harness for the distributed allocations and format 1C of pdsch.h (the same __host__ __device__ code k_pdsch_plan and
// k_pdsch_llr_set run with a non-zero lcs_set_pdsch_alloc): the VRB to PRB map, the 1C fields, the set-based element enumeration and the
// whole record.  tests/test_pdsch_dvrb_host.py compares it with the numpy statement of the rule (tests/pdsch_dvrb_ref.py),
// tests/test_gpu_pdsch_dvrb.py holds the device's record to it byte for byte.  The decoder is pdsch_host.cpp's.  Test infrastructure.
#include "pdsch_host.cpp"

extern "C" int pdsch_dvrb_host_alloc_bytes() { return (int)sizeof(lcs_pdsch_alloc); }
extern "C" int pdsch_dvrb_host_alloc_cfg_bytes() { return (int)sizeof(lcs_pdsch_alloc_cfg); }
// out = N_gap, N_VRB, the interleaving unit, N_row, N_null
extern "C" void pdsch_dvrb_host_params(int n_rb, int gap, int *out) {
  const PdsDvrb d = pds_dvrb(n_rb, gap);
  out[0] = d.n_gap; out[1] = d.n_vrb; out[2] = d.unit; out[3] = d.n_row; out[4] = d.n_null;
}
extern "C" int pdsch_dvrb_host_prb(int n_rb, int gap, int vrb, int slot) { return pds_dvrb_prb(pds_dvrb(n_rb, gap), vrb, slot & 1); }
extern "C" int pdsch_dvrb_host_tbs_1c(int i) { return PDS_TBS_1C[i]; }
extern "C" int pdsch_dvrb_host_1c_bits(int n_rb) { return (n_rb >= 50 ? 1 : 0) + pds_1c_riv_bits(n_rb) + 5; }
// the fields of a format 1C payload: out = gap, riv, riv_ok, rb_start, n_prb, i_tbs, n_step
extern "C" void pdsch_dvrb_host_1c(unsigned long long bits, int n_rb, int *out) {
  const Pds1c f = pds_1c_fields(bits, n_rb);
  out[0] = f.gap; out[1] = f.riv; out[2] = f.riv_ok; out[3] = f.rb_start; out[4] = f.n_prb; out[5] = f.i_tbs; out[6] = f.n_step;
}
extern "C" int pdsch_dvrb_host_1c_rv(int kind, int g, int sfn0, int si_window) {
  const PdsAllocIn al = {2, sfn0, si_window, 1};
  return pds_1c_rv(kind, g, al);
}
// the elements of VRBs [v0, v0 + n) as the kernel walks them: lk[2 e], lk[2 e + 1] = (l, k); returns N_RE
extern "C" int pdsch_dvrb_host_elements(int n_rb, int ports, int n_symb, int id, int sf, int tdd, int n_ctrl, int gap, int v0, int n, int *lk, int cap) {
  PdsGeom q;
  q.n_rb = n_rb; q.ports = ports; q.n_symb = n_symb; q.id = id; q.sf = sf; q.tdd = tdd; q.n_ctrl = n_ctrl; q.k_lo = q.k_hi = 0;
  unsigned long long m[PDS_SET_WORDS];
  pds_set_masks(pds_dvrb(n_rb, gap), v0, n, m);
  int cut[4], base[PDS_MAX_SYM + 1];
  uint8_t prb[2 * PDS_SET_RB] = {};
  pds_set_cut(n_rb, m[0], m[1], cut);
  pds_set_cut(n_rb, m[2], m[3], cut + 2);
  pds_set_list(n_rb, m[0], m[1], prb);
  pds_set_list(n_rb, m[2], m[3], prb + PDS_SET_RB);
  const int n_re = pds_set_bases(q, n, cut, base);
  for (int e = 0; e < n_re && e < cap; ++e) pds_set_elem_at(q, prb, cut, base, e, &lk[2 * e], &lk[2 * e + 1]);
  return n_re;
}

// pdsch_host with the setting: al as lcs_set_pdsch_alloc takes it (the 1C size index is 1 - cfg->i_1a); alloc_out [32] or null: what
// lcs_pdsch_last_alloc says of every listed block
extern "C" void pdsch_dvrb_host(const double *tfg, int n_ofdm, int n_symb, int n_rb, int id, int cp_type, int n_ports, int dl_mask, const uint32_t *jump,
                                int phich_duration, int tdd, const lcs_pdcch_info *pdc, const lcs_pdsch_cfg *cfg, const lcs_pdsch_alloc_cfg *al_cfg, double *llr_out,
                                int llr_stride, lcs_pdsch_alloc *alloc_out, lcs_pdsch_info *out) {
  const int ports = pcf_ports(n_ports), n_sf = pcf_n_sf(n_ofdm, n_symb), n_max = pdc_n_ctrl_max(n_rb);
  std::memset(out, 0, sizeof(*out));
  std::vector<int> tabs((size_t)2 * PDS_N_MCS + 2 * PDS_N_K + PDS_N_1C);
  for (int i = 0; i < 2 * PDS_N_MCS; ++i) tabs[(size_t)i] = PDS_TBS[i / PDS_N_MCS][i % PDS_N_MCS];
  for (int i = 0; i < 2 * PDS_N_K; ++i) tabs[(size_t)(2 * PDS_N_MCS + i)] = PDS_QPP[i / 2][i % 2];
  for (int i = 0; i < PDS_N_1C; ++i) tabs[(size_t)(2 * PDS_N_MCS + 2 * PDS_N_K + i)] = PDS_TBS_1C[i];
  std::vector<PdsTabHead> heads((size_t)PDS_TABS + PDS_N_1C);
  std::vector<int16_t> rank((size_t)(PDS_TABS + PDS_N_1C) * 3 * PDS_MAX_D, (int16_t)-1);
  auto table = [&](int t, int tbs) {
    const int B = tbs + 24, K = pds_k_at(pds_k_ceil_index(B));
    pds_rank_build(K, K - B, &heads[(size_t)t], rank.data() + (size_t)t * 3 * PDS_MAX_D);
  };
  for (int t = 0; t < 2 * PDS_N_MCS; ++t) table(t, PDS_TBS[t / PDS_N_MCS][t % PDS_N_MCS]);
  for (int i = 0; i < PDS_N_1C; ++i) table(PDS_TABS + i, PDS_TBS_1C[i]);
  PdsPlanIn in;
  in.n_rb = n_rb; in.ports = ports; in.n_symb = n_symb; in.id = id; in.tdd = tdd; in.i_1a = cfg->i_1a; in.rnti_mask = cfg->rnti_mask; in.max_iter = cfg->max_iter;
  in.n_forced = cfg->n_forced;
  for (int f = 0; f < LCS_PDSCH_MAX_FORCED; ++f) {
    in.forced[f] = cfg->forced[f];
    if (f < cfg->n_forced) table(2 * PDS_N_MCS + f, cfg->forced[f].tbs);
  }
  const PdsAllocIn al = {al_cfg->flags, al_cfg->sfn0, al_cfg->si_window, 1 - cfg->i_1a};
  uint32_t x1s[256];
  pds_x1_states(x1s);
  std::vector<lcs_pdsch_block> blk((size_t)PDS_GRANTS * n_sf);
  std::vector<PdsJob> job((size_t)PDS_GRANTS * n_sf);
  std::vector<unsigned long long> sets((size_t)PDS_GRANTS * PDS_SET_WORDS * n_sf, 0ull);
  std::vector<int> res((size_t)2 * PDS_GRANTS * n_sf, 0);
  std::vector<uint8_t> hard((size_t)PDS_GRANTS * n_sf * PDS_MAX_K, 0);
  for (int g = 0; g < n_sf; ++g) {
    const int r0 = 2 * g * n_symb, sf = g % 10;
    int row0 = -1;
    if (((dl_mask >> sf) & 1) && r0 + n_max - 1 < n_ofdm && !(tdd && phich_duration == 2 && (sf == 1 || sf == 6)) && r0 + 2 * n_symb <= n_ofdm &&
        !(tdd && (sf == 1 || sf == 6))) row0 = r0;
    pds_plan_sf_alloc<true>(in, al, g, row0, pdc, tabs.data(), tabs.data() + 2 * PDS_N_MCS + 2 * PDS_N_K, tabs.data() + 2 * PDS_N_MCS, heads.data(), &blk[(size_t)PDS_GRANTS * g],
                      &job[(size_t)PDS_GRANTS * g], al.flags ? &sets[(size_t)PDS_GRANTS * PDS_SET_WORDS * g] : nullptr);
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
    const bool by_set = (j.reserved & PDS_MODE_SET) != 0;
    const unsigned long long *m = &sets[(size_t)PDS_SET_WORDS * slot];
    int base[PDS_MAX_SYM + 1], cut[4] = {0, 0, 0, 0};
    uint8_t prb[2 * PDS_SET_RB] = {};
    if (by_set) {
      pds_set_cut(n_rb, m[0], m[1], cut);
      pds_set_cut(n_rb, m[2], m[3], cut + 2);
      const int n0 = pds_set_list(n_rb, m[0], m[1], prb);
      pds_set_list(n_rb, m[2], m[3], prb + PDS_SET_RB);
      pds_set_bases(q, n0, cut, base);
    } else pds_bases(q, base);
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
        int l = q.n_ctrl, k = by_set ? 0 : q.k_lo;
        if (live && by_set) pds_set_elem_at(q, prb, cut, base, e + u, &l, &k);
        else if (live) pds_elem_at(q, base, e + u, &l, &k);
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
    if (alloc_out) pds_alloc_of(n_rb, blk[(size_t)sl], job[(size_t)sl].reserved, &alloc_out[i]);
  }
  pds_summary(out, n_sf, n, over, dl_mask, n_rb, ports);
}
