// Host-side harness for pdsch_comb.h (the same __host__ __device__ code k_pdsch_comb_group, k_pdsch_comb_dec and k_pdsch_comb_fin
// run) on top of the PDSCH stage's twin, whose source is compiled into this one: the stage's record, soft bits and decoder are
// pdsch_host.cpp's.  tests/test_pdsch_comb_host.py compares it with the numpy statement of the rule (tests/pdsch_comb_ref.py),
// tests/test_gpu_pdsch_comb.py holds the device's record to it byte for byte.  With -DPDSCH_COMB_HOST_MAIN the same source is a
// stand-alone program that groups and decodes a file of soft bits: the form built with -fsanitize=address,undefined.  Test
// infrastructure.
#include "pdsch_host.cpp"
#include "../../lte-cell-scanner_amd/csrc/pdsch_comb.h"

extern "C" int pdsch_comb_host_record_bytes() { return (int)sizeof(lcs_pdsch_comb_info); }
extern "C" int pdsch_comb_host_cfg_bytes() { return (int)sizeof(lcs_pdsch_comb_cfg); }
extern "C" int pdsch_comb_host_group_bytes() { return (int)sizeof(lcs_pdsch_comb_group); }

// The combined record from the stage's record and its soft bits.  rec: the PDSCH record; llr [n_sf][2][llr_stride]: the soft bits by
// grant slot (slot = 2 subframe + the block's place among its subframe's); max_iter resolved; d_out [8][3][2244] or null: the summed
// streams of the groups that are decoded
extern "C" void pdsch_comb_host_groups(const lcs_pdsch_info *rec, const double *llr, int llr_stride, int max_iter, const lcs_pdsch_comb_cfg *cfg, double *d_out,
                                       lcs_pdsch_comb_info *out) {
  std::memset(out, 0, sizeof(*out));
  const int n = rec->n_blocks < 0 ? 0 : rec->n_blocks > LCS_PDSCH_MAX_BLOCKS ? LCS_PDSCH_MAX_BLOCKS : rec->n_blocks;
  PdsCombBlock blk[LCS_PDSCH_MAX_BLOCKS];
  int slot_of[LCS_PDSCH_MAX_BLOCKS];
  for (int i = 0; i < n; ++i) {
    const lcs_pdsch_block &b = rec->block[i];
    blk[i].kind = b.kind; blk[i].status = b.status; blk[i].subframe = b.subframe; blk[i].tbs = b.tbs; blk[i].rv = b.rv;
    int u = 0;
    for (int v = 0; v < i; ++v) u += rec->block[v].subframe == b.subframe;
    slot_of[i] = PDS_GRANTS * b.subframe + u;
  }
  PdsCombJob job[PDS_COMB_GROUPS];
  int work[PDS_COMB_WORK], n_over = 0;
  const int n_groups = pds_comb_groups(blk, n, cfg->si_window, cfg->no_sib1, work, job, &n_over);
  std::vector<int16_t> rank((size_t)3 * PDS_MAX_D);
  std::vector<double> dv((size_t)3 * PDS_MAX_D);
  std::vector<uint8_t> hard((size_t)PDS_MAX_K);
  for (int gi = 0; gi < n_groups; ++gi) {
    const PdsCombJob &j = job[gi];
    lcs_pdsch_comb_group &o = out->group[gi];
    const lcs_pdsch_block &b0 = rec->block[j.block[0]];
    o.n_members = j.n_members; o.rule = j.rule; o.tbs = j.tbs; o.K = b0.K; o.F = b0.F; o.rv_mask = j.rv_mask; o.n_ok_members = j.n_ok;
    for (int m = 0; m < PDS_COMB_MEMBERS; ++m) o.member[m] = j.block[m];
    if (j.n_ok > 0 || j.n_members < 2) {
      const lcs_pdsch_block *src = nullptr;
      for (int m = 0; m < j.n_members && !src; ++m)
        if (j.n_ok == 0 || rec->block[j.block[m]].status == LCS_PDSCH_OK) src = &rec->block[j.block[m]];
      o.status = j.n_ok > 0 ? LCS_PDSCH_COMB_MEMBER : LCS_PDSCH_COMB_CRC;
      std::memcpy(o.payload, src->payload, LCS_PDSCH_PAYLOAD);
      for (int m = 0; m < j.n_members && j.n_ok > 0; ++m) {
        const lcs_pdsch_block &bm = rec->block[j.block[m]];
        o.n_same += bm.status == LCS_PDSCH_OK && std::memcmp(bm.payload, src->payload, LCS_PDSCH_PAYLOAD) == 0;
      }
      continue;
    }
    PdsTabHead h;
    pds_rank_build(o.K, o.F, &h, rank.data());
    const double *ml[PDS_COMB_MEMBERS];
    int mG[PDS_COMB_MEMBERS], mbase[PDS_COMB_MEMBERS];
    for (int m = 0; m < PDS_COMB_MEMBERS; ++m) {
      const int bi = j.block[m < j.n_members ? m : 0];
      ml[m] = llr + (size_t)slot_of[bi] * llr_stride; mG[m] = 2 * rec->block[bi].n_re; mbase[m] = h.base[rec->block[bi].rv & 3];
    }
    const int D = o.K + 4, ki = pds_k_index(o.K);
    for (int s = 0; s < 3; ++s)
      for (int k = 0; k < D; ++k) dv[(size_t)s * D + k] = pds_comb_value(ml, mG, mbase, j.n_members, h.N, rank[(size_t)s * PDS_MAX_D + k]);
    if (d_out)
      for (int s = 0; s < 3; ++s) std::memcpy(d_out + ((size_t)gi * 3 + s) * PDS_MAX_D, dv.data() + (size_t)s * D, sizeof(double) * D);
    const int st = decode_block(dv.data(), o.K, o.F, PDS_QPP[ki][0], PDS_QPP[ki][1], max_iter, hard.data(), &o.n_iter);
    o.status = st == LCS_PDSCH_OK ? LCS_PDSCH_COMB_OK : st == LCS_PDSCH_CRC ? LCS_PDSCH_COMB_CRC : LCS_PDSCH_COMB_SILENT;
    for (int t = 0; t < LCS_PDSCH_PAYLOAD; ++t) o.payload[t] = o.status == LCS_PDSCH_COMB_SILENT ? 0 : pds_payload_byte(hard.data(), o.F, o.tbs, t);
  }
  pds_comb_summary(out, n_groups, n_over);
}

// pdsch_host's arguments, then the combining's: both records.  d_out [8][3][2244] or null
extern "C" void pdsch_comb_host(const double *tfg, int n_ofdm, int n_symb, int n_rb, int id, int cp_type, int n_ports, int dl_mask, const uint32_t *jump, int phich_duration,
                                int tdd, const lcs_pdcch_info *pdc, const lcs_pdsch_cfg *cfg, const lcs_pdsch_comb_cfg *comb_cfg, double *d_out, lcs_pdsch_info *out,
                                lcs_pdsch_comb_info *comb_out) {
  const int n_sf = pcf_n_sf(n_ofdm, n_symb), stride = 2 * 12 * n_rb * PDS_MAX_SYM;
  std::vector<double> llr((size_t)PDS_GRANTS * n_sf * stride, 0.0);
  pdsch_host(tfg, n_ofdm, n_symb, n_rb, id, cp_type, n_ports, dl_mask, jump, phich_duration, tdd, pdc, cfg, llr.data(), stride, nullptr, out);
  pdsch_comb_host_groups(out, llr.data(), stride, cfg->max_iter, comb_cfg, d_out, comb_out);
}

#ifdef PDSCH_COMB_HOST_MAIN
// file: int32 llr_stride, max_iter, n_slots, 0; lcs_pdsch_comb_cfg; lcs_pdsch_info; double llr[n_slots][llr_stride].  Prints the head
// and per group n_members, rule, status, n_iter, n_ok_members, n_same and the sum of the payload bytes.
int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int hdr[4];
  lcs_pdsch_comb_cfg cfg;
  std::vector<lcs_pdsch_info> rec(1);
  std::vector<lcs_pdsch_comb_info> o(1);
  bool ok = std::fread(hdr, sizeof(int), 4, f) == 4 && std::fread(&cfg, sizeof(cfg), 1, f) == 1 && std::fread(&rec[0], sizeof(lcs_pdsch_info), 1, f) == 1;
  ok = ok && hdr[0] > 0 && hdr[0] <= 2 * 12 * 100 * PDS_MAX_SYM && hdr[1] >= 1 && hdr[1] <= 16 && hdr[2] > 0 && hdr[2] <= PDS_GRANTS * PCF_MAX_SF;
  std::vector<double> llr(ok ? (size_t)hdr[0] * hdr[2] : 0);
  ok = ok && std::fread(llr.data(), sizeof(double), llr.size(), f) == llr.size();
  std::fclose(f);
  if (!ok) return 2;
  pdsch_comb_host_groups(&rec[0], llr.data(), hdr[0], hdr[1], &cfg, nullptr, &o[0]);
  std::printf("%d %d %d %d\n", o[0].n_groups, o[0].n_overflow, o[0].n_members, o[0].n_decoded);
  for (int i = 0; i < o[0].n_groups; ++i) {
    const lcs_pdsch_comb_group &g = o[0].group[i];
    int sum = 0;
    for (int t = 0; t < LCS_PDSCH_PAYLOAD; ++t) sum += g.payload[t];
    std::printf("%d %d %d %d %d %d %d\n", g.n_members, g.rule, g.status, g.n_iter, g.n_ok_members, g.n_same, sum);
  }
  return 0;
}
#endif
