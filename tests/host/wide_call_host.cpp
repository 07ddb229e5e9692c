// Host-side harness for wide_call.h: the refusals, the resolver and the row plans of the stages on the full-bandwidth grid, as
// lcs_api.hip runs them before anything is launched.  tests/test_wide_call_host.py compares them with the numpy statements of the
// rules.  With -DWIDE_CALL_HOST_MAIN the same source is a stand-alone program that walks the plans' whole domain, checks what a plan
// must hold and prints a digest: the form that is built with -fsanitize=address,undefined.  Test infrastructure.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../lte-cell-scanner_amd/csrc/wide_call.h"

// the text of one refusal, or null: which 0 the cell (a = n_id_1, b = n_id_2, c = cp_type), 1 n_ofdm (a, n_symb b), 2 the mask (a),
// 3 the bandwidth (the cell's n_rb_dl a, n_rb b)
extern "C" const char *wide_host_refusal(int which, int a, int b, int c) {
  if (which == 0) {
    lcs_cell cell;
    std::memset(&cell, 0, sizeof(cell));
    cell.n_id_1 = a; cell.n_id_2 = b; cell.cp_type = c;
    return wide_refuse_cell(&cell);
  }
  return which == 1 ? wide_refuse_n_ofdm(a, b) : which == 2 ? wide_refuse_mask(a) : wide_refuse_rb(a, b);
}

// the resolver: cfg_mi [10] or null; own: 0 none, else a text of the stage's own.  out [16]: duration, resource, mi[10], tdd, rnti_mask,
// cfi_force (written only where the call is accepted) -> the refusal, or null
extern "C" const char *wide_host_resolve(int cell_duration, int cell_resource, int cfg_duration, int cfg_resource, const int *cfg_mi, int rnti_mask, int cfi_force, int n_rb,
                                         int own, int *out) {
  WideShared s;
  std::memset(&s, 0, sizeof(s));
  const char *what = wide_resolve_shared(cell_duration, cell_resource, cfg_duration, cfg_resource, cfg_mi, rnti_mask, cfi_force, n_rb, own ? "the stage's own" : nullptr, &s);
  if (what) return what;
  out[0] = s.phich_duration; out[1] = s.phich_resource;
  for (int i = 0; i < 10; ++i) out[2 + i] = s.mi[i];
  out[12] = s.tdd; out[13] = s.rnti_mask; out[14] = s.cfi_force;
  return nullptr;
}

static const int KEEP[4] = {2, 4, 3, 4};
// one plan as the stage's function in lcs_api.hip makes it.  stage 0 PCFICH, 1 PDCCH (and the scan), 2 PHICH, 3 PDSCH; units [3]:
// the PHICH's map-unit counts; with_list: the sample form.  rows [KEEP[stage] PCF_MAX_SF], first / sfrow [PCF_MAX_SF], list
// [LCS_TFG_MAX_OFDM], *n_list -> n_sf
extern "C" int wide_host_plan(int stage, int n_symb, int n_ofdm, int ports, int n_rb, int dl_mask, int phich_duration, int tdd, const int *mi, const int *units,
                              int with_list, int *rows, int *first, int *sfrow, int *list, int *n_list) {
  WideShared s;
  std::memset(&s, 0, sizeof(s));
  s.phich_duration = phich_duration; s.tdd = tdd;
  for (int i = 0; i < 10; ++i) s.mi[i] = mi[i];
  int need[PCF_MAX_SF];
  std::vector<int> l;
  int rec = KEEP[stage];
  if (stage == 0) pcfich_need(n_symb, n_ofdm, ports, dl_mask, need);
  else if (stage == 1) pdcch_need(n_symb, n_ofdm, n_rb, dl_mask, s, need);
  else if (stage == 2) phich_need(n_symb, n_ofdm, ports, dl_mask, s, units, need);
  else { pdsch_need(n_symb, n_ofdm, n_rb, dl_mask, s, need); rec = pdc_n_ctrl_max(n_rb); }
  const int n_sf = wide_plan_rows(n_symb, n_ofdm, KEEP[stage], rec, need, rows, first, with_list ? &l : nullptr);
  for (int g = 0; g < n_sf; ++g) sfrow[g] = -1;
  if (stage == 3) pdsch_sfrow(n_symb, n_sf, need, first, sfrow);
  *n_list = (int)l.size();
  for (size_t i = 0; i < l.size(); ++i) list[i] = l[i];
  return n_sf;
}

// The plans' whole domain (both CPs; 1, 2, 4 ports; 6, 15, 25 resource blocks; both durations; TDD off and on; four masks; every
// n_ofdm from 2 n_symb to 4 n_symb + 4 and 122 n_symb; both forms) -> a digest of every output, or 0 where a plan breaks what it must
// hold: a list that grows strictly and stays inside the grid, rows that index it, list[rows[keep g + l]] = 2 g n_symb + l
extern "C" uint64_t wide_host_sweep(int *n_plans) {
  static const int MASKS[4] = {0x3FF, 0x021, 0x001, 0x200}, PORTS[3] = {1, 2, 4}, RBS[3] = {6, 15, 25}, MI[10] = {2, 1, 0, 1, 1, 2, 1, 0, 1, 1}, UNITS[3] = {0, 3, -1};
  uint64_t h = 1469598103934665603ull;
  auto mix = [&h](int v) { h = (h ^ (uint64_t)(uint32_t)v) * 1099511628211ull; };
  std::vector<int> rows(4 * PCF_MAX_SF), first(PCF_MAX_SF), sfrow(PCF_MAX_SF), list(LCS_TFG_MAX_OFDM);
  int n = 0;
  for (int n_symb = 6; n_symb <= 7; ++n_symb)
    for (int ports : PORTS) for (int n_rb : RBS) for (int dur = 1; dur <= 2; ++dur) for (int tdd = 0; tdd <= 1; ++tdd) for (int mask : MASKS)
      for (int k = 2 * n_symb; k <= 4 * n_symb + 5; ++k) {
        const int n_ofdm = k <= 4 * n_symb + 4 ? k : 122 * n_symb;
        for (int stage = 0; stage < 4; ++stage)
          for (int with_list = 0; with_list <= 1; ++with_list) {
            int n_list = 0;
            const int n_sf = wide_host_plan(stage, n_symb, n_ofdm, ports, n_rb, mask, dur, tdd, MI, UNITS, with_list, rows.data(), first.data(), sfrow.data(), list.data(), &n_list);
            for (int i = 0; i < n_list; ++i)
              if (list[i] < 0 || list[i] >= n_ofdm || (i > 0 && list[i] <= list[i - 1])) return 0;
            for (int g = 0; g < n_sf; ++g)
              for (int l = 0; l < KEEP[stage]; ++l) {
                const int r = rows[KEEP[stage] * g + l];
                if (r < 0) continue;
                if (with_list ? (r >= n_list || list[r] != 2 * g * n_symb + l) : r != 2 * g * n_symb + l) return 0;
              }
            mix(n_sf); mix(n_list);
            for (int i = 0; i < KEEP[stage] * n_sf; ++i) mix(rows[i]);
            for (int g = 0; g < n_sf; ++g) { mix(first[g]); mix(sfrow[g]); }
            for (int i = 0; i < n_list; ++i) mix(list[i]);
            n += 1;
          }
      }
  *n_plans = n;
  return h;
}

#ifdef WIDE_CALL_HOST_MAIN
int main() {
  int n = 0;
  const uint64_t h = wide_host_sweep(&n);
  // the resolver and the refusals on the edges of their domains
  int out[16], mi[10] = {-1, 0, 1, 2, -1, 0, 1, 2, -1, 0}, n_ref = 0;
  for (int cd = 0; cd <= 3; ++cd) for (int cr = 0; cr <= 5; ++cr) for (int fd = -1; fd <= 3; ++fd) for (int fr = -1; fr <= 5; ++fr)
    for (int cfi = -1; cfi <= 4; ++cfi) for (int rm = -1; rm <= 8; rm += 3)
      n_ref += wide_host_resolve(cd, cr, fd, fr, (cd + fr) & 1 ? mi : nullptr, rm, cfi, cr & 1 ? 6 : 25, 0, out) != nullptr;
  for (int a = -1; a <= 168; ++a) n_ref += wide_host_refusal(0, a, a % 4 - 1, a % 4) != nullptr;
  for (int a = 0; a <= 900; ++a) n_ref += (wide_host_refusal(1, a, 6 + (a & 1), 0) != nullptr) + (wide_host_refusal(2, a - 10, 0, 0) != nullptr) + (wide_host_refusal(3, a % 101, a % 103, 0) != nullptr);
  std::printf("%d %llu %d\n", n, (unsigned long long)h, n_ref);
  return h ? 0 : 1;
}
#endif
