// wide_call.h -- what the stages on the full-bandwidth grid (PCFICH, PDCCH, PDCCH scan, PHICH, PDSCH: lcs_api.hip) share before
// anything is launched: the refusals every one of them makes, what the PHICH configuration and the m_i of a call resolve to, and the
// plan of the grid rows a call needs.  Host code without a runtime call: lcs_api.hip runs it, and tests/host/wide_call_host.cpp
// compiles it for tests/test_wide_call_host.py.  A refusal is a text (the entry point puts its own name in front), null: accepted.
#pragma once
#include <vector>
#include "phich.h"

// ---- the refusals of every stage: each text exists here and nowhere else
inline bool wide_cell_identified(const lcs_cell *cell) {
  return (cell->cp_type == LCS_CP_NORMAL || cell->cp_type == LCS_CP_EXTENDED) && cell->n_id_1 >= 0 && cell->n_id_1 <= 167 && cell->n_id_2 >= 0 && cell->n_id_2 <= 2;
}
inline const char *wide_refuse_cell(const lcs_cell *cell) {
  return wide_cell_identified(cell) ? nullptr : "needs a cell with n_id_1, n_id_2 and a known cp_type";
}
inline const char *wide_refuse_n_ofdm(int n_ofdm, int n_symb) {
  return n_ofdm < 2 * n_symb || n_ofdm > 122 * n_symb ? "n_ofdm is outside 2 n_symb .. 122 n_symb (14 .. 854 normal CP, 12 .. 732 extended)" : nullptr;
}
inline const char *wide_refuse_mask(int dl_mask) {
  return meas_mask_ok(dl_mask) ? nullptr : "needs a dl_mask with at least one of the bits 0 .. 9 and none above";
}
// n_rb beyond the measurement's range: an LTE bandwidth, and the cell's where the cell says one
inline const char *wide_refuse_rb(int cell_n_rb_dl, int n_rb) {
  if (!pcf_rb_ok(n_rb)) return "n_rb is not an LTE bandwidth (6, 15, 25, 50, 75 or 100)";
  if (pcf_rb_ok(cell_n_rb_dl) && cell_n_rb_dl != n_rb) return "n_rb contradicts the cell's n_rb_dl";
  return nullptr;
}

// ---- what the PHICH configuration and the m_i of a call resolve to: the part of every stage's plan that the PDCCH, the scan and the
// PHICH configurations share.  tdd: an m_i was given (>= 0); mi: the m_i themselves, FDD's 1 where none was
struct WideShared { int phich_duration, phich_resource, mi[10], tdd, rnti_mask, cfi_force; };
// the resolved configuration of a call (the launchers' argument)
struct PdcchPlan { WideShared sh; int n_sizes, size[2]; };
struct PdcchScanPlan { WideShared sh; int n_sizes, size[LCS_PDCCH_SCAN_MAX_SIZES], min_repeat; double min_quality; };
struct PhichPlan { WideShared sh; double min_amp, min_sigma; };

// cfg_*: the call's fields, 0 deferring to the cell's; cfg_mi [10] (null: none given); rnti_mask 0: all three.  own: what the stage
// refuses about fields of its own that are checked behind the PHICH configuration and before the rest (the PDCCH's sizes), or null
inline const char *wide_resolve_shared(int cell_duration, int cell_resource, int cfg_duration, int cfg_resource, const int *cfg_mi, int rnti_mask, int cfi_force,
                                       int n_rb, const char *own, WideShared *s) {
  s->phich_duration = cfg_duration ? cfg_duration : cell_duration;
  s->phich_resource = cfg_resource ? cfg_resource : cell_resource;
  if (s->phich_duration == 0 || s->phich_resource == 0) return "the PHICH configuration is unknown: neither cfg nor the cell says it";
  if (s->phich_duration < 1 || s->phich_duration > 2) return "phich_duration is outside 1 (normal) .. 2 (extended)";
  if (s->phich_resource < 1 || s->phich_resource > 4) return "phich_resource is outside 1 (Ng = 1/6) .. 4 (Ng = 2)";
  if (own) return own;
  if (cfi_force < 0 || cfi_force > 3) return "cfi_force is outside 0 .. 3";
  if (cfi_force && s->phich_duration == 2 && pdc_n_ctrl(cfi_force, n_rb) < 3) return "the extended PHICH duration needs three control symbols: cfi_force gives fewer";
  s->cfi_force = cfi_force;
  s->tdd = 0;
  for (int i = 0; i < 10; ++i) {
    const int m = cfg_mi ? cfg_mi[i] : -1;
    if (m < -1 || m > 2) return "an m_i is outside 0 .. 2 (-1: FDD's 1)";
    s->mi[i] = m < 0 ? 1 : m;
    s->tdd = s->tdd || m >= 0;
  }
  if (rnti_mask < 0 || rnti_mask > 7) return "rnti_mask is outside 0 .. 7";
  s->rnti_mask = rnti_mask ? rnti_mask : 7;
  return nullptr;
}

// ---- the rows of a call.  A stage says, for every subframe g the grid reaches into, need[g]: how many of the subframe's leading rows
// it wants in the grid (0: the subframe is not read).  The planner answers with first[g], where the subframe's symbol 0 is, and
// rows[keep g + l] for l < min(need[g], rec), where its symbol l is: places in *list, the rows a transform is asked for -- or, with
// list null (the whole grid is there), the rows themselves; -1 elsewhere.  -> the number of subframes
inline int wide_plan_rows(int n_symb, int n_ofdm, int keep, int rec, const int *need, int *rows, int *first, std::vector<int> *list) {
  const int n_sf = pcf_n_sf(n_ofdm, n_symb);
  for (int g = 0; g < n_sf; ++g) {
    for (int l = 0; l < keep; ++l) rows[keep * g + l] = -1;
    first[g] = -1;
    if (need[g] <= 0) continue;
    const int r0 = 2 * g * n_symb;
    first[g] = list ? (int)list->size() : r0;
    if (list) for (int l = 0; l < need[g]; ++l) list->push_back(r0 + l);
    for (int l = 0; l < need[g] && l < rec; ++l) rows[keep * g + l] = first[g] + l;
  }
  return n_sf;
}

// the stages' rules.  PCFICH (keep 2): symbol 0 of a subframe of the mask, and symbol 1 with four ports
inline void pcfich_need(int n_symb, int n_ofdm, int ports, int dl_mask, int *need) {
  for (int g = 0; g < pcf_n_sf(n_ofdm, n_symb); ++g) need[g] = pcf_sf_used(g, n_ofdm, n_symb, ports, dl_mask) ? (ports == 4 ? 2 : 1) : 0;
}
// is subframe g read by the PDCCH: its bit of the mask and its symbols 0 .. n_ctrl_max - 1 inside the grid; a TDD call with the
// extended duration leaves out subframes 1 and 6
inline bool pdcch_sf_read(int g, int n_symb, int n_ofdm, int n_rb, int dl_mask, const WideShared &s) {
  const int sf = g % 10;
  if (!((dl_mask >> sf) & 1) || 2 * g * n_symb + pdc_n_ctrl_max(n_rb) - 1 >= n_ofdm) return false;
  return !(s.tdd && s.phich_duration == 2 && (sf == 1 || sf == 6));
}
// PDCCH and the scan (keep 4): the n_ctrl_max control symbols
inline void pdcch_need(int n_symb, int n_ofdm, int n_rb, int dl_mask, const WideShared &s, int *need) {
  for (int g = 0; g < pcf_n_sf(n_ofdm, n_symb); ++g) need[g] = pdcch_sf_read(g, n_symb, n_ofdm, n_rb, dl_mask, s) ? pdc_n_ctrl_max(n_rb) : 0;
}
// PHICH (keep 3): the rows the rule reads (symbol 0; symbol 1 with 4 ports; symbols 0 .. 2 at the extended duration) of a subframe
// whose map is not refused.  units [3]: n_unit of the unit table of m_i = 0 .. 2, -1: refused
inline void phich_need(int n_symb, int n_ofdm, int ports, int dl_mask, const WideShared &s, const int *units, int *need) {
  for (int g = 0; g < pcf_n_sf(n_ofdm, n_symb); ++g)
    need[g] = phi_sf_used(g, n_ofdm, n_symb, ports, s.phich_duration, s.tdd != 0, dl_mask) && units[s.mi[g % 10]] >= 0 ? phi_rows_needed(ports, s.phich_duration) : 0;
}
// PDSCH (keep 4, of which the n_ctrl_max control symbols are recorded): every row of a subframe the PDCCH reads that lies whole
// inside the grid and is no TDD special subframe, else the control symbols
inline bool pdsch_sf_whole(int g, int n_symb, int n_ofdm, const WideShared &s) {
  return 2 * (g + 1) * n_symb <= n_ofdm && !(s.tdd && (g % 10 == 1 || g % 10 == 6));
}
inline void pdsch_need(int n_symb, int n_ofdm, int n_rb, int dl_mask, const WideShared &s, int *need) {
  for (int g = 0; g < pcf_n_sf(n_ofdm, n_symb); ++g)
    need[g] = !pdcch_sf_read(g, n_symb, n_ofdm, n_rb, dl_mask, s) ? 0 : pdsch_sf_whole(g, n_symb, n_ofdm, s) ? 2 * n_symb : pdc_n_ctrl_max(n_rb);
}
// ... and sfrow[g]: where symbol 0 of a subframe that is there whole is, else -1
inline void pdsch_sfrow(int n_symb, int n_sf, const int *need, const int *first, int *sfrow) {
  for (int g = 0; g < n_sf; ++g) sfrow[g] = need[g] == 2 * n_symb ? first[g] : -1;
}
