"""GPU tests of the stage that combines redundancy versions (lcs_pdsch_comb_wide, lcs_pdsch_comb; k_pdsch_comb_group,
k_pdsch_comb_dec, k_pdsch_comb_fin).

On every scenario of tests/pdsch_comb_cases.py: the combined record byte-equal to the host twin (tests/host/pdsch_comb_host.cpp) fed
with the device's own PDCCH record, and equal to the numpy statement of the rule; the PDSCH and PDCCH records the new call returns
byte-equal to lcs_pdsch's on the same grid.  From samples with a planted SIB1 schedule: lcs_pdsch_comb_wide equals lcs_pdsch_comb on
lcs_extract_tfg_wide's grid and the twin on it, and capi.sib1_fields of the rule-1 group is what was planted -- once where both
transmissions decode alone, once where the numpy rule on the extracted grid fails both and decodes their sum.  Refusals,
sweep.measure_wideband(pdsch_comb=True)."""
import functools

import numpy as np
import pytest

import pcfich_ref as PR
import pdcch_cases as DC
import pdsch_cases as SC
import pdsch_comb_cases as CC
from conftest import load_pkg

pytestmark = pytest.mark.gpu
FS = 1.92e6
FC = DC.CAP_FC
SFN0 = 7          # the capture starts in frame 7: the grid's frame 0 is frame 8, SIB1 lies in grid subframes 5 (rv 0) and 25 (rv 2)


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def S(pkg):
    s = pkg.Searcher(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def H(pkg):
    return CC.load_twin(pkg.capi)


def _case_cell(pkg, case):
    return pkg.new_cell(n_id_1=case[0] // 3, n_id_2=case[0] % 3, cp_type=case[1], n_ports=case[2])


@pytest.mark.parametrize("sc", CC.SCENARIOS, ids=lambda s: s["name"])
def test_combined_record_against_the_host_twin_and_numpy(pkg, S, H, sc):
    capi = pkg.capi
    tfg, cfi, _ = CC.crafted(sc)
    case = sc["case"]
    n_rb, mask = case[3], CC.mask_of(sc)
    cell, cfg, pcfg, ccfg = _case_cell(pkg, case), DC.make_cfg(capi, SC.pdcch_case(case)), CC.pdsch_cfg(capi, sc), CC.comb_cfg(capi, sc)
    got, comb, pdc = S.pdsch_comb(cell, tfg, n_rb, mask, cfg, pcfg, ccfg, want_pdcch=True)
    twin, twin_comb = CC.twin_records(H, capi, sc, tfg, pdc)
    diff = lambda a, b: np.flatnonzero(np.frombuffer(bytes(a), np.uint8) != np.frombuffer(bytes(b), np.uint8))[:8]
    assert bytes(comb) == bytes(twin_comb), (sc["name"], diff(comb, twin_comb), comb.groups(), twin_comb.groups())
    assert bytes(got) == bytes(twin), (sc["name"], diff(got, twin))
    _, blocks, ref = CC.reference(sc)
    assert SC.assert_blocks_against_numpy(got, blocks, sc["name"]) == (len(blocks), 0)
    CC.assert_groups_against_numpy(comb, ref, sc["name"])
    # the stage's own records are lcs_pdsch's on the same grid, and a call of lcs_pdsch in between changes nothing
    alone, pdc_alone = S.pdsch(cell, tfg, n_rb, mask, cfg, pcfg, want_pdcch=True)
    assert bytes(alone) == bytes(got) and bytes(pdc_alone) == bytes(pdc)
    again, comb_again = S.pdsch_comb(cell, tfg, n_rb, mask, cfg, pcfg, ccfg)
    assert bytes(again) == bytes(got) and bytes(comb_again) == bytes(comb)
    print(sc["name"], [(g["members"], g["status"], g["n_iter"]) for g in comb.groups()], "overflow", comb.n_overflow)


def test_configuration_changes_the_groups_not_the_stage(pkg, S):
    """one grid under the three configurations: rule 1, rule 2 alone, both off"""
    capi = pkg.capi
    sc = CC.by_name("more-info-than-coded")
    tfg, _, _ = CC.crafted(sc)
    case = sc["case"]
    cell, cfg = _case_cell(pkg, case), DC.make_cfg(capi, SC.pdcch_case(case))
    a, ca = S.pdsch_comb(cell, tfg, case[3], CC.mask_of(sc), cfg)
    b, cb = S.pdsch_comb(cell, tfg, case[3], CC.mask_of(sc), cfg, None, capi.PdschCombCfg.make(si_window=61, sib1=False))
    c, cc = S.pdsch_comb(cell, tfg, case[3], CC.mask_of(sc), cfg, None, capi.PdschCombCfg.make(sib1=False))
    assert bytes(a) == bytes(b) == bytes(c)
    assert [g["rule"] for g in ca.groups()] == [1] and [g["rule"] for g in cb.groups()] == [2] and cc.n_groups == 0
    assert ca.groups()[0]["bytes"] == cb.groups()[0]["bytes"] and ca.groups()[0]["status"] == "ok" and not any(bytes(cc)[:16])


def test_refusals(pkg, S):
    capi = pkg.capi
    sc = CC.by_name("rows")
    tfg, _, _ = CC.crafted(sc)
    case = sc["case"]
    cell, cfg = _case_cell(pkg, case), DC.make_cfg(capi, SC.pdcch_case(case))
    for bad in (capi.PdschCombCfg.make(si_window=62), capi.PdschCombCfg.make(si_window=-1)):
        with pytest.raises(Exception, match="si_window"):
            S.pdsch_comb(cell, tfg, case[3], 0x3FF, cfg, None, bad)
    bad = capi.PdschCombCfg.make()
    bad.no_sib1 = 2
    with pytest.raises(Exception, match="no_sib1"):
        S.pdsch_comb(cell, tfg, case[3], 0x3FF, cfg, None, bad)
    with pytest.raises(Exception, match="max_iter"):
        S.pdsch_comb(cell, tfg, case[3], 0x3FF, cfg, capi.PdschCfg.make(max_iter=17))


# ---------------------------------------------------------------- from samples
CAP_SHAPES = [(1, 6, 1, 2), (2, 15, 1, 2)]      # (R, n_rb, CP type, ports)


@functools.lru_cache(maxsize=None)
def sib1_capture(R, n_rb, cp, ports):
    """one cell, four frames from frame SFN0 in noise 10 dB below a resource element, with synth.sib1_schedule planted"""
    pkg = load_pkg()
    pdcch, pdsch, what = pkg.synth.sib1_schedule(pkg.synth.sib1_message(SC.SIB1), n_rb, SFN0)
    cell = dict(n_id_1=DC.CAP_ID[0], n_id_2=DC.CAP_ID[1], cp_normal=cp == 1, n_ports=ports, f_off=0.0, t0=DC.CAP_T0, sfn0=SFN0, n_rb_dl=n_rb,
                cfi=lambda frame, sf: 3, pdcch=pdcch, pdsch=pdsch)
    x, _, _ = pkg.synth.make_wideband_cell(90 + R + cp + ports, FC, R, [(FC, R, n_rb, cell)], snr_db=10.0, n_in=4 * 19200 * R)
    x.setflags(write=False)
    return x, (19200.0 - DC.CAP_T0) * R, what


@pytest.mark.parametrize("shape", CAP_SHAPES, ids=str)
def test_from_samples_the_planted_sib1_comes_back(pkg, S, H, shape):
    import torch
    capi = pkg.capi
    R, n_rb, cp, ports = shape
    x, frame_start, what = sib1_capture(*shape)
    d = torch.from_numpy(np.array(x)).cuda()
    cell = pkg.new_cell(n_id_1=DC.CAP_ID[0], n_id_2=DC.CAP_ID[1], cp_type=cp, n_ports=ports, freq_fine=0.0, frame_start=frame_start)
    cell.n_rb_dl, cell.phich_duration, cell.phich_resource = n_rb, 1, 3
    n_ofdm, mask = 52 * PR.n_symb_of(cp), 1 << 5
    got, comb, pdc = S.pdsch_comb_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm, mask, want_pdcch=True)
    tfg, _ = S.extract_tfg_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm)
    got2, comb2, pdc2 = S.pdsch_comb(cell, tfg, n_rb, mask, want_pdcch=True)
    assert bytes(got) == bytes(got2) and bytes(comb) == bytes(comb2) and bytes(pdc) == bytes(pdc2)
    alone, pdc_alone = S.pdsch_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm, mask, want_pdcch=True)
    assert bytes(alone) == bytes(got) and bytes(pdc_alone) == bytes(pdc)
    sc = dict(case=(DC.CAP_ID[1] + 3 * DC.CAP_ID[0], cp, ports, n_rb, 3, None), forced=False, si_window=0, sib1=True, grants=(tuple(sorted(dict(g=5).items())),))
    twin, twin_comb = CC.twin_records(H, capi, sc, tfg, pdc)
    assert bytes(comb) == bytes(twin_comb) and bytes(got) == bytes(twin)
    b = got.blocks()
    assert [(x["subframe"], x["rv"], x["kind"], x["tbs"]) for x in b] == [(5, capi.sib1_rv(SFN0 + 1), "si", what["tbs"]), (25, capi.sib1_rv(SFN0 + 3), "si", what["tbs"])]
    (g,) = comb.groups()
    assert g["members"] == [0, 1] and g["rule"] == 1 and g["rvs"] == [0, 2] and g["crc_ok"] and g["n_same"] == g["n_ok_members"]
    assert g["bytes"] == np.packbits(what["bits"]).tobytes() and capi.sib1_fields(g["bytes"]) == SC.SIB1
    print(shape, g["status"], g["n_ok_members"], [(x["status"], x["n_iter"]) for x in b])


# (R, n_rb, CP type, ports), the frame the capture starts in, mcs of the padded block, L: SIB1 on ONE resource block, padded to a block
# that holds more information bits than a transmission has coded bits (6 RB: tbs 208, K = 232; 15 RB: tbs 296, K = 320), in frames whose
# redundancy versions are 1 and 0 (frames 14 and 16): see test_pdsch_comb_ref.py::test_parity_only_transmission_is_a_false_ok for rv 2, 3
FAIL_SHAPES = [((1, 6, 1, 2), 13, 7), ((2, 15, 1, 2), 13, 9)]


@functools.lru_cache(maxsize=None)
def sib1_capture_members_fail(shape, sfn0, mcs):
    R, n_rb, cp, ports = shape
    pkg = load_pkg()
    pdcch, pdsch, what = pkg.synth.sib1_schedule(pkg.synth.sib1_message(SC.SIB1), n_rb, sfn0, n_prb=1, mcs=mcs)
    cell = dict(n_id_1=DC.CAP_ID[0], n_id_2=DC.CAP_ID[1], cp_normal=cp == 1, n_ports=ports, f_off=0.0, t0=DC.CAP_T0, sfn0=sfn0, n_rb_dl=n_rb,
                cfi=lambda frame, sf: 3, pdcch=pdcch, pdsch=pdsch)
    x, _, _ = pkg.synth.make_wideband_cell(70 + R + cp + ports, FC, R, [(FC, R, n_rb, cell)], snr_db=20.0, n_in=4 * 19200 * R)
    x.setflags(write=False)
    return x, (19200.0 - DC.CAP_T0) * R, what


@pytest.mark.parametrize("shape,sfn0,mcs", FAIL_SHAPES, ids=lambda v: str(v))
def test_from_samples_every_transmission_fails_and_the_sum_decodes(pkg, S, H, shape, sfn0, mcs):
    """the whole path from samples: wide extraction, soft bits, the summed circular buffer, the decode.  The conditions on the input are
    asserted on the numpy rule on the extracted grid: every member alone ends crc, the sum decodes, nothing near a tie"""
    import torch
    import pdcch_ref as DR
    import pdsch_comb_ref as CR
    import pdsch_ref as SR
    capi = pkg.capi
    R, n_rb, cp, ports = shape
    x, frame_start, what = sib1_capture_members_fail(shape, sfn0, mcs)
    d = torch.from_numpy(np.array(x)).cuda()
    cell = pkg.new_cell(n_id_1=DC.CAP_ID[0], n_id_2=DC.CAP_ID[1], cp_type=cp, n_ports=ports, freq_fine=0.0, frame_start=frame_start)
    cell.n_rb_dl, cell.phich_duration, cell.phich_resource = n_rb, 1, 3
    n_ofdm, mask = 52 * PR.n_symb_of(cp), 1 << 5
    n_id = DC.CAP_ID[1] + 3 * DC.CAP_ID[0]
    got, comb, pdc = S.pdsch_comb_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm, mask, want_pdcch=True)
    tfg, _ = S.extract_tfg_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm)
    # the numpy rule on that grid
    pdc_ref = DR.receive(tfg, n_id, cp, ports, n_rb, np.full(26, 3), 1, 3, capi.dci_common_sizes(n_rb), mask, 7, None)
    blocks = SR.receive(tfg, n_id, cp, ports, n_rb, pdc_ref, 0, False, mask, 1)
    ref = CR.combine(blocks)
    assert [(b["subframe"], b["rv"], b["status"], b["tbs"], b["n_prb"]) for b in blocks] == [(5, 1, 2, what["tbs"], 1), (25, 0, 2, what["tbs"], 1)]
    assert all(2 * b["n_re"] < b["K"] and b["margin"] > 1e-9 for b in blocks)
    (g,) = ref["groups"]
    assert g["status"] == CR.STATUS["ok"] and g["n_iter"] >= 1 and g["margin"] > 1e-9 and np.array_equal(g["payload"], SR.payload_bytes(what["bits"], 0, what["tbs"]))
    # the device: equal to numpy, byte-equal to the twin and to the call on the extracted grid
    assert SC.assert_blocks_against_numpy(got, blocks, str(shape)) == (2, 0)
    CC.assert_groups_against_numpy(comb, ref, str(shape))
    got2, comb2, pdc2 = S.pdsch_comb(cell, tfg, n_rb, mask, want_pdcch=True)
    assert bytes(got) == bytes(got2) and bytes(comb) == bytes(comb2) and bytes(pdc) == bytes(pdc2)
    sc = dict(case=(n_id, cp, ports, n_rb, 3, None), forced=False, si_window=0, sib1=True, grants=(tuple(sorted(dict(g=5).items())),))
    twin, twin_comb = CC.twin_records(H, capi, sc, tfg, pdc)
    assert bytes(comb) == bytes(twin_comb) and bytes(got) == bytes(twin)
    (dg,) = comb.groups()
    assert dg["status"] == "ok" and dg["n_ok_members"] == 0 and dg["rvs"] == [0, 1] and capi.sib1_fields(dg["bytes"]) == SC.SIB1
    print(shape, [(b["status"], b["n_iter"], b["n_re"]) for b in blocks], dg["status"], dg["n_iter"])


def test_measure_wideband_attaches_the_combined_record_and_sib1(pkg):
    import torch
    K, fc, n_rb, ports = 4, 1.8425e9, 15, 2
    n_id = DC.CAP_ID[1] + 3 * DC.CAP_ID[0]
    pdcch, pdsch, what = pkg.synth.sib1_schedule(pkg.synth.sib1_message(SC.SIB1), n_rb, 8)
    wide = dict(n_id_1=DC.CAP_ID[0], n_id_2=DC.CAP_ID[1], n_ports=ports, port_gains=[1.0, 0.7j], f_off=1200.0, t0=4321.0, sfn0=8, cfi=lambda fr, sf: 3, n_rb_dl=n_rb,
                pdcch=pdcch, pdsch=pdsch)
    x, _, _ = pkg.synth.make_wideband_cell(13, fc, K, [(fc, 2, n_rb, wide)], snr_db=20.0, n_in=153600 * K)
    d = torch.from_numpy(x).cuda()
    carriers = np.array([fc])
    with pkg.Searcher(0) as s:
        cells = pkg.sweep.search_wideband(s, d.data_ptr(), pkg.FMT_C64, x.size, FS * K, K, fc, carriers, np.array([-5e3, 0.0, 5e3]), n_out=153584, meas=True)
        big = [c for c in cells[0] if c["n_id_cell"] == n_id and c["n_rb_dl"] == n_rb]
        assert len(big) == 1, [(c["n_id_cell"], c["n_rb_dl"]) for c in cells[0]]
        both = pkg.sweep.measure_wideband(s, d.data_ptr(), pkg.FMT_C64, x.size, FS * K, fc, K, cells, carriers, dl_mask=1 << 5, pdsch_comb=True)
    rec, comb = big[0]["pdsch"], big[0]["pdsch_comb"]
    k = cells[0].index(big[0])
    assert both[0][k][1] is rec and both[0][k][2] is comb and isinstance(comb, pkg.capi.PdschCombInfo)
    groups = comb.groups()
    print("sweep:", [(b["subframe"], b["rv"], b["status"]) for b in rec.blocks()], [(g["members"], g["status"]) for g in groups])
    assert len(groups) >= 1 and all(g["rule"] == 1 and g["crc_ok"] and g["bytes"] == np.packbits(what["bits"]).tobytes() for g in groups)
    assert sum(len(g["members"]) for g in groups) == rec.n_blocks >= 2 and big[0]["sib1"] == SC.SIB1
