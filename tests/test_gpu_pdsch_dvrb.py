"""GPU tests of distributed allocations and format 1C in the PDSCH stage (lcs_set_pdsch_alloc, lcs_pdsch_last_alloc; k_pdsch_plan's 1C
parse and VRB to PRB map, k_pdsch_llr_set's enumeration over sets).

On the crafted grids of tests/pdsch_dvrb_cases.py: the record against the numpy statement of the rule (tests/pdsch_dvrb_ref.py), soft
bits to 1e-9 of the block's largest (the project's GPU bar), the record byte-equal to the host twin (tests/host/pdsch_dvrb_host.cpp)
fed with the device's own PDCCH record, lcs_pdsch_last_alloc equal to the twin's.  With the setting zero the stage's own nine grids give
the stage's twin's record.  From samples: SIB1 scheduled by format 1C and paging by distributed 1A come back with the setting on and
do not with it off.  Combining: a SIB1 sent twice with distributed allocations, each alone crc, the sum ok."""
import ctypes as C
import functools

import numpy as np
import pytest

import pcfich_ref as PR
import pdcch_cases as DC
import pdsch_cases as SC
import pdsch_comb_cases as CC
import pdsch_dvrb_cases as VC
from conftest import load_pkg

pytestmark = pytest.mark.gpu
FS = 1.92e6
FC = DC.CAP_FC


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def S_mod(pkg):
    with pkg.Searcher(0) as s:
        yield s


@pytest.fixture()
def S(S_mod):
    S_mod.set_pdsch_alloc(None)           # every test starts from the stage without the setting
    return S_mod


@pytest.fixture(scope="module")
def H(pkg):
    return VC.load_twin(pkg.capi)


def _case_cell(pkg, case):
    return pkg.new_cell(n_id_1=case[0] // 3, n_id_2=case[0] % 3, cp_type=case[1], n_ports=case[2])


# ---------------------------------------------------------------- from samples
CAP_SFN0 = 9            # the cell's frame 0; the grid starts at its frame 1, an even frame: SIB1 is in grid subframe 5


def capture_grants(n_rb):
    """(frame, subframe) -> the grant of that subframe: SIB1 by format 1C over every VRB in subframe 5 of an even frame (rv by the frame),
    a paging block by a distributed format 1A grant of three VRBs in the others"""
    pkg = load_pkg()
    sib = pkg.synth.sib1_message(SC.SIB1)
    nv = pkg.capi.dvrb_sizes(n_rb, 0)["n_vrb"]

    def grants(frame, sf):
        if sf == 5 and (CAP_SFN0 + frame) % 2 == 0:
            i = next(i for i in range(32) if pkg.capi.tbs_1c(i) >= len(sib))
            bits = np.concatenate([sib, np.zeros(pkg.capi.tbs_1c(i) - len(sib), np.uint8)])
            return [dict(format="1c", rnti=0xFFFF, rb_start=0, n_prb=nv, i_tbs=i, rv=pkg.capi.sib1_rv(CAP_SFN0 + frame), bits=bits)]
        mcs, tpc = (sf + frame) % 6, sf & 1
        bits = np.random.default_rng(1000 * frame + sf).integers(0, 2, pkg.capi.tbs_1a(mcs, tpc)).astype(np.uint8)
        return [dict(format="1a", distributed=1, rnti=0xFFFE, rb_start=(2 * sf + frame) % (nv - 2), n_prb=3, mcs=mcs, tpc=tpc, rv=sf % 4, bits=bits)]
    return grants


@functools.lru_cache(maxsize=None)
def capture(R, n_rb, cp, ports):
    """synth.make_wideband_cell as tests/pdsch_cases.py's pdsch_capture, with capture_grants planted: noise 10 dB below a resource element"""
    pkg = load_pkg()
    grants = capture_grants(n_rb)
    n_id = DC.CAP_ID[1] + 3 * DC.CAP_ID[0]
    have = lambda fr, sf: pkg.synth.pdcch_layout(n_id, n_rb, ports, cp == 1, DC.capture_cfi(fr, sf))[1] >= 4
    payload = lambda g: pkg.synth.dci_1c_payload(g, n_rb) if g["format"] == "1c" else pkg.synth.dci_1a_payload(g, n_rb)
    cell = dict(n_id_1=DC.CAP_ID[0], n_id_2=DC.CAP_ID[1], cp_normal=cp == 1, n_ports=ports, f_off=0.0, t0=DC.CAP_T0, sfn0=CAP_SFN0, n_rb_dl=n_rb, cfi=DC.capture_cfi,
                pdcch=lambda fr, sf: [dict(rnti=g["rnti"], bits=payload(g), L=4, cce=0) for g in grants(fr, sf)] if have(fr, sf) else [],
                pdsch=lambda fr, sf: grants(fr, sf) if have(fr, sf) else [])
    x, _, _ = pkg.synth.make_wideband_cell(70 + R + cp + ports, DC.CAP_FC, R, [(DC.CAP_FC, R, n_rb, cell)], snr_db=10.0, n_in=3 * 19200 * R)
    x.setflags(write=False)
    return x, (19200.0 - DC.CAP_T0) * R


@pytest.mark.parametrize("shape", SC.CAP_SHAPES, ids=str)
def test_from_samples_sib1_by_1c_and_paging_by_distributed_1a(pkg, S, shape):
    """the test that fails without the feature: with the setting off the same samples give `distributed` and no SI block"""
    import torch
    R, n_rb, cp, ports = shape
    n = PR.n_symb_of(cp)
    n_ofdm = 30 * n + 3
    x, frame_start = capture(*shape)
    d = torch.from_numpy(np.array(x)).cuda()
    cell = pkg.new_cell(n_id_1=DC.CAP_ID[0], n_id_2=DC.CAP_ID[1], cp_type=cp, n_ports=ports, freq_fine=0.0, frame_start=frame_start)
    cell.n_rb_dl, cell.phich_duration, cell.phich_resource = n_rb, 1, 3
    off, pdc = S.pdsch_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm, want_pdcch=True)
    planted_off = {(b["subframe"], b["rnti"]): b for b in off.blocks()}
    assert not any(b["kind"] == "si" and b["crc_ok"] for b in off.blocks())
    assert all(planted_off[(g, 0xFFFE)]["status"] == "distributed" for g in range(15) if g != 5 and pdc.n_cce[g] >= 4)
    S.set_pdsch_alloc(pkg.capi.PdschAllocCfg.make(True, True, sfn0=CAP_SFN0 + 1))
    got = S.pdsch_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm)
    tfg, _ = S.extract_tfg_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm)
    assert bytes(got) == bytes(S.pdsch(cell, tfg, n_rb))
    grants = capture_grants(n_rb)
    by = {(b["subframe"], b["rnti"]): b for b in got.blocks()}
    n_planted, kinds = 0, set()
    for g in range(15):
        if pdc.n_cce[g] < 4:
            continue
        for p in grants(1 + g // 10, g % 10):
            b = by[(g, p["rnti"])]
            n_planted += 1
            kinds.add(b["kind"])
            assert b["status"] == "ok" and b["bytes"] == np.packbits(p["bits"]).tobytes() and b["rv"] == p["rv"] and (b["rb_start"], b["n_prb"]) == (p["rb_start"], p["n_prb"]), \
                (shape, g, b["status"], b["n_iter"])
            assert b["mcs"] == (p["i_tbs"] if p["format"] == "1c" else p["mcs"])
    assert n_planted >= 12 and kinds == {"si", "paging"}
    sib = [b for b in got.blocks() if b["kind"] == "si" and b["crc_ok"]]
    assert len(sib) >= 1 and sib[0]["subframe"] == 5 and all(pkg.capi.sib1_fields(b["bytes"]) == SC.SIB1 for b in sib)
    a = S.pdsch_last_alloc(got.blocks().index(sib[0]))
    assert (a["format"], a["distributed"], a["n_step"], a["n_prb"]) == ("1c", 1, 2, sib[0]["n_prb"])
    S.set_pdsch_alloc(None)
    assert bytes(S.pdsch_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm)) == bytes(off)


# ---------------------------------------------------------------- combining
def test_combining_takes_distributed_blocks_as_members(pkg, S, H):
    """a SIB1 sent twice with distributed allocations: each alone crc, the sum ok; the combined record is the comb twin's on the same blocks"""
    case = VC.CASES[1]
    tfg, _, planted = VC.crafted(case, plan="comb")
    pc = VC.pdcch_case(case)
    cell, cfg = _case_cell(pkg, case), DC.make_cfg(pkg.capi, pc)
    S.set_pdsch_alloc(pkg.capi.PdschAllocCfg.make(True, False))
    got, comb, pdc = S.pdsch_comb(cell, tfg, case[3], 0x020, cfg, want_pdcch=True)
    twin, _, llr = VC.twin_record(H, pkg.capi, case, tfg, pdc, (1, -1, 0), want_soft=True, mask=0x020)
    assert bytes(got) == bytes(twin)
    idx = [i for i, b in enumerate(got.blocks()) if b["rnti"] == 0xFFFF and b["subframe"] in (5, 25)]
    assert [(got.blocks()[i]["subframe"], got.blocks()[i]["status"]) for i in idx] == [(5, "crc"), (25, "crc")]
    assert all(S.pdsch_last_alloc(i)["distributed"] == 1 for i in idx)
    want = pkg.capi.PdschCombInfo()
    cc = pkg.capi.PdschCombCfg.make()
    CC.load_twin(pkg.capi).pdsch_comb_host_groups(C.byref(twin), SC._dp(llr), llr.shape[1], 8, C.byref(cc), None, C.byref(want))
    assert bytes(comb) == bytes(want)
    g = [x for x in comb.groups() if x["members"] == idx]
    assert len(g) == 1 and g[0]["status"] == "ok" and g[0]["bytes"] == np.packbits(planted[0]["bits"]).tobytes()


# ---------------------------------------------------------------- the stage on crafted grids
@pytest.mark.parametrize("setting", sorted(VC.SETTINGS))
@pytest.mark.parametrize("case", VC.CASES, ids=VC.case_id)
def test_stage_against_numpy_and_the_host_twin_on_crafted_grids(pkg, S, H, case, setting):
    tfg, cfi, planted = VC.crafted(case)
    pc = VC.pdcch_case(case)
    n_rb, mask = case[3], DC.dl_mask_of(pc)
    cell, cfg = _case_cell(pkg, case), DC.make_cfg(pkg.capi, pc)
    S.set_pdsch_alloc(VC.alloc_cfg(pkg.capi, setting))
    got, pdc = S.pdsch(cell, tfg, n_rb, mask, cfg, want_pdcch=True)
    blocks = VC.reference(case, setting)
    n, excused = SC.assert_blocks_against_numpy(got, blocks, VC.case_id(case))
    assert excused == 0 and n >= len(planted)         # (beyond the planted: a noise candidate whose CRC lands on a followed RNTI, as numpy finds it too)
    worst = 0.0
    for i, (b, slot) in enumerate(zip(blocks, VC.slots_of(blocks))):
        assert S.pdsch_last_alloc(i) == b["alloc"], (VC.case_id(case), i)
        if "llr" in b:
            llr = S.pdsch_last_soft(slot // 2, slot % 2, len(b["llr"]))
            rel = np.abs(llr - b["llr"]).max() / np.abs(b["llr"]).max()
            worst = max(worst, rel)
            assert rel <= 1e-9, (VC.case_id(case), b["subframe"], rel)
    twin, allocs = VC.twin_record(H, pkg.capi, case, tfg, pdc, setting)
    assert bytes(got) == bytes(twin), (VC.case_id(case), np.flatnonzero(np.frombuffer(bytes(got), np.uint8) != np.frombuffer(bytes(twin), np.uint8))[:8])
    assert [S.pdsch_last_alloc(i) for i in range(got.n_blocks)] == allocs
    with pytest.raises(pkg.SearcherError, match="no such block"):
        S.pdsch_last_alloc(got.n_blocks)
    print(VC.case_id(case), setting, "%d blocks, %d ok, worst soft bit %.2e of the block's largest" % (n, got.n_ok, worst))


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_setting_zero_gives_the_stage_s_own_record(pkg, S, case):
    """never set, set and taken back, and flags 0 with the other fields set: the stage's twin's record on its own nine grids"""
    H0 = SC.load_twin(pkg.capi)
    tfg, _, _ = SC.crafted(case)
    pc = SC.pdcch_case(case)
    n_rb, mask = case[3], DC.dl_mask_of(pc)
    cell, cfg = _case_cell(pkg, case), DC.make_cfg(pkg.capi, pc)
    got, pdc = S.pdsch(cell, tfg, n_rb, mask, cfg, want_pdcch=True)
    want = SC.twin_record(H0, pkg.capi, case, tfg, pdc)
    assert bytes(got) == bytes(want)
    S.set_pdsch_alloc(pkg.capi.PdschAllocCfg.make(True, True, 6, 10))
    on = S.pdsch(cell, tfg, n_rb, mask, cfg)
    S.set_pdsch_alloc(None)
    assert bytes(S.pdsch(cell, tfg, n_rb, mask, cfg)) == bytes(want)
    S.set_pdsch_alloc(pkg.capi.PdschAllocCfg.make(False, False, 6, 10))
    assert bytes(S.pdsch(cell, tfg, n_rb, mask, cfg)) == bytes(want)
    if any(b["status"] == "distributed" for b in want.blocks()):
        assert bytes(on) != bytes(want) and not any(b["status"] == "distributed" for b in on.blocks())


# ---------------------------------------------------------------- refusals
def test_refusals(pkg):
    case = VC.CASES[0]
    tfg, _, _ = VC.crafted(case)
    cell = _case_cell(pkg, case)
    with pkg.Searcher(0) as S:
        _refusals(pkg, S, tfg, cell)


def _refusals(pkg, S, tfg, cell):
    bad = pkg.capi.PdschAllocCfg.make(True, True)
    for field, value, text in (("flags", 4, "flags is outside"), ("flags", -1, "flags is outside"), ("sfn0", 1024, "sfn0 is outside"), ("sfn0", -2, "sfn0 is outside"),
                               ("si_window", 62, "si_window is outside"), ("reserved", 1, "reserved")):
        cfg = pkg.capi.PdschAllocCfg.make(True, True)
        setattr(cfg, field, value)
        with pytest.raises(pkg.SearcherError, match=text):
            S.set_pdsch_alloc(cfg)
    with pytest.raises(pkg.SearcherError, match="no such block"):
        S.pdsch_last_alloc(0)
    S.set_pdsch_alloc(bad)
    one = pkg.capi.PdcchCfg.make((pkg.capi.dci_common_sizes(6)[0],), phich_duration=1, phich_resource=1)
    with pytest.raises(pkg.SearcherError, match="format 1C is followed"):
        S.pdsch(cell, tfg, 6, 0x3FF, one)
    wrong = pkg.capi.PdcchCfg.make((pkg.capi.dci_common_sizes(6)[0], pkg.capi.dci_common_sizes(6)[1] + 1), phich_duration=1, phich_resource=1)
    with pytest.raises(pkg.SearcherError, match="other size is not format 1C's"):
        S.pdsch(cell, tfg, 6, 0x3FF, wrong)
    S.set_pdsch_alloc(pkg.capi.PdschAllocCfg.make(True, False))
    assert S.pdsch(cell, tfg, 6, 0x3FF, one).n_blocks > 0 and S.pdsch(cell, tfg, 6, 0x3FF, wrong).n_blocks > 0
    assert S.pdsch_alloc.flags == 1
    assert S._lib.lcs_pdsch_last_alloc(S._h, 0, None) == -2
