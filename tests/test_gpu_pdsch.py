"""GPU tests of the PDSCH stage (lcs_pdsch_wide, lcs_pdsch, lcs_turbo_decode; k_pdsch_plan, k_pdsch_llr, k_pdsch_dec, k_pdsch_fin).

The stage on the crafted grids of tests/pdsch_cases.py against the numpy statement of the rule (tests/pdsch_ref.py): soft bits to
1e-9 of the block's largest (the project's GPU bar), every other field equal; and the whole record byte-equal to the host twin
(tests/host/pdsch_host.cpp) fed with the device's own PDCCH record.  lcs_turbo_decode against the twin.  From samples: every planted
block comes back with its CRC, capi.sib1_fields reads the planted SIB1, lcs_pdsch_wide equals lcs_pdsch on lcs_extract_tfg_wide's
grid.  Forced grants, refusals, isolation, sweep.measure_wideband(pdsch=True)."""
import ctypes as C

import numpy as np
import pytest

import cell_meas_cases as CS
import pcfich_ref as PR
import pdcch_cases as DC
import pdsch_cases as SC
import pdsch_ref as SR
from conftest import load_pkg

pytestmark = pytest.mark.gpu
FS = 1.92e6
FC = DC.CAP_FC


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
    return SC.load_twin(pkg.capi)


_dev = {}


def dev(shape):
    import torch
    if shape not in _dev:
        _dev[shape] = torch.from_numpy(np.array(SC.pdsch_capture(*shape)[0])).cuda()
    return _dev[shape]


def _cell(pkg, shape):
    R, n_rb, cp, ports = shape
    c = pkg.new_cell(n_id_1=DC.CAP_ID[0], n_id_2=DC.CAP_ID[1], cp_type=cp, n_ports=ports, freq_fine=0.0, frame_start=SC.pdsch_capture(*shape)[1])
    c.n_rb_dl, c.phich_duration, c.phich_resource = n_rb, 1, 3
    return c


def _case_cell(pkg, case):
    return pkg.new_cell(n_id_1=case[0] // 3, n_id_2=case[0] % 3, cp_type=case[1], n_ports=case[2])


# ---------------------------------------------------------------- the stage on crafted grids
@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_stage_against_numpy_and_the_host_twin_on_crafted_grids(pkg, S, H, case):
    tfg, cfi, planted = SC.crafted(case)
    pc = SC.pdcch_case(case)
    n_rb, mask = case[3], DC.dl_mask_of(pc)
    cell, cfg = _case_cell(pkg, case), DC.make_cfg(pkg.capi, pc)
    got, pdc = S.pdsch(cell, tfg, n_rb, mask, cfg, want_pdcch=True)
    _, blocks = SC.reference(case)
    n, excused = SC.assert_blocks_against_numpy(got, blocks, SC.case_id(case))
    assert excused == 0
    worst, per_sf = 0.0, {}
    for b in blocks:
        u = per_sf.get(b["subframe"], 0)
        per_sf[b["subframe"]] = u + 1
        if "llr" in b:
            llr = S.pdsch_last_soft(b["subframe"], u, len(b["llr"]))
            rel = np.abs(llr - b["llr"]).max() / max(np.abs(b["llr"]).max(), 1e-300)      # (a silent grant: zeros on both sides)
            worst = max(worst, rel)
            assert rel <= 1e-9, (SC.case_id(case), b["subframe"], rel)
    twin = SC.twin_record(H, pkg.capi, case, tfg, pdc)
    assert bytes(got) == bytes(twin), (SC.case_id(case), np.flatnonzero(np.frombuffer(bytes(got), np.uint8) != np.frombuffer(bytes(twin), np.uint8))[:8])
    # the PDCCH record it read is the PDCCH stage's own on the same grid
    assert bytes(pdc) == bytes(S.pdcch(cell, tfg, n_rb, mask, cfg))
    print(SC.case_id(case), "%d blocks, %d ok, worst soft bit %.2e of the block's largest" % (n, got.n_ok, worst))


# ---------------------------------------------------------------- the decoder alone
@pytest.mark.parametrize("K,F,sigma", [(40, 0, 0.6), (64, 0, 0.9), (64, 8, 0.8), (2240, 0, 0.95), (2240, 40, 3.0)])
def test_turbo_decode_against_the_host_twin(pkg, S, H, K, F, sigma):
    """K = 40: two windows, one of 8 steps; 2240: seventy windows, two waves; decodes at once, after iterations and not at all"""
    synth = pkg.synth
    rng = np.random.default_rng(10 * K + F)
    iters = set()
    for trial in range(3):
        a = rng.integers(0, 2, K - F - 24).astype(np.uint8)
        c = np.concatenate([np.zeros(F, np.uint8), a, synth.crc24a(a)])
        d = (1 - 2.0 * synth.turbo_encode(c)) + sigma * rng.standard_normal((3, K + 4))
        d[:2, :F] = 0
        for max_iter in (0, 2):
            bits, n_iter, ok = S.turbo_decode(d, K, F, max_iter)
            tb, tn, ts = SC.twin_turbo(H, d, K, F, max_iter or 8)
            assert (n_iter, ok) == (tn, ts == 1) and np.array_equal(bits, tb), (K, F, trial, n_iter, ok, tn, ts)
            iters.add(n_iter)
            if ok:
                assert np.array_equal(bits, c)
    z = np.zeros((3, K + 4))
    assert S.turbo_decode(z, K, F)[1:] == (0, False)
    z[2, 1] = np.nan
    assert S.turbo_decode(z, K, F)[1:] == (0, False) and not S.turbo_decode(z, K, F)[0].any()
    print(K, F, "iterations seen", sorted(iters))


# ---------------------------------------------------------------- from samples
@pytest.mark.parametrize("shape", SC.CAP_SHAPES, ids=str)
def test_from_samples_every_planted_block_comes_back(pkg, S, shape):
    R, n_rb, cp, ports = shape
    n = PR.n_symb_of(cp)
    n_ofdm = 30 * n + 3
    d, cell = dev(shape), _cell(pkg, shape)
    got, pdc = S.pdsch_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm, want_pdcch=True)
    tfg, _ = S.extract_tfg_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm)
    again, pdc2 = S.pdsch(cell, tfg, n_rb, want_pdcch=True)
    assert bytes(got) == bytes(again) and bytes(pdc) == bytes(pdc2)
    assert bytes(pdc) == bytes(S.pdcch_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm))
    grants = SC.capture_grants(n_rb)
    by = {(b["subframe"], b["rnti"], b["rb_start"], b["n_prb"]): b for b in got.blocks()}
    n_planted = 0
    for g in range(15):
        if pdc.n_cce[g] < 4:
            continue
        for p in grants(1 + g // 10, g % 10):
            b = by[(g, p["rnti"], p["rb_start"], p["n_prb"])]
            n_planted += 1
            assert b["crc_ok"] and b["bytes"] == np.packbits(p["bits"]).tobytes() and b["rv"] == p["rv"] and b["mcs"] == p["mcs"], (shape, g, b["status"], b["n_iter"])
    assert n_planted >= 12 and got.n_ok >= n_planted
    sib = [b for b in got.blocks() if b["kind"] == "si" and b["crc_ok"]]
    assert len(sib) >= 1 and all(pkg.capi.sib1_fields(b["bytes"]) == SC.SIB1 for b in sib)
    # the grant of subframe 15 lies in a subframe that the grid cuts
    last = [b for b in got.blocks() if b["subframe"] == 15]
    assert all(b["status"] == "rows" for b in last) and (len(last) >= 1) == (n_rb > 10)
    print(shape, "planted %d, all back; %d blocks, %d ok, iterations %s" % (n_planted, got.n_blocks, got.n_ok, sorted({b["n_iter"] for b in got.blocks()})))
    # the mask picks subframes
    part = S.pdsch_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm, 0x021)
    assert {b["subframe"] for b in part.blocks()} <= {0, 5, 10, 15} and [b for b in part.blocks() if b["subframe"] == 5] == [b for b in got.blocks() if b["subframe"] == 5]


# ---------------------------------------------------------------- forced grants
def test_forced_grants_replace_the_pdcch_s(pkg, S, H):
    case = SC.CASES[3]
    n_id, cp, ports, n_rb, res, _ = case
    tfg, cfi, planted = SC.crafted(case)
    pc = SC.pdcch_case(case)
    cell, cfg = _case_cell(pkg, case), DC.make_cfg(pkg.capi, pc)
    p = next(p for p in planted if p["bits"] is not None and not p["silent"] and p["g"] == 1)
    forced = [(1, p["rnti"], p["rb_start"], p["n_prb"], p["tbs"], p["rv"]), (7, 0xFFFF, 2, 3, 100, 2), (12, 0xFFFF, 0, 2, 56, 0), (7, 61, 9, 2, 33, 1)]
    for it in (0, 3):
        ps = pkg.capi.PdschCfg.make(forced=forced, max_iter=it)
        got, pdc = S.pdsch(cell, tfg, n_rb, 0x3FF, cfg, ps, want_pdcch=True)
        twin = SC.twin_record(H, pkg.capi, case, tfg, pdc, cfg=SC.make_cfg(pkg.capi, forced=forced, max_iter=it or 8))
        assert bytes(got) == bytes(twin)
    b = got.blocks()
    assert [x["subframe"] for x in b] == [1, 7, 7, 12] and b[0]["crc_ok"] and b[0]["bytes"] == np.packbits(p["bits"]).tobytes()
    assert (b[1]["K"], b[1]["F"]) == (128, 4) and b[3]["status"] == "rows" and max(x["n_iter"] for x in b) <= 3
    # the tables of other forced sizes replace these, and these come back
    other = S.pdsch(cell, tfg, n_rb, 0x3FF, cfg, pkg.capi.PdschCfg.make(forced=[(1, p["rnti"], p["rb_start"], p["n_prb"], p["tbs"] + 8, p["rv"])]))
    assert other.n_blocks == 1 and not other.blocks()[0]["crc_ok"]
    assert bytes(S.pdsch(cell, tfg, n_rb, 0x3FF, cfg, ps)) == bytes(got)
    # rnti_mask: SI alone
    plain = S.pdsch(cell, tfg, n_rb, 0x3FF, cfg)
    si = S.pdsch(cell, tfg, n_rb, 0x3FF, cfg, pkg.capi.PdschCfg.make(rnti_mask=1))
    assert si.n_blocks == si.n_si == plain.n_si > 0 and plain.n_paging + plain.n_ra > 0


# ---------------------------------------------------------------- refusals
def test_refusals_launch_nothing_and_leave_the_context_usable(pkg, S):
    shape = SC.CAP_SHAPES[1]
    R, n_rb, cp, ports = shape
    d, cell = dev(shape), _cell(pkg, shape)
    mk, pm = pkg.capi.PdcchCfg.make, pkg.capi.PdschCfg.make
    args = (cell, d, FC, FC, FS * R, 256, 15, 213, 0x3FF)
    before = S.pdsch_wide(*args, mk((22, 10)))
    assert before.n_ok > 0
    nf = pm()
    nf.n_forced = 5
    cases = [(mk((22, 10)), pm(max_iter=17), "max_iter is outside"), (mk((22, 10)), pm(max_iter=-1), "max_iter is outside"),
             (mk((22, 10)), pm(i_1a=2), "i_1a is outside"), (mk((22,)), pm(i_1a=1), "i_1a is outside"), (mk((22, 10)), pm(rnti_mask=8), "rnti_mask is outside"),
             (mk((22, 10)), nf, "n_forced is outside"),
             (mk((22, 10)), pm(forced=[(0, 0xFFFF, 14, 2, 56, 0)]), "outside the grid's resource blocks"), (mk((22, 10)), pm(forced=[(0, 0xFFFF, 0, 16, 56, 0)]), "outside the grid's resource blocks"),
             (mk((22, 10)), pm(forced=[(0, 0xFFFF, -1, 2, 56, 0)]), "outside the grid's resource blocks"), (mk((22, 10)), pm(forced=[(16, 0xFFFF, 0, 2, 56, 0)]), "outside the grid's subframes"),
             (mk((22, 10)), pm(forced=[(0, 0, 0, 2, 56, 0)]), "rnti is outside"), (mk((22, 10)), pm(forced=[(0, 1, 0, 2, 56, 4)]), "rv is outside"),
             (mk((22, 10)), pm(forced=[(0, 1, 0, 2, 2217, 0)]), "tbs is outside"), (mk((22, 10)), pm(forced=[(3, 1, 0, 2, 56, 0)] * 3), "more than two forced grants"),
             (mk((22, 49)), pm(), "payload size is outside"), (mk((22, 10), cfi_force=4), pm(), "cfi_force is outside")]
    for cfg, ps, text in cases:
        with pytest.raises(pkg.SearcherError, match=text):
            S.pdsch_wide(*args, cfg, ps)
    grid = np.ones((213, 180), np.complex128)
    with pytest.raises(pkg.SearcherError, match="max_iter is outside"):
        S.pdsch(cell, grid, 15, 0x3FF, mk((22, 10)), pm(max_iter=99))
    with pytest.raises(pkg.SearcherError, match="n_ofdm is outside"):
        S.pdsch(cell, grid[:11], 15, 0x3FF, mk((22, 10)))
    for K, F, it, text in ((41, 0, 8, "not one of the 127"), (2304, 0, 8, "not one of the 127"), (40, 40, 8, "F is outside"), (40, -1, 8, "F is outside"), (40, 0, 17, "max_iter is outside")):
        with pytest.raises(pkg.SearcherError, match=text):
            S.turbo_decode(np.ones((3, K + 4)), K, F, it)
    lib, rec, cfg = S._lib, pkg.PdschInfo(), mk((22, 10))
    assert lib.lcs_pdsch_wide(S._h, C.byref(cell), C.c_void_p(d.data_ptr()), d.numel(), FC, FC, FS * R, 256, 15, 213, 0x3FF, C.byref(cfg), None, None, None) == -2
    assert b"null pointer" in lib.lcs_last_error(S._h)
    assert lib.lcs_pdsch_wide(S._h, C.byref(cell), C.c_void_p(d.data_ptr()), d.numel(), FC, FC, FS * R, 256, 15, 213, 0x3FF, None, None, C.byref(rec), None) == -2
    assert lib.lcs_turbo_decode(S._h, None, 40, 0, 8, None, None, None) == -2
    with pytest.raises(pkg.SearcherError, match="no such grant slot"):
        S.pdsch_last_soft(16, 0, 10)
    with pytest.raises(pkg.SearcherError, match="was not followed"):
        S.pdsch_last_soft(0, 1, 10)                     # (one grant per subframe in this capture: slot 1 is empty)
    with pytest.raises(pkg.SearcherError, match="was not followed"):
        S.pdsch_last_soft(15, 0, 10)                    # (listed with status rows)
    with pytest.raises(pkg.SearcherError, match="was not followed"):
        S.pdsch_last_soft(0, 0, 2 * before.block[0].n_re + 1)
    assert S.pdsch_last_soft(0, 0, 2 * before.block[0].n_re).size == 2 * before.block[0].n_re and before.block[0].subframe == 0
    S.turbo_decode(np.ones((3, 44)), 40)
    with pytest.raises(pkg.SearcherError, match="no such grant slot"):
        S.pdsch_last_soft(0, 0, 10)
    assert bytes(S.pdsch_wide(*args, mk((22, 10)))) == bytes(before)


# ---------------------------------------------------------------- the chain, the measurement, the PCFICH and the PDCCH are left alone
def test_the_chain_and_the_other_stages_are_left_alone(pkg):
    shape = SC.CAP_SHAPES[1]
    R, n_rb, cp, ports = shape
    d, cell = dev(shape), _cell(pkg, shape)
    args = (cell, d, FC, FC, FS * R, 128 * R, n_rb, 30 * PR.n_symb_of(cp) + 3, 0x339)
    batch = lambda s: s.search_capbuf(CS.cap(1), CS.GRID, CS.FC, CS.FC, FS)[0]
    with pkg.Searcher(0) as s:              # a context that never calls the stage
        want_cells = [bytes(c) for c in batch(s)]
        want_pcfich = bytes(s.pcfich_wide(*args))
        want_pdcch = bytes(s.pdcch_wide(*args))
        want_meas = bytes(s.cell_meas_wide(*args))
        forced3 = bytes(s.pdcch_wide(*args, pkg.capi.PdcchCfg.make(pkg.capi.dci_common_sizes(n_rb), cfi_force=3)))
        want_next = [bytes(c) for c in batch(s)]
    with pkg.Searcher(0) as s:
        plain, pdc = s.pdsch_wide(*args, want_pdcch=True)
        assert plain.n_ok > 0 and bytes(pdc) == want_pdcch
        assert [bytes(c) for c in batch(s)] == want_cells
        assert bytes(s.pdsch_wide(*args)) == bytes(plain)
        # the PDCCH stage's own record and tables beside it: another configuration there changes nothing here, and the reverse
        assert bytes(s.pdcch_wide(*args, pkg.capi.PdcchCfg.make(pkg.capi.dci_common_sizes(n_rb), cfi_force=3))) == forced3
        assert bytes(s.pdsch_wide(*args)) == bytes(plain)
        assert bytes(s.pdcch_wide(*args)) == want_pdcch and bytes(s.pcfich_wide(*args)) == want_pcfich and bytes(s.cell_meas_wide(*args)) == want_meas
        bits, n_iter, ok = s.turbo_decode(np.random.default_rng(1).standard_normal((3, 44)), 40)
        assert n_iter == 8 and not ok
        assert bytes(s.pdsch_wide(*args)) == bytes(plain)
        assert [bytes(c) for c in batch(s)] == want_next
    with pkg.Searcher(0) as s:
        s.stream_open(pkg.FMT_IQ_U8, 153600, CS.FC, CS.FC, FS)
        assert bytes(s.pdsch_wide(*args)) == bytes(plain)
        s.stream_close()
        assert bytes(s.pdsch_wide(*args)) == bytes(plain)


# ---------------------------------------------------------------- the sweep
def test_measure_wideband_gives_the_direct_call_s_record(pkg):
    import torch
    K, fc, n_rb, ports = 4, 1.8425e9, 15, 2
    grants = SC.capture_grants(n_rb)
    n_id = DC.CAP_ID[1] + 3 * DC.CAP_ID[0]
    have = lambda fr, sf: pkg.synth.pdcch_layout(n_id, n_rb, ports, True, DC.capture_cfi(fr, sf))[1] >= 4
    wide = dict(n_id_1=DC.CAP_ID[0], n_id_2=DC.CAP_ID[1], n_ports=ports, port_gains=[1.0, 0.7j], f_off=1200.0, t0=4321.0, sfn0=8, cfi=DC.capture_cfi, n_rb_dl=n_rb,
                pdcch=lambda fr, sf: [dict(rnti=g["rnti"], bits=SC.pack_1a(g, n_rb, False), L=4, cce=0) for g in grants(fr, sf)] if have(fr, sf) else [],
                pdsch=lambda fr, sf: grants(fr, sf) if have(fr, sf) else [])
    x, _, _ = pkg.synth.make_wideband_cell(13, fc, K, [(fc, 2, n_rb, wide)], snr_db=20.0, n_in=153600 * K)
    d = torch.from_numpy(x).cuda()
    carriers = np.array([fc])
    with pkg.Searcher(0) as s:
        cells = pkg.sweep.search_wideband(s, d.data_ptr(), pkg.FMT_C64, x.size, FS * K, K, fc, carriers, np.array([-5e3, 0.0, 5e3]), n_out=153584, meas=True)
        big = [c for c in cells[0] if c["n_id_cell"] == n_id and c["n_rb_dl"] == n_rb]
        assert len(big) == 1, [(c["n_id_cell"], c["n_rb_dl"]) for c in cells[0]]
        calls = []
        real = s.pdsch_wide
        s.pdsch_wide = lambda *a, **k: (calls.append(real(*a, **k)), calls[-1])[1]
        both = pkg.sweep.measure_wideband(s, d.data_ptr(), pkg.FMT_C64, x.size, FS * K, fc, K, cells, carriers, pdsch=True)
        del s.pdsch_wide
        rec = big[0]["pdsch"]
        k = cells[0].index(big[0])
        assert both[0][k][1] is rec and isinstance(both[0][k][0], pkg.CellMeasWide) and any(c is rec for c in calls)
    ok = [b for b in rec.blocks() if b["crc_ok"]]
    print("sweep: %d blocks, %d ok, kinds %s" % (rec.n_blocks, len(ok), sorted({b["kind"] for b in ok})))
    assert rec.n_blocks == 32 and rec.n_overflow > 0 and len(ok) >= 28 and {"si", "paging", "ra"} <= {b["kind"] for b in ok}      # (the record holds 32)
    sib = [b for b in ok if b["kind"] == "si"]
    assert len(sib) >= 2 and all(pkg.capi.sib1_fields(b["bytes"]) == SC.SIB1 for b in sib)
