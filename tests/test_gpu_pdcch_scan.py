"""GPU tests of the blind search of every CCE (lcs_pdcch_scan_wide, lcs_pdcch_scan, lcs_pdcch_scan_decodes; k_pscan_llr, k_pscan_dec,
k_pscan_acc, k_pscan_fin).

The decoder is integer arithmetic and the soft bits are the host twin's fp64 sums in the same order, so the bar is equality: on
every crafted grid of tests/pdcch_scan_cases.py the record and the decode table of every subframe are byte-equal to the host twin
(tests/host/pdcch_scan_host.cpp, which tests/test_pdcch_scan_host.py holds to the numpy rule), and the CFI used is S.pcfich's.
cfi_force, silence and values that are not finite; from samples; refusals; isolation; sweep.measure_wideband(pdcch_scan=...)."""
import ctypes as C

import numpy as np
import pytest

import pcfich_ref as PR
import pdcch_cases as DC
import pdcch_scan_cases as SC
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


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch.from_numpy(np.array(SC.scan_capture()[0])).cuda()


def _cap_cell(pkg):
    R, n_rb, cp, ports = SC.CAP_SHAPE
    c = pkg.new_cell(n_id_1=DC.CAP_ID[0], n_id_2=DC.CAP_ID[1], cp_type=cp, n_ports=ports, freq_fine=0.0, frame_start=SC.scan_capture()[1])
    c.n_rb_dl, c.phich_duration, c.phich_resource = n_rb, 1, 3
    return c


def _case_cell(pkg, case):
    return pkg.new_cell(n_id_1=case[0] // 3, n_id_2=case[0] % 3, cp_type=case[1], n_ports=case[2])


def _tables_equal(S, twin_tab, rec, what):
    for g in range(rec.n_sf):
        got = S.pdcch_scan_decodes(g)
        want = SC.table_of(twin_tab, g, rec.sf[g].n_cand, len(rec.sizes))
        assert len(got) == len(want) == rec.sf[g].n_cand * len(rec.sizes), (what, g)
        assert b"".join(bytes(d) for d in got) == b"".join(bytes(d) for d in want), (what, g)


# ---------------------------------------------------------------- the stage on crafted grids
@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_record_and_every_decode_table_equal_the_host_twin_on_crafted_grids(pkg, S, H, case):
    tfg, cfi, planted = SC.crafted(case)
    n_rb, mask = case[3], SC.dl_mask_of(case)
    cell, cfg = _case_cell(pkg, case), SC.make_cfg(pkg.capi, case)
    got = S.pdcch_scan(cell, tfg, n_rb, mask, cfg)
    pc = S.pcfich(cell, tfg, n_rb, mask)
    read = got.cfi > 0
    assert np.array_equal(got.cfi[read], pc.cfi[read]) and np.array_equal(pc.cfi[read], cfi[read]) and read.sum() >= 4
    twin, tab, _ = SC.twin_record(H, pkg.capi, case, tfg, pc.cfi)
    assert bytes(got) == bytes(twin), (SC.case_id(case), np.flatnonzero(np.frombuffer(bytes(got), np.uint8) != np.frombuffer(bytes(twin), np.uint8))[:8])
    _tables_equal(S, tab, got, SC.case_id(case))
    want = {(p["g"], p["L"], p["cce"], p["i"], p["bits"], p["rnti"]) for p in planted if p["kind"] in ("a", "b", "common")}
    assert want <= {(m["subframe"], m["L"], m["cce"], m["size_index"], m["bits"], m["rnti"]) for m in got.listed() if m["flags"] & 2}
    print(SC.case_id(case), "n_cce", list(got.n_cce), "listed %d, accepted %d, UE %d, RNTIs %d" % (got.n_msg, got.n_accepted, got.n_ue, got.n_rnti))


def test_cfi_force_and_grids_without_a_signal(pkg, S, H):
    case = SC.CASES[4]                                        # 25 RB, 2 ports, CFI 3, 2, 3, 3, 3, 1
    tfg, cfi, planted = SC.crafted(case)
    cell = _case_cell(pkg, case)
    key = lambda m: (m["L"], m["cce"], m["size_index"], m["bits"], m["rnti"])
    for force in (1, 2, 3):
        cfg = SC.make_cfg(pkg.capi, case, cfi_force=force)
        rec = S.pdcch_scan(cell, tfg, 25, 0x3FF, cfg)
        twin, tab, _ = SC.twin_record(H, pkg.capi, case, tfg, cfi, cfg=cfg)
        assert (rec.cfi == force).all() and bytes(rec) == bytes(twin)
        _tables_equal(S, tab, rec, force)
        for g in range(SC.N_SF):
            want = {key(dict(p, size_index=p["i"])) for p in planted if p["g"] == g and p["kind"] != "out"}
            found = {key(m) for m in rec.listed() if m["subframe"] == g}
            assert want <= found if cfi[g] == force else not (want & found), (force, g)      # a wrong CFI finds nothing of what was planted
    cfg = SC.make_cfg(pkg.capi, case, cfi_force=3)
    zero = np.zeros((42, 300), np.complex128)
    for grid in (zero, np.full((42, 300), np.nan + 0j)):
        rec = S.pdcch_scan(cell, grid, 25, 0x3FF, cfg)
        twin, tab, _ = SC.twin_record(H, pkg.capi, case, grid, np.zeros(3, np.int32), cfg=cfg)
        assert bytes(rec) == bytes(twin) and rec.n_accepted == 0 and rec.n_msg == 0 and rec.n_read == 3
        _tables_equal(S, tab, rec, "no signal")
        flags = {d.flags for g in range(3) for d in S.pdcch_scan_decodes(g)}
        assert flags == ({1} if grid is zero else {0})         # silent: decoded, all zero; values that are not finite: zero entries
        assert all((d.bits, d.rnti_x, d.n_obs, d.quality) == (0, 0, 0, 0.0) for d in S.pdcch_scan_decodes(0))

# ---------------------------------------------------------------- from samples
def test_from_samples_equals_the_stage_on_the_extracted_grid_and_lists_what_was_planted(pkg, S, dev):
    R, n_rb, cp, ports = SC.CAP_SHAPE
    n_ofdm = 2 * SC.CAP_N_SF * PR.n_symb_of(cp)
    cell = _cap_cell(pkg)
    cfg = pkg.capi.PdcchScanCfg.make(SC.cap_sizes())
    got = S.pdcch_scan_wide(cell, dev, FC, FC, FS * R, 128 * R, n_rb, n_ofdm, 0x3FF, cfg)
    tables = [b"".join(bytes(d) for d in S.pdcch_scan_decodes(g)) for g in range(got.n_sf)]
    tfg, _ = S.extract_tfg_wide(cell, dev, FC, FC, FS * R, 128 * R, n_rb, n_ofdm)
    again = S.pdcch_scan(cell, tfg, n_rb, 0x3FF, cfg)
    assert bytes(got) == bytes(again) and got.sizes == SC.cap_sizes()
    assert tables == [b"".join(bytes(d) for d in S.pdcch_scan_decodes(g)) for g in range(got.n_sf)]
    assert got.n_sf == got.n_read == SC.CAP_N_SF and list(got.cfi) == [DC.capture_cfi(1 + g // 10, g % 10) for g in range(SC.CAP_N_SF)]
    msgs = {(m["subframe"], m["L"], m["cce"], m["size_index"], m["bits"], m["rnti"]): m for m in got.listed()}
    planted = SC.cap_planted()
    for p in planted:
        m = msgs.get((p["g"], p["L"], p["cce"], p["i"], p["bits"], p["rnti"]))
        print("planted", p["g"], p["L"], p["cce"], p["i"], hex(p["rnti"]), None if m is None else (m["flags"], m["n_repeat"], round(m["quality"], 3)))
        if m is None:
            e = S.pdcch_scan_decodes(p["g"])[pkg.capi.scan_candidates(int(got.n_cce[p["g"]])).index((p["L"], p["cce"])) * len(got.sizes) + p["i"]]
            print("   its decode: flags %d, rnti_x %#x, quality %.3f, n_err %d of %d, payload bits wrong %d" % (e.flags, e.rnti_x, e.quality, e.n_err, e.n_obs, bin(e.bits ^ p["bits"]).count("1")))
    assert len(planted) >= 20 and {p["L"] for p in planted} == {2, 4, 8}
    for p in planted:
        m = msgs[(p["g"], p["L"], p["cce"], p["i"], p["bits"], p["rnti"])]
        assert m["flags"] & 2 and m["flags"] & 4 and m["n_repeat"] >= 2
    assert set(got.rntis()) >= set(SC.CAP_RNTIS) and got.n_rnti >= 2


# ---------------------------------------------------------------- refusals
def test_refusals_launch_nothing_and_leave_the_context_usable(pkg, dev):
    R, n_rb, cp, ports = SC.CAP_SHAPE
    cell = _cap_cell(pkg)
    mk = lambda sizes=(22, 23), **kw: pkg.capi.PdcchScanCfg.make(sizes, **kw)
    args = lambda c=cell, n_rb=15, n_ofdm=140, mask=0x3FF: (c, dev, FC, FC, FS * R, 256, n_rb, n_ofdm, mask)
    with pkg.Searcher(0) as S:
        with pytest.raises(pkg.SearcherError, match="has run no scan"):
            S.pdcch_scan_decodes(0)
        before = S.pdcch_scan_wide(*args(), mk())
        assert before.n_read == 10 and before.n_accepted > 0
        table = b"".join(bytes(d) for d in S.pdcch_scan_decodes(3))
        n7 = mk()
        n7.n_sizes = 7
        n0 = mk()
        n0.n_sizes = 0
        res = mk()
        res.reserved[1] = 1
        mi_bad = mk()
        mi_bad.phich_mi[3] = 3
        unknown = _cap_cell(pkg)
        unknown.phich_duration = unknown.phich_resource = 0
        cases = [(args(), n7, "n_sizes is outside"), (args(), n0, "n_sizes is outside"), (args(), mk((7, 23)), "payload size is outside"),
                 (args(), mk((22, 65)), "payload size is outside"), (args(), mk(min_repeat=0), "min_repeat"), (args(), mk(min_repeat=-1), "min_repeat"),
                 (args(), mk(min_quality=1.5), "min_quality"), (args(), mk(min_quality=-0.1), "min_quality"), (args(), mk(min_quality=float("nan")), "min_quality"),
                 (args(), res, "reserved"),
                 # the PDCCH's own
                 (args(unknown), mk(), "PHICH configuration is unknown"), (args(), mk(phich_duration=3), "phich_duration is outside"),
                 (args(), mk(phich_resource=5), "phich_resource is outside"), (args(), mk(cfi_force=4), "cfi_force is outside"),
                 (args(), mk(phich_duration=2, cfi_force=2), "three control symbols"), (args(), mi_bad, "m_i is outside"), (args(), mk(rnti_mask=8), "rnti_mask is outside"),
                 (args(n_rb=14), mk(), "n_rb is outside|not an LTE bandwidth"), (args(n_rb=6), mk(), "contradicts the cell's n_rb_dl"),
                 (args(mask=0), mk(), "dl_mask"), (args(n_ofdm=11), mk(), "n_ofdm is outside"),
                 (args(pkg.new_cell(n_id_2=1, cp_type=cp)), mk(), "n_id_1, n_id_2 and a known cp_type")]
        for a, cfg, text in cases:
            with pytest.raises(pkg.SearcherError, match=text):
                S.pdcch_scan_wide(*a, cfg)
        grid = np.ones((140, 180), np.complex128)
        for a, cfg, text in [((cell, grid, 15), mk((22, 70)), "payload size is outside"), ((cell, grid[:11], 15), mk(), "n_ofdm is outside"),
                             ((cell, grid, 15, 0x400), mk(), "dl_mask"), ((cell, grid, 15), mk(min_repeat=0), "min_repeat")]:
            with pytest.raises(pkg.SearcherError, match=text):
                S.pdcch_scan(*a, cfg=cfg) if len(a) == 3 else S.pdcch_scan(*a, cfg)
        lib, rec = S._lib, pkg.PdcchScanInfo()
        assert lib.lcs_pdcch_scan_wide(S._h, C.byref(cell), C.c_void_p(dev.data_ptr()), dev.numel(), FC, FC, FS * R, 256, 15, 140, 0x3FF, None, C.byref(rec)) == -2
        assert b"null pointer" in lib.lcs_last_error(S._h)
        assert lib.lcs_pdcch_scan(S._h, C.byref(cell), grid.ctypes.data_as(C.POINTER(C.c_double)), 140, 15, 0x3FF, C.byref(mk()), None) == -2
        # a refused call leaves the last scan's table where it was; g out of range and a cap that is too small are refused
        assert b"".join(bytes(d) for d in S.pdcch_scan_decodes(3)) == table
        for g in (-1, 10, 72):
            with pytest.raises(pkg.SearcherError, match="outside the subframes"):
                S.pdcch_scan_decodes(g)
        buf = (pkg.capi.PdcchScanDec * 4)()
        assert lib.lcs_pdcch_scan_decodes(S._h, 3, buf, 4) == -2 and lib.lcs_pdcch_scan_decodes(S._h, 3, None, 990) == -2
        after = S.pdcch_scan_wide(*args(), mk())
        assert bytes(after) == bytes(before)


# ---------------------------------------------------------------- the other stages' records are left alone
def test_the_pdcch_pdsch_and_pcfich_records_are_left_alone(pkg, dev):
    R, n_rb, cp, ports = SC.CAP_SHAPE
    cell = _cap_cell(pkg)
    args = (cell, dev, FC, FC, FS * R, 128 * R, n_rb, 140, 0x3FF)
    with pkg.Searcher(0) as s:
        want = (bytes(s.pdcch_wide(*args)), bytes(s.pdsch_wide(*args)), bytes(s.pcfich_wide(*args)))
        scan = s.pdcch_scan_wide(*args, pkg.capi.PdcchScanCfg.make(SC.cap_sizes()))
        assert scan.n_accepted > 0
        assert (bytes(s.pdcch_wide(*args)), bytes(s.pdsch_wide(*args)), bytes(s.pcfich_wide(*args))) == want
        assert bytes(s.pdcch_scan_wide(*args, pkg.capi.PdcchScanCfg.make(SC.cap_sizes()))) == bytes(scan)


# ---------------------------------------------------------------- the sweep
def test_measure_wideband_attaches_the_direct_call_s_record(pkg):
    import torch
    K, fc = 8, 1.8425e9
    sizes = (pkg.capi.dci_ue_sizes(25, 2)["0/1A"], pkg.capi.dci_common_sizes(25)[1])
    wide = dict(n_id_1=DC.CAP_ID[0], n_id_2=DC.CAP_ID[1], n_ports=2, port_gains=[1.0, 0.7j], f_off=1200.0, t0=4321.0, sfn0=8, cfi=DC.capture_cfi,
                pdcch=DC.capture_plan(25, 1, 2), pdcch_fill=0.5)
    x, _, _ = pkg.synth.make_wideband_cell(12, fc, K, [(fc, 4, 25, wide)], snr_db=20.0, n_in=153600 * K)
    d = torch.from_numpy(x).cuda()
    carriers = np.array([fc])
    cfg = pkg.capi.PdcchScanCfg.make(sizes)
    with pkg.Searcher(0) as s:
        cells = pkg.sweep.search_wideband(s, d.data_ptr(), pkg.FMT_C64, x.size, FS * K, K, fc, carriers, np.array([-5e3, 0.0, 5e3]), n_out=153584, meas=True)
        big = [c for c in cells[0] if c["n_id_cell"] == DC.CAP_ID[0] * 3 + DC.CAP_ID[1] and c["n_rb_dl"] == 25]
        assert len(big) == 1, [(c["n_id_cell"], c["n_rb_dl"]) for c in cells[0]]
        calls = []
        real = s.pdcch_scan_wide
        s.pdcch_scan_wide = lambda *a, **k: (calls.append((real(*a, **k), a, k)), calls[-1][0])[1]
        both = pkg.sweep.measure_wideband(s, d.data_ptr(), pkg.FMT_C64, x.size, FS * K, fc, K, cells, carriers, pdcch_scan=cfg)
        del s.pdcch_scan_wide
        rec = big[0]["pdcch_scan"]
        k = cells[0].index(big[0])
        assert both[0][k][-1] is rec and isinstance(both[0][k][0], pkg.CellMeasWide) and len(calls) >= 1
        mine = [c for c in calls if c[0] is rec][0]
        assert bytes(s.pdcch_scan_wide(*mine[1], **mine[2])) == bytes(rec)          # the direct call on the sweep's buffer
    assert rec.n_rb == 25 and rec.sizes == sizes and rec.n_read >= 25 and rec.n_si > 0 and rec.n_paging > 0
    print("sweep: %d subframes read, %d listed, accepted %d (SI %d, paging %d, RA %d, UE %d)" % (rec.n_read, rec.n_msg, rec.n_accepted, rec.n_si, rec.n_paging, rec.n_ra, rec.n_ue))
