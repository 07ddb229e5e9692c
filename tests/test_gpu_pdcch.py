"""GPU tests of the PDCCH common-search-space stage (lcs_pdcch_wide, lcs_pdcch; k_pdcch_llr, k_pdcch_dec, k_pdcch_fin).

The stage on the crafted grids of tests/pdcch_cases.py against the numpy statement of the rule (tests/pdcch_ref.py): every integer
equal (with the tie exclusion of tests/test_pdcch_host.py), quality to 1e-9, the PCFICH's GPU bar; and the whole record bit-equal
to the host twin (tests/host/pdcch_host.cpp).  The CFI it reads with is S.pcfich's.  From samples: lcs_pdcch_wide equals lcs_pdcch
on lcs_extract_tfg_wide's grid and finds every planted DCI.  cfi_force, refusals, isolation, sweep.measure_wideband(pdcch=True)."""
import ctypes as C

import numpy as np
import pytest

import cell_meas_cases as CS
import pcfich_ref as PR
import pdcch_cases as DC
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
    return DC.load_twin(pkg.capi)


_dev = {}


def dev(shape):
    import torch
    if shape not in _dev:
        _dev[shape] = torch.from_numpy(np.array(DC.pdcch_capture(*shape)[0])).cuda()
    return _dev[shape]


def _cell(pkg, shape, **kw):
    R, n_rb, cp, ports = shape
    c = pkg.new_cell(n_id_1=DC.CAP_ID[0], n_id_2=DC.CAP_ID[1], cp_type=cp, n_ports=ports, freq_fine=0.0, frame_start=kw.pop("frame_start", DC.pdcch_capture(*shape)[1]))
    c.n_rb_dl, c.phich_duration, c.phich_resource = kw.pop("n_rb_dl", n_rb), kw.pop("phich_duration", 1), kw.pop("phich_resource", 3)
    return c


def _case_cell(pkg, case):
    return pkg.new_cell(n_id_1=case[0] // 3, n_id_2=case[0] % 3, cp_type=case[1], n_ports=case[2])


# ---------------------------------------------------------------- the stage on crafted grids
@pytest.mark.parametrize("case", DC.CASES, ids=DC.case_id)
def test_stage_against_numpy_and_the_host_twin_on_crafted_grids(pkg, S, H, case):
    tfg, cfi, planted = DC.crafted(case)
    n_rb, mask = case[3], DC.dl_mask_of(case)
    cell, cfg = _case_cell(pkg, case), DC.make_cfg(pkg.capi, case)
    got = S.pdcch(cell, tfg, n_rb, mask, cfg)
    # the CFI it used is the PCFICH stage's, which reads the planted one
    pc = S.pcfich(cell, tfg, n_rb, mask)
    read = got.cfi > 0
    assert np.array_equal(got.cfi[read], pc.cfi[read]) and np.array_equal(pc.cfi[read], cfi[read]) and read.sum() >= 3
    worst, n, excused = DC.assert_record_against_numpy(got, DC.reference(case), planted, 1e-9, DC.case_id(case))
    twin = DC.twin_record(H, pkg.capi, case, tfg, pc.cfi)
    assert bytes(got) == bytes(twin), (DC.case_id(case), np.flatnonzero(np.frombuffer(bytes(got), np.uint8) != np.frombuffer(bytes(twin), np.uint8))[:8])
    print(DC.case_id(case), "worst |quality - numpy| %.2e, %d decodes, %d excused" % (worst, n, excused))


def test_cfi_force_and_grids_without_a_signal(pkg, S, H):
    case = DC.CASES[8]                                        # 25 RB, 2 ports, CFI 1 .. 3 by subframe
    tfg, cfi, planted = DC.crafted(case)
    cell = _case_cell(pkg, case)
    plain = S.pdcch(cell, tfg, 25, 0x3FF, DC.make_cfg(pkg.capi, case))
    found = lambda rec, g: {(m["cce"], m["bits"], m["rnti"]) for m in rec.messages() if m["subframe"] == g}
    for force in (1, 2, 3):
        rec = S.pdcch(cell, tfg, 25, 0x3FF, DC.make_cfg(pkg.capi, case, cfi_force=force))
        assert (rec.cfi == force).all() and bytes(rec) == bytes(DC.twin_record(H, pkg.capi, case, tfg, cfi, cfg=DC.make_cfg(pkg.capi, case, cfi_force=force)))
        for g in range(DC.N_SF):
            want = {(p["cce"], p["bits"], p["rnti"]) for p in planted if p["g"] == g and p["rnti"] != 0x1234}
            if cfi[g] == force:
                assert [bytes(rec.dec[g][s][i]) for s in range(6) for i in range(2)] == [bytes(plain.dec[g][s][i]) for s in range(6) for i in range(2)]
                assert want <= found(rec, g)
            else:
                assert not (want & found(rec, g)), (force, g)      # a wrong CFI finds nothing of what was planted
    # rnti_mask: SI alone
    si = S.pdcch(cell, tfg, 25, 0x3FF, DC.make_cfg(pkg.capi, case, rnti_mask=1))
    assert si.n_accepted == si.n_si == plain.n_si > 0 and si.n_paging == si.n_ra == 0
    # silence and values that are not finite
    cfg = DC.make_cfg(pkg.capi, case, cfi_force=3)
    for grid in (np.zeros((44, 300), np.complex128), np.full((44, 300), np.nan + 0j)):
        rec = S.pdcch(cell, grid, 25, 0x3FF, cfg)
        assert bytes(rec) == bytes(DC.twin_record(H, pkg.capi, case, grid, np.zeros(4, np.int32), cfg=cfg)) and rec.n_accepted == 0 and rec.n_read == 3
    assert all((d.bits, d.rnti_x, d.flags, d.quality) == (0, 0, 1, 0.0) for _, _, _, d in S.pdcch(cell, np.zeros((44, 300), np.complex128), 25, 0x3FF, cfg).entries())


# ---------------------------------------------------------------- from samples
@pytest.mark.parametrize("shape", DC.CAP_SHAPES, ids=str)
def test_from_samples_equals_the_stage_on_the_extracted_grid_and_finds_what_was_planted(pkg, S, shape):
    R, n_rb, cp, ports = shape
    n = PR.n_symb_of(cp)
    n_ofdm = 30 * n + 3
    d, cell = dev(shape), _cell(pkg, shape)
    got = S.pdcch_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm)
    tfg, _ = S.extract_tfg_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm)
    again = S.pdcch(cell, tfg, n_rb)
    assert bytes(got) == bytes(again) and got.sizes == pkg.capi.dci_common_sizes(n_rb)
    pc = S.pcfich_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm)
    read = got.cfi > 0
    assert got.n_sf == 16 and got.n_read == read.sum() == (15 if n_rb <= 10 else 16) and np.array_equal(got.cfi[read], pc.cfi[read])
    assert list(got.cfi[:15]) == [DC.capture_cfi(1 + g // 10, g % 10) for g in range(15)]
    msgs = {(m["subframe"], m["cce"], m["bits"], m["rnti"], m["size"]): m for m in got.messages()}      # (an L = 8 DCI is listed once, at the better level)
    sizes = pkg.capi.dci_common_sizes(n_rb)
    planted = DC.capture_planted(n_rb, cp, ports, 15)
    for p in planted:
        m = msgs[(p["g"], p["cce"], p["bits"], p["rnti"], sizes[p["i"]])]
        assert m["L"] in (4, p["L"])
        assert m["kind"] == ("si" if p["rnti"] == 0xFFFF else "paging" if p["rnti"] == 0xFFFE else "ra") and m["quality"] > 0.5
        if p["i"] == 0:
            want = DC.fields_1a(1 + p["g"] // 10, p["g"] % 10, n_rb)
            f = pkg.capi.dci_1a_fields(m["bits"], n_rb)
            assert {k: f[k] for k in want} == want
    print(shape, "planted %d, all listed; messages %d, accepted entries %d" % (len(planted), len(msgs), got.n_accepted))
    # the mask picks subframes
    part = S.pdcch_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm, 0x021)
    assert list(np.flatnonzero(part.cfi)) == [0, 5, 10, 15][:part.n_read] and bytes(part.dec[5]) == bytes(got.dec[5]) and not any(g == 1 for g, _, _, _ in part.entries())


# ---------------------------------------------------------------- refusals
def test_refusals_launch_nothing_and_leave_the_context_usable(pkg, S):
    shape = DC.CAP_SHAPES[1]
    R, n_rb, cp, ports = shape
    d, cell = dev(shape), _cell(pkg, shape)
    mk = pkg.capi.PdcchCfg.make
    args = lambda c=cell, n_rb=15, n_ofdm=213, mask=0x3FF: (c, d, FC, FC, FS * R, 256, n_rb, n_ofdm, mask)
    before = S.pdcch_wide(*args(), mk((22, 10)))
    assert before.n_read == 16 and before.n_accepted > 0
    unknown = _cell(pkg, shape, phich_duration=0, phich_resource=0)
    mi_bad = mk((22, 10))
    mi_bad.phich_mi[3] = 3
    n0 = mk((22, 10))
    n0.n_sizes = 0
    n3 = mk((22, 10))
    n3.n_sizes = 3
    cases = [(args(unknown), mk((22, 10)), "PHICH configuration is unknown"), (args(unknown), mk((22, 10), phich_duration=1), "PHICH configuration is unknown"),
             (args(), mk((22, 10), phich_duration=3), "phich_duration is outside"), (args(), mk((22, 10), phich_resource=5), "phich_resource is outside"),
             (args(), mk((22, 10), phich_resource=-1), "phich_resource is outside"),
             (args(), mk((7, 10)), "payload size is outside"), (args(), mk((22, 49)), "payload size is outside"), (args(), n0, "n_sizes is outside"), (args(), n3, "n_sizes is outside"),
             (args(), mk((22, 10), cfi_force=4), "cfi_force is outside"), (args(), mk((22, 10), cfi_force=-1), "cfi_force is outside"),
             (args(), mk((22, 10), phich_duration=2, cfi_force=2), "three control symbols"), (args(), mi_bad, "m_i is outside"),
             (args(), mk((22, 10), rnti_mask=8), "rnti_mask is outside"),
             # the PCFICH entry points' own
             (args(n_rb=14), mk((22, 10)), "n_rb is outside|not an LTE bandwidth"), (args(n_rb=6), mk((22, 10)), "contradicts the cell's n_rb_dl"),
             (args(mask=0), mk((22, 10)), "dl_mask"), (args(n_ofdm=11), mk((22, 10)), "n_ofdm is outside"),
             (args(pkg.new_cell(n_id_2=1, cp_type=cp)), mk((22, 10)), "n_id_1, n_id_2 and a known cp_type")]
    for a, cfg, text in cases:
        with pytest.raises(pkg.SearcherError, match=text):
            S.pdcch_wide(*a, cfg)
    grid = np.ones((213, 180), np.complex128)
    for a, cfg, text in [((unknown, grid, 15), mk((22, 10)), "PHICH configuration is unknown"), ((cell, grid, 15), mk((22, 60)), "payload size is outside"),
                         ((cell, grid[:11], 15), mk((22, 10)), "n_ofdm is outside"), ((cell, grid, 15, 0x400), mk((22, 10)), "dl_mask"),
                         ((cell, np.ones((213, 300), np.complex128), 25), mk((22, 10)), "contradicts the cell's n_rb_dl")]:
        with pytest.raises(pkg.SearcherError, match=text):
            S.pdcch(*a, cfg=cfg) if len(a) == 3 else S.pdcch(*a, cfg)
    with pytest.raises(ValueError):
        S.pdcch(cell, grid, 25)
    lib, rec, cfg = S._lib, pkg.PdcchInfo(), mk((22, 10))
    assert lib.lcs_pdcch_wide(S._h, C.byref(cell), C.c_void_p(d.data_ptr()), d.numel(), FC, FC, FS * R, 256, 15, 213, 0x3FF, None, C.byref(rec)) == -2
    assert b"null pointer" in lib.lcs_last_error(S._h)
    assert lib.lcs_pdcch_wide(S._h, C.byref(cell), C.c_void_p(d.data_ptr()), d.numel(), FC, FC, FS * R, 256, 15, 213, 0x3FF, C.byref(cfg), None) == -2
    assert lib.lcs_pdcch(S._h, C.byref(cell), grid.ctypes.data_as(C.POINTER(C.c_double)), 213, 15, 0x3FF, None, C.byref(rec)) == -2
    assert b"lcs_pdcch: a null pointer" in lib.lcs_last_error(S._h)
    after = S.pdcch_wide(*args(), mk((22, 10)))
    assert bytes(after) == bytes(before)


# ---------------------------------------------------------------- the chain, the measurement and the PCFICH are left alone
def test_the_chain_the_measurement_and_the_pcfich_are_left_alone(pkg):
    shape = DC.CAP_SHAPES[2]
    R, n_rb, cp, ports = shape
    d, cell = dev(shape), _cell(pkg, shape)
    args = (cell, d, FC, FC, FS * R, 128 * R, n_rb, 30 * PR.n_symb_of(cp) + 3, 0x339)
    batch = lambda s: s.search_capbuf(CS.cap(1), CS.GRID, CS.FC, CS.FC, FS)[0]
    table = lambda s: [bytes(t) for t in s.last_cell_meas(1, 16)[0]]
    with pkg.Searcher(0) as s:              # a context that never calls the stage
        s.set_cell_meas(True)
        want_cells = [bytes(c) for c in batch(s)]
        want_table = table(s)
        want_pcfich = bytes(s.pcfich_wide(*args))
        want_meas = bytes(s.cell_meas_wide(*args))
        want_next = [bytes(c) for c in batch(s)]
    with pkg.Searcher(0) as s:
        plain = s.pdcch_wide(*args)
        assert plain.n_read > 0 and plain.n_accepted > 0
        s.set_cell_meas(True)
        assert [bytes(c) for c in batch(s)] == want_cells and table(s) == want_table
        assert bytes(s.pdcch_wide(*args)) == bytes(plain) and s.cell_meas_mode is True and table(s) == want_table
        assert bytes(s.pcfich_wide(*args)) == want_pcfich and bytes(s.cell_meas_wide(*args)) == want_meas
        assert bytes(s.pdcch_wide(*args)) == bytes(plain)
        assert bytes(s.pdcch_wide(*args, pkg.capi.PdcchCfg.make(pkg.capi.dci_common_sizes(n_rb), cfi_force=3))) != bytes(plain)       # (other tables ...)
        assert bytes(s.pdcch_wide(*args)) == bytes(plain)                                                                             # (... and back)
        assert [bytes(c) for c in batch(s)] == want_next and table(s) == want_table
    with pkg.Searcher(0) as s:
        s.stream_open(pkg.FMT_IQ_U8, 153600, CS.FC, CS.FC, FS)
        assert bytes(s.pdcch_wide(*args)) == bytes(plain)
        s.stream_close()
        assert bytes(s.pdcch_wide(*args)) == bytes(plain)


# ---------------------------------------------------------------- the sweep
def test_measure_wideband_gives_the_direct_call_s_record(pkg):
    import torch
    K, fc = 8, 1.8425e9
    plan = DC.capture_plan(25, 1, 2)
    wide = dict(n_id_1=DC.CAP_ID[0], n_id_2=DC.CAP_ID[1], n_ports=2, port_gains=[1.0, 0.7j], f_off=1200.0, t0=4321.0, sfn0=8, cfi=DC.capture_cfi, pdcch=plan, pdcch_fill=0.5)
    x, _, _ = pkg.synth.make_wideband_cell(12, fc, K, [(fc, 4, 25, wide)], snr_db=20.0, n_in=153600 * K)
    d = torch.from_numpy(x).cuda()
    carriers = np.array([fc])
    with pkg.Searcher(0) as s:
        cells = pkg.sweep.search_wideband(s, d.data_ptr(), pkg.FMT_C64, x.size, FS * K, K, fc, carriers, np.array([-5e3, 0.0, 5e3]), n_out=153584, meas=True)
        big = [c for c in cells[0] if c["n_id_cell"] == DC.CAP_ID[0] * 3 + DC.CAP_ID[1] and c["n_rb_dl"] == 25]
        assert len(big) == 1, [(c["n_id_cell"], c["n_rb_dl"]) for c in cells[0]]
        calls = []
        real = s.pdcch_wide
        s.pdcch_wide = lambda *a, **k: (calls.append(real(*a, **k)), calls[-1])[1]
        both = pkg.sweep.measure_wideband(s, d.data_ptr(), pkg.FMT_C64, x.size, FS * K, fc, K, cells, carriers, pcfich=True, pdcch=True)
        del s.pdcch_wide
        rec = big[0]["pdcch"]
        k = cells[0].index(big[0])
        assert both[0][k][2] is rec and both[0][k][1] is big[0]["pcfich"] and isinstance(both[0][k][0], pkg.CellMeasWide)
        # the direct call's record, from the buffer the sweep channelized for the measurement
        assert any(c is rec for c in calls) and rec.n_rb == 25 and rec.sizes == pkg.capi.dci_common_sizes(25)
        read = rec.cfi > 0
        assert np.array_equal(rec.cfi[read], big[0]["pcfich"].cfi[read]) and rec.n_read == read.sum() >= 25
    kinds = {m["kind"] for m in rec.messages()}
    print("sweep: %d subframes read, %d messages %s" % (rec.n_read, len(rec.messages()), sorted(kinds)))
    assert {"si", "paging"} <= kinds and all(m["quality"] > 0.5 for m in rec.messages() if m["L"] == 8)
    # every 1A message carries fields of the plan of its subframe (the grid's frame offset is the search's to choose: any frame)
    ok = 0
    for m in rec.messages():
        if m["size"] == 25 and m["kind"] in ("si", "paging"):
            f = pkg.capi.dci_1a_fields(m["bits"], 25)
            ok += any(all(f[k] == v for k, v in DC.fields_1a(fr, m["subframe"] % 10, 25).items()) for fr in range(12))
    assert ok >= 20
