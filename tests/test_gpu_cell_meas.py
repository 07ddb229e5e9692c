"""GPU tests of the cell measurement (lcs_set_cell_meas, lcs_cell_meas, lcs_last_cell_meas; k_cell_meas).

The stage against the numpy reference (tests/cell_meas_ref.py) on crafted grids: every sum to 1e-9 of its scale -- the project's bar
for a device fp64 stage against numpy --, the derived fields to 1e-9 of E_p / (12 n_rows) or rssi, the integers exact.  Then the
fused chain on planted cells (tests/cell_meas_cases.py, tests/tdd_config_cases.py): with the mode on the records are byte for byte
the mode-off records, lcs_last_cell_meas equals lcs_cell_meas on lcs_extract_tfg's grid of the same record with the record's dl_mask
field for field -- the chain's raw grid is that grid --, and agrees with the numpy rule on the oracle's grid."""
import os

import numpy as np
import pytest

import cell_meas_cases as CS
import cell_meas_ref as MR
import oracle as O
import tdd_config_cases as K
from conftest import load_pkg

pytestmark = pytest.mark.gpu
FS = CS.FS
NB = len(CS.BUFFERS)
MAXC = 16
TOL = 1e-9


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module", autouse=True)
def _oracle_mode():
    O.set_legacy(False)
    O.set_threads(min(16, os.cpu_count() or 1))


@pytest.fixture(scope="module")
def S(pkg):
    s = pkg.Searcher(0)
    s.set_cell_meas(True)
    yield s
    s.close()


def _rec(t):
    return (t.status, t.n_rows, t.n_ports, t.dl_mask, tuple(t.rsrp), tuple(t.noise), t.rssi, t.rsrq, tuple(t.a_re_im))


def _none(pkg, t):
    n = pkg.MEAS_NOT_MEASURED
    return _rec(t) == (n, n, n, n, (0.0, 0.0), (0.0, 0.0), 0.0, 0.0, (0.0,) * 4)


def _cell(pkg, n_id, cp, n_ports=-1):
    return pkg.new_cell(n_id_1=n_id // 3, n_id_2=n_id % 3, cp_type=cp, n_ports=n_ports)


def _bytes(cells):
    return [bytes(c) for c in cells]


# ---------------------------------------------------------------- the stage on crafted grids
@pytest.mark.parametrize("shape", CS.SHAPES, ids=[str(s) for s in CS.SHAPES])
def test_stage_against_the_numpy_reference(pkg, S, shape):
    n_id, cp, n_ofdm, ports = shape
    assert sorted({s[0] % 6 for s in CS.SHAPES}) == [0, 1, 2, 3, 4, 5] and CS.MASKS == [0x3FF, 0x021, 0x200, pkg.tdd_dl_mask(2)]
    tfg = CS.shape_grid(shape)
    worst = 0.0
    for mask in CS.MASKS:
        ref = MR.measure(n_id, cp, tfg, mask, ports)
        got = S.cell_meas(_cell(pkg, n_id, cp, ports), tfg, mask)
        assert ref["status"] == 0 and ref["n_rows"] > 0
        worst = max(worst, MR.assert_record_close(got, ref, TOL, (shape, hex(mask))))
    print(shape, "worst stage error / scale %.2e" % worst)


def test_stage_ports_and_python_record(pkg, S):
    shape = CS.SHAPES[6]
    tfg = CS.shape_grid(shape)
    for n_ports, P in ((0, 1), (-1, 1), (1, 1), (2, 2), (4, 2)):
        got = S.cell_meas(_cell(pkg, shape[0], shape[1], n_ports), tfg)
        MR.assert_record_close(got, MR.measure(shape[0], shape[1], tfg, 0x3FF, n_ports), TOL, n_ports)
        assert got.n_ports == P and got.dl_mask == 0x3FF and len(got.sinr) == len(got.rsrp_db) == len(got.sinr_db) == P
        assert got.sinr[0] == got.rsrp[0] / got.noise[0] and abs(got.sinr_db[0] - 10 * np.log10(got.sinr[0])) < 1e-12
        assert abs(got.rsrq_db - 10 * np.log10(got.rsrq)) < 1e-12 and abs(got.rsrp_db[0] - 10 * np.log10(got.rsrp[0])) < 1e-12
    m = pkg.CellMeas()
    m.status, m.n_ports = 0, 2
    m.rsrp[0], m.rsrp[1], m.noise[0], m.noise[1] = 1.0, 2.0, 0.0, -1e-3
    assert m.sinr == (float("inf"), float("inf")) and m.sinr_db == (float("inf"), float("inf"))
    assert [pkg.tdd_dl_mask(c) for c in range(-1, 8)] == [MR.tdd_dl_mask(c) for c in range(-1, 8)]


# ---------------------------------------------------------------- grids without a number, refusals
def test_grids_that_get_no_number(pkg, S):
    for tfg in (np.zeros((854, 72), np.complex128), np.full((854, 72), np.nan + 0j)):
        for n_ports in (1, 2):
            got = S.cell_meas(_cell(pkg, 7, 1, n_ports), tfg, 0x021)
            assert _rec(got) == (-1, len([r for r in MR.TR.ref_rows(854, 1) if r[3] in (0, 5)]), n_ports, 0x021, (0.0, 0.0), (0.0, 0.0), 0.0, 0.0, (0.0,) * 4)
    g = CS.shape_grid(CS.SHAPES[0]).copy()
    clean = S.cell_meas(_cell(pkg, 96, 1, 1), g, 0x021)
    g[28, 5] = np.nan          # subframe 2: outside the mask
    assert _rec(S.cell_meas(_cell(pkg, 96, 1, 1), g, 0x021)) == _rec(clean) and clean.status == 0
    g[0, 71] = np.nan          # subframe 0, no reference element: only w sees it
    assert S.cell_meas(_cell(pkg, 96, 1, 1), g, 0x021).status == -1


def test_refusals(pkg, S):
    tfg = CS.shape_grid(CS.SHAPES[0])
    for cell, n_ofdm, mask, text in ((pkg.new_cell(n_id_2=1, cp_type=1), 854, 0x3FF, "n_id_1, n_id_2 and a known cp_type"),
                                     (pkg.new_cell(n_id_1=5, cp_type=1), 854, 0x3FF, "n_id_1, n_id_2 and a known cp_type"),
                                     (pkg.new_cell(n_id_1=5, n_id_2=1), 854, 0x3FF, "n_id_1, n_id_2 and a known cp_type"),
                                     (_cell(pkg, 96, 1), 279, 0x3FF, "at least two frames"),
                                     (_cell(pkg, 96, 2), 239, 0x3FF, "at least two frames"),
                                     (_cell(pkg, 96, 1), 855, 0x3FF, "at most LCS_TFG_MAX_OFDM"),
                                     (_cell(pkg, 96, 1), 854, 0, "dl_mask"),
                                     (_cell(pkg, 96, 1), 854, 0x400, "dl_mask"),
                                     (_cell(pkg, 96, 1), 854, 0x7FF, "dl_mask"),
                                     (_cell(pkg, 96, 1), 854, -1, "dl_mask")):
        g = np.zeros((n_ofdm, 72), np.complex128)
        g[:min(n_ofdm, 854)] = tfg[:min(n_ofdm, 854)]
        with pytest.raises(pkg.SearcherError, match=text):
            S.cell_meas(cell, g, mask)
    with pkg.Searcher(0) as s:
        assert s.cell_meas_mode is False
        with pytest.raises(pkg.SearcherError, match="lcs_search_capbuf or a batch"):
            s.last_cell_meas()
        assert s._lib.lcs_set_cell_meas(s._h, 2) == -2 and b"neither 0 nor 1" in s._lib.lcs_last_error(s._h)
        s.set_cell_meas(True)
        assert s.cell_meas_mode is True
        with pytest.raises(pkg.SearcherError, match="does not carry the cell measurement"):
            s.stream_open(pkg.FMT_IQ_U8, 153600, CS.FC, CS.FC, FS)
        s.set_cell_meas(False)
        s.stream_open(pkg.FMT_IQ_U8, 153600, CS.FC, CS.FC, FS)
        with pytest.raises(pkg.SearcherError, match="cannot change under an open stream"):
            s.set_cell_meas(True)
        s.set_cell_meas(False)      # no change: accepted
        s.stream_close()
        s.set_cell_meas(True)


def test_stage_works_whatever_the_modes_and_leaves_the_table_alone(pkg):
    shape = CS.SHAPES[2]
    tfg, cell = CS.shape_grid(shape), _cell(pkg, shape[0], shape[1], shape[3])
    with pkg.Searcher(0) as s:
        plain = s.cell_meas(cell, tfg, 0x339)
        assert plain.status == 0
        for duplex, unwrap, tdd, meas in ((pkg.DUPLEX_TDD, False, True, False), (pkg.DUPLEX_TDD, True, True, True), (pkg.DUPLEX_FDD, False, False, True)):
            s.set_duplex(duplex), s.set_foe_unwrap(unwrap), s.set_tdd_config(tdd), s.set_cell_meas(meas)
            assert _rec(s.cell_meas(cell, tfg, 0x339)) == _rec(plain)
        cells, _ = s.search_capbuf(CS.cap(1), CS.GRID, CS.FC, CS.FC, FS)
        before = [_rec(t) for t in s.last_cell_meas(1, MAXC)[0]]
        assert before[0][0] == 0 and len(cells) >= 1
        assert _rec(s.cell_meas(cell, tfg, 0x200)) != _rec(plain)
        assert [_rec(t) for t in s.last_cell_meas(1, MAXC)[0]] == before


# ---------------------------------------------------------------- the fused chain, FDD
def _check_table(pkg, S, cells, info, cap, fc, want_mask, ref_cells=None):
    """info[k] belongs to cells[k]: it equals the stage on extract_tfg's grid of that record with the record's dl_mask, field for
    field (want_mask(cell): the mask the chain must have used, None: any); the entries behind the cells read NOT_MEASURED.  ref_cells: (oracle cell, oracle raw grid) to hold the numpy rule against"""
    assert len(info) == MAXC
    for k, c in enumerate(cells):
        tfg, _ = S.extract_tfg(c, cap, fc, fc, FS)
        assert info[k].status == 0 and want_mask(c) in (None, info[k].dl_mask), (k, _rec(info[k]))
        assert info[k].n_ports == (2 if c.n_ports >= 2 else 1)
        stage = S.cell_meas(c, tfg, info[k].dl_mask)
        assert _rec(info[k]) == _rec(stage), (k, _rec(info[k]), _rec(stage))
    for k in range(len(cells), MAXC):
        assert _none(pkg, info[k])
    worst = 0.0
    if ref_cells is not None:
        assert [c.n_id_cell() for c in cells] == [oc.n_id_2 + 3 * oc.n_id_1 for oc, _, _ in ref_cells]
        for k, (oc, tfg, _) in enumerate(ref_cells):
            ref = MR.measure(oc.n_id_2 + 3 * oc.n_id_1, oc.cp_type, tfg, info[k].dl_mask, oc.n_ports)
            worst = max(worst, MR.assert_record_close(info[k], ref, TOL, ("oracle grid", k)))
    return worst


@pytest.fixture(scope="module")
def off_single(pkg):
    with pkg.Searcher(0) as s:
        out = [_bytes(s.search_capbuf(CS.cap(b), CS.GRID, CS.FC, CS.FC, FS)[0]) for b in range(NB)]
        assert all(_none(pkg, t) for t in s.last_cell_meas(1, MAXC)[0])
    return out


def test_search_capbuf_with_the_mode_on(pkg, S, off_single):
    worst, n = 0.0, 0
    for b in range(NB):
        cells, _ = S.search_capbuf(CS.cap(b), CS.GRID, CS.FC, CS.FC, FS)
        info = S.last_cell_meas(1, MAXC)[0]
        assert _bytes(cells) == off_single[b], "the records are the mode-off records"
        worst = max(worst, _check_table(pkg, S, cells, info, CS.cap(b), CS.FC, lambda c: 0x3FF, CS.recovered(b)))
        n += len(cells)
    print("fused chain against the numpy rule on the oracle's grid: worst error / scale %.2e over %d cells" % (worst, n))
    assert n == 7      # one cell per buffer, two in the fifth
    # the SINR follows the planted SNR
    sinr = [10 * np.log10(S.cell_meas(c, S.extract_tfg(c, CS.cap(b), CS.FC, CS.FC, FS)[0]).sinr[0])
            for b in range(4) for c in S.search_capbuf(CS.cap(b), CS.GRID, CS.FC, CS.FC, FS)[0]]
    assert len(sinr) == 4 and all(snr - 2.0 <= v <= snr + 0.5 for v, snr in zip(sinr, CS.SNR_SERIES)) and sinr == sorted(sinr, reverse=True), sinr


def _batch(pkg, s, fmt, u8, cap, n_cap, grid, fc):
    import torch
    if fmt == pkg.FMT_IQ_U8:
        d = torch.from_numpy(np.stack(u8)).cuda()
    else:
        d = torch.from_numpy(np.stack([x.astype(np.complex64) for x in cap])).cuda()
    cells = s.search_batch(d.data_ptr(), fmt, len(u8), n_cap, grid, fc, fc, FS, pkg.STAGE_FULL, MAXC)
    del d
    return cells


def _fdd_batch(pkg, s, fmt):
    return _batch(pkg, s, fmt, [CS.u8(b) for b in range(NB)], [CS.cap(b) for b in range(NB)], 153600, CS.GRID, CS.FC)


@pytest.mark.parametrize("fmt", ["u8", "c64"])
def test_batches_with_the_mode_on(pkg, S, fmt):
    f = pkg.FMT_IQ_U8 if fmt == "u8" else pkg.FMT_C64
    with pkg.Searcher(0) as off:
        ref = _fdd_batch(pkg, off, f)
        assert all(_none(pkg, t) for row in off.last_cell_meas(NB, MAXC) for t in row)
    cells = _fdd_batch(pkg, S, f)
    info = S.last_cell_meas(NB, MAXC)
    for b in range(NB):
        assert _bytes(cells[b]) == _bytes(ref[b]), "the records are the mode-off records"
        _check_table(pkg, S, cells[b], info[b], CS.cap(b), CS.FC, lambda c: 0x3FF, CS.recovered(b) if fmt == "u8" else None)


def test_rounds_cells_without_a_mib_and_on_then_off(pkg, S, off_single):
    one = _fdd_batch(pkg, S, pkg.FMT_IQ_U8)
    info_one = S.last_cell_meas(NB, MAXC)
    with pkg.Searcher(0) as s:
        s.set_cell_meas(True)
        s.set_max_cells_in_flight(2)
        two = _fdd_batch(pkg, s, pkg.FMT_IQ_U8)
        info_two = s.last_cell_meas(NB, MAXC)
        stats = s.last_batch_stats()
        for b in range(NB):
            assert _bytes(two[b]) == _bytes(one[b])
            assert [_rec(t) for t in info_two[b]] == [_rec(t) for t in info_one[b]]
        # cells without a MIB read not-measured: the table holds exactly one measured record per cell handed out, although more
        # peaks went through the per-cell chain than decoded (noise peaks pass peak_search on every buffer)
        assert sum(t.status == 0 for row in info_two for t in row) == sum(len(c) for c in two) == 7
        # on -> off: the table reads not-measured, the records stay
        s.set_cell_meas(False)
        off = _fdd_batch(pkg, s, pkg.FMT_IQ_U8)
        assert all(_none(pkg, t) for row in s.last_cell_meas(NB, MAXC) for t in row)
        assert [_bytes(c) for c in off] == [_bytes(c) for c in one]
        cells = s.search_capbuf(CS.cap(4), CS.GRID, CS.FC, CS.FC, FS)[0]
        assert _bytes(cells) == off_single[4] and all(_none(pkg, t) for t in s.last_cell_meas(1, MAXC)[0])
    print("batch stats", stats)


# ---------------------------------------------------------------- the fused chain, TDD
def _tdd(pkg, tdd_config, meas):
    s = pkg.Searcher(0)
    s.set_duplex(pkg.DUPLEX_TDD)
    s.set_tdd_config(tdd_config)
    s.set_cell_meas(meas)
    return s


def _tdd_batch(pkg, s):
    n = len(K.BUFFERS)
    return _batch(pkg, s, pkg.FMT_IQ_U8, [K.u8(b) for b in range(n)], [K.cap(b) for b in range(n)], 153600, K.GRID, K.FC)


def test_tdd_masks_with_and_without_the_configuration(pkg):
    n = len(K.BUFFERS)
    with _tdd(pkg, True, False) as ref:
        ref_cells = _tdd_batch(pkg, ref)
        ref_info = [[bytes(t) for t in row] for row in ref.last_tdd_info(n, MAXC)]
        assert all(_none(pkg, t) for row in ref.last_cell_meas(n, MAXC) for t in row)
    with _tdd(pkg, False, True) as s:
        cells = _tdd_batch(pkg, s)
        info = s.last_cell_meas(n, MAXC)
        for b in range(n):
            assert _bytes(cells[b]) == _bytes(ref_cells[b])
            _check_table(pkg, s, cells[b], info[b], K.cap(b), K.FC, lambda c: 0x021)
    seen = set()
    with _tdd(pkg, True, True) as s:
        cells = _tdd_batch(pkg, s)
        info = s.last_cell_meas(n, MAXC)
        assert [[bytes(t) for t in row] for row in s.last_tdd_info(n, MAXC)] == ref_info, "last_tdd_info is unchanged by the new mode"
        for b in range(n):
            want = K.planted(b)
            assert _bytes(cells[b]) == _bytes(ref_cells[b]) and {c.n_id_cell() for c in cells[b]} >= set(want)
            _check_table(pkg, s, cells[b], info[b], K.cap(b), K.FC, lambda c: pkg.tdd_dl_mask(want[c.n_id_cell()][0]) if c.n_id_cell() in want else None)
            seen |= {info[b][k].dl_mask for k, c in enumerate(cells[b]) if c.n_id_cell() in want}
        # and search_capbuf takes the same path
        c3 = s.search_capbuf(K.cap(3), K.GRID, K.FC, K.FC, FS)[0]
        assert [_rec(t) for t in s.last_cell_meas(1, MAXC)[0]] == [_rec(t) for t in info[3]] and _bytes(c3) == _bytes(cells[3])
    assert seen == {pkg.tdd_dl_mask(c) for c in range(7)}
