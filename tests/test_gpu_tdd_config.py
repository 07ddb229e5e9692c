"""GPU tests of the uplink-downlink configuration estimate (lcs_set_tdd_config, lcs_tdd_config, lcs_last_tdd_info; k_tdd_config).

The stage against the numpy reference (tests/tdd_config_ref.py) on crafted grids: T, R and the margin to 1e-9 -- the project's
bar for a device fp64 stage against numpy --, the decisions equal under the asserted condition that the reference sits at least
1e-6 clear of every threshold.  Then the fused chain on planted cells (tests/tdd_config_cases.py): with the mode on the records are
byte for byte the mode-off records, lcs_last_tdd_info equals lcs_tdd_config on lcs_extract_tfg's grid of the same record field for
field -- the chain's raw grid is that grid --, and the configurations are the planted ones."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as O
import tdd_config_ref as TR
import tdd_config_cases as K
from conftest import golden, iq_u8_to_capbuf, load_pkg

pytestmark = pytest.mark.gpu
FS, FC, GRID = K.FS, K.FC, K.GRID
NB = len(K.BUFFERS)
MAXC = 16


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module", autouse=True)
def _oracle_mode():
    O.set_legacy(False)
    O.set_threads(min(16, os.cpu_count() or 1))


def _tdd(pkg, mode=None):
    s = pkg.Searcher(0)
    s.set_duplex(pkg.DUPLEX_TDD)
    if mode is not None:
        s.set_tdd_config(mode)
    return s


@pytest.fixture(scope="module")
def S(pkg):
    s = _tdd(pkg, True)
    yield s
    s.close()


def _rec(t):
    return (t.ul_dl_config, t.dwpts_rs_rows, t.margin, tuple(t.T), tuple(t.R))


def _none(t):
    return _rec(t) == (pkg_not_estimated(), pkg_not_estimated(), 0.0, (0.0,) * 10, (0.0,) * 4)


def pkg_not_estimated():
    return load_pkg().TDD_NOT_ESTIMATED


# ---------------------------------------------------------------- the stage on crafted grids
# (n_id_cell, cp, configuration, DwPTS rows, n_ofdm, ports): two frames, a row count that is no multiple of n_symb, 854 / 732 rows,
# 1 and 4 ports, every n_id_cell mod 6 (the reference signals' frequency shift)
STAGE = [(96, 1, 0, 1, 854, 1), (97, 2, 1, 3, 732, 4), (98, 1, 2, 4, 280, 1), (99, 2, 3, 2, 240, 4), (100, 1, 4, 3, 283, 1), (101, 2, 5, 1, 245, 4),
         (503, 1, 6, 2, 854, 4), (0, 2, 6, 4, 732, 1), (250, 1, 1, 3, 285, 4)]


def _grid(case):
    n_id, cp, cfg, rows, n_ofdm, ports = case
    return TR.crafted_grid(n_id, cp, TR.SUBFRAMES[cfg], TR.DWPTS_OF_ROWS[cp][rows], n_ofdm, seed=1000 + n_id, n_ports=ports, uplink_gain=1.5 if n_ofdm >= 700 else 0.5)


def _cell(pkg, n_id, cp):
    return pkg.new_cell(n_id_1=n_id // 3, n_id_2=n_id % 3, cp_type=cp)


@pytest.mark.parametrize("case", STAGE, ids=[str(c) for c in STAGE])
def test_stage_against_the_numpy_reference(pkg, S, case):
    n_id, cp, cfg, rows, n_ofdm, _ = case
    assert sorted({c[0] % 6 for c in STAGE}) == [0, 1, 2, 3, 4, 5]
    tfg = _grid(case)
    ref = TR.estimate(n_id, cp, tfg)
    got = S.tdd_config(_cell(pkg, n_id, cp), tfg)
    eT, eR = np.abs(np.array(got.T) - ref["T"]).max(), np.abs(np.array(got.R) - ref["R"]).max()
    print(case, "T error %.2e R error %.2e margin error %.2e clearance %.3f" % (eT, eR, abs(got.margin - ref["margin"]), TR.clearance(ref)))
    assert eT <= 1e-9 and eR <= 1e-9 and abs(got.margin - ref["margin"]) <= 1e-9
    assert TR.clearance(ref) >= 1e-6, "the grid is chosen to sit clear of every threshold"
    assert (got.ul_dl_config, got.dwpts_rs_rows) == (ref["ul_dl_config"], ref["dwpts_rs_rows"]) == (cfg, rows)


def test_stage_on_grids_that_get_no_number(pkg, S):
    for tfg in (np.zeros((854, 72), np.complex128), np.full((854, 72), np.nan + 0j)):
        got = S.tdd_config(_cell(pkg, 7, 1), tfg)
        assert (got.ul_dl_config, got.dwpts_rs_rows, got.margin) == (-1, -1, 0.0)
    for kinds in ("DDDDDDDDDD", "DSUDUDSDUU"):      # CRS in subframe 2; a pattern outside the table
        tfg = TR.crafted_grid(7, 2, kinds, 8, 732, seed=4)
        ref, got = TR.estimate(7, 2, tfg), S.tdd_config(_cell(pkg, 7, 2), tfg)
        assert TR.clearance(ref) >= 1e-6
        assert got.ul_dl_config == ref["ul_dl_config"] == -1 and got.dwpts_rs_rows == -1 and abs(got.margin - ref["margin"]) <= 1e-9 and got.margin > 0.05
        assert np.abs(np.array(got.T) - ref["T"]).max() <= 1e-9


def test_stage_works_whatever_the_modes(pkg):
    """the stage needs neither the TDD duplex mode nor the chain's setting, and leaves the last fused call's table alone"""
    case = STAGE[0]
    with pkg.Searcher(0) as s:
        got = s.tdd_config(_cell(pkg, case[0], case[1]), _grid(case))
        assert (got.ul_dl_config, got.dwpts_rs_rows) == (case[2], case[3])


# ---------------------------------------------------------------- refusals
def test_refusals(pkg, S):
    tfg = _grid(STAGE[0])
    for cell, n_ofdm, text in ((pkg.new_cell(n_id_2=1, cp_type=1), 854, "n_id_1, n_id_2 and a known cp_type"),
                               (pkg.new_cell(n_id_1=5, cp_type=1), 854, "n_id_1, n_id_2 and a known cp_type"),
                               (pkg.new_cell(n_id_1=5, n_id_2=1), 854, "n_id_1, n_id_2 and a known cp_type"),
                               (_cell(pkg, 96, 1), 279, "at least two frames"),
                               (_cell(pkg, 96, 2), 239, "at least two frames"),
                               (_cell(pkg, 96, 1), 855, "at most LCS_TFG_MAX_OFDM")):
        g = np.zeros((n_ofdm, 72), np.complex128)
        g[:min(n_ofdm, 854)] = tfg[:min(n_ofdm, 854)]
        with pytest.raises(pkg.SearcherError, match=text):
            S.tdd_config(cell, g)
    with pkg.Searcher(0) as s:
        assert s.tdd_config_mode is False
        with pytest.raises(pkg.SearcherError, match="lcs_search_capbuf or a batch"):
            s.last_tdd_info()
        assert s._lib.lcs_set_tdd_config(s._h, 2) == -2 and b"neither 0 nor 1" in s._lib.lcs_last_error(s._h)
        s.set_tdd_config(True)
        assert s.tdd_config_mode is True
        with pytest.raises(pkg.SearcherError, match="does not carry the uplink-downlink estimate"):
            s.stream_open(pkg.FMT_IQ_U8, 153600, FC, FC, FS)
        s.set_tdd_config(False)
        s.stream_open(pkg.FMT_IQ_U8, 153600, FC, FC, FS)
        with pytest.raises(pkg.SearcherError, match="cannot change under an open stream"):
            s.set_tdd_config(True)
        s.set_tdd_config(False)      # no change: accepted
        s.stream_close()
        s.set_tdd_config(True)


# ---------------------------------------------------------------- the fused chain on planted cells
def _bytes(cells):
    return [bytes(c) for c in cells]


def _check_table(pkg, S, cells, info, cap, want):
    """info[k] belongs to cells[k]: it equals the stage on extract_tfg's grid of that record, field for field, and names the
    planted configuration; the entries behind the cells read NOT_ESTIMATED"""
    assert len(info) == MAXC
    ids = [c.n_id_cell() for c in cells]
    assert set(want) <= set(ids), (ids, want)
    for k, c in enumerate(cells):
        tfg, _ = S.extract_tfg(c, cap, FC, FC, FS)
        stage = S.tdd_config(c, tfg)
        assert _rec(info[k]) == _rec(stage), (k, _rec(info[k]), _rec(stage))
        if c.n_id_cell() in want:
            cfg, rows, cp = want[c.n_id_cell()]
            assert (info[k].ul_dl_config, info[k].dwpts_rs_rows, c.cp_type) == (cfg, rows, cp)
            assert info[k].margin >= 0.1
    for k in range(len(cells), MAXC):
        assert _none(info[k])


@pytest.fixture(scope="module")
def off_single(pkg):
    with _tdd(pkg) as s:
        return [_bytes(s.search_capbuf(K.cap(b), GRID, FC, FC, FS)[0]) for b in range(NB)]


def test_search_capbuf_with_the_mode_on(pkg, S, off_single):
    seen = set()
    for b in range(NB):
        cells, _ = S.search_capbuf(K.cap(b), GRID, FC, FC, FS)
        info = S.last_tdd_info(1, MAXC)[0]
        assert _bytes(cells) == off_single[b], "the records are the mode-off records"
        _check_table(pkg, S, cells, info, K.cap(b), K.planted(b))
        seen |= {info[k].ul_dl_config for k, c in enumerate(cells) if c.n_id_cell() in K.planted(b)}
    assert seen == set(range(7))


def _batch(pkg, s, fmt):
    import torch
    if fmt == pkg.FMT_IQ_U8:
        d = torch.from_numpy(np.stack([K.u8(b) for b in range(NB)])).cuda()
    else:
        d = torch.from_numpy(np.stack([K.cap(b).astype(np.complex64) for b in range(NB)])).cuda()
    cells = s.search_batch(d.data_ptr(), fmt, NB, 153600, GRID, FC, FC, FS, pkg.STAGE_FULL, MAXC)
    del d
    return cells


@pytest.mark.parametrize("fmt", ["u8", "c64"])
def test_batches_with_the_mode_on(pkg, S, fmt):
    f = pkg.FMT_IQ_U8 if fmt == "u8" else pkg.FMT_C64
    with _tdd(pkg) as off:
        ref = _batch(pkg, off, f)
        assert all(_none(t) for row in off.last_tdd_info(NB, MAXC) for t in row)
    cells = _batch(pkg, S, f)
    info = S.last_tdd_info(NB, MAXC)
    for b in range(NB):
        assert _bytes(cells[b]) == _bytes(ref[b]), "the records are the mode-off records"
        _check_table(pkg, S, cells[b], info[b], K.cap(b), K.planted(b))


def test_two_per_cell_rounds_give_the_same_table(pkg, S):
    one = _batch(pkg, S, pkg.FMT_IQ_U8)
    info_one = S.last_tdd_info(NB, MAXC)
    with _tdd(pkg, True) as s:
        s.set_max_cells_in_flight(2)
        two = _batch(pkg, s, pkg.FMT_IQ_U8)
        info_two = s.last_tdd_info(NB, MAXC)
        stats = (C.c_int * 8)()
        assert s._lib.lcs_last_batch_stats(s._h, stats) == 0
        assert stats[5] > 2, "more cells passed SSS than a round holds: the batch ran several per-cell rounds"
    assert sum(len(c) for c in one) >= 7
    for b in range(NB):
        assert _bytes(two[b]) == _bytes(one[b])
        assert [_rec(t) for t in info_two[b]] == [_rec(t) for t in info_one[b]]


def test_mode_off_fdd_and_on_then_off_change_nothing(pkg, off_single):
    g = golden("capbuf_0000")
    fc, f = float(g["fc"][0]), np.array([30e3, 35e3, 40e3])
    fdd_cap = iq_u8_to_capbuf(g["iq_u8"])
    with pkg.Searcher(0) as never, pkg.Searcher(0) as fdd_on:
        fdd_on.set_tdd_config(True)
        a, b = never.search_capbuf(fdd_cap, f, fc, fc, FS), fdd_on.search_capbuf(fdd_cap, f, fc, fc, FS)
        assert [c.n_id_cell() for c in a[0]] == [277, 271]
        assert _bytes(a[0]) == _bytes(b[0]) and _bytes(a[1]) == _bytes(b[1])
        assert all(_none(t) for t in fdd_on.last_tdd_info(1, MAXC)[0]) and all(_none(t) for t in never.last_tdd_info(1, MAXC)[0])
    with _tdd(pkg, False) as off, _tdd(pkg, True) as flip:
        x = flip.search_capbuf(K.cap(2), GRID, FC, FC, FS)[0]
        assert not all(_none(t) for t in flip.last_tdd_info(1, MAXC)[0])
        flip.set_tdd_config(False)
        for s in (off, flip):
            cells = s.search_capbuf(K.cap(2), GRID, FC, FC, FS)[0]
            assert _bytes(cells) == off_single[2] == _bytes(x)
            assert all(_none(t) for t in s.last_tdd_info(1, MAXC)[0])
            batch = _batch(pkg, s, pkg.FMT_IQ_U8)
            assert all(_none(t) for row in s.last_tdd_info(NB, MAXC) for t in row)
            assert _bytes(batch[2]) == _bytes(_batch(pkg, off, pkg.FMT_IQ_U8)[2])
