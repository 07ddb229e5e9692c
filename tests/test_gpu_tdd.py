"""GPU tests of the duplex mode (lcs_set_duplex): SSS detection and the PSS/SSS frequency estimate for TDD cells (36.211 frame
structure type 2), through every entry point that runs them.

The CPU oracle is FDD only.  The reference for the two stages is tests/sss_duplex_ref.py -- the numpy restatement that
test_sss_duplex_ref.py pins to the oracle in FDD -- run with the TDD geometry; everything behind the two stages is the oracle's.
The bars are those tests/test_gpu_cells.py holds the FDD stages and chain to against the oracle: 1e-9 of an array's largest
magnitude, frame_start to 1e-9 samples and freq_fine to 1e-6 Hz stage by stage; frame_start to 1e-6 and the frequencies to
1e-3 Hz through the fused chain.  The arithmetic is the same; only window positions differ."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle as O
import sss_duplex_ref as R
from conftest import ROOT, golden, iq_u8_to_capbuf, load_pkg

pytestmark = pytest.mark.gpu
FS = 1.92e6
FC = 1.9e9            # band 39
GRID = np.arange(-5e3, 5e3 + 1, 2.5e3)
TDD = R.GEO["tdd"]
BASE = dict(n_id_1=77, n_id_2=2, cp_normal=True, n_ports=2, n_rb_dl=25, sfn0=500, f_off=300.0, tdd=(2, 10))
INT_FIELDS = ("ind", "n_id_2", "n_id_1", "cp_type", "n_ports", "n_rb_dl", "phich_duration", "phich_resource", "sfn")


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module", autouse=True)
def _oracle_mode():
    O.set_legacy(False)
    O.set_threads(min(16, os.cpu_count() or 1))


@pytest.fixture(scope="module")
def T(pkg):
    """a searcher set to TDD"""
    s = pkg.Searcher(0)
    s.set_duplex(pkg.DUPLEX_TDD)
    yield s
    s.close()


def _t0(peak, cp_normal, half=0):
    """the timing that puts the peak of a PSS occurrence (the start of its cyclic prefix) at sample `peak`"""
    P = 2204 if cp_normal else 2272
    return float((P - (peak + 9) + 9600 * half) % 19200)


def _cell(**kw):
    c = dict(BASE)
    c.update(kw)
    return c


_cache = {}


def _u8(pkg, seed, cells, snr=8.0, n_cap=153600):
    key = (seed, repr(cells), snr, n_cap)
    if key not in _cache:
        _cache[key] = pkg.synth.make_capbuf(seed, FC, cells, snr_db=snr, n_cap=n_cap)[0]
    return _cache[key]


def _close(a, b, rtol=1e-9):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() <= rtol * np.abs(b).max()


# ---------------------------------------------------------------- 3. stage parity
# (id, n_cap, cell keys, the peak record's ind, its freq, occurrences the range rule leaves, moved by the TDD room rule)
STAGE_SHAPES = [
    ("normal CP, 80 ms", 153600, dict(t0=_t0(5000, True)), 5000, 0.0, 16, False),
    ("extended CP, 80 ms", 153600, dict(cp_normal=False, tdd=(1, 9), t0=_t0(7000, False)), 7000, 0.0, 16, False),
    ("24000 samples, three occurrences", 24000, dict(t0=_t0(2000, True)), 2000, 0.0, 3, False),
    ("24000 samples, two occurrences, hypothesis 2500 Hz", 24000, dict(t0=_t0(6000, True), f_off=2200.0), 6000, 2500.0, 2, False),
    ("peak at 95: moved in both modes", 24000, dict(t0=_t0(95, True)), 95, 0.0, 2, True),
    ("peak at 300: moved in TDD only", 24000, dict(t0=_t0(300, True)), 300, 0.0, 2, True),
    ("peak at 472: moved in TDD only", 24000, dict(cp_normal=False, tdd=(0, 3), t0=_t0(472, False)), 472, 0.0, 2, True),
    ("peak at 473: not moved", 24000, dict(cp_normal=False, tdd=(0, 3), t0=_t0(473, False)), 473, 0.0, 3, False),
    ("late peak: the last occurrence is cut by the range rule", 24000, dict(t0=_t0(4700, True)), 4700, 0.0, 2, False),
]


@pytest.mark.parametrize("name, n_cap, keys, ind, freq, n_occ, moved", STAGE_SHAPES, ids=[s[0] for s in STAGE_SHAPES])
def test_stage_parity_in_tdd_mode(pkg, T, name, n_cap, keys, ind, freq, n_occ, moved):
    cell = _cell(**keys)
    cap = iq_u8_to_capbuf(_u8(pkg, 21, [cell], snr=15.0, n_cap=n_cap))
    kw = dict(pss_pow=1.0, ind=ind, freq=freq, n_id_2=cell["n_id_2"], fc_requested=FC, fc_programmed=FC)
    peak_loc, _, n_pss = R.sss_geometry(O.new_cell(**kw), n_cap, FC, FC, TDD)
    assert n_pss == n_occ and (peak_loc != ind) == moved
    assert (R.sss_geometry(O.new_cell(**kw), n_cap, FC, FC, R.GEO["fdd"])[0] != ind) == (ind + 9 < 162)
    cr, dr = R.sss_detect(O.new_cell(**kw), cap, 3.0, FC, FC, FS, TDD)
    cg, dg = T.sss_detect(pkg.new_cell(**kw), cap, 3.0, FC, FC, FS)
    worst = {}
    for k in ("h1_np", "h2_np", "h1_nrm", "h2_nrm", "h1_ext", "h2_ext", "ll_nrm", "ll_ext"):
        worst[k] = np.abs(dg[k] - dr[k]).max() / np.abs(dr[k]).max()
    print("worst relative errors:", {k: float("%.2e" % v) for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 1e-9, (k, v)
    assert (cg.n_id_1, cg.cp_type) == (cr.n_id_1, cr.cp_type)
    assert (cr.n_id_1, cr.cp_type) == (cell["n_id_1"], 1 if cell["cp_normal"] else 2), "the planted cell is what both find"
    assert abs(cg.frame_start - cr.frame_start) < 1e-9, (cg.frame_start, cr.frame_start)
    planted = (-cell["t0"]) % 19200 - 2
    assert abs((cr.frame_start - planted + 9600) % 19200 - 9600) <= 1.0
    fr = R.pss_sss_foe(cr, cap, FC, FC, FS, TDD)
    fg = T.pss_sss_foe(cg, cap, FC, FC, FS)
    print("frame_start", cg.frame_start - cr.frame_start, "freq_fine", fg.freq_fine - fr.freq_fine)
    assert abs(fg.freq_fine - fr.freq_fine) < 1e-6, (fg.freq_fine, fr.freq_fine)
    assert abs(fr.freq_fine - cell["f_off"]) < 150.0


# ---------------------------------------------------------------- 4. the chain
def _six(pkg):
    rng = np.random.default_rng(8)
    empty = np.clip(np.rint(rng.normal(127.0, 19.0, 2 * 153600)), 0, 255).astype(np.uint8)
    return [
        _u8(pkg, 31, [_cell(t0=5000.0)]),
        _u8(pkg, 32, [_cell(cp_normal=False, tdd=(0, 3), n_id_1=12, n_id_2=0, n_ports=4, t0=7777.0)]),
        _u8(pkg, 33, [_cell(t0=_t0(300, True), n_id_1=150, n_id_2=1, n_ports=1, f_off=-900.0)]),      # moved by the room rule
        _u8(pkg, 34, [_cell(t0=3000.0, tdd=(1, 9)), _cell(t0=11111.0, n_id_1=3, n_id_2=0, tdd=(5, 11), f_off=-2700.0, gain_db=-2.0)]),
        empty,
        _u8(pkg, 36, [_cell(tdd=None, t0=4000.0)]),                                                     # an FDD cell
    ]


def _key(c):
    return tuple(getattr(c, k) for k in INT_FIELDS)


def _cells_match(got, exp):
    assert [_key(c) for c in got] == [_key(c) for c in exp], ([_key(c) for c in got], [_key(c) for c in exp])
    for a, b in zip(got, exp):
        assert a.freq == b.freq
        assert abs(a.frame_start - b.frame_start) < 1e-6, (a.frame_start, b.frame_start)
        assert abs(a.freq_fine - b.freq_fine) < 1e-3 and abs(a.freq_superfine - b.freq_superfine) < 1e-3


@pytest.fixture(scope="module")
def chain(pkg, T):
    """the six buffers one by one (search_capbuf) with the reference run on the GPU's own peak lists"""
    import torch
    bufs = _six(pkg)
    single, ref = [], []
    for b in bufs:
        cap = iq_u8_to_capbuf(b)
        cells, peaks = T.search_capbuf(cap, GRID, FC, FC, FS)
        single.append(cells)
        ref.append(R.search_peaks(peaks, cap, FC, FC, FS, TDD))
    d = torch.from_numpy(np.stack(bufs)).cuda()
    batch = T.search_batch(d.data_ptr(), pkg.FMT_IQ_U8, 6, 153600, GRID, FC, FC, FS, pkg.STAGE_FULL)
    return dict(single=single, ref=ref, batch=batch)


def test_chain_in_tdd_mode_single_buffers(chain):
    for b in range(6):
        _cells_match(chain["single"][b], chain["ref"][b])
    ids = [[c.n_id_cell() for c in r] for r in chain["ref"]]
    assert ids[0] == [77 * 3 + 2] and ids[1] == [12 * 3] and ids[2] == [150 * 3 + 1] and sorted(ids[3]) == sorted([77 * 3 + 2, 3 * 3]) and ids[4] == []
    assert [c.cp_type for c in chain["ref"][1]] == [2] and [c.n_ports for c in chain["ref"][1]] == [4]


def test_chain_in_tdd_mode_batch_equals_single(chain):
    """The batch runs the same kernels; its timing estimate sums over two workgroups per cell where the single buffer's sums over
    four (Launch::tfoec_parts), so the continuous fields are held to the chain's bars and everything else is equal."""
    for b in range(6):
        _cells_match(chain["batch"][b], chain["ref"][b])
        _cells_match(chain["batch"][b], chain["single"][b])


# ---------------------------------------------------------------- 5. mode hygiene
def _golden_run(pkg, s):
    import torch
    g = golden("capbuf_0000")
    fc = float(g["fc"][0])
    f = np.array([30e3, 35e3, 40e3])
    cells, peaks = s.search_capbuf(iq_u8_to_capbuf(g["iq_u8"]), f, fc, fc, FS)
    d = torch.from_numpy(np.ascontiguousarray(g["iq_u8"])).cuda()
    batch = s.search_batch(d.data_ptr(), pkg.FMT_IQ_U8, 1, 153600, f, fc, fc, FS, pkg.STAGE_FULL)[0]
    rb = s.batch_readback(0, 3)
    return [bytes(c) for c in cells], [bytes(c) for c in peaks], [bytes(c) for c in batch], rb, [c.n_id_cell() for c in cells]


def test_default_is_fdd_and_a_round_trip_changes_nothing(pkg):
    with pkg.Searcher(0) as fresh, pkg.Searcher(0) as s:
        assert fresh.duplex == pkg.DUPLEX_FDD == 0 and pkg.DUPLEX_TDD == 1
        s.set_duplex(pkg.DUPLEX_TDD)
        assert s.duplex == pkg.DUPLEX_TDD
        s.set_duplex(pkg.DUPLEX_FDD)
        assert s.duplex == pkg.DUPLEX_FDD
        a, b = _golden_run(pkg, fresh), _golden_run(pkg, s)
        assert a[4] == [277, 271]
        assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]
        for k in a[3]:
            assert np.array_equal(a[3][k], b[3][k]), k


def test_bad_values_and_an_open_stream_refuse_the_setter(pkg):
    with pkg.Searcher(0) as s:
        for bad in (2, -1, 7):
            with pytest.raises(pkg.SearcherError, match="LCS_ERR_BAD_ARG.*duplex"):
                s.set_duplex(bad)
        assert s.duplex == pkg.DUPLEX_FDD
        s.stream_open(pkg.FMT_IQ_U8, 153600, FC, FC, FS)
        with pytest.raises(pkg.SearcherError, match="LCS_ERR_BAD_ARG.*stream"):
            s.set_duplex(pkg.DUPLEX_TDD)
        assert s.duplex == pkg.DUPLEX_FDD
        s.stream_close()
        s.set_duplex(pkg.DUPLEX_TDD)
        assert s.duplex == pkg.DUPLEX_TDD


def test_two_contexts_keep_their_own_modes(pkg, chain):
    cap = iq_u8_to_capbuf(_six(pkg)[0])
    with pkg.Searcher(0) as t, pkg.Searcher(0) as f:
        t.set_duplex(pkg.DUPLEX_TDD)
        for _ in range(2):
            ct, _ = t.search_capbuf(cap, GRID, FC, FC, FS)
            cf, _ = f.search_capbuf(cap, GRID, FC, FC, FS)
            assert [bytes(c) for c in ct] == [bytes(c) for c in chain["single"][0]] and len(ct) == 1
            assert [c.n_id_cell() for c in cf] == []          # FDD reads the wrong window: the TDD cell is not found
        assert (t.duplex, f.duplex) == (pkg.DUPLEX_TDD, pkg.DUPLEX_FDD)
        assert _golden_run(pkg, f)[4] == [277, 271]


# ---------------------------------------------------------------- 6. streaming mode and the hypothesis split
def test_streaming_mode_and_hypothesis_split_in_tdd_mode(pkg, chain):
    buf = _six(pkg)[0]
    want = chain["ref"][0]
    with pkg.Searcher(0) as s:
        s.set_duplex(pkg.DUPLEX_TDD)
        s.stream_open(pkg.FMT_IQ_U8, 153600, FC, FC, FS)
        s.stream_push(buf, 0.0)
        cells, dup, _ = s.stream_collect()
        s.stream_close()
        assert dup == 0 and [c.n_id_cell() for c in cells] == [c.n_id_cell() for c in want] == [77 * 3 + 2]
        assert (cells[0].cp_type, cells[0].n_ports, cells[0].n_rb_dl, cells[0].sfn) == (want[0].cp_type, want[0].n_ports, want[0].n_rb_dl, want[0].sfn)
        assert abs(cells[0].frame_start - want[0].frame_start) < 1e-6 and abs(cells[0].freq_superfine - want[0].freq_superfine) < 1e-3
        got, _ = pkg.sweep.search_capbuf_foe_split_dev(s, iq_u8_to_capbuf(buf), GRID, FC, FC, FS)
        assert [(c["n_id_1"], c["n_id_2"], c["cp_type"], c["n_ports"], c["n_rb_dl"], c["sfn"]) for c in got] == \
               [(c.n_id_1, c.n_id_2, c.cp_type, c.n_ports, c.n_rb_dl, c.sfn) for c in want]
        assert abs(got[0]["frame_start"] - want[0].frame_start) < 1e-6 and abs(got[0]["freq_superfine"] - want[0].freq_superfine) < 1e-3


# ---------------------------------------------------------------- 7. CLI
def test_cellsearch_x_tdd(pkg, tmp_path):
    exe = os.path.join(ROOT, "host", "CellSearch")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    h = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "-x --duplex fdd|tdd" in h
    pkg.itfile.write_it(str(tmp_path / "capbuf_0000.it"), {"capbuf": iq_u8_to_capbuf(_six(pkg)[0]), "fc": np.array([int(FC)], np.int32)})
    r = subprocess.run([exe, "-s", str(int(FC)), "-p", "2", "-x", "tdd", "-l", "-d", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert re.search(r"cell.ID..%d\b" % (77 * 3 + 2), r.stdout), r.stdout
    r = subprocess.run([exe, "-s", str(int(FC)), "-p", "2", "-l", "-d", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "No LTE cells were found..." in r.stdout          # the default stays FDD


# ---------------------------------------------------------------- band search from one wideband capture
def test_band_search_over_a_wideband_capture_with_tdd_cells(pkg, T):
    import torch
    decim, fc_centre = 4, 1.9e9
    carriers = np.array([fc_centre - 1.5e6, fc_centre + 1.2e6])
    placed = [(carriers[0], [_cell(t0=6000.0, f_off=-800.0)]), (carriers[1], [_cell(n_id_1=100, n_id_2=1, cp_normal=False, tdd=(6, 8), t0=900.0, f_off=1100.0)])]
    iq, _ = pkg.synth.make_wideband(51, fc_centre, decim, placed, snr_db=10.0, fmt=pkg.FMT_IQ_S16)
    d = torch.from_numpy(iq).cuda()
    grid = pkg.f_search_set_for(fc_centre, 2, step=2.5e3)
    assert np.array_equal(grid, GRID)
    got = pkg.sweep.search_wideband(T, d.data_ptr(), pkg.FMT_IQ_S16, iq.size // 2, FS * decim, decim, fc_centre, carriers, grid)
    assert [[(c.n_id_cell(), c.cp_type) for c in g] for g in got] == [[(77 * 3 + 2, 1)], [(100 * 3 + 1, 2)]]
    assert abs(got[0][0].freq_superfine + 800.0) < 100.0 and abs(got[1][0].freq_superfine - 1100.0) < 100.0
    with pkg.Searcher(0) as fdd:
        none = pkg.sweep.search_wideband(fdd, d.data_ptr(), pkg.FMT_IQ_S16, iq.size // 2, FS * decim, decim, fc_centre, carriers, grid)
    assert none == [[], []]
