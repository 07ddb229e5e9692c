"""GPU tests of the PCFICH stage (lcs_pcfich_wide, lcs_pcfich; k_pcfich, k_pcfich_fin).

The stage on crafted grids against the numpy statement of the rule (tests/pcfich_ref.py): corr and margin to 1e-9, the project's bar
for a device fp64 stage against numpy; decisions and summary equal; the record bit-equal to the host twin
(tests/host/pcfich_host.cpp) on the same grid.  From samples: captures with the generator's PCFICH in them (three frames, 20 dB) read
the planted value in every decoded subframe, and the record is lcs_pcfich's on lcs_extract_tfg_wide's grid of the same call, field
for field.  Refusals, isolation from the chain and the stream, and sweep.measure_wideband(pcfich=True)."""
import ctypes as C

import numpy as np
import pytest

import cell_meas_cases as CS
import meas_wide_cases as WC
import pcfich_cases as PC
import pcfich_ref as PR
from conftest import load_pkg

pytestmark = pytest.mark.gpu
FS = 1.92e6
FC = WC.FC
# (R, n_rb, CP type, ports, mask) from samples: the issue's four shapes, extended CP at (2, 15), four ports at (4, 25)
SAMPLE_CASES = [(1, 6, 1, 1, 0x3FF), (2, 15, 2, 2, 0x3FF), (4, 25, 1, 4, 0x339), (16, 100, 1, 2, 0x3FF)]


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
    return PC.load_twin(pkg.capi)


_dev = {}


def dev(R, n_rb, cp, n_ports):
    import torch
    key = (R, n_rb, cp, n_ports)
    if key not in _dev:
        _dev[key] = torch.from_numpy(PC.pcfich_capture(*key)).cuda()
    return _dev[key]


def _cell(pkg, cp, R, n_ports, n_rb_dl=-1, **kw):
    c = pkg.new_cell(n_id_1=WC.CELL_ID[0], n_id_2=WC.CELL_ID[1], cp_type=cp, n_ports=n_ports, freq_fine=kw.pop("freq_fine", 0.0),
                     frame_start=kw.pop("frame_start", WC.FRAME_START * R), **kw)
    c.n_rb_dl = n_rb_dl
    return c


# ---------------------------------------------------------------- the stage on crafted grids
@pytest.mark.parametrize("shape", PC.SHAPES, ids=[str(s) for s in PC.SHAPES])
def test_stage_against_numpy_and_the_host_twin_on_crafted_grids(pkg, S, H, shape):
    n_rb, cp = shape
    worst = 0.0
    for n_id, n_ports, mask, tfg, planted in PC.crafted_cases(n_rb, cp):
        what = (shape, n_id, n_ports, hex(mask), tfg.shape[0])
        cell = pkg.new_cell(n_id_1=n_id // 3, n_id_2=n_id % 3, cp_type=cp, n_ports=n_ports)
        got = S.pcfich(cell, tfg, n_rb, mask)
        ref = PR.decode(tfg, n_id, cp, n_ports, n_rb, mask)
        assert ref["min_margin"] >= 1e-6 and ref["n_decoded"] > 0, what
        worst = max(worst, PR.assert_record_close(got, ref, 1e-9, what))
        twin = PC.twin_record(H, pkg.capi, n_id, cp, tfg, n_rb, n_ports, mask)
        assert bytes(got) == bytes(twin), (what, np.flatnonzero(np.frombuffer(bytes(got), np.uint8) != np.frombuffer(bytes(twin), np.uint8))[:8])
        dec = got.cfi > 0
        assert np.array_equal(got.cfi[dec], planted[dec]), what
    print(shape, "worst |device - numpy| %.2e" % worst)


def test_grids_without_a_decision(pkg, S, H):
    cell = pkg.new_cell(n_id_1=2, n_id_2=1, cp_type=1, n_ports=4)
    for tfg in (np.zeros((40, 300), np.complex128), np.full((40, 300), np.nan + 0j)):
        got = S.pcfich(cell, tfg, 25)
        assert (got.n_sf, got.n_decoded, got.mean_n_ctrl_sym, got.min_margin) == (3, 0, 0.0, 0.0) and not got.cfi.any()
        assert bytes(got) == bytes(PC.twin_record(H, pkg.capi, 7, 1, tfg, 25, 4, 0x3FF))
    # a mask whose subframe the grid does not reach: no row is read
    got = S.pcfich(cell, np.ones((14, 300), np.complex128), 25, 0x200)
    assert (got.n_sf, got.n_decoded, got.dl_mask) == (1, 0, 0x200)


# ---------------------------------------------------------------- from samples
@pytest.mark.parametrize("case", SAMPLE_CASES, ids=[str(c[:4]) for c in SAMPLE_CASES])
def test_from_samples_reads_the_planted_cfi_and_equals_the_stage_on_the_extracted_grid(pkg, S, case):
    R, n_rb, cp, n_ports, mask = case
    n = PR.n_symb_of(cp)
    n_ofdm = 50 * n + 3                                       # two and a half frames and the head of a subframe
    d = dev(R, n_rb, cp, n_ports)
    cell = _cell(pkg, cp, R, n_ports, n_rb_dl=n_rb)
    got = S.pcfich_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm, mask)
    want = np.array([(mask >> (g % 10)) & 1 for g in range(26)], bool)
    assert got.n_sf == 26 and got.n_decoded == want.sum() and np.array_equal(got.cfi > 0, want)
    planted = PC.planted_of_grid(26)
    print(case, "margins %.3f .. %.3f" % (got.margin[want].min(), got.margin[want].max()))
    assert np.array_equal(got.cfi[want], planted[want]), (got.cfi, planted)
    assert (got.dl_mask, got.n_rb, got.n_ports) == (mask, n_rb, n_ports) and list(got.n_cfi) == [int((planted[want] == c).sum()) for c in (1, 2, 3)]
    assert got.min_margin == got.margin[want].min() > 0.2
    tfg, _ = S.extract_tfg_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm)
    again = S.pcfich(cell, tfg, n_rb, mask)
    assert bytes(got) == bytes(again)
    # a frequency offset and a grid of one subframe
    off = _cell(pkg, cp, R, n_ports, freq_fine=137.0)
    one = S.pcfich_wide(off, d, FC, FC, FS * R, 128 * R, n_rb, 2 * n, 0x001)
    tfg1, _ = S.extract_tfg_wide(off, d, FC, FC, FS * R, 128 * R, n_rb, 2 * n)
    assert (one.n_sf, one.n_decoded) == (1, 1) and bytes(one) == bytes(S.pcfich(off, tfg1, n_rb, 0x001))


# ---------------------------------------------------------------- refusals
def test_refusals_launch_nothing_and_leave_the_context_usable(pkg, S):
    R, n_rb, cp, n_ports = 2, 15, 2, 2
    d = dev(R, n_rb, cp, n_ports)
    n = d.numel()
    ok = dict(cell=_cell(pkg, cp, R, n_ports), ptr=d.data_ptr(), n_cap=n, fs=FS * R, n_fft=256, n_rb=15, n_ofdm=240, mask=0x3FF)
    before = S.pcfich_wide(ok["cell"], d, FC, FC, FS * R, 256, 15, 240)
    assert before.n_decoded == 20
    cases = [(dict(ptr=0), "null pointer"), (dict(ptr=d.data_ptr() + 4), "not aligned"),
             (dict(n_fft=384), "n_fft is not"), (dict(n_fft=4096), "n_fft is not"),
             (dict(fs=FS * R * 1.0011), "15 kHz x n_fft"), (dict(fs=float("nan")), "15 kHz x n_fft"),
             (dict(n_rb=5), "n_rb is outside"), (dict(n_rb=25), "n_rb is outside"), (dict(n_fft=2048, fs=FS * 16, n_rb=101), "n_rb is outside"),
             (dict(n_rb=10), "not an LTE bandwidth"), (dict(n_rb=14), "not an LTE bandwidth"),
             (dict(n_rb=6), "contradicts the cell's n_rb_dl"), (dict(cell=_cell(pkg, cp, R, n_ports, n_rb_dl=25)), "contradicts the cell's n_rb_dl"),
             (dict(n_ofdm=11), "n_ofdm is outside"), (dict(n_ofdm=122 * 6 + 1), "n_ofdm is outside"),
             (dict(mask=0), "dl_mask"), (dict(mask=0x400), "dl_mask"), (dict(mask=-1), "dl_mask"),
             (dict(cell=pkg.new_cell(n_id_2=1, cp_type=cp)), "n_id_1, n_id_2 and a known cp_type"),
             (dict(cell=pkg.new_cell(n_id_1=5, n_id_2=1)), "n_id_1, n_id_2 and a known cp_type"),
             (dict(n_cap=int(ok["cell"].frame_start) + 19200 * R), "does not hold the last requested row"),
             (dict(cell=_cell(pkg, cp, R, n_ports, frame_start=-40.0 * R)), "before sample 0"),
             (dict(cell=_cell(pkg, cp, R, n_ports, frame_start=float("nan"))), "no finite positions")]
    known = _cell(pkg, cp, R, n_ports, n_rb_dl=15)
    for change, text in cases:
        a = dict(ok, **change)
        if change.get("n_rb") == 6:
            a["cell"] = known
        with pytest.raises(pkg.SearcherError, match=text):
            S.pcfich_wide(a["cell"], a["ptr"], FC, FC, a["fs"], a["n_fft"], a["n_rb"], a["n_ofdm"], a["mask"], n_cap=a["n_cap"])
    # the stage on a host grid
    grid = np.ones((240, 180), np.complex128)
    host_cases = [(dict(n_rb=10, grid=np.ones((240, 120), np.complex128)), "not an LTE bandwidth"), (dict(cell=known, n_rb=25, grid=np.ones((240, 300), np.complex128)), "contradicts the cell's n_rb_dl"),
                  (dict(grid=grid[:11]), "n_ofdm is outside"), (dict(grid=np.ones((733, 180), np.complex128)), "n_ofdm is outside"),
                  (dict(mask=0), "dl_mask"), (dict(mask=0x400), "dl_mask"),
                  (dict(cell=pkg.new_cell(n_id_1=5, cp_type=cp)), "n_id_1, n_id_2 and a known cp_type")]
    for change, text in host_cases:
        a = dict(dict(cell=ok["cell"], grid=grid, n_rb=15, mask=0x3FF), **change)
        with pytest.raises(pkg.SearcherError, match=text):
            S.pcfich(a["cell"], a["grid"], a["n_rb"], a["mask"])
    with pytest.raises(ValueError):
        S.pcfich(ok["cell"], grid, 25)                        # the grid's width is not 12 n_rb
    # null pointers through the C ABI
    lib, cell, rec = S._lib, ok["cell"], pkg.PcfichInfo()
    assert lib.lcs_pcfich_wide(S._h, C.byref(cell), C.c_void_p(d.data_ptr()), n, FC, FC, FS * R, 256, 15, 240, 0x3FF, None) == -2
    assert lib.lcs_pcfich_wide(S._h, None, C.c_void_p(d.data_ptr()), n, FC, FC, FS * R, 256, 15, 240, 0x3FF, C.byref(rec)) == -2
    assert b"null pointer" in lib.lcs_last_error(S._h)
    assert lib.lcs_pcfich(S._h, C.byref(cell), None, 240, 15, 0x3FF, C.byref(rec)) == -2
    assert lib.lcs_pcfich(S._h, C.byref(cell), grid.ctypes.data_as(C.POINTER(C.c_double)), 240, 15, 0x3FF, None) == -2
    assert b"lcs_pcfich: a null pointer" in lib.lcs_last_error(S._h)
    # one whole subframe is enough
    assert S.pcfich_wide(ok["cell"], d, FC, FC, FS * R, 256, 15, 12).n_decoded == 1
    after = S.pcfich_wide(ok["cell"], d, FC, FC, FS * R, 256, 15, 240)
    assert bytes(after) == bytes(before)


# ---------------------------------------------------------------- modes, the last fused call's tables, an open stream
def test_the_chain_and_an_open_stream_are_left_alone(pkg):
    R, n_rb, cp, n_ports = 4, 25, 1, 4
    d = dev(R, n_rb, cp, n_ports)
    cell = _cell(pkg, cp, R, n_ports)
    args = (cell, d, FC, FC, FS * R, 512, 25, 283, 0x339)
    batch = lambda s: s.search_capbuf(CS.cap(1), CS.GRID, CS.FC, CS.FC, FS)[0]
    table = lambda s: [bytes(t) for t in s.last_cell_meas(1, 16)[0]]
    with pkg.Searcher(0) as s:              # a context that never calls the stage
        s.set_cell_meas(True)
        want_cells = [bytes(c) for c in batch(s)]
        want_table = table(s)
        want_next = [bytes(c) for c in batch(s)]
        assert len(want_cells) >= 1 and s.last_cell_meas(1, 16)[0][0].status == 0 and table(s) == want_table
    with pkg.Searcher(0) as s:
        plain = s.pcfich_wide(*args)
        assert plain.n_decoded > 0
        s.set_cell_meas(True)
        assert [bytes(c) for c in batch(s)] == want_cells and table(s) == want_table
        assert bytes(s.pcfich_wide(*args)) == bytes(plain) and s.cell_meas_mode is True
        tfg, _ = s.extract_tfg_wide(*args[:-1])
        assert bytes(s.pcfich(cell, tfg, 25, 0x339)) == bytes(plain)
        assert table(s) == want_table
        assert [bytes(c) for c in batch(s)] == want_next and table(s) == want_table
    with pkg.Searcher(0) as s:
        s.stream_open(pkg.FMT_IQ_U8, 153600, CS.FC, CS.FC, FS)
        assert bytes(s.pcfich_wide(*args)) == bytes(plain)
        s.stream_close()
        assert bytes(s.pcfich_wide(*args)) == bytes(plain)


# ---------------------------------------------------------------- the sweep
def test_measure_wideband_reads_the_planted_pattern_from_the_measurement_s_buffer(pkg):
    import torch
    K, fc = 8, 1.8425e9
    wide = dict(n_id_1=52, n_id_2=1, n_ports=2, port_gains=[1.0, 0.7j], f_off=1200.0, t0=4321.0, sfn0=8)
    x, _, _ = pkg.synth.make_wideband_cell(11, fc, K, [(fc, 4, 25, wide)], snr_db=20.0, n_in=153600 * K, cfi=PC.planted_cfi)
    d = torch.from_numpy(x).cuda()
    carriers = np.array([fc])
    with pkg.Searcher(0) as s:
        cells = pkg.sweep.search_wideband(s, d.data_ptr(), pkg.FMT_C64, x.size, FS * K, K, fc, carriers, np.array([-5e3, 0.0, 5e3]), n_out=153584, meas=True)
        big = [c for c in cells[0] if c["n_id_cell"] == 52 * 3 + 1 and c["n_rb_dl"] == 25]
        assert len(big) == 1, [(c["n_id_cell"], c["n_rb_dl"]) for c in cells[0]]
        calls = []
        chan = s.channelize
        s.channelize = lambda *a, **k: (calls.append(a), chan(*a, **k))[1]
        today = pkg.sweep.measure_wideband(s, d.data_ptr(), pkg.FMT_C64, x.size, FS * K, fc, K, cells, carriers)
        assert all("pcfich" not in c for c in cells[0])
        n_today = len(calls)
        both = pkg.sweep.measure_wideband(s, d.data_ptr(), pkg.FMT_C64, x.size, FS * K, fc, K, cells, carriers, pcfich=True)
        assert len(calls) == 2 * n_today                     # the PCFICH reads the measurement's buffer: no channelizer call of its own
        del s.channelize
    for c, t, b in zip(cells[0], today[0], both[0]):
        if c["n_rb_dl"] == -1:
            assert t is None and b is None and "pcfich" not in c
            continue
        assert isinstance(t, pkg.CellMeasWide) and bytes(b[0]) == bytes(t) and b[0] is c["meas_wide"] and b[1] is c["pcfich"]
    rec = big[0]["pcfich"]
    dec = rec.cfi > 0
    print("sweep: %d subframes, margins %.3f .. %.3f" % (rec.n_decoded, rec.margin[dec].min(), rec.margin[dec].max()))
    assert rec.n_sf == 61 and rec.n_decoded == 61 and rec.n_rb == 25 and rec.n_ports == 2
    assert np.array_equal(rec.cfi, PC.planted_of_grid(61))
    # the cell's own bandwidth or nothing
    with pkg.Searcher(0) as s:
        narrow = pkg.sweep.measure_wideband(s, d.data_ptr(), pkg.FMT_C64, x.size, FS * K, fc, K, cells, carriers, n_rb=6, pcfich=True)
    assert all(b is None or (b[0].n_rb == 6 and b[1] is None) for b in narrow[0])
