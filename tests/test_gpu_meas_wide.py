"""GPU tests of the full-bandwidth grid and measurement (lcs_extract_tfg_wide, lcs_cell_meas_wide; k_tfg_wide, k_cell_meas_wide,
k_cell_meas_wide_fin).

The grid stage against the numpy reference (tests/meas_wide_ref.py) at every transform length, with a frequency offset of several
subcarriers and a fractional frame_start: 1e-10 of the grid's largest magnitude, the bar tests/test_gpu_cells.py holds
lcs_extract_tfg to; timestamps equal.  The measurement against the same reference: 1e-9 of scale, the project's bar for a device fp64
stage against numpy.  Against the host twin (tests/host/meas_wide_host.cpp) on the device's own grid: every double bit-equal.  The
anchor: at 128 points on the golden capture the stage agrees with lcs_cell_meas on lcs_extract_tfg's grid."""
import ctypes as C

import numpy as np
import pytest

import cell_meas_cases as CS
import meas_wide_cases as WC
import meas_wide_ref as WR
import tdd_config_ref as TR
from conftest import load_pkg

pytestmark = pytest.mark.gpu
FS = 1.92e6
FC = WC.FC
N_ID = WC.CELL_ID[1] + 3 * WC.CELL_ID[0]


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
    return WC.load_twin(pkg.capi)


_dev = {}


def dev(R, cp):
    """the test capture of that rate and CP type on the device (uploaded once)"""
    import torch
    if (R, cp) not in _dev:
        _dev[(R, cp)] = torch.from_numpy(WC.cell_capture(R, cp)).cuda()
    return _dev[(R, cp)]


def _cell(pkg, cp, R, freq_fine=0.0, n_ports=2, frame_start=None):
    return pkg.new_cell(n_id_1=WC.CELL_ID[0], n_id_2=WC.CELL_ID[1], cp_type=cp, n_ports=n_ports, freq_fine=freq_fine,
                        frame_start=WC.FRAME_START * R if frame_start is None else frame_start)


def _doubles(r):
    return bytes(r)[32:]


# ---------------------------------------------------------------- the grid stage
@pytest.mark.parametrize("shape", WC.SHAPES, ids=[str(s) for s in WC.SHAPES])
def test_grid_against_the_numpy_reference(pkg, S, shape):
    R, n_rb = shape
    cp = WC.CP_OF[shape]
    n_ofdm = 40 * TR.n_symb_of(cp)
    f_off = 3.3 * 15e3                                      # several subcarriers
    cell = _cell(pkg, cp, R, f_off)
    tfg, ts = S.extract_tfg_wide(cell, dev(R, cp), FC, FC, FS * R, 128 * R, n_rb, n_ofdm)
    ref, ts_ref = WR.grid(WC.cell_capture(R, cp), cell.frame_start, f_off, cp, FC, FC, FS * R, 128 * R, n_rb, n_ofdm)
    assert tfg.shape == (n_ofdm, 12 * n_rb) and np.array_equal(ts, ts_ref)
    assert np.any(np.abs(np.rint(ts) - ts) > 0.1), "the rows are taken off the sample grid"
    err = np.abs(tfg - ref).max() / np.abs(ref).max()
    print(shape, "cp", cp, "grid error / largest magnitude %.2e" % err)
    assert err <= 1e-10


# ---------------------------------------------------------------- the measurement stage
@pytest.mark.parametrize("shape", WC.SHAPES, ids=[str(s) for s in WC.SHAPES])
def test_measurement_against_the_numpy_reference_and_the_host_twin(pkg, S, H, shape):
    R, n_rb = shape
    cp = WC.CP_OF[shape]
    n_ofdm = 40 * TR.n_symb_of(cp) + 3                      # a partial last slot
    worst = 0.0
    for i, mask in enumerate(WC.MASKS):
        n_ports = (2, 1, 4, 0)[i]
        cell = _cell(pkg, cp, R, 137.0, n_ports)
        got = S.cell_meas_wide(cell, dev(R, cp), FC, FC, FS * R, 128 * R, n_rb, n_ofdm, mask)
        ref = WR.measure_capture(WC.cell_capture(R, cp), N_ID, cp, n_ports, cell.frame_start, 137.0, FC, FC, FS * R, 128 * R, n_rb, n_ofdm, mask)
        assert ref["status"] == 0 and ref["n_rows"] > 0
        worst = max(worst, WR.assert_record_close(got, ref, 1e-9, (shape, hex(mask))))
        # the host twin on the device's own grid: the same additions in the same order
        tfg, _ = S.extract_tfg_wide(cell, dev(R, cp), FC, FC, FS * R, 128 * R, n_rb, n_ofdm)
        _, twin = WC.twin_record(H, pkg.capi, N_ID, cp, tfg, n_rb, 128 * R, n_ports, mask)
        assert bytes(got)[:32] == bytes(twin)[:32]
        assert _doubles(got) == _doubles(twin), (shape, hex(mask), np.flatnonzero(np.frombuffer(_doubles(got), np.float64) != np.frombuffer(_doubles(twin), np.float64))[:8])
    # the cell is there: 20 dB of SNR, and a flat profile
    full = S.cell_meas_wide(_cell(pkg, cp, R, 0.0, 2), dev(R, cp), FC, FC, FS * R, 128 * R, n_rb, n_ofdm)
    assert full.status == 0 and full.n_rb == n_rb and full.n_fft == 128 * R and 15.0 < full.sinr_db[0] < 25.0
    assert full.rsrp_rb.shape == (2, n_rb) and np.all(np.abs(full.rsrp_rb[0] / full.rsrp[0] - 1) < 0.2)
    print(shape, "cp", cp, "worst stage error / scale %.2e; sinr %.1f dB, rsrq %.1f dB" % (worst, full.sinr_db[0], full.rsrq_db))


# ---------------------------------------------------------------- the anchor: the chain's own measurement at 128 points
def test_anchor_on_the_golden_capture(pkg, S, capbuf_0000):
    """complex<float> samples are the only difference to lcs_extract_tfg + lcs_cell_meas, and the golden capture is dongle-valued, hence
    exact in float: the bar is 1e-9 of scale (the issue's 1e-7, tightened because it holds)"""
    import torch
    cap, fc = capbuf_0000
    cells, _ = S.search_capbuf(cap, np.array([30e3, 35e3, 40e3]), fc, fc, FS)
    assert len(cells) >= 1
    d = torch.from_numpy(cap.astype(np.complex64)).cuda()
    assert np.array_equal(cap.astype(np.complex64).astype(np.complex128), cap)
    for c in cells:
        n_symb = TR.n_symb_of(c.cp_type)
        tfg, ts = S.extract_tfg(c, cap, fc, fc, FS)
        tfg_w, ts_w = S.extract_tfg_wide(c, d, fc, fc, FS, 128, 6, 122 * n_symb)
        assert np.array_equal(ts, ts_w) and np.abs(tfg_w - tfg).max() <= 1e-10 * np.abs(tfg).max()
        for mask in (0x3FF, 0x021):
            want = S.cell_meas(c, tfg, mask)
            got = S.cell_meas_wide(c, d, fc, fc, FS, 128, 6, 122 * n_symb, mask)
            assert (got.status, got.n_rows, got.n_ports, got.dl_mask, got.n_rb, got.n_fft) == (want.status, want.n_rows, want.n_ports, want.dl_mask, 6, 128) and want.status == 0
            unit = [want.rsrp[p] + max(want.noise[p], 0.0) for p in range(2)]
            err = [abs(got.rsrp[p] - want.rsrp[p]) / unit[p] for p in range(want.n_ports)] + [abs(got.noise[p] - want.noise[p]) / unit[p] for p in range(want.n_ports)]
            err += [abs(got.rssi - want.rssi) / want.rssi, abs(got.rsrq - want.rsrq) / (6 * unit[0] / want.rssi)]
            err += [abs(complex(*got.a_re_im[2 * p:2 * p + 2]) - complex(*want.a_re_im[2 * p:2 * p + 2])) / (11 * want.n_rows * unit[p]) for p in range(want.n_ports)]
            print("anchor, cell %d, mask %#x: worst error / scale %.2e" % (c.n_id_cell(), mask, max(err)))
            assert max(err) <= 1e-9
            assert abs(got.rssi_rb.sum() - got.rssi) <= 1e-12 * got.rssi


# ---------------------------------------------------------------- refusals
def test_refusals_launch_nothing_and_leave_the_context_usable(pkg, S):
    import torch
    R, cp = 2, 2
    d = dev(R, cp)
    n = d.numel()
    ok = dict(cell=_cell(pkg, cp, R), ptr=d.data_ptr(), n_cap=n, fs=FS * R, n_fft=256, n_rb=15, n_ofdm=240, mask=0x3FF)
    before = S.cell_meas_wide(ok["cell"], d, FC, FC, FS * R, 256, 15, 240)
    cases = [(dict(ptr=0), "null pointer"), (dict(ptr=d.data_ptr() + 4), "not aligned"),
             (dict(n_fft=384), "n_fft is not"), (dict(n_fft=64), "n_fft is not"), (dict(n_fft=4096), "n_fft is not"),
             (dict(fs=FS * R * 1.0011), "15 kHz x n_fft"), (dict(fs=FS), "15 kHz x n_fft"), (dict(fs=float("nan")), "15 kHz x n_fft"),
             (dict(n_rb=5), "n_rb is outside"), (dict(n_rb=16), "n_rb is outside"), (dict(n_fft=2048, fs=FS * 16, n_rb=101), "n_rb is outside"),
             (dict(n_ofdm=11), "n_ofdm is outside"), (dict(n_ofdm=122 * 6 + 1), "n_ofdm is outside"),
             (dict(mask=0), "dl_mask"), (dict(mask=0x400), "dl_mask"), (dict(mask=-1), "dl_mask"),
             (dict(cell=pkg.new_cell(n_id_2=1, cp_type=cp)), "n_id_1, n_id_2 and a known cp_type"),
             (dict(cell=pkg.new_cell(n_id_1=5, cp_type=cp)), "n_id_1, n_id_2 and a known cp_type"),
             (dict(cell=pkg.new_cell(n_id_1=5, n_id_2=1)), "n_id_1, n_id_2 and a known cp_type"),
             (dict(n_cap=int(ok["cell"].frame_start) + 19200 * R), "does not hold the last requested row"),
             (dict(cell=_cell(pkg, cp, R, frame_start=-40.0 * R)), "before sample 0"),
             (dict(cell=_cell(pkg, cp, R, frame_start=float("nan"))), "no finite positions")]
    for change, text in cases:
        a = dict(ok, **change)
        for grid in (False, True):
            if grid and "mask" in change:
                continue
            with pytest.raises(pkg.SearcherError, match=text):
                if grid:
                    S.extract_tfg_wide(a["cell"], a["ptr"], FC, FC, a["fs"], a["n_fft"], a["n_rb"], a["n_ofdm"], n_cap=a["n_cap"])
                else:
                    S.cell_meas_wide(a["cell"], a["ptr"], FC, FC, a["fs"], a["n_fft"], a["n_rb"], a["n_ofdm"], a["mask"], n_cap=a["n_cap"])
    # null host pointers through the C ABI
    lib, cell = S._lib, ok["cell"]
    assert lib.lcs_cell_meas_wide(S._h, C.byref(cell), C.c_void_p(d.data_ptr()), n, FC, FC, FS * R, 256, 15, 240, 0x3FF, None) == -2
    assert lib.lcs_extract_tfg_wide(S._h, C.byref(cell), C.c_void_p(d.data_ptr()), n, FC, FC, FS * R, 256, 15, 240, None, None) == -2
    assert lib.lcs_cell_meas_wide(S._h, None, C.c_void_p(d.data_ptr()), n, FC, FC, FS * R, 256, 15, 240, 0x3FF, C.byref(pkg.CellMeasWide())) == -2
    assert b"null pointer" in lib.lcs_last_error(S._h)
    with pytest.raises(ValueError):
        S.cell_meas_wide(cell, torch.zeros(16, dtype=torch.complex64), FC, FC, FS * R, 256, 15, 240)      # a host tensor
    # the first row may start at sample 0 exactly, and the last may end on the capture's last sample
    edge = _cell(pkg, cp, R, frame_start=-32.0 * R)
    ts, _ = WR.positions(edge.frame_start, 0.0, cp, FC, FC, FS * R, 240)
    assert int(np.rint(ts[0])) == 0
    S.extract_tfg_wide(edge, d, FC, FC, FS * R, 256, 15, 240, n_cap=int(np.rint(ts[-1])) + 256)
    with pytest.raises(pkg.SearcherError, match="does not hold the last requested row"):
        S.extract_tfg_wide(edge, d, FC, FC, FS * R, 256, 15, 240, n_cap=int(np.rint(ts[-1])) + 255)
    after = S.cell_meas_wide(ok["cell"], d, FC, FC, FS * R, 256, 15, 240)
    assert bytes(after) == bytes(before) and before.status == 0


# ---------------------------------------------------------------- modes, the last fused call's tables, an open stream
def test_modes_tables_and_an_open_stream_are_left_alone(pkg):
    R, cp = 4, 1
    d = dev(R, cp)
    cell = _cell(pkg, cp, R)
    args = (cell, d, FC, FC, FS * R, 512, 25, 283, 0x339)
    with pkg.Searcher(0) as s:
        plain = s.cell_meas_wide(*args)
        assert plain.status == 0
        for duplex, unwrap, tdd, meas in ((pkg.DUPLEX_TDD, False, True, False), (pkg.DUPLEX_TDD, True, True, True), (pkg.DUPLEX_FDD, False, False, True)):
            s.set_duplex(duplex), s.set_foe_unwrap(unwrap), s.set_tdd_config(tdd), s.set_cell_meas(meas)
            assert bytes(s.cell_meas_wide(*args)) == bytes(plain)
            assert s.cell_meas_mode is meas
            dv = C.c_int(-1)
            s._lib.lcs_get_duplex(s._h, C.byref(dv))
            assert dv.value == duplex
        cells, _ = s.search_capbuf(CS.cap(1), CS.GRID, CS.FC, CS.FC, FS)
        table = [bytes(t) for t in s.last_cell_meas(1, 16)[0]]
        tdd_table = [bytes(t) for t in s.last_tdd_info(1, 16)[0]]
        assert len(cells) >= 1 and s.last_cell_meas(1, 16)[0][0].status == 0
        assert bytes(s.cell_meas_wide(*args)) == bytes(plain)
        s.extract_tfg_wide(cell, d, FC, FC, FS * R, 512, 25, 14)
        assert [bytes(t) for t in s.last_cell_meas(1, 16)[0]] == table and [bytes(t) for t in s.last_tdd_info(1, 16)[0]] == tdd_table
        assert [bytes(c) for c in s.search_capbuf(CS.cap(1), CS.GRID, CS.FC, CS.FC, FS)[0]] == [bytes(c) for c in cells]
    with pkg.Searcher(0) as s:
        s.stream_open(pkg.FMT_IQ_U8, 153600, CS.FC, CS.FC, FS)
        assert bytes(s.cell_meas_wide(*args)) == bytes(plain)
        tfg, _ = s.extract_tfg_wide(cell, d, FC, FC, FS * R, 512, 25, 283)
        assert tfg.shape == (283, 300) and np.isfinite(tfg).all()
        s.stream_close()
        assert bytes(s.cell_meas_wide(*args)) == bytes(plain)


def test_python_record_mirrors_the_header(pkg, H):
    assert C.sizeof(pkg.CellMeasWide) == H.meas_wide_host_record_bytes() == 2528
