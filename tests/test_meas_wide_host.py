"""cell_meas_wide.h compiled for the HOST -- the __host__ __device__ code k_cell_meas_wide and k_cell_meas_wide_fin run: the totals of a
grid [n_ofdm][12 n_rb] under a mask, the per-RB profile and the record -- against the numpy reference (tests/meas_wide_ref.py).

Bars: every sum to 1e-12 of its scale (the project's bar for a host twin of an fp64 sum), the derived fields to 1e-12 of their units
(meas_wide_ref.assert_record_close), integers exact.  At n_rb = 6 the twin equals cell_meas.h's twin bit for bit.  The generalised
RS_DL row (lte_device.h: rs_dl_row_wide) equals the numpy sequence bit for bit.  The record's size and layout are pinned here.  The
same source is built once more as a stand-alone program with -fsanitize=address,undefined: nothing is loaded into Python under a
sanitizer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import meas_wide_cases as WC
import meas_wide_ref as WR
import tdd_config_ref as TR
from conftest import load_pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lte-cell-scanner_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "meas_wide_host.cpp")
SAN = os.path.join(ROOT, "tests", "host", "meas_wide_host_san")
NARROW_SRC = os.path.join(ROOT, "tests", "host", "cell_meas_host.cpp")
NARROW_LIB = os.path.join(ROOT, "tests", "host", "libcell_meas_host.so")
HIPCC = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include")]
_dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
_ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
TOL = 1e-12
N_FFT_OF = {6: 128, 15: 256, 25: 512, 50: 1024, 75: 2048, 100: 2048}


_stale = lambda target, src=SRC: WC.stale(target, src)


@pytest.fixture(scope="module")
def capi():
    return load_pkg().capi


@pytest.fixture(scope="module")
def H(capi):
    return WC.load_twin(capi)


host = WC.twin_record


def _check(H, capi, n_id, cp, tfg, n_rb, n_ports, mask, what):
    ref = WR.measure(n_id, cp, tfg, n_rb, N_FFT_OF[n_rb], mask, n_ports)
    tot, o = host(H, capi, n_id, cp, tfg, n_rb, N_FFT_OF[n_rb], n_ports, mask)
    s = ref["sums"]
    worst = 0.0
    for p in range(ref["n_ports"]):
        worst = max(worst, abs(complex(tot[2 * p], tot[2 * p + 1]) - s["A"][p]) / s["scale"]["A"][p], abs(tot[4 + p] - s["E"][p]) / s["E"][p])
    for p in range(ref["n_ports"], 2):
        assert tot[2 * p] == tot[2 * p + 1] == tot[4 + p] == 0.0
    worst = max(worst, abs(tot[6] - s["W"]) / s["W"])
    assert worst <= TOL, (what, worst)
    return max(worst, WR.assert_record_close(o, ref, TOL, what)), o


@pytest.mark.parametrize("n_rb", [6, 15, 25, 50, 75, 100])
@pytest.mark.parametrize("cp", [1, 2])
def test_sums_profile_and_record_on_crafted_and_random_grids(H, capi, n_rb, cp):
    n = TR.n_symb_of(cp)
    crafted = WC.shape_grid(n_rb, cp)                     # two frames and three rows: a partial last slot
    rng = np.random.default_rng(n_rb + cp)
    rand = rng.standard_normal((20 * n + 1, 12 * n_rb)) + 1j * rng.standard_normal((20 * n + 1, 12 * n_rb))
    worst = 0.0
    for tfg, name in ((crafted, "crafted"), (rand, "random")):
        for i, mask in enumerate(WC.MASKS):
            w, o = _check(H, capi, 100 + n_rb, cp, tfg, n_rb, 2 - (i & 1), mask, (name, n_rb, cp, hex(mask)))
            assert o.status == 0 and o.n_rb == n_rb and o.n_fft == N_FFT_OF[n_rb] and o.rsrp_rb.shape == (2, n_rb) and o.rssi_rb.shape == (n_rb,)
            worst = max(worst, w)
    # ports: 0 / unknown and 1 measure port 0 alone, 2 and 4 ports 0 and 1
    for n_ports, P in ((0, 1), (-1, 1), (1, 1), (2, 2), (4, 2)):
        _, o = _check(H, capi, 100 + n_rb, cp, crafted, n_rb, n_ports, 0x3FF, ("ports", n_ports))
        assert o.n_ports == P and (P == 2 or not o.rsrp_rb[1].any())
    print(n_rb, cp, "worst error / scale %.2e" % worst)


def test_six_resource_blocks_are_the_narrow_rule_bit_for_bit(H, capi):
    if _stale(NARROW_LIB, NARROW_SRC):
        subprocess.check_call(HIPCC + ["-O2", "-fPIC", "-shared", "-o", NARROW_LIB, NARROW_SRC])
    N = C.CDLL(NARROW_LIB)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    N.meas_host.argtypes = [dp, C.c_int, C.c_int, dp, ip, C.c_int, C.c_int, dp, dp, C.POINTER(capi.CellMeas)]
    N.meas_host.restype = None
    for cp in (1, 2):
        tfg = np.ascontiguousarray(WC.shape_grid(6, cp))
        rs, sh = WR.rs_wide(106, cp, 6)
        rs, sh = np.ascontiguousarray(rs), np.ascontiguousarray(sh, np.int32)
        for mask in WC.MASKS:
            tot_w, w = host(H, capi, 106, cp, tfg, 6, 128, 2, mask)
            tot_n, scale, o = np.zeros(7), np.zeros(7), capi.CellMeas()
            N.meas_host(_dp(tfg.view(np.float64)), tfg.shape[0], TR.n_symb_of(cp), _dp(rs.view(np.float64)), _ip(sh), 2, mask, _dp(tot_n), _dp(scale), C.byref(o))
            assert tot_w.tobytes() == tot_n.tobytes()
            assert (w.status, w.n_rows, w.n_ports, w.dl_mask) == (o.status, o.n_rows, o.n_ports, o.dl_mask) and w.status == 0
            assert list(w.rsrp) + list(w.noise) + [w.rssi, w.rsrq] + list(w.a_re_im) == list(o.rsrp) + list(o.noise) + [o.rssi, o.rsrq] + list(o.a_re_im)


def test_grids_without_a_number(H, capi):
    n_rb = 25
    shape = (283, 12 * n_rb)
    for tfg in (np.zeros(shape, np.complex128), np.full(shape, np.nan + 0j), np.full(shape, np.inf + 0j)):
        for n_ports in (1, 2):
            _, o = host(H, capi, 7, 1, tfg, n_rb, 512, n_ports, 0x3FF)
            ref = WR.measure(7, 1, tfg, n_rb, 512, 0x3FF, n_ports)
            assert o.status == ref["status"] == -1 and o.n_rows == ref["n_rows"] > 0
            WR.assert_record_close(o, ref, TOL)
    g = WC.shape_grid(n_rb, 1).copy()
    clean = host(H, capi, 125, 1, g, n_rb, 512, 1, 0x021)[1]
    g[28, 5] = np.nan           # slot 4 symbol 0: subframe 2, outside the mask
    o = host(H, capi, 125, 1, g, n_rb, 512, 1, 0x021)[1]
    assert o.status == 0 and bytes(o) == bytes(clean)
    g[0, 12 * n_rb - 1] = np.nan    # one element of a used row (port 0's last reference element: 125 mod 6 = 5)
    o = host(H, capi, 125, 1, g, n_rb, 512, 1, 0x021)[1]
    assert o.status == -1 and not np.ctypeslib.as_array(o._rssi_rb).any() and not np.ctypeslib.as_array(o._rsrp_rb).any()
    # an empty mask, and a mask whose subframe the grid does not reach: no used row
    for tfg, mask in ((g, 0), (g[:14], 0x200)):
        o = host(H, capi, 125, 1, tfg, n_rb, 512, 1, mask)[1]
        assert (o.status, o.n_rows, o.dl_mask, o.n_rb, o.n_fft) == (-1, 0, mask, n_rb, 512) and o.rssi == 0.0


def _pn_jump(steps):
    out = []
    for b in range(32):
        x = (1 << b) if b < 31 else 1
        for _ in range(steps):
            n = ((x >> 3) ^ (x >> 2) ^ (x >> 1) ^ x) & 1 if b < 31 else ((x >> 3) ^ x) & 1
            x = (x >> 1) | (n << 30)
        out.append(x)
    return np.array(out, np.uint32)


@pytest.mark.parametrize("n_rb", [6, 75, 100])
def test_generalised_rs_row_equals_the_numpy_sequence_bit_for_bit(H, n_rb):
    jump = _pn_jump(1600 + 2 * (110 - n_rb))
    for n_id, cp in ((0, 1), (503, 2), (96, 1)):
        rs, sh = WR.rs_wide(n_id, cp, n_rb)
        n = TR.n_symb_of(cp)
        for slot in (0, 7, 19):
            for t in (0, 2):
                got, s4 = np.zeros(2 * n_rb, np.complex128), np.zeros(4)
                H.meas_wide_host_rs_row(slot, t, n_id, cp, n, n_rb, jump.ctypes.data_as(C.POINTER(C.c_uint32)), _dp(got.view(np.float64)), _dp(s4))
                b = 2 * slot + (t != 0)
                assert got.tobytes() == np.ascontiguousarray(rs[b]).tobytes()
                assert list(s4) == [float(sh[b, 0]), float(sh[b, 1]), -1.0, -1.0]


def test_columns_of_the_grid_row(H):
    for n_fft, n_rb in ((128, 6), (256, 15), (2048, 100), (2048, 75), (1024, 6)):
        cols, cns = [], []
        for k in range(n_fft):
            cn = C.c_int(0)
            c = H.meas_wide_host_col_of_bin(k, n_fft, n_rb, C.byref(cn))
            if c >= 0:
                cols.append(c), cns.append(cn.value)
        order = np.argsort(cols)
        assert sorted(cols) == list(range(12 * n_rb))
        assert [cns[i] for i in order] == list(range(-6 * n_rb, 0)) + list(range(1, 6 * n_rb + 1))
    assert [H.meas_wide_host_max_rb(n) for n in (128, 256, 512, 1024, 2048, 64, 384)] == [6, 15, 25, 50, 100, -1, -1]


def test_record_size_and_layout(H, capi):
    W = capi.CellMeasWide
    assert C.sizeof(W) == 2528 == H.meas_wide_host_record_bytes() and capi.MEAS_WIDE_MAX_RB == WR.MAX_RB == 100
    want = dict(status=0, n_rows=4, n_ports=8, dl_mask=12, n_rb=16, n_fft=20, reserved_i=24, rsrp=32, noise=48, rssi=64, rsrq=72, a_re_im=80,
                reserved=112, _rsrp_rb=128, _rssi_rb=1728)
    assert {k: getattr(W, k).offset for k in want} == want
    assert C.sizeof(capi.CellMeas) == 128      # lcs_meas_info does not change
    o = W()
    o.n_rb, o.n_ports = 15, 2
    o.rsrp[0], o.rsrp[1], o.noise[0], o.noise[1], o.rsrq = 2.0, 1.0, 0.5, 0.0, 0.25
    o._rsrp_rb[1][14], o._rssi_rb[14] = 3.0, 4.0
    assert o.rsrp_rb.shape == (2, 15) and o.rsrp_rb[1, 14] == 3.0 and o.rssi_rb[14] == 4.0
    assert o.sinr == (4.0, float("inf")) and abs(o.rsrp_db[0] - 10 * np.log10(2.0)) < 1e-12 and abs(o.rsrq_db - 10 * np.log10(0.25)) < 1e-12
    c = o.copy()
    o._rssi_rb[14] = 5.0
    assert c.rssi_rb[14] == 4.0 and bytes(c) != bytes(o)


def test_stand_alone_program_under_address_and_undefined_sanitizers(H, capi, tmp_path):
    """the same source with its own main, built with -fsanitize=address,undefined: a clean exit, and the record the library form gives"""
    if _stale(SAN):
        subprocess.check_call(HIPCC + ["-O1", "-g", "-DMEAS_WIDE_HOST_MAIN", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                                       "-fno-sanitize-recover=undefined", "-o", SAN, SRC])
    cases = [(100 + n_rb, cp, n_rb, WC.shape_grid(n_rb, cp), 2, WC.MASKS[i % 4]) for i, (n_rb, cp) in enumerate(((6, 1), (15, 2), (75, 1), (100, 2)))]
    cases.append((7, 1, 50, np.zeros((283, 600), np.complex128), 1, 0x3FF))
    cases.append((7, 2, 100, np.full((240, 1200), np.nan + 0j), 2, 0x021))
    for n_id, cp, n_rb, tfg, ports, mask in cases:
        rs, sh = WR.rs_wide(n_id, cp, n_rb)
        path = tmp_path / "grid.bin"
        with open(path, "wb") as f:
            f.write(np.array([tfg.shape[0], TR.n_symb_of(cp), n_rb, N_FFT_OF[n_rb], ports, mask], np.int32).tobytes() + np.ascontiguousarray(sh, np.int32).tobytes() +
                    np.ascontiguousarray(rs).tobytes() + np.ascontiguousarray(tfg, np.complex128).tobytes())
        r = subprocess.run([SAN, str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
        v = r.stdout.split()
        o = host(H, capi, n_id, cp, tfg, n_rb, N_FFT_OF[n_rb], ports, mask)[1]
        assert [int(x) for x in v[:6]] == [o.status, o.n_rows, o.n_ports, o.dl_mask, o.n_rb, o.n_fft]
        rb = [x for i in range(n_rb) for x in (o.rsrp_rb[0, i], o.rsrp_rb[1, i], o.rssi_rb[i])]
        assert [float(x) for x in v[6:]] == list(o.rsrp) + list(o.noise) + [o.rssi, o.rsrq] + list(o.a_re_im) + rb
