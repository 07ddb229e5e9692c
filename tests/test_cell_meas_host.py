"""cell_meas.h compiled for the HOST -- the __host__ __device__ code k_cell_meas runs: the seven totals of a grid under a mask and
the record from them -- against the numpy reference (tests/cell_meas_ref.py) on crafted grids, and the rule's edges.

Bars: every sum to 1e-12 of its scale (the project's bar for a host twin of an fp64 sum; A_p against sum |h_m| |h_{m+1}|, E_p and W
against themselves: their terms are non-negative), the derived fields to 1e-12 of E_p / (12 n_rows) or rssi, counts, status and dl_mask
exact.  The same source is built once more as a stand-alone program with -fsanitize=address,undefined and run on the same grids:
nothing is loaded into Python under a sanitizer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cell_meas_cases as CS
import cell_meas_ref as MR
import oracle as O
import tdd_config_ref as TR
from conftest import load_pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lte-cell-scanner_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "cell_meas_host.cpp")
LIB = os.path.join(ROOT, "tests", "host", "libcell_meas_host.so")
SAN = os.path.join(ROOT, "tests", "host", "cell_meas_host_san")
HIPCC = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include")]
_dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
_ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
TOL = 1e-12


def _stale(target):
    dep = [SRC] + [os.path.join(CSRC, h) for h in ("cell_meas.h", "tdd_config.h", "lte_device.h", "lcs_internal.h")] + [os.path.join(ROOT, "include", "lcs.h")]
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in dep)


@pytest.fixture(scope="module")
def CellMeas():
    return load_pkg().capi.CellMeas


@pytest.fixture(scope="module")
def H(CellMeas):
    if _stale(LIB):
        subprocess.check_call(HIPCC + ["-O2", "-fPIC", "-shared", "-o", LIB, SRC])
    h = C.CDLL(LIB)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    h.meas_host.argtypes = [dp, C.c_int, C.c_int, dp, ip, C.c_int, C.c_int, dp, dp, C.POINTER(CellMeas)]
    h.meas_host.restype = None
    h.meas_host_tdd_dl_mask.argtypes = [C.c_int]
    h.meas_host_n_rows.argtypes = [C.c_int, C.c_int, C.c_int]
    return h


def _tables(n_id_cell, cp):
    """RS_DL by bin b = 2 slot + (sym != 0): values [40][12], the shifts of ports 0 and 1 [40][2]"""
    rs, sh = O.rs_dl(n_id_cell, cp)
    n = TR.n_symb_of(cp)
    rows = [slot * n + sym for slot in range(20) for sym in (0, n - 3)]
    return np.ascontiguousarray(rs[rows]), np.ascontiguousarray(sh[rows, :2].astype(np.int32))


def _host(H, CellMeas, n_id_cell, cp, tfg, n_ports, mask):
    rs, sh = _tables(n_id_cell, cp)
    tfg = np.ascontiguousarray(tfg, np.complex128)
    tot, scale = np.zeros(7), np.zeros(7)
    o = CellMeas()
    H.meas_host(_dp(tfg.view(np.float64)), tfg.shape[0], TR.n_symb_of(cp), _dp(rs.view(np.float64)), _ip(sh), n_ports, mask, _dp(tot), _dp(scale), C.byref(o))
    return tot, scale, o


def _check(H, CellMeas, n_id, cp, tfg, n_ports, mask, what):
    ref = MR.measure(n_id, cp, tfg, mask, n_ports)
    tot, scale, o = _host(H, CellMeas, n_id, cp, tfg, n_ports, mask)
    s = ref["sums"]
    assert H.meas_host_n_rows(tfg.shape[0], TR.n_symb_of(cp), mask) == ref["n_rows"] == o.n_rows
    worst = 0.0
    for p in range(ref["n_ports"]):
        assert abs(scale[2 * p] - s["scale"]["A"][p]) <= TOL * s["scale"]["A"][p]
        worst = max(worst, abs(complex(tot[2 * p], tot[2 * p + 1]) - s["A"][p]) / s["scale"]["A"][p], abs(tot[4 + p] - s["E"][p]) / s["E"][p])
    for p in range(ref["n_ports"], 2):
        assert tot[2 * p] == tot[2 * p + 1] == tot[4 + p] == 0.0
    worst = max(worst, abs(tot[6] - s["W"]) / s["W"])
    assert worst <= TOL, (what, worst)
    worst = max(worst, MR.assert_record_close(o, ref, TOL, what))
    return worst, o


@pytest.mark.parametrize("shape", CS.SHAPES, ids=[str(s) for s in CS.SHAPES])
def test_sums_and_record_on_crafted_grids(H, CellMeas, shape):
    n_id, cp, n_ofdm, ports = shape
    tfg = CS.shape_grid(shape)
    worst = max(_check(H, CellMeas, n_id, cp, tfg, ports, mask, (shape, hex(mask)))[0] for mask in CS.MASKS)
    print(shape, "worst error / scale %.2e" % worst)


def test_edges_of_mask_rows_and_ports(H, CellMeas):
    tfg = CS.shape_grid(CS.SHAPES[3])      # 240 rows, extended CP: 80 reference rows, two per bin
    n_id, cp = CS.SHAPES[3][:2]
    # a mask of one subframe, every subframe in turn
    for s in range(10):
        _, o = _check(H, CellMeas, n_id, cp, tfg, 2, 1 << s, ("one subframe", s))
        assert (o.status, o.n_rows, o.dl_mask) == (0, 8, 1 << s)
    # bins of one row each in a 240-row grid: with the normal CP 240 rows are 34 slots and two symbols, 69 reference rows -- bins
    # 0 .. 28 hold two rows, bins 29 .. 39 one; subframes 8 and 9 are bins 32 .. 39
    g = CS.shape_grid(CS.SHAPES[2])[:240]
    _, o = _check(H, CellMeas, 98, 1, g, 2, 0x300, "one row per bin, 240 rows")
    assert o.n_rows == 8
    # ... and with the extended CP on one frame and one slot: bins 0, 1 hold two rows, every other bin one
    part = tfg[:126]
    _, o = _check(H, CellMeas, n_id, cp, part, 2, 0x3FE, "one row per bin")
    assert o.n_rows == 36
    _, o = _check(H, CellMeas, n_id, cp, part, 2, 0x3FF, "one or two rows per bin")
    assert o.n_rows == 42
    # a partial last slot: 283 rows (normal CP) end on symbol 2 of slot 40 -- its row 0 counts, its row n_symb - 3 does not;
    # 245 rows (extended CP) end on symbol 4 of slot 40: both count
    for shape, want in ((CS.SHAPES[4], 9), (CS.SHAPES[5], 10)):
        g = CS.shape_grid(shape)
        _, o = _check(H, CellMeas, shape[0], shape[1], g, 2, 0x001, ("partial slot", shape))
        assert o.n_rows == want      # subframe 0 of frames 0 and 1 (4 + 4) and what the third frame's first slot has
    # ports: 0 / unknown and 1 measure port 0 alone, 2 and 4 ports 0 and 1
    g = CS.shape_grid(CS.SHAPES[6])
    for n_ports, P in ((0, 1), (-1, 1), (1, 1), (2, 2), (4, 2)):
        _, o = _check(H, CellMeas, 503, 1, g, n_ports, 0x3FF, ("ports", n_ports))
        assert o.n_ports == P
        if P == 1:
            assert o.rsrp[1] == o.noise[1] == o.a_re_im[2] == o.a_re_im[3] == 0.0


def test_grids_without_a_number(H, CellMeas):
    for tfg in (np.zeros((854, 72), np.complex128), np.full((854, 72), np.nan + 0j), np.full((280, 72), np.inf + 0j)):
        for n_ports in (1, 2):
            tot, scale, o = _host(H, CellMeas, 7, 1, tfg, n_ports, 0x3FF)
            ref = MR.measure(7, 1, tfg, 0x3FF, n_ports)
            assert o.status == ref["status"] == -1 and o.n_rows == ref["n_rows"] > 0 and o.dl_mask == 0x3FF and o.n_ports == n_ports
            assert list(o.rsrp) + list(o.noise) + [o.rssi, o.rsrq] + list(o.a_re_im) == [0.0] * 10
    # a NaN outside the mask's rows changes nothing; one inside takes the number away
    g = CS.shape_grid(CS.SHAPES[0]).copy()
    clean = _host(H, CellMeas, 96, 1, g, 1, 0x021)[2]
    g[14 * 2, 5] = np.nan      # slot 4 symbol 0: subframe 2
    o = _host(H, CellMeas, 96, 1, g, 1, 0x021)[2]
    assert o.status == 0 and bytes(o) == bytes(clean)
    g[0, 71] = np.nan          # subframe 0, no reference element of port 0 (n_id_cell mod 6 = 0): only w sees it
    assert _host(H, CellMeas, 96, 1, g, 1, 0x021)[2].status == -1
    # no used row at all: a grid shorter than the first subframe of the mask
    o = _host(H, CellMeas, 96, 1, g[:10], 1, 0x200)[2]
    assert (o.status, o.n_rows) == (-1, 0)


def test_tdd_dl_mask_against_the_table(H):
    for cfg in range(-1, 8):
        want = sum(1 << s for s, k in enumerate(TR.SUBFRAMES[cfg]) if k == "D") if 0 <= cfg <= 6 else -1
        assert H.meas_host_tdd_dl_mask(cfg) == MR.tdd_dl_mask(cfg) == want
    assert H.meas_host_tdd_dl_mask(2) == 0x339 and H.meas_host_tdd_dl_mask(0) == 0x021


def test_stand_alone_program_under_address_and_undefined_sanitizers(H, CellMeas, tmp_path):
    """the same source with its own main, built with -fsanitize=address,undefined, on the crafted grids: a clean exit, and the
    record the library form gives"""
    if _stale(SAN):
        subprocess.check_call(HIPCC + ["-O1", "-g", "-DMEAS_HOST_MAIN", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                                       "-fno-sanitize-recover=undefined", "-o", SAN, SRC])
    cases = [(shape, CS.shape_grid(shape), CS.MASKS[i % len(CS.MASKS)]) for i, shape in enumerate(CS.SHAPES)]
    cases.append(((7, 1, 854, 2), np.zeros((854, 72), np.complex128), 0x3FF))
    cases.append(((7, 2, 240, 1), np.full((240, 72), np.nan + 0j), 0x021))
    for (n_id, cp, n_ofdm, ports), tfg, mask in cases:
        rs, sh = _tables(n_id, cp)
        path = tmp_path / "grid.bin"
        with open(path, "wb") as f:
            f.write(np.array([n_ofdm, TR.n_symb_of(cp), ports, mask], np.int32).tobytes() + sh.tobytes() + rs.tobytes() + np.ascontiguousarray(tfg).tobytes())
        r = subprocess.run([SAN, str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
        v = r.stdout.split()
        o = _host(H, CellMeas, n_id, cp, tfg, ports, mask)[2]
        assert [int(x) for x in v[:4]] == [o.status, o.n_rows, o.n_ports, o.dl_mask]
        assert [float(x) for x in v[4:]] == list(o.rsrp) + list(o.noise) + [o.rssi, o.rsrq] + list(o.a_re_im)
