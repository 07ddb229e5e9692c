"""tdd_config.h compiled for the HOST -- the __host__ __device__ code k_tdd_config runs: the bins of a grid and the decision
from them -- against the numpy reference (tests/tdd_config_ref.py) on the crafted grids, and the decision's edges.

Bars: C[s][j] to 1e-12 of sum_r sum_m |h_m| |h_{m+1}| (the project's bar for a host twin of an fp64 sum: four rounded products
per term, eleven terms in a four-level tree, at most seven rows), T and R to 1e-12 absolute (they are of order 1), the decisions
exact.  The same source is built once more as a stand-alone program with -fsanitize=address,undefined and run on the same grids:
nothing is loaded into Python under a sanitizer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import tdd_config_ref as TR
from conftest import load_pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lte-cell-scanner_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "tdd_config_host.cpp")
LIB = os.path.join(ROOT, "tests", "host", "libtdd_config_host.so")
SAN = os.path.join(ROOT, "tests", "host", "tdd_config_host_san")
HIPCC = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include")]
_dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
_ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))


def _stale(target):
    dep = [SRC] + [os.path.join(CSRC, h) for h in ("tdd_config.h", "lte_device.h", "lcs_internal.h")] + [os.path.join(ROOT, "include", "lcs.h")]
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in dep)


@pytest.fixture(scope="module")
def TddInfo():
    return load_pkg().capi.TddInfo


@pytest.fixture(scope="module")
def H(TddInfo):
    if _stale(LIB):
        subprocess.check_call(HIPCC + ["-O2", "-fPIC", "-shared", "-o", LIB, SRC])
    h = C.CDLL(LIB)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    h.tdd_host_bins.argtypes = [dp, C.c_int, C.c_int, dp, ip, dp, ip, dp]
    h.tdd_host_bins.restype = None
    h.tdd_host_decide.argtypes = [dp, ip, C.POINTER(TddInfo)]
    h.tdd_host_decide.restype = None
    h.tdd_host_n_ref_rows.argtypes = [C.c_int, C.c_int]
    h.tdd_host_config_of_pattern.argtypes = [C.c_int]
    return h


def _tables(n_id_cell, cp):
    """RS_DL of port 0 by bin b = 2 slot + (sym != 0): values [40][12], shifts [40]"""
    rs, sh = O.rs_dl(n_id_cell, cp)
    n = TR.n_symb_of(cp)
    rows = [slot * n + sym for slot in range(20) for sym in (0, n - 3)]
    return np.ascontiguousarray(rs[rows]), np.ascontiguousarray(sh[rows, 0].astype(np.int32))


def _host(H, TddInfo, n_id_cell, cp, tfg):
    rs, sh = _tables(n_id_cell, cp)
    tfg = np.ascontiguousarray(tfg, np.complex128)
    Cb, N, S = np.zeros(40, np.complex128), np.zeros(40, np.int32), np.zeros(40)
    H.tdd_host_bins(_dp(tfg.view(np.float64)), tfg.shape[0], TR.n_symb_of(cp), _dp(rs.view(np.float64)), _ip(sh), _dp(Cb.view(np.float64)), _ip(N), _dp(S))
    o = TddInfo()
    H.tdd_host_decide(_dp(Cb.view(np.float64)), _ip(N), C.byref(o))
    return Cb.reshape(10, 4), N.reshape(10, 4), S.reshape(10, 4), o


def _decide(H, TddInfo, Cb, N):
    Cb, N = np.ascontiguousarray(Cb, np.complex128).reshape(40), np.ascontiguousarray(N, np.int32).reshape(40)
    o = TddInfo()
    H.tdd_host_decide(_dp(Cb.view(np.float64)), _ip(N), C.byref(o))
    return o


# (n_id_cell, cp, configuration, DwPTS rows, n_ofdm, ports)
GRIDS = [(100, 1, 0, 1, 854, 1), (101, 2, 1, 3, 732, 4), (102, 1, 2, 4, 280, 1), (103, 2, 3, 2, 240, 1), (104, 1, 4, 3, 283, 4), (105, 2, 5, 1, 245, 1),
         (5, 1, 6, 2, 854, 1), (503, 2, 6, 4, 500, 4)]


def _grid(case):
    n_id, cp, cfg, rows, n_ofdm, ports = case
    # (a short grid has two rows per bin: the uplink is kept weak there, or a row of the special subframe reads anything)
    return TR.crafted_grid(n_id, cp, TR.SUBFRAMES[cfg], TR.DWPTS_OF_ROWS[cp][rows], n_ofdm, seed=n_id, n_ports=ports, uplink_gain=1.5 if n_ofdm >= 700 else 0.5)


@pytest.mark.parametrize("case", GRIDS, ids=[str(g) for g in GRIDS])
def test_bins_and_decision_on_crafted_grids(H, TddInfo, case):
    n_id, cp, cfg, rows, n_ofdm, _ = case
    tfg = _grid(case)
    ref = TR.estimate(n_id, cp, tfg)
    Cb, N, S, o = _host(H, TddInfo, n_id, cp, tfg)
    assert H.tdd_host_n_ref_rows(n_ofdm, TR.n_symb_of(cp)) == len(TR.ref_rows(n_ofdm, cp)) == N.sum()
    assert np.array_equal(N, ref["N"])
    assert np.all(np.abs(S - ref["scale"]) <= 1e-12 * ref["scale"])
    worst = (np.abs(Cb - ref["C"]) / ref["scale"]).max()
    print(case, "worst |C error| / scale %.2e" % worst, "T error %.2e" % np.abs(np.array(o.T) - ref["T"]).max())
    assert worst <= 1e-12
    assert np.abs(np.array(o.T) - ref["T"]).max() <= 1e-12 and np.abs(np.array(o.R) - ref["R"]).max() <= 1e-12
    assert abs(o.margin - ref["margin"]) <= 1e-12
    assert (o.ul_dl_config, o.dwpts_rs_rows) == (ref["ul_dl_config"], ref["dwpts_rs_rows"]) == (cfg, rows)


def test_no_decision_grids(H, TddInfo):
    for tfg in (np.zeros((854, 72), np.complex128), np.full((854, 72), np.nan + 0j)):
        o = _host(H, TddInfo, 7, 1, tfg)[3]
        assert (o.ul_dl_config, o.dwpts_rs_rows, o.margin) == (-1, -1, 0.0)
    g = TR.crafted_grid(7, 1, "DDDDDDDDDD", 9, 854, seed=2)
    o, ref = _host(H, TddInfo, 7, 1, g)[3], TR.estimate(7, 1, g)
    assert o.ul_dl_config == ref["ul_dl_config"] == -1 and o.dwpts_rs_rows == -1 and abs(o.margin - ref["margin"]) <= 1e-12 and o.margin > 0.3


def _bins_for(T, R6=None, R1=(1.0, 1.0, 1.0, 0.0)):
    """bins (one row each) whose statistic comes out as T per subframe: C[s][j] = T[s] / 4 on an equal share, ref real"""
    Cb, N = np.zeros((10, 4), np.complex128), np.ones((10, 4), np.int32)
    for s in range(10):
        Cb[s] = T[s]
    Cb[1] = R1
    if R6 is not None:
        Cb[6] = R6
    return Cb, N


def test_threshold_edges_prefix_rule_and_counts_of_zero(H, TddInfo):
    up, dn = np.nextafter(0.5, 1.0), np.nextafter(0.5, 0.0)
    # with C[0] = C[5] = 1 per row, ref = 8, n_ref = 8, N[s] = 4: T[s] = (4 v) 8 / 64 * 8 / 4 = v exactly for these v
    for v, is_down in ((up, True), (0.5, False), (dn, False)):
        T = [1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, v]
        Cb, N = _bins_for(T, R6=(1.0, 1.0, 1.0, 0.0))
        o, ref = _decide(H, TddInfo, Cb, N), TR.decide(Cb, N)
        assert o.T[9] == v == ref["T"][9]
        assert o.ul_dl_config == ref["ul_dl_config"] == (6 if is_down else 0), v
        assert o.margin == ref["margin"] == abs(v - 0.5)
        # and subframe 2 a hair over the threshold takes the number away
        T[2] = v
        Cb, N = _bins_for(T)
        assert _decide(H, TddInfo, Cb, N).ul_dl_config == TR.decide(Cb, N)["ul_dl_config"] == (-1 if is_down else 0)
    # every pattern of (3, 4, 7, 8, 9) against the table
    for pat in range(32):
        bits = [(pat >> (4 - k)) & 1 for k in range(5)]
        T = [1.0, 1.0, 0.0, bits[0], bits[1], 1.0, 1.0, bits[2], bits[3], bits[4]]
        Cb, N = _bins_for([float(t) for t in T], R6=(1.0, 1.0, 1.0, 0.0))
        want = TR.PATTERNS.get("".join("D" if b else "U" for b in bits), -1)
        assert _decide(H, TddInfo, Cb, N).ul_dl_config == H.tdd_host_config_of_pattern(pat) == TR.decide(Cb, N)["ul_dl_config"] == want
    # the prefix rule: rows present must be 1.., starting with row 0
    T = [1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0]      # configuration 3: subframe 6 is downlink and does not join
    for R1, rows in (((1, 0, 0, 0), 1), ((1, 1, 0, 0), 2), ((1, 1, 1, 0), 3), ((1, 1, 1, 1), 4), ((0, 0, 0, 0), -1), ((0, 1, 1, 1), -1), ((1, 0, 1, 0), -1), ((1, 1, 0, 1), -1),
                     ((up, dn, 0, 0), 1), ((up, up, 0.5, 0), 2)):
        Cb, N = _bins_for(T, R1=[float(x) for x in R1])
        o, ref = _decide(H, TddInfo, Cb, N), TR.decide(Cb, N)
        assert (o.ul_dl_config, o.dwpts_rs_rows) == (ref["ul_dl_config"], ref["dwpts_rs_rows"]) == (3, rows), R1
    # subframe 6 joins where the configuration has it special: rows present in subframe 1 only read 1/2 of a row, not over 1/2
    T = [1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    Cb, N = _bins_for(T, R1=(1.0, 1.0, 0.0, 0.0), R6=(1.0, 0.0, 0.0, 0.0))
    o, ref = _decide(H, TddInfo, Cb, N), TR.decide(Cb, N)
    assert (o.ul_dl_config, o.dwpts_rs_rows) == (ref["ul_dl_config"], ref["dwpts_rs_rows"]) == (6, 1) and list(o.R) == list(ref["R"]) == [1.0, 0.5, 0.0, 0.0]
    # counts of zero: a subframe without rows, a special-subframe row without rows, no reference rows at all
    T = [1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    Cb, N = _bins_for(T)
    N[8] = 0
    o, ref = _decide(H, TddInfo, Cb, N), TR.decide(Cb, N)
    assert (o.ul_dl_config, o.dwpts_rs_rows, o.margin) == (ref["ul_dl_config"], ref["dwpts_rs_rows"], ref["margin"]) == (-1, -1, 0.0) and o.T[8] == 0.0
    Cb, N = _bins_for(T)
    N[1, 3] = 0
    o, ref = _decide(H, TddInfo, Cb, N), TR.decide(Cb, N)
    assert (o.ul_dl_config, o.dwpts_rs_rows) == (ref["ul_dl_config"], ref["dwpts_rs_rows"]) == (3, -1) and o.margin == ref["margin"] > 0
    Cb, N = _bins_for(T)
    N[0] = 0
    N[5] = 0
    o = _decide(H, TddInfo, Cb, N)
    assert (o.ul_dl_config, o.dwpts_rs_rows, o.margin) == (-1, -1, 0.0) and TR.decide(Cb, N)["ul_dl_config"] == -1
    # ref not finite
    Cb, N = _bins_for(T)
    Cb[5, 2] = np.inf
    assert _decide(H, TddInfo, Cb, N).ul_dl_config == TR.decide(Cb, N)["ul_dl_config"] == -1


def test_stand_alone_program_under_address_and_undefined_sanitizers(H, TddInfo, tmp_path):
    """the same source with its own main, built with -fsanitize=address,undefined, on the crafted grids: a clean exit, and the
    record the library form gives"""
    if _stale(SAN):
        subprocess.check_call(HIPCC + ["-O1", "-g", "-DTDD_HOST_MAIN", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                                       "-fno-sanitize-recover=undefined", "-o", SAN, SRC])
    for case in GRIDS + [(7, 1, -1, -1, 854, 1)]:
        n_id, cp, cfg, rows, n_ofdm, _ = case
        tfg = _grid(case) if cfg >= 0 else np.zeros((n_ofdm, 72), np.complex128)
        rs, sh = _tables(n_id, cp)
        path = tmp_path / "grid.bin"
        with open(path, "wb") as f:
            f.write(np.array([n_ofdm, TR.n_symb_of(cp)], np.int32).tobytes() + sh.tobytes() + rs.tobytes() + np.ascontiguousarray(tfg).tobytes())
        r = subprocess.run([SAN, str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
        v = r.stdout.split()
        o = _host(H, TddInfo, n_id, cp, tfg)[3]
        assert (int(v[0]), int(v[1])) == (o.ul_dl_config, o.dwpts_rs_rows) == (cfg, rows)
        assert [float(x) for x in v[2:]] == [o.margin] + list(o.T) + list(o.R)
