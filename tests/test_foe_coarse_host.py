"""foe_coarse.h compiled for the HOST: the half sums of one PSS window, the coarse estimate and the decision that unwraps
pss_sss_foe with it -- the __host__ __device__ code k_foe_fin_unwrap runs -- against the numpy reference
(tests/pss_coarse_ref.py) on the windows of the crafted cells (tests/foe_unwrap_cases.py).

Bars: A and B to 1e-12 of sum |z| (128 products and a six-level tree of additions per half in fp64: a few 1e-16 per operation, and the host's
cos / sin may differ from numpy's in the last bit), f_coarse to 1e-6 Hz, the decision exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import pss_coarse_ref as PC
import sss_duplex_ref as R
import foe_unwrap_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lte-cell-scanner_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "foe_coarse_host.cpp")
LIB = os.path.join(ROOT, "tests", "host", "libfoe_coarse_host.so")
_dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))


@pytest.fixture(scope="module")
def H():
    dep = [SRC] + [os.path.join(CSRC, h) for h in ("foe_coarse.h", "lte_device.h", "lcs_internal.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in dep):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC",
                               "-shared", "-I" + os.path.join(ROOT, "include"), "-o", LIB, SRC])
    h = C.CDLL(LIB)
    d, i, dp, ip = C.c_double, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)
    h.foe_host_halves.argtypes = [dp, d, dp, dp, dp, dp]
    h.foe_host_halves.restype = None
    h.foe_host_coarse.argtypes = [dp, dp, i, d, dp, ip]
    h.foe_host_coarse.restype = d
    h.foe_host_usable.argtypes = [d, d, i]
    h.foe_host_unwrap.argtypes = [d, d, d, d, i, i, ip]
    h.foe_host_unwrap.restype = d
    return h


@pytest.fixture(scope="module", autouse=True)
def _oracle_mode():
    O.set_legacy(False)
    O.set_threads(min(16, os.cpu_count() or 1))


def _unwrap(H, native, freq, f_coarse, fs, dist, usable=True):
    n = C.c_int(7)
    out = H.foe_host_unwrap(native, freq, f_coarse, fs, dist, 1 if usable else 0, C.byref(n))
    return out, n.value


@pytest.mark.parametrize("name, snr, cp_normal, f_off, n, native_ok", K.CRAFTED[:6], ids=[c[0] for c in K.CRAFTED[:6]])
def test_half_sums_estimate_and_decision_on_crafted_windows(H, name, snr, cp_normal, f_off, n, native_ok):
    r = K.crafted_ref(snr, cp_normal, f_off)
    det, cz, cap = r["detected"], r["coarse"], r["cap"]
    _, dist, first, _, step, n_sss = R.foe_geometry(det, cap.size, K.FC, K.FC, K.FS, K.TDD)
    assert n_sss == cz["n_occ"] >= 15
    kph = np.pi * (-det.freq) / (cz["fs"] / 2)
    p = np.ascontiguousarray(PC.pss_useful(det.n_id_2))
    A, B = np.zeros(n_sss, np.complex128), np.zeros(n_sss, np.complex128)
    worst = 0.0
    for k in range(n_sss):
        win = np.ascontiguousarray(cap[R._round_i(first + k * step) + dist + 2:][:128])
        a, b, s = np.zeros(2), np.zeros(2), C.c_double(0)
        H.foe_host_halves(_dp(win.view(np.float64)), kph, _dp(p.view(np.float64)), _dp(a), _dp(b), C.byref(s))
        A[k], B[k] = complex(*a), complex(*b)
        scale = np.abs(cz["z"][k]).sum()
        assert abs(s.value - scale) <= 1e-12 * scale
        worst = max(worst, abs(A[k] - cz["A"][k]) / scale, abs(B[k] - cz["B"][k]) / scale)
    Cc, ok = np.zeros(2), C.c_int(-1)
    f_coarse = H.foe_host_coarse(_dp(A.view(np.float64)), _dp(B.view(np.float64)), n_sss, cz["fs"], _dp(Cc), C.byref(ok))
    print(name, "worst |A, B error| / sum |z| %.2e" % worst, "f_coarse", f_coarse, "reference", cz["f_coarse"])
    assert worst <= 1e-12
    assert abs(complex(*Cc) - cz["C"]) <= 1e-12 * cz["scale"]
    assert abs(f_coarse - cz["f_coarse"]) <= 1e-6
    assert ok.value == 1
    got, n_got = _unwrap(H, r["native"].freq_fine, det.freq, cz["f_coarse"], cz["fs"], dist)
    assert n_got == r["n"] == n and got == r["unwrapped"].freq_fine      # == on the doubles
    if n == 0:
        assert got == r["native"].freq_fine


def test_decision_edges(H):
    fs, dist, freq, native = K.FS, 412, 5000.0, 6234.5
    period = fs / dist
    for q, n in ((0.49, 0), (-0.49, 0), (0.51, 1), (-0.51, -1), (1.6, 1), (-1.6, -1), (1e9, 1), (-1e9, -1)):
        f_coarse = (native - freq) + q * period
        got, n_got = _unwrap(H, native, freq, f_coarse, fs, dist)
        assert n_got == n == PC.unwrap_n(native, freq, f_coarse, fs, dist), q
        assert got == PC.unwrap(native, freq, f_coarse, fs, dist) == (native if n == 0 else native + n * period)
    # nothing usable: no occurrence, C zero, C not finite -- and a NaN that reaches the rule decides nothing either
    assert [H.foe_host_usable(*a) for a in ((1.0, 1.0, 0), (0.0, 0.0, 5), (-0.0, 0.0, 5), (np.nan, 1.0, 5), (1.0, np.inf, 5), (1e-300, 0.0, 1))] == [0, 0, 0, 0, 0, 1]
    assert _unwrap(H, native, freq, 3000.0, fs, dist, usable=False) == (native, 0)
    assert _unwrap(H, native, freq, float("nan"), fs, dist) == (native, 0)
    out, n = _unwrap(H, float("nan"), freq, 100.0, fs, dist)
    assert n == 0 and np.isnan(out)
    Cc, ok = np.zeros(2), C.c_int(-1)
    z = np.zeros(2, np.complex128)
    assert H.foe_host_coarse(_dp(z.view(np.float64)), _dp(z.view(np.float64)), 2, fs, _dp(Cc), C.byref(ok)) == 0.0 and ok.value == 0
    assert H.foe_host_coarse(_dp(z.view(np.float64)), _dp(z.view(np.float64)), 0, fs, _dp(Cc), C.byref(ok)) == 0.0 and ok.value == 0


def test_decision_with_the_extended_cp_distance_of_a_dongle(H):
    """quirk Q4: the extended-CP distance is round(480 k_factor), without the sample-rate ratio; with fc_programmed != fc_requested and a
    nonzero hypothesis the period is fs_programmed k_factor / dist"""
    fc_req, fc_prog, fs_prog = 1.9e9, 1.9e9 * (1 - 30e-6), 1.92e6 * 1.00002
    cell = O.new_cell(pss_pow=1.0, ind=3000, freq=5000.0, n_id_2=1, n_id_1=10, cp_type=2, frame_start=1234.5, fc_requested=fc_req, fc_programmed=fc_prog)
    k_factor, dist, _, _, _, _ = R.foe_geometry(cell, 153600, fc_req, fc_prog, fs_prog, K.TDD)
    assert dist == int(np.rint(480 * k_factor)) == 480 and k_factor != 1.0
    fs = fs_prog * k_factor
    period = fs / dist
    assert period != 4000.0
    for res_true in (-2400.0, -1990.0, 0.0, 1999.0, 2001.0, 2450.0):
        native = cell.freq + (res_true + period / 2) % period - period / 2      # what the native estimate makes of it
        for err in (-900.0, 0.0, 900.0):
            got, n = _unwrap(H, native, cell.freq, res_true + err, fs, dist)
            assert n == int(np.rint((cell.freq + res_true - native) / period)) == PC.unwrap_n(native, cell.freq, res_true + err, fs, dist)
            assert got == PC.unwrap(native, cell.freq, res_true + err, fs, dist)
            assert abs(got - (cell.freq + res_true)) < 1e-9
