"""Grids and captures the tests of the full-bandwidth measurement share (tests/test_meas_wide_host.py, tests/test_gpu_meas_wide.py)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import meas_wide_ref as WR
import tdd_config_ref as TR
from conftest import load_pkg

# (R, n_rb) of the issue's set: every transform length, the widest n_rb of each, a narrower one at 2048 (three passes of the wave),
# and 6 RB on a long transform; the CP types alternate over the set
SHAPES = [(1, 6), (2, 15), (4, 25), (8, 50), (16, 100), (16, 75), (8, 6)]
CP_OF = {s: 1 + (i & 1) for i, s in enumerate(SHAPES)}
MASKS = [0x3FF, 0x021, 0x200, 0x339]
FC = 739e6


def crafted_grid(n_id_cell, cp_type, n_rb, n_ofdm, seed=0, snr_db=15.0, n_ports=2):
    """A grid [n_ofdm][12 n_rb] whose rows carry the n_rb reference sequence of ports < n_ports times a smooth channel (a common phase
    per row, a phase ramp over the subcarriers like a timing offset, a slow amplitude ripple), QPSK data elsewhere, and noise."""
    rng = np.random.default_rng(seed)
    rs, sh = WR.rs_wide(n_id_cell, cp_type, n_rb)
    n, nc = TR.n_symb_of(cp_type), 12 * n_rb
    k = np.arange(nc)
    qpsk = lambda size: ((1 - 2.0 * rng.integers(0, 2, size)) + 1j * (1 - 2.0 * rng.integers(0, 2, size))) / np.sqrt(2.0)
    sigma = 10 ** (-snr_db / 20) / np.sqrt(2.0)
    tau, f_row = 0.37 + 0.2 * rng.random(), 0.013 * (rng.random() - 0.5)
    gain = np.exp(2j * np.pi * rng.random(2)) * (0.8 + 0.4 * rng.random(2))
    tfg = np.zeros((n_ofdm, nc), np.complex128)
    for r in range(n_ofdm):
        sym, slot = r % n, (r // n) % 20
        ramp = np.exp(-2j * np.pi * tau * (k - (nc - 1) / 2) / (128.0 * n_rb / 6)) * np.exp(2j * np.pi * f_row * r)
        ripple = 1.0 + 0.25 * np.cos(2 * np.pi * k / nc + r / 57.0)
        row = 0.7 * qpsk(nc) * ramp * ripple * gain[0]
        if sym in (0, n - 3):
            b = 2 * slot + (sym != 0)
            for port in range(2):
                idx = int(sh[b, port]) + 6 * np.arange(2 * n_rb)
                row[idx] = rs[b] * ramp[idx] * ripple[idx] * gain[port] if port < n_ports else 0.0
        tfg[r] = row + sigma * (rng.standard_normal(nc) + 1j * rng.standard_normal(nc))
    return tfg


@functools.lru_cache(maxsize=None)
def shape_grid(n_rb, cp_type, n_ofdm=None, n_ports=2):
    n = TR.n_symb_of(cp_type)
    return crafted_grid(100 + n_rb, cp_type, n_rb, 40 * n + 3 if n_ofdm is None else n_ofdm, seed=n_rb, n_ports=n_ports)


@functools.lru_cache(maxsize=None)
def noise_capture(R, seed=0):
    """25 ms of complex64 noise-like samples at 1.92e6 R: any capture serves where the grid stage is held to numpy"""
    rng = np.random.default_rng(1000 + seed)
    n = int(0.025 * 1.92e6 * R)
    return (0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


# ---------------------------------------------------------------- the host twin (tests/host/meas_wide_host.cpp)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lte-cell-scanner_amd", "csrc")
TWIN_SRC = os.path.join(ROOT, "tests", "host", "meas_wide_host.cpp")
TWIN_LIB = os.path.join(ROOT, "tests", "host", "libmeas_wide_host.so")
HIPCC = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include")]
_dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
_ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))


def stale(target, src):
    dep = [src] + [os.path.join(CSRC, h) for h in ("cell_meas_wide.h", "cell_meas.h", "tdd_config.h", "lte_device.h", "lcs_internal.h")] + [os.path.join(ROOT, "include", "lcs.h")]
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in dep)


def load_twin(capi):
    """cell_meas_wide.h compiled for the host (built where it is missing or older than its sources)"""
    if stale(TWIN_LIB, TWIN_SRC):
        subprocess.check_call(HIPCC + ["-O2", "-fPIC", "-shared", "-o", TWIN_LIB, TWIN_SRC])
    h = C.CDLL(TWIN_LIB)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    h.meas_wide_host.argtypes = [dp, C.c_int, C.c_int, C.c_int, C.c_int, dp, ip, C.c_int, C.c_int, dp, C.POINTER(capi.CellMeasWide)]
    h.meas_wide_host.restype = None
    h.meas_wide_host_rs_row.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_uint32), dp, dp]
    h.meas_wide_host_rs_row.restype = None
    h.meas_wide_host_col_of_bin.argtypes = [C.c_int, C.c_int, C.c_int, ip]
    return h


def twin_record(H, capi, n_id_cell, cp, tfg, n_rb, n_fft, n_ports, mask):
    """-> (the seven totals, the record) of the host twin on a grid [n_ofdm][12 n_rb]"""
    rs, sh = WR.rs_wide(n_id_cell, cp, n_rb)
    rs, sh = np.ascontiguousarray(rs), np.ascontiguousarray(sh, np.int32)
    tfg = np.ascontiguousarray(tfg, np.complex128)
    tot = np.zeros(7)
    o = capi.CellMeasWide()
    H.meas_wide_host(_dp(tfg.view(np.float64)), tfg.shape[0], TR.n_symb_of(cp), n_rb, n_fft, _dp(rs.view(np.float64)), _ip(sh), n_ports, mask, _dp(tot), C.byref(o))
    return tot, o


# ---------------------------------------------------------------- captures with a wide cell in them
GEN_RB = {1: 6, 2: 15, 4: 25, 8: 50, 16: 100}      # the generator's bandwidth per rate; a test may measure fewer RBs
CELL_ID = (41, 2)                                   # n_id_1, n_id_2
FRAME_START = 1234.37                               # in 1.92 Msps samples: times R in the capture's


@functools.lru_cache(maxsize=None)
def cell_capture(R, cp_type, snr_db=20.0):
    """three frames of a two-port cell at 1.92e6 R behind FRAME_START R samples (rounded down) of silence, in noise, as complex64"""
    pkg = load_pkg()
    rng = np.random.default_rng(77 + R + cp_type)
    w = pkg.synth.cell_waveform_wide(3, CELL_ID[0], CELL_ID[1], R, GEN_RB[R], cp_type == 1, n_ports=2, rng=rng)
    cap = np.concatenate([np.zeros(int(FRAME_START * R), np.complex128), w])
    sigma = np.sqrt(0.5 / 10 ** (snr_db / 10) / 2)
    return (0.2 * (cap + sigma * (rng.standard_normal(cap.size) + 1j * rng.standard_normal(cap.size)))).astype(np.complex64)
