"""The PBCH de-rate-matching tables of lte_tables.cpp compiled for the host (tests/host/pbch_host.cpp) -- the very functions
lcs_create calls for the `derm_inv` table that the decoder reads -- against the oracle's de-rate-matcher probed with one-hot inputs:
a 1 at position t of e_est comes out at coded bit (stream, column) as 1 / (number of observations of that bit)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import pbch_ref as PB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lte-cell-scanner_amd", "csrc")
TWIN_SRC = os.path.join(ROOT, "tests", "host", "pbch_host.cpp")
TWIN_LIB = os.path.join(ROOT, "tests", "host", "libpbch_host.so")
HIPCC = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include")]


@pytest.fixture(scope="module")
def H():
    dep = [TWIN_SRC, os.path.join(CSRC, "lte_tables.cpp"), os.path.join(CSRC, "lcs_internal.h")]
    if not os.path.exists(TWIN_LIB) or any(os.path.getmtime(d) > os.path.getmtime(TWIN_LIB) for d in dep):
        subprocess.check_call(HIPCC + ["-O2", "-fPIC", "-shared", "-o", TWIN_LIB, TWIN_SRC])
    h = C.CDLL(TWIN_LIB)
    h.pbch_host_deratematch_map.argtypes = [C.c_int, C.POINTER(C.c_uint8)]
    h.pbch_host_deratematch_map.restype = None
    h.pbch_host_derm_inv.argtypes = [C.c_int, C.POINTER(C.c_int16)]
    return h


def oracle_probe(n_e):
    """position -> coded bit, and the observation count of every coded bit, from one-hot inputs"""
    which, count = np.empty(n_e, np.int64), np.zeros(120, np.int64)
    for t in range(n_e):
        e = np.zeros(n_e)
        e[t] = 1.0
        d = O.conv_deratematch(e).reshape(-1)
        nz = np.flatnonzero(d)
        assert nz.size == 1, (n_e, t)
        which[t] = nz[0]
        n = 1.0 / d[nz[0]]
        assert abs(n - round(n)) < 1e-9
        count[nz[0]] = int(round(n))
    return which, count


@pytest.mark.parametrize("n_e", [1920, 1728])
def test_tables_against_the_oracles_deratematcher(H, n_e):
    which, count = oracle_probe(n_e)
    assert np.array_equal(np.bincount(which, minlength=120), count) and count.sum() == n_e
    fwd = np.zeros(n_e, np.uint8)
    H.pbch_host_deratematch_map(n_e, fwd.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert np.array_equal(fwd.astype(np.int64), which)
    inv = np.full((120, 16), -7, np.int16)
    assert H.pbch_host_derm_inv(n_e, inv.ctypes.data_as(C.POINTER(C.c_int16))) == 1
    assert count.max() <= 16 and count.min() >= 1
    for bit in range(120):
        lst = inv[bit]
        n = int(count[bit])
        assert np.array_equal(lst[:n], np.flatnonzero(which == bit)), bit            # every position that carries the bit, ascending
        assert (np.diff(lst[:n]) > 0).all() and (lst[n:] == -1).all(), bit
    # the numpy reference's map (the generator's rate matcher run on the bits' numbers) is the same one
    assert np.array_equal(PB.coded_bit_of(n_e), which)


def test_a_longer_sequence_is_refused(H):
    """17 observations of a coded bit do not fit a row of the table"""
    inv = np.zeros((120, 16), np.int16)
    assert H.pbch_host_derm_inv(1921, inv.ctypes.data_as(C.POINTER(C.c_int16))) == 0
