"""The dongle-data predicate (lte_device.h dongle_component_f32 / _f64: what k_c64_probe_u8 and k_ingest_c128 decide by) compiled for
the HOST and pinned to its specification: a component is accepted iff it COMPARES EQUAL to (b - 127) / 128 for a byte b, and the byte
returned is that b.  The float flavour runs over ALL 2^32 bit patterns against a sorted table built by integer arithmetic (exactly 257
accepted: the 256 codes and -0.0); the double flavour over the codes, their 1- and 2-ulp neighbours, zeros, subnormals, scaled codes,
the first values beyond the range, NaN and the infinities.  The expression the float probe used before (x * 128 + 127 tested after
the addition rounded) is swept too and must FAIL the specification: it accepts 1 711 277 695 patterns -- every |x| < 2^-25 and
every value within half an ulp of the sum beside a code."""
import ctypes as C
import os
import subprocess
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "probe_host.cpp")
LIB = os.path.join(ROOT, "tests", "host", "libprobe_host.so")
N_THREADS = 16          # sized for a 16-CPU machine whatever os.cpu_count() says: ~1 ns per pattern per thread


@pytest.fixture(scope="module")
def H():
    dep = [SRC, os.path.join(ROOT, "lte-cell-scanner_amd", "csrc", "lte_device.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in dep):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC",
                               "-shared", "-pthread", "-I" + os.path.join(ROOT, "include"), "-o", LIB, SRC])
    h = C.CDLL(LIB)
    h.probe_host_sweep_f32.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_ulonglong)]
    h.probe_host_sweep_f32.restype = None
    for name, t in (("probe_host_f32", C.c_float), ("probe_host_f64", C.c_double), ("probe_host_old_f32", C.c_float)):
        getattr(h, name).argtypes = [t, C.POINTER(C.c_ubyte)]
    return h


def _one(fn, x):
    b = C.c_ubyte(0)
    return bool(fn(float(x), C.byref(b))), b.value      # (float() of a numpy float32 is exact)


def test_float_predicate_over_all_bit_patterns(H):
    out = (C.c_ulonglong * 4)()
    t0 = time.time()
    H.probe_host_sweep_f32(0, N_THREADS, out)
    print(f"2^32 float patterns through dongle_component_f32 on {N_THREADS} threads: {time.time() - t0:.1f} s; accepted {out[0]}")
    assert out[2] == 257, "the reference table itself: 256 codes and -0.0"
    assert out[1] == 0, f"{out[1]} patterns decided differently from the table, the first 0x{out[3]:08x}"
    assert out[0] == 257


def test_the_rounded_sum_expression_fails_the_same_sweep(H):
    """x * 128 + 127 (one fma) tested for integrality AFTER the addition rounded -- what k_c64_probe_u8 did: the sweep that passes
    above must refuse it."""
    out = (C.c_ulonglong * 4)()
    H.probe_host_sweep_f32(1, N_THREADS, out)
    print(f"old expression: accepted {out[0]} of 2^32 patterns, {out[1]} decided differently from the table")
    assert out[2] == 257
    assert out[0] > 257 and out[1] == out[0] - 257      # it takes every true code (with the right byte) and far too many others
    # the examples the predicate's comment names
    for x in (np.float32(2.0 ** -30), np.nextafter(np.float32(1 / 128), np.float32(1)), np.float32(1e-40)):
        assert _one(H.probe_host_old_f32, x)[0] and not _one(H.probe_host_f32, x)[0], x


def _codes64():
    return [(b, (b - 127) / 128.0) for b in range(256)]


def test_double_predicate_on_the_codes_and_their_neighbours(H):
    f64 = H.probe_host_f64
    for b, x in _codes64():
        assert _one(f64, x) == (True, b), b
        for away in (-np.inf, np.inf):
            y = x
            for _ in range(2):                               # 1 and 2 ulps to either side
                y = float(np.nextafter(y, away))
                assert y != x and not _one(f64, y)[0], (b, y)
        if b != 127:
            assert not _one(f64, x * 2.0 ** -30)[0], b      # a code scaled down: exact in double, off the grid
            assert not _one(f64, x * 0.5)[0] or (b - 127) % 2 == 0, b
    assert _one(f64, 0.0) == (True, 127) and _one(f64, -0.0) == (True, 127)
    tiny = np.finfo(np.float64).tiny
    for x in (5e-324, -5e-324, tiny / 2, -tiny / 2, tiny, 2.0 ** -30, -2.0 ** -30, 2.0 ** -60, 1e-300,
              1 + 1 / 128, -(1 + 1 / 128), 129 / 128, -1.0, -128 / 128, 1.5, 255.0, 1e300, np.nan, np.inf, -np.inf):
        assert not _one(f64, float(x))[0], x
    assert _one(f64, 1.0) == (True, 255) and _one(f64, -127 / 128) == (True, 0)


def test_float_predicate_on_the_named_edges(H):
    """The same edges through the float flavour by value (the sweep above covers them by pattern; these name them)."""
    f32 = H.probe_host_f32
    for b, x in _codes64():
        assert _one(f32, np.float32(x)) == (True, b)
        for away in (-np.inf, np.inf):
            y = np.float32(x)
            for _ in range(2):
                y = np.nextafter(y, np.float32(away))
                assert not _one(f32, y)[0], (b, y)
    assert _one(f32, np.float32(-0.0)) == (True, 127)
    for x in (1e-45, -1e-45, 1e-39, 2.0 ** -30, 2.0 ** -25, 2.0 ** -24, 1 + 1 / 128, -1.0, np.nan, np.inf, -np.inf):
        assert not _one(f32, np.float32(x))[0], x
