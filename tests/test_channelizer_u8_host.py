"""The 8-bit channelizer output's two rules as the device runs them (channelizer.h: chan_u8_exponent, chan_u8_code, compiled for
the host in tests/host/chan_u8_host.cpp) against their numpy restatement (tests/chan_u8_ref.py), and the new symbol's ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import chan_rate_twin as T
import chan_u8_cases as K
import chan_u8_ref as U
from conftest import ROOT, load_pkg


@pytest.fixture(scope="module")
def host():
    L = T.host_lib("chan_u8_host")      # built here when build() has not left it, as the other twins' tests do
    L.chan_u8_host_exponents.argtypes = [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]
    L.chan_u8_host_codes.argtypes = [C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_ubyte)]
    return L


def _exponents(host, P):
    P = np.ascontiguousarray(P, np.float64)
    e = np.zeros(P.size, np.int32)
    host.chan_u8_host_exponents(P.ctypes.data_as(C.POINTER(C.c_double)), P.size, e.ctypes.data_as(C.POINTER(C.c_int)))
    return e


def _codes(host, z):
    z = np.ascontiguousarray(z, np.float32)
    c = np.zeros(z.size, np.uint8)
    host.chan_u8_host_codes(z.ctypes.data_as(C.POINTER(C.c_float)), z.size, c.ctypes.data_as(C.POINTER(C.c_ubyte)))
    return c


def test_exponent_at_every_power_of_two_boundary_and_its_float_neighbours(host):
    """P = 2^j * 512 sits ON an end of the interval for every other j (4^e P / 2 = 16^2 is outside, 32^2 inside): the value and its
    two float neighbours, j = -60 .. 60."""
    P = []
    for j in range(-60, 61):
        p = np.float32(np.ldexp(512.0, j))
        P += [float(np.nextafter(p, np.float32(0))), float(p), float(np.nextafter(p, np.float32(np.inf)))]
    P = np.array(P)
    got, want = _exponents(host, P), np.array([U.exponent(p) for p in P])
    assert np.array_equal(got, want), [(p, g, w) for p, g, w in zip(P, got, want) if g != w][:5]
    v = np.ldexp(P, 2 * got) / 2.0                      # the rule itself, in exact arithmetic
    assert np.all((v > U.LO) & (v <= U.HI))
    assert len(set(got)) >= 60                          # the cases do cross the exponents
    # the double neighbours too: the device sums P in double
    Pd = np.concatenate([[np.nextafter(p, 0.0), np.nextafter(p, np.inf)] for p in np.ldexp(512.0, np.arange(-60, 61))])
    assert np.array_equal(_exponents(host, Pd), [U.exponent(p) for p in Pd])


def test_exponent_of_zero_and_non_finite_power_is_zero(host):
    assert list(_exponents(host, [0.0, -0.0, np.inf, -np.inf, np.nan, -1.0])) == [0] * 6
    assert [U.exponent(p) for p in (0.0, np.inf, np.nan)] == [0, 0, 0]


def test_code_rounds_ties_to_even_and_clamps(host):
    half = np.arange(-130.0, 130.01, 0.5)               # every half-integer (and integer) in [-130, 130]
    z = np.concatenate([half, [127.5, -127.5, 128.5, -127.49]])
    got, want = _codes(host, z), U.code(z)
    assert np.array_equal(got, want), [(a, g, w) for a, g, w in zip(z, got, want) if g != w][:5]
    by = dict(zip(z.tolist(), got.tolist()))
    assert (by[0.5], by[1.5], by[2.5], by[-0.5], by[-1.5]) == (127, 129, 129, 127, 125)      # ties go to the even integer
    assert (by[127.5], by[128.5], by[128.0], by[130.0]) == (255, 255, 255, 255)
    assert (by[-127.5], by[-127.49], by[-127.0], by[-126.5], by[-130.0]) == (0, 0, 0, 1, 0)


def test_code_of_a_non_finite_value_is_127(host):
    z = np.array([np.nan, np.inf, -np.inf], np.float32)
    assert list(_codes(host, z)) == [127, 127, 127] == list(U.code(z))


def test_reference_quantiser_follows_the_rule():
    rng = np.random.default_rng(8)
    y = (rng.standard_normal((3, 4001)) + 1j * rng.standard_normal((3, 4001))) * np.array([1e-3, 1.0, 700.0])[:, None]
    y[1, 5] = 1e3                                       # one burst: clamps
    codes, g, z = U.quantise_ref(y)
    P = np.mean(np.abs(y) ** 2, axis=1)
    assert np.all((g * g * P / 2 > U.LO) & (g * g * P / 2 <= U.HI)) and len(set(g)) == 3
    assert codes.shape == (3, 4001, 2) and codes[1, 5, 0] == 255
    assert np.array_equal(codes, np.clip(127 + np.rint(z), 0, 255).astype(np.uint8))


def test_gpu_cases_hold_their_premises():
    """What tests/test_gpu_channelizer_u8.py rests on, from the reference alone: in every array case the rounding band holds under 1 % of
    a carrier's components, every carrier's 4^e P / 2 is at least 1 % away from both ends of (16^2, 32^2], and the exponents differ."""
    cases = [K.arrays_case(1, D, fmt, 257) for D, fmt in K.INTEGER] + [K.arrays_case(u, d, "s16", T.corner_n_out(u, d)) for u, d in K.RATIONAL]
    for c in cases:
        share, margin = K.premises(c)
        assert share < 0.01 and margin >= 0.01, (c["up"], c["down"], c["fmt"], share, margin)
        assert len(set(c["gain"])) >= 2
        if c["fmt"] == "c64":
            assert c["gain"].min() < 1.0
    b = K.burst_case()
    assert (b["codes"] == 0).sum() >= 4 and (b["codes"] == 255).sum() >= 4


def test_new_symbol_is_declared_exported_and_prototyped():
    pkg = load_pkg()
    hdr = open(os.path.join(ROOT, "include", "lcs.h")).read()
    assert re.search(r"\bint lcs_channelize_u8\s*\(lcs_ctx \*ctx, const void \*d_wide, int fmt, uint64_t n_in, double fs_in, int up, int down,", hdr)
    assert "lcs_channelize_u8" in pkg.capi.EXPORTS
    lib = pkg.capi.load()
    assert hasattr(lib, "lcs_channelize_u8")
    assert len(lib.lcs_channelize_u8.argtypes) == 12
    assert lib.lcs_channelize_u8(None, None, 0, 0, 0.0, 1, 2, None, 0, None, 0, None) == -2      # no context: refused without touching a GPU
