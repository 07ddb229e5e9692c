"""The bound the batch screen decides by (csrc/screen_bound.h, compiled for the host in tests/host/screen_bound_host.cpp), against
brute-force integer correlations in NumPy: what dropping digit 0 of the 24-bit template integers changes in a window's correlation,
in the power summed over 2, 3 and 15 windows, in its box filter and in the maximum over columns never exceeds the function's value --
and adversarial captures (every sample +-127 / -128, aligned in sign with the dropped digit) come within a factor of two of it, so the
bound under test is one that is approached.  Also the branch that tells the caller to flag everything."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "lte-cell-scanner_amd", "csrc", "screen_bound.h")
SRC = os.path.join(ROOT, "tests", "host", "screen_bound_host.cpp")
LIB = os.path.join(ROOT, "tests", "host", "libscreen_bound_host.so")
K, DS, W = 137, 2, 180                     # taps, box-filter arm, distance of the window starts in the synthetic captures
LAGS = 9                                   # lags correlated per case: 5 box-filtered positions
QMAX = 8.3e6


@pytest.fixture(scope="module")
def B():
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in (SRC, HEADER)):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC",
                               "-shared", "-o", LIB, SRC])
    b = C.CDLL(LIB)
    b.screen_err.argtypes = [C.c_double]
    b.screen_bound.argtypes = [C.c_double, C.c_double]
    b.screen_slack.argtypes = [C.c_int, C.c_int]
    b.screen_threshold.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double]
    for f in (b.screen_err, b.screen_bound, b.screen_slack, b.screen_threshold):
        f.restype = C.c_double
    return b


def digits(v):
    """v = d0 + 256 d1 + 65536 d2 with balanced digits, as the fill kernel splits it."""
    d0 = ((v + 128) & 255) - 128
    v1 = (v - d0) >> 8
    d1 = ((v1 + 128) & 255) - 128
    return d0, d1, (v1 - d1) >> 8


def columns(rng):
    """Template integers [column][tap] (re, im).  Column 0: every dropped digit -128 and the upper digits pointing the same way (the
    worst case: one capture is aligned with it at every lag).  Column 1: random dropped digits under a strong upper part.  Column 2:
    random 24-bit integers."""
    c0 = np.full((K, 2), -128 - 256 * 128 - 65536 * 126, np.int64)
    d0 = rng.integers(-128, 128, (K, 2))
    c1 = d0 + 256 * rng.integers(-128, 128, (K, 2)) + 65536 * np.where(d0 < 0, -120, 120)
    c2 = rng.integers(-8300000, 8300001, (K, 2))
    t = np.stack([c0, c1, c2])
    assert np.abs(t).max() <= QMAX
    return t


def capture(n_win, align_to, lag, rng):
    """int8 pairs of n_win windows: random +-127 / -128 everywhere, and at lag `lag` of every window aligned in sign with the dropped
    digit of the column `align_to` [tap][2] so that the real part of the dropped sum is as large as it can be."""
    n = (n_win - 1) * W + K + LAGS
    a = np.where(rng.integers(0, 2, (n, 2)) == 1, 127, -128).astype(np.int64)
    if align_to is not None:
        d0 = digits(align_to)[0]
        for w in range(n_win):
            s = w * W + lag
            # Re sum(a d) = sum ar dr - ai di: ar follows the sign of dr, ai the opposite of di's
            a[s:s + K, 0] = np.where(d0[:, 0] < 0, -128, 127)
            a[s:s + K, 1] = np.where(d0[:, 1] < 0, 127, -128)
    return a


def correlate(a, t, n_win):
    """Complex integer correlations [window][lag][column] of the kernel's operands: x = sum_k a_k t_k."""
    out = np.zeros((n_win, LAGS, t.shape[0], 2), np.int64)
    for w in range(n_win):
        for l in range(LAGS):
            s = a[w * W + l: w * W + l + K]
            out[w, l, :, 0] = (s[None, :, 0] * t[:, :, 0] - s[None, :, 1] * t[:, :, 1]).sum(1)
            out[w, l, :, 1] = (s[None, :, 0] * t[:, :, 1] + s[None, :, 1] * t[:, :, 0]).sum(1)
    return out


def powers(x, sc, n_win):
    """single [lag][column], its box filter [position][column] and the maximum over the columns [position], in the kernel's units."""
    single = (x.astype(np.float64) ** 2).sum(-1).sum(0) * sc[None, :] ** 2 / n_win
    box = np.stack([single[p - DS:p + DS + 1].mean(0) for p in range(DS, LAGS - DS)])
    return single, box, box.max(1)


@pytest.mark.parametrize("n_win", [2, 3, 15])
def test_the_dropped_digit_stays_within_the_bound_and_comes_close(B, n_win):
    rng = np.random.default_rng(7 + n_win)
    t = columns(rng)
    t_hi = t - digits(t)[0]                                  # what the two upper digit passes multiply
    sc = np.array([1.0 / (128.0 * QMAX / m) for m in (0.11, 0.10, 0.09)])      # 1 / (128 q), q = QMAX / largest tap
    e = np.array([B.screen_err(float(s)) for s in sc])
    closest = 0.0
    const = np.tile(np.array([[-128, 127]], np.int64), ((n_win - 1) * W + K + LAGS, 1))      # aligned with column 0 at EVERY lag
    cases = [const, capture(n_win, t[1], LAGS // 2, rng), capture(n_win, t[2], LAGS // 2, rng), capture(n_win, None, 0, rng)]
    for a in cases:
        x, xs = correlate(a, t, n_win), correlate(a, t_hi, n_win)
        # a window's correlation moves by at most E = e / sc
        d = np.sqrt(((x - xs).astype(np.float64) ** 2).sum(-1))
        assert (d <= e / sc * (1 + 1e-12)).all()
        for v, vs, ee in zip(powers(x, sc, n_win), powers(xs, sc, n_win), (e[None, :], e[None, :], e.max())):
            bound = 2.0 * ee * np.sqrt(v) + ee * ee
            ref = np.vectorize(B.screen_bound)(np.broadcast_to(ee, v.shape), v)
            assert np.allclose(ref, bound, rtol=1e-14, atol=0)
            ratio = np.abs(vs - v) / ref
            assert (ratio <= 1 + 1e-12).all(), ratio.max()
            closest = max(closest, float(ratio.max()))
        # the threshold: an exact collapsed power V has a screened twin at or above T(V)
        _, _, vmax = powers(x, sc, n_win)
        _, _, vsmax = powers(xs, sc, n_win)
        for V, Vs in zip(vmax, vsmax):
            T = B.screen_threshold(n_win, DS, float(sc.max()), float(V))
            assert T < V
            assert T < 0 or Vs >= T, (V, Vs, T)
    assert closest >= 0.5, closest                           # the bound is approached: it is being tested


def test_where_no_threshold_exists_the_caller_is_told_to_flag_everything(B):
    sc = 1.0 / (128.0 * QMAX / 0.1)
    e = B.screen_err(sc)
    assert e == pytest.approx(np.sqrt(2.0) * 128 * 274 * 128 * sc, rel=1e-15) and e >= np.sqrt(2.0) * 128 * 274 * 128 * sc
    for n_win in (2, 15):
        # not increasing in Z at and below e^2 (a silent buffer), not positive a little above it
        for Z in (0.0, -1.0, 1e-300, 0.5 * e * e, e * e, 2.0 * e * e, 5.8 * e * e, float("nan"), float("inf")):
            assert B.screen_threshold(n_win, DS, sc, Z) == -1.0, Z
        assert B.screen_threshold(n_win, DS, 0.0, 1.0) == -1.0 and B.screen_threshold(n_win, DS, float("nan"), 1.0) == -1.0
        assert B.screen_threshold(n_win, DS, float("inf"), 1.0) == -1.0
        # above that: positive, below Z by the bound and the slack, and increasing
        zs = e * e * np.geomspace(6.0, 1e12, 400)
        ts = np.array([B.screen_threshold(n_win, DS, sc, float(z)) for z in zs])
        assert (ts > 0).all() and (np.diff(ts) > 0).all()
        want = (zs - (2 * e * np.sqrt(zs) + e * e)) * (1 - B.screen_slack(n_win, DS))
        assert np.allclose(ts, want, rtol=1e-14, atol=0) and (ts < zs).all()
    # the slack covers the roundings it is derived from: (4 n + 2 ds + 4) 2^-23 of both epilogues and the collapse, and 1e-7 beside
    for n_win in (2, 3, 15):
        assert B.screen_slack(n_win, DS) >= (4 * n_win + 2 * DS + 4) * 2.0 ** -23 + 1e-7
