"""The PSS correlation's routing rule (csrc/xcorr_route.h: xc_route, compiled for the host in tests/host/xc_route_host.cpp) over its
whole domain, against the table written out below: which kernel a call takes, which of the kernels' buffer sets it ensures, whether a
complex<float> batch may be probed for dongle data, which tap limit its grid is packed for.  Also the two packing limits against the
kernels' tile constants, and the premise that lets lcs_batch_enqueue size its workspace by the int8 packing alone."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from test_pss_ref_host import H, N_CAP, PARAMS, _dp, _grid, _ip      # noqa: F401  (H: the fixture that loads pss_ref.h's host twin)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "lte-cell-scanner_amd", "csrc", "xcorr_route.h")
SRC = os.path.join(ROOT, "tests", "host", "xc_route_host.cpp")
LIB = os.path.join(ROOT, "tests", "host", "libxc_route_host.so")
CALLERS = ("host", "batch", "stream")
VERDICTS = ("unknown", "dongle", "other")

# caller, source (None: any), condition on (stream open, int8 set ready, fp16 set ready), sets ensured, kernel; "verdict": int8 if
# the ingest found every component to be dongle data, else fp32
TABLE = [
    ("host", None, lambda st, i8, f16: i8 or not st, {"i8"}, "verdict"),
    ("host", None, lambda st, i8, f16: st and not i8, set(), "fp32"),
    ("batch", "u8", lambda st, i8, f16: True, {"i8"}, "i8"),
    ("batch", "c64", lambda st, i8, f16: f16 or not st, {"f16"}, "f16"),
    ("batch", "c64", lambda st, i8, f16: st and not f16, set(), "fp32"),
    ("stream", "u8", lambda st, i8, f16: True, {"i8", "btab"}, "i8"),
    ("stream", "c64", lambda st, i8, f16: True, {"btab"}, "fp32"),
]


@pytest.fixture(scope="module")
def R():
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in (SRC, HEADER)):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC",
                               "-shared", "-I" + os.path.join(ROOT, "include"), "-o", LIB, SRC])
    r = C.CDLL(LIB)
    r.xc_route_call.argtypes = [C.c_int] * 9 + [C.POINTER(C.c_int)]
    r.xc_route_call.restype = C.c_char_p
    r.xc_route_probe_fits.argtypes = [C.c_ulonglong, C.c_ulonglong]
    r.xc_route_limits.argtypes = [C.POINTER(C.c_int)]
    lim = np.zeros(7, np.int32)
    r.xc_route_limits(_ip(lim))
    r.taps = dict(zip(("fp32", "i8", "f16", "single_exact"), (int(v) for v in lim[:4])))
    r.i8_off, r.kp2_max, r.kp2_unroll = (int(v) for v in lim[4:])
    return r


def test_the_rule_is_the_table_over_its_whole_domain(R):
    n = 0
    for caller, src, st, i8, f16, verdict, n_comb, probe_on, fits in itertools.product(CALLERS, ("u8", "c64"), (0, 1), (0, 1), (0, 1), VERDICTS,
                                                                                       (1, 2, 15), (0, 1), (0, 1)):
        rows = [r for r in TABLE if r[0] == caller and r[1] in (None, src) and r[2](st, i8, f16)]
        assert len(rows) == 1, (caller, src, st, i8, f16)                           # the table's conditions split the domain
        _, _, _, sets, kernel = rows[0]
        if kernel == "verdict":
            kernel = "i8" if verdict == "dongle" else "fp32"
        packed_for = kernel                                                        # ... before k_single_exact takes a one-window call over
        if n_comb == 1:
            kernel = "single_exact"
        out = np.zeros(5, np.int32)
        got = R.xc_route_call(CALLERS.index(caller), src == "u8", st, i8, f16, n_comb, VERDICTS.index(verdict), probe_on, fits, _ip(out)).decode()
        case = (caller, src, st, i8, f16, verdict, n_comb, probe_on, fits)
        assert got == kernel, case
        assert {s for s, on in zip(("i8", "f16", "btab"), out[:3]) if on} == sets, case
        # the float probe: a complex<float> batch, the probe switched on, the int8 set there or allowed, an even sample count at a
        # 16-byte aligned address
        assert bool(out[3]) == (caller == "batch" and src == "c64" and bool(probe_on) and bool(i8 or not st) and bool(fits)), case
        # the host caller packs for the kernel it takes, the batch caller for the int8 limit whatever follows (the stream has one hypothesis)
        if caller == "host":
            assert out[4] == R.taps[packed_for], case
        elif caller == "batch":
            assert out[4] == R.taps["i8"], case
        n += 1
    assert n == 3 * 2 * 8 * 3 * 3 * 4


def test_probe_fits_even_counts_at_aligned_addresses(R):
    for n, addr, want in [(153600, 0x7F0000000000, 1), (153601, 0x7F0000000000, 0), (2 * 19437, 0x7F0000000010, 1), (153600, 0x7F0000000008, 0),
                          (153600, 0x7F0000000004, 0), (3 * 19437, 0x7F0000000000, 0), ((1 << 32) + 2, 1 << 40, 1)]:
        assert R.xc_route_probe_fits(n, addr) == want, (n, hex(addr))


def test_tap_limits_follow_the_kernels_tiles(R):
    """int8 (and fp16, which shares its packing): 137 taps + delays below LCS_I8_OFF; fp32: LCS_KP2_MAX tap pairs less one unrolled
    step.  k_single_exact reads no operand image: it takes the int8 packing."""
    assert R.taps["i8"] == R.taps["f16"] == R.taps["single_exact"] == 137 + R.i8_off - 1 == 152
    assert R.taps["fp32"] == 2 * (R.kp2_max - R.kp2_unroll) == 248


def test_int8_packing_never_has_fewer_groups_than_fp32_packing(R, H):
    """lcs_batch_enqueue packs for the int8 limit and sizes the workspace by that G alone, although a complex<float> batch under an
    open stream falls back to the fp32 kernel: the fp32 limit is the larger one, so its packing of the same grid is at least as dense."""
    assert (H.max_taps_i8, H.max_taps_f32) == (R.taps["i8"], R.taps["fp32"]) and R.taps["i8"] < R.taps["fp32"]
    thinner = 0
    for prm in PARAMS:
        for n_f in (1, 3, 31, 37, 125):
            for step in (5e3, 10e3, 20e3, 40e3, 100e3, 400e3):
                f = _grid(n_f, step)
                g8, g32 = np.zeros(4, np.int32), np.zeros(4, np.int32)
                H.pss_ref_pack_grid(N_CAP, n_f, 2, _dp(f), *prm, R.taps["i8"], _ip(g8))
                H.pss_ref_pack_grid(N_CAP, n_f, 2, _dp(f), *prm, R.taps["fp32"], _ip(g32))
                assert g8[1] >= g32[1] and g8[0] <= g32[0], (prm, n_f, step, g8.tolist(), g32.tolist())
                thinner += int(g8[1] > g32[1])
    assert thinner > 0      # (the grids do reach packings where the two limits differ)


def test_the_header_needs_neither_hip_nor_a_context():
    subprocess.check_call(["c++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-include", HEADER, "-x", "c++", os.devnull])
