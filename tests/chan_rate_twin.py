"""The host twin of the rational channelizer (tests/host/chan_rate_host.cpp: a workgroup of channelizer_rate.hip walked on the CPU
with the kernel's own index helpers of channelizer.h), built on demand and wrapped for numpy; the rate domain and its corners.
Shared by tests/test_channelizer_rate_twin_host.py and tests/test_gpu_channelizer_rate.py; host_lib builds and loads the other
host twins of channelizer.h the same way (tests/test_channelizer_u8_host.py, tests/test_channelizer_args_host.py)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lte-cell-scanner_amd", "csrc")
FMT = {"c64": 0, "s8": 3, "s16": 4}          # LCS_FMT_C64, LCS_FMT_IQ_S8, LCS_FMT_IQ_S16 (include/lcs.h)
CR_LDS_MAX = 48 * 1024

# every rate lcs_channelize_rational takes on its own kernel: gcd 1, 2 <= up < down <= 128, down <= 16 up
PAIRS = [(u, d) for u in range(2, 128) for d in range(u + 1, 129) if d <= 16 * u and math.gcd(u, d) == 1]
MARKETED = [(12, 125), (3, 4), (24, 125), (8, 25), (15, 16), (96, 125)]
# (up, down, format): 127 residues dealt to four waves; G = 64, the longest window, ratio 15.9; down at its limit; the LDS maximum
# (49140 bytes, NI = 2, 62 tiles); NI = 3 and NI = 2 held there by the LDS cap; the smallest up and down (NI = 4); NI = 4 with 62 tap
# groups; 28 tiles; 33 tiles, one wave gets a ninth
CORNERS = [(127, 128, "s16"), (8, 127, "s16"), (9, 128, "s16"), (31, 94, "c64"), (3, 47, "s16"), (5, 79, "s16"), (2, 3, "s8"), (2, 31, "s16"),
           (7, 8, "s16"), (33, 64, "s16")]

_lib = None


def noise_and_tones(seed, n_in, fs_in):
    """the signal of tests/test_gpu_channelizer.py"""
    rng = np.random.default_rng(seed)
    x = 0.1 * (rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in))
    n = np.arange(n_in, dtype=np.float64)
    for f, a in ((0.013e6, 0.2), (-0.31e6, 0.15), (0.21 * fs_in, 0.25), (-0.449 * fs_in, 0.2)):
        x += a * np.exp(2j * np.pi * (f / fs_in) * n + 1j * rng.uniform(0, 2 * np.pi))
    return x


def shifts17(fs_in):
    """one full block of 16 carriers plus one: 0, +-100 kHz, two off the raster, +-0.45 fs_in, the Nyquist edge, nine more"""
    return np.array([0.0, 100e3, -100e3, 0.0617283 * fs_in, -0.0493827 * fs_in, 0.45 * fs_in, -0.45 * fs_in, 0.5 * fs_in]
                    + [(-0.41 + 0.097 * k) * fs_in for k in range(9)])


def host_lib(name):
    """tests/host/lib<name>.so of tests/host/<name>.cpp, a host twin of channelizer.h, rebuilt when a file it is compiled from is newer"""
    src, lib_path = os.path.join(ROOT, "tests", "host", name + ".cpp"), os.path.join(ROOT, "tests", "host", "lib" + name + ".so")
    dep = [src, os.path.join(CSRC, "channelizer.h"), os.path.join(CSRC, "lcs_internal.h"), os.path.join(ROOT, "include", "lcs.h")]
    if not os.path.exists(lib_path) or any(os.path.getmtime(d) > os.path.getmtime(lib_path) for d in dep):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC",
                               "-shared", "-I" + os.path.join(ROOT, "include"), "-o", lib_path, src])
    return C.CDLL(lib_path)


def lib():
    """the twin of the rational kernel"""
    global _lib
    if _lib is None:
        h = host_lib("chan_rate_host")
        ip, fp, up = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_ulonglong)
        h.cr_host_geometry.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_longlong)]
        h.cr_host_geometry.restype = None
        h.cr_host_table.argtypes = [up, fp, C.c_int, C.c_int, C.c_int, fp]
        h.cr_host_table.restype = None
        h.cr_host_read_offsets.argtypes = [C.c_int, C.c_int, ip]
        h.cr_host_read_offsets.restype = None
        h.cr_host_stage_offsets.argtypes = [C.c_int, C.c_int, ip]
        h.cr_host_stage_offsets.restype = None
        h.cr_host_store_census.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint, ip]
        h.cr_host_store_census.restype = C.c_longlong
        h.cr_host_run.argtypes = [C.c_int, C.c_void_p, C.c_ulonglong, C.c_int, C.c_int, up, fp, C.c_int, fp, C.c_uint]
        h.cr_host_run.restype = C.c_longlong
        _lib = h
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def geometry(U, D):
    """-> (G, NI, xrows, LDS bytes) of the launcher"""
    g = np.zeros(4, np.int64)
    lib().cr_host_geometry(U, D, _p(g, C.c_longlong))
    return tuple(int(v) for v in g)


def corner_n_out(U, D):
    """one full workgroup, a second nearly empty one, a partial residue cycle"""
    return 32 * geometry(U, D)[1] * U + U + 1


def step(f_shift, fs_in):
    """lcs_chan_step: 2^64 frac(df / fs_in) in two's complement"""
    v = math.ldexp(float(f_shift) / float(fs_in), 64)
    return 1 << 63 if v >= 2.0 ** 63 else int(np.rint(v)) % (1 << 64)


def steps(f_shift, fs_in):
    return np.array([step(f, fs_in) for f in f_shift], np.uint64)


def table(st, taps, U, D):
    """k_chan_rate_tables -> [n_rb][U][G][64 lanes][4]"""
    st, taps = np.ascontiguousarray(st, np.uint64), np.ascontiguousarray(taps, np.float32)
    G, n_rb = geometry(U, D)[0], (st.size + 15) // 16
    tab = np.full((n_rb, U, G, 64, 4), np.nan, np.float32)
    lib().cr_host_table(_p(st, C.c_ulonglong), _p(taps, C.c_float), st.size, U, D, _p(tab, C.c_float))
    return tab


def read_offsets(U, D):
    """-> [U NI tiles][4 G k-steps][64 lanes] LDS float offsets"""
    G, NI, _, _ = geometry(U, D)
    o = np.full((U * NI, 4 * G, 64), -1, np.int32)
    lib().cr_host_read_offsets(U, D, _p(o, C.c_int))
    return o


def stage_offsets(U, D):
    o = np.full(geometry(U, D)[2] * D, -1, np.int32)
    lib().cr_host_stage_offsets(U, D, _p(o, C.c_int))
    return o


def store_census(U, D, n_ch, n_out):
    cnt = np.zeros((n_ch, n_out), np.int32)
    outside = lib().cr_host_store_census(U, D, n_ch, n_out, _p(cnt, C.c_int))
    return cnt, int(outside)


def run(q, fmt, n_in, U, D, st, taps, n_out, fill=np.nan):
    """the launch on the CPU.  q: the capture as the device takes it (tests/chan_ref.py quantise); -> [n_ch][n_out] complex64"""
    q, st, taps = np.ascontiguousarray(q), np.ascontiguousarray(st, np.uint64), np.ascontiguousarray(taps, np.float32)
    assert taps.size == 16 * D and q.size == (n_in if fmt == "c64" else 2 * n_in)
    out = np.full((st.size, n_out), fill, np.complex64)
    outside = lib().cr_host_run(FMT[fmt], q.ctypes.data_as(C.c_void_p), n_in, U, D, _p(st, C.c_ulonglong), _p(taps, C.c_float), st.size,
                                out.ctypes.data_as(C.POINTER(C.c_float)), n_out)
    assert outside == 0, outside
    return out


def nonfinite_case(seed=34):
    """3/4, c64, one Inf in mid-capture -> (capture, n_in, fs_in, shifts, n_out, must be clean [n_out], must be non-finite [n_out]).
    Output m reads the samples [s, s + L) (its taps) and the kernel multiplies [s, s + 4 G) (zero taps behind them): 0 * Inf = NaN."""
    U, D = 3, 4
    G = geometry(U, D)[0]
    n_out = corner_n_out(U, D)
    n_in, fs_in = ((n_out - 1) * D + 16 * D - 1) // U + 1, 1.92e6 * D / U
    x = noise_and_tones(seed, n_in, fs_in).astype(np.complex64)
    n_bad = n_in // 2 + 1
    x[n_bad] = np.inf
    m = np.arange(n_out)
    s = -(-m * D // U)
    last = (m * D + 16 * D - 1) // U
    dirty = (s <= n_bad) & (n_bad <= last)
    clean = ~((s <= n_bad) & (n_bad < s + 4 * G))
    # a window of 16 D / U samples moves on by D / U per output: the sample is in 16 windows, in 4 G U / D = 18 padded ones
    assert 15 <= dirty.sum() <= 17 and n_out - 19 <= clean.sum() < n_out - dirty.sum() and not (dirty & clean).any()
    return x, n_in, fs_in, shifts17(fs_in), n_out, clean, dirty


def check_nonfinite(y, ref, clean, dirty, rtol):
    assert np.isfinite(y[:, clean]).all()
    ratios = [float(np.abs(y[k, clean] - ref[k, clean]).max() / np.abs(ref[k, clean]).max()) for k in range(len(ref))]
    assert max(ratios) <= rtol, ratios
    assert not np.isfinite(y[:, dirty]).any()
    return max(ratios)
