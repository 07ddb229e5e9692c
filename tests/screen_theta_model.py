"""A CPU model of the batch screen's flag kernel (k_screen_flag) for tests/test_screen_theta_host.py and
tests/test_gpu_screen_theta.py: the rule itself is the C++ of csrc/screen_bound.h compiled for the host
(tests/host/screen_theta_host.cpp); around it the buffer's largest column scale as k_i8_scales forms it, the collapse in NumPy, the
tiles an oracle peak needs, and the crafted loud / quiet captures.  Not a test module."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "lte-cell-scanner_amd", "csrc", "screen_bound.h")
SRC = os.path.join(ROOT, "tests", "host", "screen_theta_host.cpp")
LIB = os.path.join(ROOT, "tests", "host", "libscreen_theta_host.so")
N_IDX, TILE, N_TILES, DS = 9600, 512, 19, 2
QMAX = 8300000.0                           # I8_QMAX
FS = 1.92e6
MODE_NONE, MODE_BY_T, MODE_ALL = 0, 1, 2

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in (SRC, HEADER)):
            subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC",
                                   "-shared", "-o", LIB, SRC])
        b = C.CDLL(LIB)
        dp, fp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int)
        b.theta_lower.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double]
        b.theta_lower.restype = C.c_double
        b.theta_in_s.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double]
        b.theta_decide.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, fp, dp]
        b.theta_hot.argtypes = [C.c_double, C.c_double]
        b.theta_rule.argtypes = [C.c_int, C.c_int, C.c_double, dp, fp, C.c_int, C.c_int, ip, fp, dp, ip]
        b.zmin_rule.argtypes = [C.c_int, C.c_int, C.c_double, dp, fp, C.c_int, C.c_int, ip, dp]
        _lib = b
    return _lib


def buffer_scale(f, fc):
    """The buffer's largest column scale, as k_i8_scales forms it: per template the largest |component| of its fp32 taps
    (conj(pss_td * exp(j k m)) / 137, pss_ref.h), q = QMAX / that, sc = float(1 / (128 q))."""
    m = np.arange(137)
    sc = 0.0
    for f_off in np.asarray(f, np.float64):
        kf = (fc - f_off) / fc
        k = np.pi * f_off / ((FS * kf) / 2)
        for t in range(3):
            tap = (np.conj(O.pss_td(t) * np.exp(1j * k * m)) / 137).astype(np.complex64)
            mx = float(max(np.abs(tap.real).max(), np.abs(tap.imag).max()))
            sc = max(sc, float(np.float32(1.0 / (128.0 * (QMAX / mx)))))
    return sc


def collapse(single):
    """single [3][9600][n_f] f32 -> (pow f32 [3][9600], frq i32): the circular box over 2 DS + 1 lags in fp32 in the reference's order,
    the first maximum over the hypotheses."""
    s = np.asarray(single, np.float32)
    v = s.copy()
    for d in range(1, DS + 1):
        v = v + (np.roll(s, d, 1) + np.roll(s, -d, 1))
    v = (v / np.float32(2 * DS + 1)).astype(np.float32)
    return v.max(2), v.argmax(2).astype(np.int32)


def theta_rule(n_comb, sc, z, vs):
    """-> dict(mode, flags bool [19], theta, T, n_s)"""
    z = np.ascontiguousarray(z, np.float64)
    vs = np.ascontiguousarray(vs, np.float32)
    flags = np.zeros(N_TILES, np.int32)
    th, T, ns = C.c_float(0), C.c_double(0), C.c_int(0)
    mode = lib().theta_rule(int(n_comb), DS, float(sc), z.ctypes.data_as(C.POINTER(C.c_double)), vs.ctypes.data_as(C.POINTER(C.c_float)), N_IDX, TILE,
                            flags.ctypes.data_as(C.POINTER(C.c_int)), C.byref(th), C.byref(T), C.byref(ns))
    return dict(mode=mode, flags=flags.astype(bool), theta=float(th.value), T=float(T.value), n_s=ns.value)


def zmin_rule(n_comb, sc, z, vs):
    z = np.ascontiguousarray(z, np.float64)
    vs = np.ascontiguousarray(vs, np.float32)
    flags = np.zeros(N_TILES, np.int32)
    T = C.c_double(0)
    every = lib().zmin_rule(int(n_comb), DS, float(sc), z.ctypes.data_as(C.POINTER(C.c_double)), vs.ctypes.data_as(C.POINTER(C.c_float)), N_IDX, TILE,
                            flags.ctypes.data_as(C.POINTER(C.c_int)), C.byref(T))
    return dict(all=bool(every), flags=flags.astype(bool), T=float(T.value))


def tiles_of(inds):
    """The tiles that hold ind - DS, ind, ind + DS (circular) of each index."""
    out = np.zeros(N_TILES, bool)
    for i in inds:
        for d in (-DS, 0, DS):
            out[((int(i) + d) % N_IDX) // TILE] = True
    return out


_parts = {}


def crafted(pkg, fc, n_cap, gain_w_db, gain_s_db=6.0, loud=8.0, snr_db=0.0, seed=31, tone_hz=None):
    """A capture whose noise power alternates by the factor `loud` between the halves of the 5 ms period: a weak cell (PSS 1) whose
    peak lies in the middle of the quiet half and a strong one (PSS 0) half a period later.  gain_*_db are relative to a cell that
    stands snr_db above the quiet noise.  The waveforms and the noise are drawn once per (fc, n_cap, seed); only the weak cell's gain
    differs between two calls.  tone_hz: the loud half's extra power is a carrier at that offset instead of noise -- outside the 0.93 MHz
    the PSS occupies it lifts the loud half's thresholds (they follow the sample power) by the same factor but hardly its correlations,
    so -- without the strong cell, gain_s_db=None, whose sidelobes would -- nothing in the loud half outranks a quiet-half cell that just
    reaches its own threshold.  -> iq u8."""
    key = (fc, n_cap, seed)
    if key not in _parts:
        rng = np.random.default_rng(seed)
        t0 = 4000.0
        sw, ref_pow, _ = pkg.synth.make_signal(rng, fc, [dict(n_id_1=77, n_id_2=1, f_off=3000.0, t0=t0, sfn0=5)], n_cap)
        ss, _, _ = pkg.synth.make_signal(rng, fc, [dict(n_id_1=20, n_id_2=0, f_off=-4000.0, t0=t0 + 4800.0, sfn0=9)], n_cap)
        _parts[key] = (sw, ss, ref_pow, rng.standard_normal(n_cap) + 1j * rng.standard_normal(n_cap), t0)
    sw, ss, ref_pow, unit, t0 = _parts[key]
    # the PSS of a cell at t0 ends the first slot: symbol 6 of 7, 960 samples per slot at 1.92 Msps; its correlation peak lies near
    # 960 - 137 - t0 modulo 9600
    p_w = int(round(960 - 137 - t0)) % N_IDX
    n = np.arange(n_cap)
    quiet = ((n - p_w - 68 + 2400) % N_IDX) < 4800
    npow = ref_pow / 10 ** (snr_db / 10)
    if tone_hz is None:
        floor = np.sqrt(npow / 2) * unit * np.where(quiet, 1.0, np.sqrt(loud))
    else:
        u = (n - p_w - 68 + 2400) % N_IDX                            # the carrier is ramped over 256 samples: a hard edge would splatter into the PSS's band
        env = np.where(quiet, 0.0, np.sin(0.5 * np.pi * np.clip((u - 4800) / 256.0, 0, 1)) ** 2 * np.sin(0.5 * np.pi * np.clip((N_IDX - u) / 256.0, 0, 1)) ** 2)
        floor = np.sqrt(npow / 2) * unit + env * np.sqrt((loud - 1.0) * npow) * np.exp(2j * np.pi * tone_hz * n / FS)
    x = 10 ** (gain_w_db / 20) * sw + (0.0 if gain_s_db is None else 10 ** (gain_s_db / 20)) * ss + floor
    x = x * (0.15 / np.sqrt(np.mean(np.abs(x) ** 2)))
    iq = np.empty(2 * n_cap, np.uint8)
    iq[0::2] = np.clip(np.rint(128 * x.real + 127), 0, 255).astype(np.uint8)
    iq[1::2] = np.clip(np.rint(128 * x.imag + 127), 0, 255).astype(np.uint8)
    return iq


def oracle_of(pkg, iq, f, fc, n_cap):
    """-> (xcorr dict, z, peaks) of the CPU oracle"""
    cap = pkg.synth.iq_u8_to_complex(iq)[:n_cap]
    r = O.xcorr_pss(cap, f, DS, fc, fc, FS)
    z = O.z_th1(r["sp_incoherent"], r["n_comb_xc"])
    return r, z, O.peak_search(r["pow"], r["frq"], z, f, fc, fc, r["single"], DS)


def pick_crafted(pkg, f, fc, n_cap):
    """The two crafted captures, their gains chosen with the oracle: A -- the weak quiet-half cell and the strong loud-half cell are
    both recorded; B -- the weak cell reaches its own threshold but a loud-half entry BELOW its own threshold outranks it, so the
    reference's loop stops before it.  -> dict(A=(iq, r, z, peaks), B=...); asserts the premises on the oracle's values."""
    out = {}
    for g in np.arange(6.0, -8.0, -1.0):                              # (A: the weakest gain that still is recorded)
        iq = crafted(pkg, fc, n_cap, g)
        r, z, pk = oracle_of(pkg, iq, f, fc, n_cap)
        i_w = int(np.argmax(r["pow"][1] / z))
        v_w, rec = float(r["pow"][1, i_w]), [(p.n_id_2, p.ind) for p in pk]
        sub = r["pow"] < z[None, :]                                   # entries below their own threshold
        outranked = bool((r["pow"][sub] > v_w).any())
        if any(t == 1 and abs(i - i_w) <= DS for t, i in rec) and any(t == 0 for t, _ in rec) and not outranked:
            out["A"] = (iq, r, z, pk, i_w)
        if "B" not in out and v_w >= z[i_w] and outranked and all(t != 1 for t, _ in rec) and any(t == 0 for t, _ in rec):
            out["B"] = (iq, r, z, pk, i_w)
    assert set(out) == {"A", "B"}, sorted(out)
    for k, (iq, r, z, pk, i_w) in out.items():
        assert z.max() / z.min() >= 3.0, (k, z.max() / z.min())     # the loud half's thresholds against the quiet half's
        i_s = int(np.argmax(r["pow"][0]))
        assert z[i_w] < 1.5 * z.min() and z[i_s] > 2.5 * z.min(), (k, z[i_w] / z.min(), z[i_s] / z.min())   # which cell sits in which half
    return out
