"""The cancellation rule compiled for the host (tests/host/sic_host.cpp: csrc/sic.h and csrc/lte_pbch_enc.cpp, the text the kernels
and their launcher compile): the PBCH encoder against synth.pbch_symbols, the symbol intervals against a walk over the samples, the
element maps against tests/sic_ref.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import sic_cases as K
import sic_edge_cases as E
import sic_ref as R
from conftest import load_pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lte-cell-scanner_amd", "csrc")
TWIN_SRC = os.path.join(ROOT, "tests", "host", "sic_host.cpp")
TWIN_LIB = os.path.join(ROOT, "tests", "host", "libsic_host.so")
HIPCC = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include")]
DP = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def H():
    dep = [TWIN_SRC] + [os.path.join(CSRC, f) for f in ("sic.h", "lte_pbch_enc.cpp", "lte_tables.cpp", "lcs_internal.h")]
    if not os.path.exists(TWIN_LIB) or any(os.path.getmtime(d) > os.path.getmtime(TWIN_LIB) for d in dep):
        subprocess.check_call(HIPCC + ["-O2", "-fPIC", "-shared", "-o", TWIN_LIB, TWIN_SRC])
    h = C.CDLL(TWIN_LIB)
    h.sic_host_pbch.argtypes = [C.c_int] * 7 + [DP]
    h.sic_host_geometry.argtypes = [C.c_double, C.c_double, C.c_int, C.c_uint32, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_int)]
    h.sic_host_tiles.argtypes = [C.c_double, C.c_double, C.c_int, C.c_uint32, C.c_double, C.c_double, C.c_double]
    h.sic_host_tiles_raster.argtypes = [C.c_double, C.c_double, C.c_long, C.c_double, C.c_int, C.c_uint32, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_int)]
    h.sic_host_tiles_raster.restype = C.c_long
    h.sic_host_pbch_map.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, DP, DP]
    h.sic_host_interp.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), DP]
    h.sic_host_sync_kind.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    return h


@pytest.mark.parametrize("cp_normal", [True, False])
@pytest.mark.parametrize("n_ports", [1, 2, 4])
def test_pbch_encoder_equals_synth(H, n_ports, cp_normal):
    """a whole 40 ms period, for several identities, bandwidths, PHICH fields and frame numbers (the SFN's two low bits are not sent)"""
    synth = load_pkg().synth
    n = 960 if cp_normal else 864
    for id_, n_rb, dur_ext, res, sfn in ((0, 6, 0, 0, 0), (31, 50, 0, 2, 8), (232, 100, 1, 3, 1023), (503, 25, 1, 1, 514), (77, 15, 0, 2, 255), (300, 75, 0, 0, 640)):
        out = np.zeros(2 * 960)
        assert H.sic_host_pbch(id_, n_ports, n_rb, 2 if dur_ext else 1, res + 1, sfn, 1 if cp_normal else 2, out.ctypes.data_as(DP)) == 1
        want = synth.pbch_symbols(id_, n_ports, n_rb, dur_ext, res, sfn - sfn % 4, cp_normal)
        assert want.size == n
        assert np.array_equal(out[:2 * n].view(np.complex128), want)
        assert not out[2 * n:].any()


def test_pbch_encoder_refuses_what_no_mib_carries(H):
    out = np.zeros(2 * 960)
    p = out.ctypes.data_as(DP)
    assert H.sic_host_pbch(31, 2, 50, 1, 3, 8, 1, p) == 1
    for bad in ((31, 3, 50, 1, 3, 8, 1), (31, 2, 49, 1, 3, 8, 1), (31, 2, -1, 1, 3, 8, 1), (31, 2, 50, 0, 3, 8, 1), (31, 2, 50, 1, 0, 8, 1), (504, 2, 50, 1, 3, 8, 1), (31, 2, 50, 1, 3, 8, 0)):
        assert H.sic_host_pbch(*bad, p) == 0


@pytest.mark.parametrize("cp_type", [1, 2])
@pytest.mark.parametrize("ppm", [-120.0, 0.0, 120.0])
def test_intervals_tile(H, cp_type, ppm):
    """every frame_start on a raster of 0.37 samples across a whole frame and beyond both its ends (-3 .. 19203: 51908 positions) on a
    capture of two slots and a bit, and a coarser raster on the full-length capture: no gap, no overlap, +-1 sample against the
    nominal length, and the closed form names the walk's symbol and offset for every sample"""
    why = C.c_int(0)
    bad = H.sic_host_tiles_raster(-3.0, 0.37, 51908, -ppm * 1e-6 * K.FC, cp_type, 2400, K.FC, K.FC, K.FS, C.byref(why))
    assert bad == -1, (bad, -3.0 + 0.37 * bad, why.value)
    for fs0 in np.concatenate([np.arange(-3.0, 19203.0, 417.37), np.arange(5000.0, 5003.0, 0.37)]):
        assert H.sic_host_tiles(float(fs0), -ppm * 1e-6 * K.FC, cp_type, 153600, K.FC, K.FC, K.FS) == 0, fs0
    assert H.sic_host_tiles(14198.0, -ppm * 1e-6 * K.FC, cp_type, 19200, K.FC, K.FC, K.FS) == 0       # a short capture
    assert H.sic_host_tiles(14198.0, -ppm * 1e-6 * K.FC, cp_type, 400000, K.FC, K.FC, K.FS) == 0      # a long one


def test_geometry_equals_ref(H):
    for cp_type, fs0, ppm in ((1, 14198.0, 0.4), (2, 3.3, -100.0), (1, 19195.2, 120.0), (2, 9000.5, 0.0)):
        c = O.new_cell(frame_start=fs0, freq_fine=-ppm * 1e-6 * K.FC, freq_superfine=0.0, cp_type=cp_type)
        geo = R.geometry(c, 153600, K.FC, K.FC, K.FS)
        out = (C.c_int * 6)()
        assert H.sic_host_geometry(fs0, c.freq_fine, cp_type, 153600, K.FC, K.FC, K.FS, out) == 1
        n_symb = geo["n_symb"]
        assert (out[0], out[1]) == (geo["t_lo"], geo["t_hi"])
        assert (out[2], out[3]) == (geo["t_lo"] // n_symb, geo["t_hi"] // n_symb - geo["t_lo"] // n_symb + 1)
        assert out[4] == (geo["t_lo"] // n_symb) // 20 and out[5] <= 10
    assert H.sic_host_geometry(float("nan"), 0.0, 1, 153600, K.FC, K.FC, K.FS, (C.c_int * 6)()) == 0
    assert H.sic_host_geometry(100.0, 0.0, 0, 153600, K.FC, K.FC, K.FS, (C.c_int * 6)()) == 0


def test_geometry_equals_ref_on_the_edge_table(H):
    """every record of tests/sic_edge_cases.py: the symbols, slots and frames sic_geometry finds are sic_ref.geometry's"""
    n = 0
    for c in E.CASES:
        for b, buf in enumerate(c["bufs"]):
            for i, spec in enumerate(buf["cells"]):
                geo = E.case_geo(c, b, i)
                out = (C.c_int * 6)()
                assert H.sic_host_geometry(spec["frame_start"], spec["ff"], spec["cp"], c["n_cap"], buf["fc"][0], buf["fc"][1], c["fs"], out) == 1
                assert list(out) == [geo[k] for k in ("t_lo", "t_hi", "j_lo", "n_slots", "f_lo", "n_frames")], (c["name"], b, i)
                # ... and sic_owner names the walk's symbol and offset for every sample of the case's capture
                assert H.sic_host_tiles(spec["frame_start"], spec["ff"], spec["cp"], c["n_cap"], buf["fc"][0], buf["fc"][1], c["fs"]) == 0, (c["name"], b, i)
                n += 1
    assert n >= len(E.CASES)
    # the launcher's refusal (tests/test_gpu_sic_edges.py): at 1.0 Msps a 268800-sample capture spans more frames than a PBCH table holds
    out = (C.c_int * 6)()
    assert H.sic_host_geometry(5000.3, 0.0, 1, 268800, E.FC, E.FC, 1.0e6, out) == 1 and out[5] > 16
    assert out[5] == E.geo_of(E.rec(155, 2, 1, 5000.3), 268800, fs=1.0e6)["n_frames"]


@pytest.mark.parametrize("cp_type", [1, 2])
@pytest.mark.parametrize("rate", [-3e-4, 3e-4])
def test_intervals_tile_off_nominal_rates(H, cp_type, rate):
    """the walk with fs_programmed away from 1.92 MHz and fc_programmed away from fc_requested (step = 1 +- 3e-4 and a bit): the cases
    of the table's rates group, and every frame_start on the 0.37-sample raster across a frame on a capture of two slots and a bit"""
    rates = [c for c in E.CASES if c["group"] == "rates" and (c["fs"] > E.FS) == (rate > 0) and c["bufs"][0]["cells"][0]["cp"] == cp_type]
    assert rates
    for c in rates:
        spec, buf = c["bufs"][0]["cells"][0], c["bufs"][0]
        assert H.sic_host_tiles(spec["frame_start"], spec["ff"], cp_type, c["n_cap"], buf["fc"][0], buf["fc"][1], c["fs"]) == 0, c["name"]
    why = C.c_int(0)
    bad = H.sic_host_tiles_raster(-3.0, 0.37, 51908, 5000.0 if rate > 0 else -5000.0, cp_type, 2400, E.FC_OFF[0], E.FC_OFF[1], E.FS * (1 + rate), C.byref(why))
    assert bad == -1, (bad, -3.0 + 0.37 * bad, why.value)
    assert H.sic_host_tiles(14198.0, 0.0, cp_type, 268800, E.FC_OFF[0], E.FC_OFF[1], E.FS * (1 + rate)) == 0      # the longest capture


@pytest.mark.parametrize("normal", [True, False])
@pytest.mark.parametrize("n_ports", [1, 2, 4])
def test_pbch_map_equals_ref(H, n_ports, normal):
    rng = np.random.default_rng(5)
    per = [48, 48, 72, 72] if normal else [48, 48, 72, 48]
    q = (rng.standard_normal(sum(per)) + 1j * rng.standard_normal(sum(per)))
    for id_ in (0, 31, 232):
        for sym in range(4):
            out = np.zeros((4, 72), np.complex128)
            H.sic_host_pbch_map(int(normal), n_ports, id_, sym, np.ascontiguousarray(q).ctypes.data_as(DP), out.ctypes.data_as(DP))
            skip = sym in (0, 1) or (sym == 3 and not normal)
            sc = np.array([k for k in range(72) if not (skip and k % 3 == id_ % 3)])
            want = np.zeros((4, 72), np.complex128)
            want[:n_ports, sc] = R.pbch_layers(q[sum(per[:sym]):sum(per[:sym]) + per[sym]], n_ports)
            assert np.allclose(out, want, rtol=0, atol=1e-15)


def test_interp_and_sync_positions(H):
    cn = R.cn()
    for c3 in range(3):
        qm = c3 + 3 * np.arange(24)
        for k in range(72):
            m0, fr = C.c_int(0), C.c_double(0)
            H.sic_host_interp(k, c3, C.byref(m0), C.byref(fr))
            lo = int(np.clip((k - c3) // 3, 0, 22))
            assert m0.value == lo and fr.value == (cn[k] - cn[qm[lo]]) / (cn[qm[lo + 1]] - cn[qm[lo]])
    for cp_type, n_symb in ((1, 7), (2, 6)):
        geo = dict(n_symb=n_symb, t_lo=-n_symb * 20, t_hi=n_symb * 40)
        for duplex in (R.FDD, R.TDD):
            want = {t: (1 if kind == "pss" else 2, s) for t, kind, s in R.sync_symbols(geo, duplex)}
            for t in range(geo["t_lo"], geo["t_hi"] + 1):
                s = C.c_int(0)
                kind = H.sic_host_sync_kind(cp_type, t, duplex, C.byref(s))
                assert (kind, s.value if kind else 0) == want.get(t, (0, 0)), (cp_type, duplex, t)
