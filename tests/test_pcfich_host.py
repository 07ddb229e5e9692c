"""pcfich.h compiled for the HOST -- the __host__ __device__ code k_pcfich and k_pcfich_fin run -- against the numpy statement of the
rule (tests/pcfich_ref.py) on crafted grids with planted PCFICH elements (tests/pcfich_cases.py).

Bars: corr and margin to 1e-12 (ratios of order one; the project's bar for a host twin of an fp64 sum), every decision and the
summary equal.  Every crafted case keeps a numpy margin >= 1e-6, so no decision hangs on a tie, and reads the planted value.  The
record's size and layout are pinned here.  The same source is built once more as a stand-alone program with
-fsanitize=address,undefined: nothing is loaded into Python under a sanitizer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pcfich_cases as PC
import pcfich_ref as PR
from conftest import load_pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "host", "pcfich_host_san")
TOL = 1e-12


@pytest.fixture(scope="module")
def capi():
    return load_pkg().capi


@pytest.fixture(scope="module")
def H(capi):
    return PC.load_twin(capi)


def test_the_case_set_covers_what_it_says():
    assert {i % 6 for i in PC.IDS} == set(range(6))
    for n_rb, _ in PC.SHAPES:
        cols = [PR.columns(i, n_rb) for i in PC.IDS]
        assert any(c[0] < 6 for c in cols), "kbar = 0"
        assert any((np.diff(c[0::4]) < 0).any() for c in cols), "a quadruplet beyond the last column"
        for i, c in zip(PC.IDS, cols):
            assert len(set(c)) == 16 and c.min() >= 0 and c.max() < 12 * n_rb and not (c % 3 == i % 3).any()
            assert [int(c[4 * q]) // 6 for q in range(4)] == [((i % (2 * n_rb)) + (q * n_rb) // 2) % (2 * n_rb) for q in range(4)]
    assert any(n_rb & 1 for n_rb, _ in PC.SHAPES)           # floor(i n_rb / 2) with an odd n_rb


@pytest.mark.parametrize("shape", PC.SHAPES, ids=[str(s) for s in PC.SHAPES])
def test_twin_against_numpy_on_crafted_grids(H, capi, shape):
    n_rb, cp = shape
    worst, least = 0.0, np.inf
    for n_id, n_ports, mask, tfg, planted in PC.crafted_cases(n_rb, cp):
        what = (shape, n_id, n_ports, hex(mask), tfg.shape[0])
        ref = PR.decode(tfg, n_id, cp, n_ports, n_rb, mask)
        o = PC.twin_record(H, capi, n_id, cp, tfg, n_rb, n_ports, mask)
        worst = max(worst, PR.assert_record_close(o, ref, TOL, what))
        dec = ref["cfi"] > 0
        # which subframes are read: the mask's, with their rows inside the grid
        n = PR.n_symb_of(cp)
        want = np.array([bool((mask >> (g % 10)) & 1) and 2 * g * n + (1 if n_ports == 4 else 0) < tfg.shape[0] for g in range(ref["n_sf"])])
        assert np.array_equal(dec, want), what
        assert ref["n_sf"] == 13 and dec.any()
        assert np.array_equal(ref["cfi"][dec], planted[dec]), (what, ref["cfi"], planted)
        assert ref["min_margin"] >= 1e-6, what
        least = min(least, ref["min_margin"])
    print(shape, "worst |twin - numpy| %.2e, smallest margin %.3f" % (worst, least))


def test_ports_unknown_count_as_one(H, capi):
    tfg, planted = PC.planted_grid(68, 1, 15, 1)
    one = PC.twin_record(H, capi, 68, 1, tfg, 15, 1, 0x3FF)
    for n_ports in (0, -1, 3):
        o = PC.twin_record(H, capi, 68, 1, tfg, 15, n_ports, 0x3FF)
        assert bytes(o) == bytes(one) and o.n_ports == 1
        PR.assert_record_close(o, PR.decode(tfg, 68, 1, n_ports, 15), TOL)


def test_grids_without_a_decision(H, capi):
    n_rb, cp = 25, 1
    for tfg in (np.zeros((40, 300), np.complex128), np.full((40, 300), np.nan + 0j), np.full((40, 300), np.inf + 0j)):
        for n_ports in PC.PORTS:
            o = PC.twin_record(H, capi, 7, cp, tfg, n_rb, n_ports, 0x3FF)
            ref = PR.decode(tfg, 7, cp, n_ports, n_rb)
            assert o.n_sf == 3 and o.n_decoded == 0 and not o.cfi.any() and o.mean_n_ctrl_sym == 0.0 and o.min_margin == 0.0
            PR.assert_record_close(o, ref, TOL)
    # a NaN in a subframe outside the mask changes nothing; in a subframe of the mask it takes that subframe alone
    tfg = np.array(PC.planted_grid(7, cp, n_rb, 2)[0])
    clean = PC.twin_record(H, capi, 7, cp, tfg, n_rb, 2, 0x021)
    tfg[2 * 7 * 2, 5] = np.nan
    assert bytes(PC.twin_record(H, capi, 7, cp, tfg, n_rb, 2, 0x021)) == bytes(clean)
    tfg[2 * 7 * 5] = np.nan
    o = PC.twin_record(H, capi, 7, cp, tfg, n_rb, 2, 0x021)
    assert o.cfi[5] == 0 and o.n_decoded == clean.n_decoded - 1 and o.cfi[0] == clean.cfi[0] and o.cfi[10] == clean.cfi[10]
    PR.assert_record_close(o, PR.decode(tfg, 7, cp, 2, n_rb, 0x021), TOL)
    # a mask whose subframe the grid does not reach
    o = PC.twin_record(H, capi, 7, cp, tfg[:14], n_rb, 2, 0x200)
    assert (o.n_sf, o.n_decoded, o.dl_mask, o.n_rb, o.n_ports) == (1, 0, 0x200, n_rb, 2)


def test_scrambling_bits_equal_the_gold_sequence(H):
    pn = load_pkg().synth._pn
    jump = PC.jump_tables(6)[32:].copy()
    for n_id in (0, 1, 277, 503):
        for sf in range(10):
            word = H.pcfich_host_scramble(sf, n_id, jump.ctypes.data_as(C.POINTER(C.c_uint32)))
            assert [(word >> i) & 1 for i in range(32)] == list(pn((sf + 1) * (2 * n_id + 1) * 512 + n_id, 32))


def test_record_size_and_layout(H, capi):
    P = capi.PcfichInfo
    assert C.sizeof(P) == 2640 == H.pcfich_host_record_bytes() and capi.PCFICH_MAX_SF == H.pcfich_host_max_sf() == 72
    want = dict(n_sf=0, n_decoded=4, n_cfi=8, dl_mask=20, n_rb=24, n_ports=28, mean_n_ctrl_sym=32, min_margin=40, _cfi=48, _corr=336, _margin=2064)
    assert {k: getattr(P, k).offset for k in want} == want
    o = P()
    o.n_sf, o.n_rb = 3, 6
    o._cfi[0], o._cfi[2], o._margin[2], o._corr[2][1] = 1, 3, 0.5, 0.25
    assert list(o.cfi) == [1, 0, 3] and list(o.n_ctrl_sym) == [2, 0, 4] and o.margin[2] == 0.5 and o.corr.shape == (3, 3) and o.corr[2, 1] == 0.25
    c = o.copy()
    o._cfi[0] = 2
    assert c.cfi[0] == 1 and bytes(c) != bytes(o)


def test_stand_alone_program_under_address_and_undefined_sanitizers(H, capi, tmp_path):
    """the same source with its own main, built with -fsanitize=address,undefined: a clean exit, and the record the library form gives"""
    if PC.stale(SAN):
        subprocess.check_call(PC.HIPCC + ["-O1", "-g", "-DPCFICH_HOST_MAIN", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                                          "-fno-sanitize-recover=undefined", "-o", SAN, PC.TWIN_SRC])
    cases = [(PC.IDS[i], cp, n_rb, PC.planted_grid(PC.IDS[i], cp, n_rb, ports)[0], ports, mask)
             for i, ((n_rb, cp), ports, mask) in enumerate(zip(PC.SHAPES, (1, 2, 4, 4, 2), (0x3FF, 0x021, 0x200, 0x3FF, 0x3FF)))]
    cases.append((503, 1, 100, np.array(PC.planted_grid(503, 1, 100, 4, PC.n_ofdm_of(1, 1))[0]), 4, 0x3FF))
    cases.append((7, 2, 50, np.full((25, 600), np.nan + 0j), 2, 0x3FF))
    for n_id, cp, n_rb, tfg, ports, mask in cases:
        path = tmp_path / "grid.bin"
        with open(path, "wb") as f:
            f.write(np.array([tfg.shape[0], PR.n_symb_of(cp), n_rb, n_id, cp, ports, mask, 0], np.int32).tobytes() + PC.jump_tables(n_rb).tobytes() +
                    np.ascontiguousarray(tfg, np.complex128).tobytes())
        r = subprocess.run([SAN, str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
        v = r.stdout.split()
        o = PC.twin_record(H, capi, n_id, cp, tfg, n_rb, ports, mask)
        assert [int(x) for x in v[:8]] == [o.n_sf, o.n_decoded] + list(o.n_cfi) + [o.dl_mask, o.n_rb, o.n_ports]
        assert [float(x) for x in v[8:10]] == [o.mean_n_ctrl_sym, o.min_margin]
        per = [x for g in range(o.n_sf) for x in (float(o.cfi[g]), o.corr[g, 0], o.corr[g, 1], o.corr[g, 2], o.margin[g])]
        assert [float(x) for x in v[10:]] == per
