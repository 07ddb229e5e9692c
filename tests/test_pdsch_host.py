"""The host twin of the PDSCH stage (tests/host/pdsch_host.cpp: pdsch.h compiled for the host, the code the kernels run) against the
numpy statement of the rule (tests/pdsch_ref.py), on the CPU: the tables, the resource map, the grant's fields, the soft bits, the
de-rate-matching, the windowed decoder and the whole record on the crafted grids."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import pcfich_cases as PC
import pcfich_ref as PR
import pdcch_cases as DC
import pdsch_cases as SC
import pdsch_ref as SR
from conftest import load_pkg


@pytest.fixture(scope="module")
def H():
    return SC.load_twin(load_pkg().capi)


def test_layouts(H):
    capi = load_pkg().capi
    assert H.pdsch_host_record_bytes() == C.sizeof(capi.PdschInfo) == 10832
    assert H.pdsch_host_cfg_bytes() == C.sizeof(capi.PdschCfg) == 112 and H.pdsch_host_block_bytes() == C.sizeof(capi.PdschBlock) == 336


def test_tables_are_the_packages(H):
    pkg = load_pkg()
    f = np.zeros(2, np.int32)
    for i, K in enumerate(pkg.synth.TURBO_K):
        assert H.pdsch_host_k_at(i) == K and H.pdsch_host_k_index(K) == i and H.pdsch_host_k_index(K + 1) == -1
        H.pdsch_host_qpp(i, SC._ip(f))
        assert tuple(f) == pkg.synth.TURBO_QPP[K]
    for B in (1, 40, 41, 512, 513, 1025, 2049, 2240):
        assert pkg.synth.TURBO_K[H.pdsch_host_k_ceil_index(B)] == next(k for k in pkg.synth.TURBO_K if k >= B)
    assert H.pdsch_host_k_ceil_index(2241) == -1
    assert [[H.pdsch_host_tbs(c, m) for m in range(27)] for c in range(2)] == pkg.capi._TBS_1A
    for K in (40, 1504, 2240):
        perm = np.zeros(K, np.int32)
        H.pdsch_host_perm(K, SC._ip(perm))
        assert np.array_equal(perm, pkg.synth.turbo_interleaver(K))


def test_crc24a(H):
    synth = load_pkg().synth
    rng = np.random.default_rng(3)
    for n in (1, 31, 32, 33, 500):
        a = rng.integers(0, 2, n).astype(np.uint8)
        assert H.pdsch_host_crc24a(SC._bp(a), n) == int("".join(map(str, synth.crc24a(a))), 2)


def test_fields_of_format_1a(H):
    capi = load_pkg().capi
    rng = np.random.default_rng(4)
    out = np.zeros(7, np.int32)
    for n_rb in (6, 15, 25, 50, 75, 100):
        for tdd in (False, True):
            size = capi.dci_common_sizes(n_rb, tdd)[0]
            for _ in range(40):
                bits = int(rng.integers(0, 1 << 62)) & ((1 << size) - 1)
                H.pdsch_host_1a(bits, n_rb, int(tdd), SC._ip(out))
                f = capi.dci_1a_fields(bits, n_rb, tdd)
                assert tuple(out) == (f["flag_1a"], f["distributed"], f["rb_start"], f["n_rb_alloc"], f["mcs"], f["rv"], f["tpc"])


def test_elements_closed_form_against_brute_force(H):
    lk = np.zeros(2 * 12 * 100 * 14, np.int32)
    n_cases = 0
    for n_id, cp, ports, n_rb in ((0, 1, 1, 6), (1, 2, 2, 6), (68, 1, 4, 6), (5, 1, 1, 15), (141, 2, 2, 15), (256, 1, 4, 15), (9, 1, 2, 25), (503, 2, 4, 25), (4, 1, 1, 100), (2, 1, 4, 100)):
        for sf in (0, 3, 5):
            for tdd in (0, 1):
                for n_ctrl in (1, 3, 4):
                    for s, n in ((0, n_rb), (0, 1), (n_rb - 1, 1), (n_rb // 2 - 1, 2), (n_rb // 2 - 3, 5), (1, n_rb - 1)):
                        if s < 0:
                            continue
                        want = SR.elements(n_id, cp, ports, n_rb, sf, n_ctrl, s, n, bool(tdd))
                        got = H.pdsch_host_elements(n_rb, ports, PR.n_symb_of(cp), n_id, sf, tdd, n_ctrl, s, n, SC._ip(lk), lk.size // 2)
                        assert got == len(want) and [tuple(v) for v in lk[:2 * got].reshape(-1, 2)] == want, (n_id, cp, ports, n_rb, sf, tdd, n_ctrl, s, n)
                        n_cases += 1
    assert n_cases > 1000


@pytest.mark.parametrize("K,F", [(40, 0), (64, 8), (528, 0), (2240, 40)])
def test_derm_against_numpy(H, K, F):
    rng = np.random.default_rng(K)
    n_w = 3 * (K + 4) - 2 * F
    for rv in range(4):
        for G in (n_w // 2, n_w, 2 * n_w + 10, 0):
            llr = rng.standard_normal(G)
            d = np.zeros((3, K + 4))
            H.pdsch_host_derm(SC._dp(llr) if G else None, G, K, F, rv, SC._dp(d))
            assert np.array_equal(d, SR.derm(llr, K, F, rv)), (K, F, rv, G)


@pytest.mark.parametrize("K,F,sigma", [(40, 0, 0.5), (64, 0, 0.9), (64, 8, 0.7), (512, 0, 0.9), (528, 16, 0.9), (2240, 0, 0.95), (2240, 40, 3.0)])
def test_decoder_against_numpy(H, K, F, sigma):
    """blocks that decode at once, after several iterations and not at all: decisions, iterations and status equal"""
    synth = load_pkg().synth
    rng = np.random.default_rng(10 * K + F)
    for trial in range(3):
        a = rng.integers(0, 2, K - F - 24).astype(np.uint8)
        c = np.concatenate([np.zeros(F, np.uint8), a, synth.crc24a(a)])
        d = (1 - 2.0 * synth.turbo_encode(c)) + sigma * rng.standard_normal((3, K + 4))
        d[:2, :F] = 0
        ref = SR.turbo_decode(d, K, F, 8)
        bits, n_iter, st = SC.twin_turbo(H, d, K, F, 8)
        assert ref["margin"] > 1e-9
        assert (st, n_iter) == (ref["status"], ref["n_iter"]) and np.array_equal(bits, ref["bits"]), (K, F, trial, st, n_iter, ref["status"], ref["n_iter"])
    z = np.zeros((3, K + 4))
    assert SC.twin_turbo(H, z, K, F)[1:] == (0, 7)
    z[1, 3] = np.inf
    assert SC.twin_turbo(H, z, K, F)[1:] == (0, 7)
    assert H.pdsch_host_turbo(SC._dp(z), K + 1, 0, 8, SC._bp(np.zeros(K + 1, np.uint8)), C.byref(C.c_int32())) == -1


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_record_against_numpy(H, case):
    """soft bits to 1e-12 of the block's largest, the de-rate-matched values likewise; payloads, iterations and status equal"""
    capi = load_pkg().capi
    tfg, cfi, _ = SC.crafted(case)
    _, blocks = SC.reference(case)
    pdc = SC.pdcch_twin_record(capi, case, tfg, cfi)
    rec, llr, d = SC.twin_record(H, capi, case, tfg, pdc, want_soft=True)
    n, excused = SC.assert_blocks_against_numpy(rec, blocks, SC.case_id(case))
    assert excused == 0
    per_sf = {}
    for b in blocks:
        u = per_sf.get(b["subframe"], 0)
        per_sf[b["subframe"]] = u + 1
        if "llr" not in b:
            continue
        slot = 2 * b["subframe"] + u
        G = len(b["llr"])
        assert np.abs(llr[slot, :G] - b["llr"]).max() <= 1e-12 * np.abs(b["llr"]).max(), (SC.case_id(case), b["subframe"])
        assert np.abs(d[slot, :, :b["K"] + 4] - b["d"]).max() <= 1e-12 * max(np.abs(b["d"]).max(), 1e-300)
    st = [0] * 10
    for b in blocks:
        st[b["status"]] += 1
    assert list(rec.n_status) == st and rec.n_ok == st[1] and rec.n_overflow == 0
    assert (rec.n_si, rec.n_paging, rec.n_ra) == tuple(sum(b["kind"] == k for b in blocks) for k in (1, 2, 4))
    assert [x["bytes"] for x in rec.blocks()] == [bytes(b["payload"][:(b["tbs"] + 7) // 8]) if b["status"] in (1, 2) else b"" for b in blocks]


def test_forced_grants_and_filler(H):
    """forced grants replace the PDCCH's; a forced tbs that needs fillers; a forced grant in a subframe that is not there whole"""
    capi = load_pkg().capi
    case = SC.CASES[3]
    n_id, cp, ports, n_rb, res, _ = case
    tfg, cfi, planted = SC.crafted(case)
    pdc_ref, _ = SC.reference(case)
    p = next(p for p in planted if p["bits"] is not None and not p["silent"] and p["g"] == 1)
    forced = [(1, p["rnti"], p["rb_start"], p["n_prb"], p["tbs"], p["rv"]), (7, 0xFFFF, 2, 3, 100, 2), (12, 0xFFFF, 0, 2, 56, 0), (7, 61, 9, 2, 33, 1)]
    cfg = SC.make_cfg(capi, forced=forced)
    pdc = SC.pdcch_twin_record(capi, case, tfg, cfi)
    rec = SC.twin_record(H, capi, case, tfg, pdc, cfg=cfg)
    blocks = SR.receive(tfg, n_id, cp, ports, n_rb, pdc_ref, forced=forced)
    assert SC.assert_blocks_against_numpy(rec, blocks, "forced") == (4, 0)
    b = rec.blocks()
    assert [x["subframe"] for x in b] == [1, 7, 7, 12] and [x["slot"] for x in b] == [0, 1, 3, 2] and [x["mcs"] for x in b] == [-1] * 4
    assert b[0]["crc_ok"] and b[0]["bytes"] == np.packbits(p["bits"]).tobytes()
    assert (b[1]["K"], b[1]["F"]) == (128, 4) and (b[2]["K"], b[2]["F"]) == (64, 7) and b[3]["status"] == "rows" and b[2]["kind"] == "other"


def test_overflow_and_order(H):
    """more grants than the record holds: the first 32 in (subframe, slot) order, the rest counted"""
    capi = load_pkg().capi
    case = SC.CASES[0]
    tfg, cfi, _ = SC.crafted(case)
    pdc = SC.pdcch_twin_record(capi, case, tfg, cfi)
    big = np.tile(tfg[:24 * 7], (3, 1))[:60 * 7]
    pdc_big = capi.PdcchInfo()
    n = 0
    for g in range(30):
        src = g % 12
        pdc_big._cfi[g] = pdc._cfi[src]
        pdc_big.dec[g][0][0] = pdc.dec[src][0][0]
        pdc_big.dec[g][1][0] = pdc.dec[src][0][0]
        pdc_big.dec[g][1][0].bits ^= 1 << 20
        n += 2 * bool(pdc.dec[src][0][0].flags & 2)
    rec = SC.twin_record(H, capi, case, big, pdc_big)
    assert n > 32 and rec.n_blocks == 32 and rec.n_overflow == n - 32
    key = [(b["subframe"], b["slot"]) for b in rec.blocks()]
    assert key == sorted(key)


def test_stand_alone_program_under_address_and_undefined_sanitizers(H, tmp_path):
    """the same source with its own main, built with -fsanitize=address,undefined: a clean exit, and what the library form gives -- the
    stage on crafted grids (forced grants with fillers among them, a grid that is not finite) and the decoder alone at its sizes' ends"""
    pkg = load_pkg()
    capi = pkg.capi
    if SC.stale(SC.SAN):
        subprocess.check_call(PC.HIPCC + ["-O1", "-g", "-DPDSCH_HOST_MAIN", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                                          "-fno-sanitize-recover=undefined", "-o", SC.SAN, SC.TWIN_SRC])
    rng = np.random.default_rng(8)
    direct = []
    for K, F, sigma in ((40, 0, 0.5), (64, 8, 0.8), (2240, 40, 0.9), (2240, 0, 3.0)):
        a = rng.integers(0, 2, K - F - 24).astype(np.uint8)
        d = (1 - 2.0 * pkg.synth.turbo_encode(np.concatenate([np.zeros(F, np.uint8), a, pkg.synth.crc24a(a)]))) + sigma * rng.standard_normal((3, K + 4))
        direct.append((K, F, 8, d))
    direct.append((40, 0, 8, np.zeros((3, 44))))
    forced = [(1, 0xFFFF, 13, 1, 32, 0), (7, 0xFFFF, 2, 3, 100, 2), (12, 0xFFFF, 0, 2, 56, 0), (7, 61, 9, 2, 33, 1)]
    runs = [(SC.CASES[i], None, None) for i in (0, 4, 7, 8)] + [(SC.CASES[3], None, forced), (SC.CASES[3], np.full((45, 180), np.nan + 0j), forced)]
    for case, grid, fg in runs:
        tfg, cfi, _ = SC.crafted(case)
        pdc = SC.pdcch_twin_record(capi, case, tfg, cfi)
        tfg = tfg if grid is None else grid
        n_id, cp, ports, n_rb = case[:4]
        cfg = SC.make_cfg(capi, forced=fg or ())
        mask = DC.dl_mask_of(SC.pdcch_case(case))
        path = tmp_path / "grid.bin"
        with open(path, "wb") as f:
            f.write(np.array([tfg.shape[0], PR.n_symb_of(cp), n_rb, n_id, cp, ports, mask, 1, int(SC.tdd_of(case)), len(direct)], np.int32).tobytes() +
                    SC.jump_tables(n_rb).tobytes() + bytes(cfg) + bytes(pdc) + np.ascontiguousarray(tfg, np.complex128).tobytes())
            for K, F, it, d in direct:
                f.write(np.array([K, F, it, 0], np.int32).tobytes() + np.ascontiguousarray(d).tobytes())
        r = subprocess.run([SC.SAN, str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
        lines = [[int(x) for x in l.split()] for l in r.stdout.splitlines()]
        o = SC.twin_record(H, capi, case, tfg, pdc, cfg=cfg)
        assert lines[0] == [o.n_sf, o.n_blocks, o.n_ok, o.n_si, o.n_paging, o.n_ra, o.n_overflow]
        want = [[b.subframe, b.slot, b.status, b.n_iter, b.n_re, b.K, int(np.ctypeslib.as_array(b.payload).sum())] for b in (o.block[i] for i in range(o.n_blocks))]
        assert lines[1:1 + o.n_blocks] == want
        for (K, F, it, d), got in zip(direct, lines[1 + o.n_blocks:]):
            bits, n_iter, st = SC.twin_turbo(H, d, K, F, it)
            assert got == [st, n_iter, H.pdsch_host_crc24a(SC._bp(bits), K)]
        assert len(lines) == 1 + o.n_blocks + len(direct)
