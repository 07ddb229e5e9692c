"""pdcch_scan.h compiled for the HOST -- the __host__ __device__ code k_pscan_llr, k_pscan_dec, k_pscan_acc and k_pscan_fin run, and the very
functions that build the kernels' tables -- against the numpy statement of the rule (tests/pdcch_scan_ref.py) on noise-free code
words and on crafted grids (tests/pdcch_scan_cases.py).

Bars.  The decoder is integer arithmetic after one fp64 division and one rint, so every integer of every decode is EQUAL; the only
excuse is a decode where numpy sees some 127 d / m within 1e-9 of a half-integer: at most 1 % of the decodes, never a planted one.
Quality to 1e-12 (one fp64 division of equal integers).  Soft bits to 1e-12 of the subframe's largest (the project's bar for a host
twin of an fp64 sum); the first 1152 equal the PDCCH stage's twin bit for bit.  False accepts -- accepted messages that are neither
planted nor a re-reading of a planted one -- at most 0.5 % of the decodes examined per grid, for the twin and for numpy alone.  The
same source is built once more as a stand-alone program with -fsanitize=address,undefined: nothing is loaded into Python under a
sanitizer."""
import ctypes as C
import itertools
import subprocess

import numpy as np
import pytest

import pcfich_cases as PC
import pcfich_ref as PR
import pdcch_cases as DC
import pdcch_ref as DR
import pdcch_scan_cases as SC
import pdcch_scan_ref as SR
from conftest import load_pkg

TOL = 1e-12
_dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
_ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))


@pytest.fixture(scope="module")
def capi():
    return load_pkg().capi


@pytest.fixture(scope="module")
def H(capi):
    return SC.load_twin(capi)


# ---------------------------------------------------------------- record, candidates, search space, tables
def test_record_size_and_layout(H, capi):
    P = capi.PdcchScanInfo
    assert C.sizeof(P) == 43616 == H.pscan_host_record_bytes() and C.sizeof(capi.PdcchScanCfg) == 104 == H.pscan_host_cfg_bytes()
    want = dict(n_sf=0, n_read=4, n_accepted=8, n_si=12, n_paging=16, n_ra=20, dl_mask=24, n_rb=28, n_ports=32, n_ue=36, n_rnti=40, n_msg=44, n_dropped=48, n_sizes=52,
                sf=64, msg=64 + 72 * 36)
    assert {k: getattr(P, k).offset for k in want} == want
    assert {k: getattr(capi.PdcchScanDec, k).offset for k in ("bits", "rnti_x", "flags", "n_err", "n_obs", "n_repeat", "quality")} == dict(
        bits=0, rnti_x=8, flags=12, n_err=16, n_obs=18, n_repeat=20, quality=24)
    assert {k: getattr(capi.PdcchScanMsg, k).offset for k in ("g", "L", "cce", "size_index", "d")} == dict(g=0, L=2, cce=3, size_index=4, d=8)
    assert capi.PdcchScanCfg.min_quality.offset == 96 and capi.PdcchScanCfg.min_repeat.offset == 84
    cfg = capi.PdcchScanCfg.make((22, 23, 31))
    assert (cfg.n_sizes, cfg.min_repeat, cfg.min_quality) == (3, 2, capi.PDCCH_SCAN_MIN_QUALITY) and list(cfg.phich_mi) == [-1] * 10
    with pytest.raises(ValueError):
        capi.PdcchScanCfg.make(range(8, 15))


def test_candidates_are_every_level_and_start_in_order(H, capi):
    for n_cce in range(0, 89):
        want = SR.candidates(n_cce)
        assert want == capi.scan_candidates(n_cce) and len(want) == H.pscan_host_n_cand(n_cce) <= 165
        got = []
        for i in range(-1, len(want) + 2):
            L, cce = C.c_int32(), C.c_int32()
            if H.pscan_host_cand(i, n_cce, C.byref(L), C.byref(cce)):
                got.append((L.value, cce.value))
        assert got == want, n_cce
    assert H.pscan_host_n_cand(88) == 165 and all(c % L == 0 and c + L <= 84 for L, c in SR.candidates(84))


def test_search_space_equals_the_twin_for_every_level_size_and_subframe(H, capi):
    rng = np.random.default_rng(5)
    rnti = np.concatenate([[0x003D, 0xFFF3, 0x0100, 0x8000], rng.integers(0x3D, 0xFFF4, 196)]).astype(np.uint32)
    out = np.zeros((rnti.size, 10, 88, 4, 6), np.int8)
    H.pscan_host_spaces(rnti.ctypes.data_as(C.POINTER(C.c_uint32)), rnti.size, out.ctypes.data_as(C.POINTER(C.c_int8)))
    wraps = nothing = 0
    for r, x in enumerate(rnti):
        for sf, n_cce, lv in itertools.product(range(10), range(1, 89), range(4)):
            L = 1 << lv
            sp = capi.ue_search_space(int(x), sf, n_cce, L)
            assert sp == SR.search_space(int(x), sf, n_cce, L)
            assert all(c % L == 0 and 0 <= c and c + L <= n_cce for c in sp) and len(sp) == (0 if n_cce < L else 6 if L <= 2 else 2)
            got = [int(c) for c in out[r, sf, n_cce - 1, lv] if c >= 0]
            assert got == sorted(set(sp)), (hex(x), sf, n_cce, L)
            wraps += 0 < n_cce // L < len(sp) and len(set(sp)) == n_cce // L
            nothing += n_cce < L
    assert wraps > 1000 and nothing > 1000
    # outside the C-RNTI range nothing is in space (the twin's list is empty); Y_k of 36.213 for one hand-computed value
    edge = np.array([0, 0x3C, 0xFFF4, 0xFFFF], np.uint32)
    out = np.zeros((4, 10, 88, 4, 6), np.int8)
    H.pscan_host_spaces(edge.ctypes.data_as(C.POINTER(C.c_uint32)), 4, out.ctypes.data_as(C.POINTER(C.c_int8)))
    assert (out == -1).all()
    assert capi.ue_search_space(1, 0, 88, 1)[0] == 39827 % 65537 % 88 and capi.ue_search_space(1, 1, 88, 8)[0] == 8 * ((39827 * 39827 % 65537) % 11)


def test_maps_at_the_larger_cap_equal_numpy_and_contain_the_pdcch_stage_s(H):
    n_maps = beyond = 0
    for n_rb, ports, cp, cfi, res, dur in itertools.product(PR.BANDWIDTHS, (1, 2, 4), (1, 2), (1, 2, 3), (1, 2, 3, 4), (1, 2)):
        for n_id, mi in ((0, 1), (503, 1), (257, 2 if res < 4 else 0)):
            if n_id and n_rb in (50, 75):
                continue
            lay = DR.layout(n_id, cp, ports, n_rb, cfi, dur, res, mi)
            n_reg, n_cce = C.c_int32(), C.c_int32()
            re, small = np.zeros(3168, np.int32), np.zeros(576, np.int32)
            ok = H.pscan_host_map(n_rb, ports, cp, n_id, dur, res, mi, cfi, C.byref(n_reg), C.byref(n_cce), _ip(re), _ip(small))
            what = (n_rb, ports, cp, cfi, res, dur, n_id, mi)
            assert ok in (4, 7) and (lay is None) == (ok == 4), what
            if lay is None:
                assert n_reg.value == 0 and (re == -1).all()
                continue
            n_maps += 1
            assert (n_reg.value, n_cce.value) == (lay["n_reg"], lay["n_cce"]) and lay["n_cce"] <= 88, what
            q = DR.quad_of_reg(lay["n_reg"], n_id)
            want = np.full(3168, -1, np.int64)
            for i, (k, l) in enumerate(lay["order"]):
                if q[i] < 9 * lay["n_cce"]:
                    want[4 * q[i]:4 * q[i] + 4] = [(l << 16) | c for c in DR.reg_columns(k, l, n_id, ports, cp)]
            assert np.array_equal(re, want), what
            assert np.array_equal(re[:576], small), what                   # pdc_build_map's 576 entries are the first 576
            beyond += lay["n_cce"] > 64
    print("maps compared:", n_maps, "with more than 64 CCEs:", beyond)
    assert n_maps > 1000 and beyond > 20


def test_scrambling_by_jumps_and_the_wide_rnti(H):
    pn = load_pkg().synth._pn
    for n_id, sf in ((0, 0), (1, 3), (277, 9), (503, 5)):
        words, w36 = np.zeros(198, np.uint32), np.zeros(36, np.uint32)
        H.pscan_host_scramble(sf, n_id, words.ctypes.data_as(C.POINTER(C.c_uint32)), w36.ctypes.data_as(C.POINTER(C.c_uint32)))
        assert [(int(words[i >> 5]) >> (i & 31)) & 1 for i in range(6336)] == list(pn(sf * 512 + n_id, 6336))
        assert np.array_equal(words[:36], w36)                              # pdc_scramble_word's, which clocks from zero
    rng, synth = np.random.default_rng(3), load_pkg().synth
    for A, rnti in ((8, 0xFFFF), (27, 0x0001), (48, 0x8001), (49, 0x4A31), (64, 0xC0DE), (57, 0x003D)):
        a = rng.integers(0, 2, A)
        c = np.concatenate([a, synth.crc16(a) ^ np.array([(rnti >> (15 - t)) & 1 for t in range(16)], np.uint8)])
        v = sum(int(b) << t for t, b in enumerate(c))
        narrow = C.c_uint32()
        assert H.pscan_host_rnti_x(v & (2 ** 64 - 1), v >> 64, A, C.byref(narrow)) == rnti
        assert A > 48 or narrow.value == rnti                               # pdc_rnti_x where it reaches


# ---------------------------------------------------------------- the decoder on noise-free code words
def _decode(H, capi, cl, L, A, sf=0, n_cce=88, cce=0):
    d, q, st = capi.PdcchScanDec(), np.zeros(240, np.int32), np.zeros(2, np.int32)
    assert H.pscan_host_decode(_dp(np.ascontiguousarray(cl, np.float64)), L, A, sf, n_cce, cce, 7, C.byref(d), _ip(q), _ip(st)) == 1
    return d, q, st


def test_every_code_word_length_decodes_exactly_where_the_rate_rule_forms_it(H, capi):
    rng = np.random.default_rng(21)
    n_ok = n_refused = 0
    for A in range(8, 65):
        K = A + 16
        for L in (1, 2, 4, 8):
            bits = rng.integers(0, 2, A)
            rnti = int(rng.integers(0x3D, 0xFFF4))
            cl = (1.0 - 2.0 * DR.dci_codeword(bits, rnti, L)) * (0.25 + rng.random(72 * L))
            d, q, st = _decode(H, capi, cl, L, A)
            ref = SR.decode_batch(cl[None, :], L, A)[0]
            if not SR.rate_ok(K, L):
                assert 4 * K > 216 * L and ref is None and bytes(d) == bytes(capi.PdcchScanDec()), (A, L)      # above the rate: a zero entry
                n_refused += 1
                continue
            want = sum(int(b) << t for t, b in enumerate(bits))
            assert (d.bits, d.rnti_x, d.n_err, d.quality) == (want, rnti, 0, 1.0) and d.flags & 9 == 9 and st[0] == st[1], (A, L)
            assert d.n_obs == np.count_nonzero(q[:3 * K]) and np.abs(q[:3 * K]).max() == 127
            assert (ref["bits"], ref["rnti_x"], ref["tb_ok"], ref["n_obs"], ref["n_err"], ref["quality"]) == (want, rnti, True, d.n_obs, 0, 1.0), (A, L)
            n_ok += 1
    assert n_refused == 64 - 39 + 1 and n_ok == 4 * 57 - n_refused          # L = 1 holds A <= 38 (K <= 54); every other level holds every size
    # noise, ties, punctured bits and silence: the twin's integers are numpy's
    for A, L in ((22, 1), (38, 1), (39, 2), (64, 2), (27, 4), (64, 8), (8, 8)):
        cl = rng.standard_normal((6, 72 * L))
        cl[4] = np.round(cl[4])                                             # many equal magnitudes and zeros: ties
        cl[5] = 0.0
        for row, ref in zip(cl, SR.decode_batch(cl, L, A)):
            d, _, _ = _decode(H, capi, row, L, A)
            assert (d.bits, d.rnti_x, d.n_err, d.n_obs, bool(d.flags & 8)) == (ref["bits"], ref["rnti_x"], ref["n_err"], ref["n_obs"], ref["tb_ok"]) and d.quality == ref["quality"], (A, L)
        assert ref["silent"] and (d.flags, d.bits, d.rnti_x, d.quality) == (1, 0, 0, 0.0)
        bad = cl[0].copy()
        bad[7] = np.inf
        assert bytes(_decode(H, capi, bad, L, A)[0]) == bytes(capi.PdcchScanDec()) and SR.decode_batch(bad[None, :], L, A)[0] is None


# ---------------------------------------------------------------- crafted grids
def test_the_case_set_covers_what_it_says():
    cases = SC.CASES
    assert {c[2] for c in cases} == {1, 2, 4} and {c[1] for c in cases} == {1, 2} and {c[3] for c in cases} >= {6, 15, 25, 50, 100}
    assert any(c[6] for c in cases) and {c[4] for c in cases} == {1, 2}
    kinds, levels, n_cces = set(), set(), {}
    for case in cases:
        tfg, cfi, planted = SC.crafted(case)
        ref = SC.reference(case)
        assert ref["n_sf"] == SC.N_SF and 4 <= ref["n_read"] <= 6 and tfg.shape == (2 * SC.N_SF * PR.n_symb_of(case[1]), 12 * case[3])
        n_cces.setdefault(case[3], set()).update(s["n_cce"] for s in ref["sf"] if s["cfi"])
        kinds |= {p["kind"] for p in planted}
        levels |= {p["L"] for p in planted if p["kind"] in ("a", "b")}
        assert not any(p["g"] == SC.SILENT_SF for p in planted)
        for p in planted:
            n_cce = ref["sf"][p["g"]]["n_cce"]
            assert SR.in_space(p["rnti"], p["g"] % 10, n_cce, p["L"], p["cce"]) == (p["kind"] in ("a", "b", "once")), p
    assert kinds == {"a", "b", "once", "out", "common"} and levels == {1, 2, 4, 8}
    assert n_cces[6] >= {2, 4, 6} and 20 in n_cces[25] and 41 in n_cces[50] and max(n_cces[100]) >= 84
    big = [p for p in SC.crafted(cases[-1])[2] if p["kind"] in ("a", "b", "once")]
    assert sum(p["cce"] > 15 for p in big) >= 3 and any(p["cce"] >= 64 for p in big) and any(9 * p["cce"] >= 576 for p in big)
    mid = [p for p in SC.crafted(cases[-2])[2] if p["kind"] in ("a", "b", "once")]
    assert any(p["cce"] > 15 for p in mid) and any(p["cce"] >= 32 for p in mid)
    # wrap-around: at 6 RB a space of six candidates falls onto fewer starts
    assert any(len(set(SR.search_space(SC.RNTI_A, g, s["n_cce"], 1))) < 6 for g, s in enumerate(SC.reference(cases[0])["sf"]) if s["cfi"])


def _compare(o, tab, ref, planted, what):
    """every decode of the twin against numpy -> (decodes, excused)"""
    n = excused = 0
    plant = {(p["g"], p["L"], p["cce"], p["i"]) for p in planted}
    for g, s in enumerate(ref["sf"]):
        t = o.sf[g]
        assert (t.cfi, t.n_reg, t.n_cce, t.n_cand) == (s["cfi"], s["n_reg"], s["n_cce"], s["n_cand"]), (what, g)
    for (g, i, si), r in ref["dec"].items():
        d = tab[(g * 165 + i) * 6 + si]
        n += 1
        if r["near_half"]:
            assert (g, r["L"], r["cce"], si) not in plant, (what, g, i, si)
            excused += 1
            continue
        assert (d.bits, d.rnti_x, d.flags, d.n_err, d.n_obs, d.n_repeat) == (r["bits"], r["rnti_x"], r["flags"], r["n_err"], r["n_obs"], r["n_repeat"]), (what, g, i, si)
        assert abs(d.quality - r["quality"]) <= TOL, (what, g, i, si)
    return n, excused


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_twin_against_numpy_on_crafted_grids(H, capi, case):
    tfg, cfi, planted = SC.crafted(case)
    ref = SC.reference(case)
    o, tab, llr = SC.twin_record(H, capi, case, tfg, cfi, want_llr=True)
    worst = 0.0
    for g, want in ref["llr"].items():
        assert np.abs(want).max() > 0 and not llr[g][want.size:].any()
        worst = max(worst, np.abs(llr[g][:want.size] - want).max() / np.abs(want).max())
    assert worst <= TOL, worst
    n, excused = _compare(o, tab, ref, planted, SC.case_id(case))
    assert excused <= 0.01 * n
    if not excused:
        head = ("n_read", "n_accepted", "n_si", "n_paging", "n_ra", "n_ue", "n_rnti", "n_msg", "n_dropped")
        assert {k: getattr(o, k) for k in head} == {k: ref[k] for k in head}
        assert [(m["subframe"], capi.scan_candidates(ref["sf"][m["subframe"]]["n_cce"]).index((m["L"], m["cce"])), m["size_index"]) for m in o.listed()] == ref["msg"]
        for g, s in enumerate(ref["sf"]):
            assert (o.sf[g].n_common, o.sf[g].n_ue, list(o.sf[g].cce_mask)) == (s["n_common"], s["n_ue"], s["cce_mask"]), g
    assert (o.n_sf, o.dl_mask, o.n_rb, o.n_ports, o.n_sizes) == (SC.N_SF, SC.dl_mask_of(case), case[3], case[2], len(SC.sizes_of(case)))
    # what was planted
    listed = {(m["subframe"], m["L"], m["cce"], m["size_index"]): m for m in o.listed()}
    once1, _, _ = SC.twin_record(H, capi, case, tfg, cfi, cfg=SC.make_cfg(capi, case, min_repeat=1))
    listed1 = {(m["subframe"], m["L"], m["cce"], m["size_index"]): m for m in once1.listed()}
    for p in planted:
        key = (p["g"], p["L"], p["cce"], p["i"])
        if p["kind"] == "out":
            n_cce = ref["sf"][p["g"]]["n_cce"]
            d = tab[(p["g"] * 165 + capi.scan_candidates(n_cce).index((p["L"], p["cce"]))) * 6 + p["i"]]
            assert (d.bits, d.rnti_x) == (p["bits"], p["rnti"]) and d.flags & 1 and not d.flags & 6 and key not in listed, p
            continue
        m = listed[key]
        assert (m["bits"], m["rnti"]) == (p["bits"], p["rnti"]) and m["quality"] >= SC.min_quality(), p
        if p["kind"] == "once":
            assert m["n_repeat"] == 1 and m["flags"] & 4 and not m["flags"] & 2 and listed1[key]["flags"] & 2, p
        elif p["kind"] == "common":
            assert m["flags"] & 18 == 18 and m["n_repeat"] == 0, p
        else:
            assert m["flags"] & 6 == 6 and m["n_repeat"] >= 2, p
    # false accepts, twin and numpy alone
    fa = [m for m in o.listed() if m["flags"] & 2 and not SC.rereading(m, planted)]
    fa_ref = [k for k, d in ref["dec"].items() if d["flags"] & 2 and not SC.rereading(dict(subframe=k[0], L=d["L"], cce=d["cce"], size_index=k[2], bits=d["bits"], rnti=d["rnti_x"]), planted)]
    assert len(fa) <= 0.005 * n and len(fa_ref) <= 0.005 * n, (len(fa), len(fa_ref), n)
    # messages(): a planted DCI once, at the largest accepted level; rntis(): the recurring ones
    msgs = o.messages()
    for p in planted:
        if p["kind"] in ("a", "b", "common"):
            same = [m for m in msgs if (m["subframe"], m["rnti"], m["size_index"], m["bits"]) == (p["g"], p["rnti"], p["i"], p["bits"]) and
                    m["cce"] < p["cce"] + p["L"] and p["cce"] < m["cce"] + m["L"]]
            assert len(same) == 1 and same[0]["L"] >= p["L"], p
    want_rntis = {r: sum(p["rnti"] == r for p in planted) for r in (SC.RNTI_A, SC.RNTI_B) if sum(p["rnti"] == r for p in planted) >= 2}
    assert {r: c for r, c in o.rntis().items() if r in want_rntis} == want_rntis and o.n_rnti >= len(want_rntis)
    print(SC.case_id(case), "worst soft bit %.2e, %d decodes, %d excused, %d planted, false accepts %d (numpy %d)" % (worst, n, excused, len(planted), len(fa), len(fa_ref)))


@pytest.mark.parametrize("case", DC.CASES, ids=DC.case_id)
def test_on_the_pdcch_stage_s_grids_the_first_soft_bits_and_the_common_messages_are_that_stage_s(H, capi, case):
    tfg, cfi, planted = DC.crafted(case)
    HP = DC.load_twin(capi)
    old, old_llr = DC.twin_record(HP, capi, case, tfg, cfi, want_llr=True)
    scase = case + (None,)
    cfg = capi.PdcchScanCfg.make(DC.sizes_of(case), phich_duration=case[4], phich_resource=case[5], phich_mi=case[6])
    o, tab, llr = SC.twin_record(H, capi, scase, tfg, cfi, cfg=cfg, want_llr=True)
    assert o.n_sf == old.n_sf and np.array_equal(o.cfi, old.cfi) and np.array_equal(o.n_cce, old.n_cce) and old.n_read >= 3
    assert llr[:, :1152].tobytes() == old_llr.tobytes()
    mine = {(m["subframe"], m["L"], m["cce"], m["size_index"], m["bits"], m["rnti"]) for m in o.listed() if m["flags"] & 18 == 18}
    n = 0
    for g, s, i, d in old.entries():
        L, cce = old.slot_candidate(s)
        if d.flags & 2 and any((p["g"], p["slot"], p["i"]) == (g, s, i) for p in planted):
            assert (g, L, cce, i, d.bits, d.rnti_x) in mine, (g, s, i)
            n += 1
    assert n >= 2


def test_the_message_cap_and_n_dropped(H, capi):
    case = SC.CASES[4]
    tfg, cfi, _ = SC.crafted(case)
    full, _, _ = SC.twin_record(H, capi, case, tfg, cfi)
    assert full.n_dropped == 0 and full.n_msg > 12
    cut, tab, _ = SC.twin_record(H, capi, case, tfg, cfi, msg_cap=12)
    assert (cut.n_msg, cut.n_dropped) == (12, full.n_msg - 12) and bytes(cut.msg)[:12 * 40] == bytes(full.msg)[:12 * 40] and not any(bytes(cut.msg)[12 * 40:])
    # the cap cuts the list alone: counts, masks and n_repeat are taken over every entry
    for k in ("n_accepted", "n_ue", "n_rnti", "n_si", "n_paging", "n_ra"):
        assert getattr(cut, k) == getattr(full, k)
    assert bytes(cut.sf) == bytes(full.sf)
    ref = SR.receive(tfg, *case[:4], cfi, case[4], case[5], SC.sizes_of(case), SC.min_quality(), msg_cap=12)
    assert (ref["n_msg"], ref["n_dropped"]) == (12, full.n_msg - 12)
    # min_quality 0 with the recurrence rule off lists every in-space decode
    lax, _, _ = SC.twin_record(H, capi, case, tfg, cfi, cfg=SC.make_cfg(capi, case, min_quality=0.0, min_repeat=1))
    assert lax.n_msg > full.n_msg and lax.n_ue > full.n_ue and all(m["flags"] & 2 for m in lax.listed() if m["flags"] & 4 and m["quality"] >= 0)


# ---------------------------------------------------------------- sizes, field readers, load
def test_dci_ue_sizes_equal_their_derivation_and_the_known_figures(capi):
    for n_rb, ports, tdd in itertools.product(PR.BANDWIDTHS, (1, 2, 4), (False, True)):
        sizes = capi.dci_ue_sizes(n_rb, ports, tdd)
        assert set(sizes) == ({"0/1A", "1"} if ports == 1 else {"0/1A", "1", "1B/1D", "2A", "2"})
        for name, a in sizes.items():
            assert a == capi.dci_ue_size_derived(name, n_rb, ports, tdd) and a not in capi._DCI_AMBIGUOUS and 8 <= a <= 64, (n_rb, ports, tdd, name)
        assert sizes["1"] != sizes["0/1A"] == capi.dci_common_sizes(n_rb, tdd)[0]
    table = {"1": (19, 23, 27, 31, 33, 39), "2A": (28, 31, 36, 41, 42, 48), "2": (31, 34, 39, 43, 45, 51)}
    for name, row in table.items():
        assert tuple(capi.dci_ue_sizes(n, 2)[name] for n in (6, 15, 25, 50, 75, 100)) == row
    assert max(a for n in PR.BANDWIDTHS for p in (1, 2, 4) for a in capi.dci_ue_sizes(n, p).values()) == 54 == capi.dci_ue_sizes(100, 4)["2"]


def _bits(pairs, size):
    out = []
    for v, n in pairs:
        out += [(v >> (n - 1 - i)) & 1 for i in range(n)]
    assert len(out) <= size
    return out + [0] * (size - len(out))


def _riv(start, length, n_rb):
    return n_rb * (length - 1) + start if length - 1 <= n_rb // 2 else n_rb * (n_rb - length + 1) + (n_rb - 1 - start)


def pack_0(f, n_rb, capi):
    return _bits([(0, 1), (f["hopping"], 1), (_riv(f["rb_start"], f["n_rb_alloc"], n_rb), (n_rb * (n_rb + 1) // 2 - 1).bit_length()), (f["mcs"], 5), (f["ndi"], 1), (f["tpc"], 2),
                  (f["cyclic_shift"], 3), (f["cqi_request"], 1)], capi.dci_ue_sizes(n_rb, 1)["0/1A"])


def pack_1(f, n_rb, capi):
    head = [(f["ra_type"], 1)] if n_rb > 10 else []
    return _bits(head + [(f["ra"], -(-n_rb // capi._RBG_P[n_rb])), (f["mcs"], 5), (f["harq"], 3), (f["ndi"], 1), (f["rv"], 2), (f["tpc"], 2)], capi.dci_ue_sizes(n_rb, 1)["1"])


def pack_2x(f, n_rb, ports, fmt, capi):
    head = [(f["ra_type"], 1)] if n_rb > 10 else []
    pre = {("2A", 2): 0, ("2A", 4): 2, ("2", 2): 3, ("2", 4): 6}[(fmt, ports)]
    tb = [(v, n) for t in f["tb"] for v, n in ((t["mcs"], 5), (t["ndi"], 1), (t["rv"], 2))]
    return _bits(head + [(f["ra"], -(-n_rb // capi._RBG_P[n_rb])), (f["tpc"], 2), (f["harq"], 3), (f["swap"], 1)] + tb + [(f["precoding"], pre)], capi.dci_ue_sizes(n_rb, ports)[fmt])


def test_field_readers_return_what_the_packers_put_in(capi):
    rng = np.random.default_rng(8)
    as_int = lambda b: sum(int(v) << t for t, v in enumerate(b))
    for n_rb in PR.BANDWIDTHS:
        P, nb = capi._RBG_P[n_rb], -(-n_rb // capi._RBG_P[n_rb])
        for _ in range(20):
            start = int(rng.integers(0, n_rb))
            f0 = dict(hopping=int(rng.integers(2)), rb_start=start, n_rb_alloc=int(rng.integers(1, n_rb - start + 1)), mcs=int(rng.integers(32)), ndi=int(rng.integers(2)),
                      tpc=int(rng.integers(4)), cyclic_shift=int(rng.integers(8)), cqi_request=int(rng.integers(2)))
            got = capi.dci_0_fields(as_int(pack_0(f0, n_rb, capi)), n_rb)
            assert {k: got[k] for k in f0} == f0 and got["prbs"] == list(range(start, start + f0["n_rb_alloc"]))
            f1 = dict(ra_type=int(rng.integers(2)) if n_rb > 10 else 0, ra=int(rng.integers(1 << nb)), mcs=int(rng.integers(32)), harq=int(rng.integers(8)), ndi=int(rng.integers(2)),
                      rv=int(rng.integers(4)), tpc=int(rng.integers(4)))
            got = capi.dci_1_fields(pack_1(f1, n_rb, capi), n_rb)
            assert {k: got[k] for k in f1} == f1 and got["prbs"] == capi.ra_type01_prbs(f1["ra_type"], f1["ra"], n_rb)
            for ports, fmt in itertools.product((2, 4), ("2A", "2")):
                pre = {("2A", 2): 0, ("2A", 4): 2, ("2", 2): 3, ("2", 4): 6}[(fmt, ports)]
                f2 = dict(ra_type=f1["ra_type"], ra=f1["ra"], tpc=1, harq=5, swap=1, tb=[dict(mcs=int(rng.integers(32)), ndi=1, rv=2), dict(mcs=3, ndi=0, rv=int(rng.integers(4)))],
                          precoding=int(rng.integers(1 << pre)))
                got = capi.dci_2x_fields(as_int(pack_2x(f2, n_rb, ports, fmt, capi)), n_rb, ports, fmt)
                assert {k: got[k] for k in f2} == f2
        # type 0: RBG i is PRBs P i .. P i + P - 1 (the last one shorter); every RBG set gives every PRB once
        assert capi.ra_type01_prbs(0, (1 << nb) - 1, n_rb) == list(range(n_rb))
        assert capi.ra_type01_prbs(0, 1 << (nb - 1), n_rb) == list(range(P)) and capi.ra_type01_prbs(0, 1, n_rb) == list(range(P * (nb - 1), n_rb))
        if n_rb > 10:
            # type 1: the PRBs of subset p are those of RBGs p, p + P, ..; without a shift bit i is the i-th of them
            lp, n1 = (P - 1).bit_length(), nb - (P - 1).bit_length() - 1
            for p in range(P):
                subset = [r for r in range(n_rb) if (r // P) % P == p]
                full = capi.ra_type01_prbs(1, (p << (nb - lp)) | ((1 << n1) - 1), n_rb)
                assert full == subset[:n1], (n_rb, p)
                shifted = capi.ra_type01_prbs(1, (p << (nb - lp)) | (1 << n1) | ((1 << n1) - 1), n_rb)
                assert shifted == subset[len(subset) - n1:] if len(subset) >= n1 else set(shifted) <= set(subset), (n_rb, p)


def test_load_counts_the_grants_of_a_grid_with_known_grants(H, capi):
    case = SC.CASES[4]                                       # 25 RB, two ports
    n_rb, sizes = 25, SC.sizes_of(case)
    a01, a1, a2a = capi.dci_ue_sizes(25, 2)["0/1A"], capi.dci_ue_sizes(25, 2)["1"], capi.dci_ue_sizes(25, 2)["2A"]
    assert sizes[:3] == (a01, a1, a2a)
    up = dict(hopping=0, rb_start=3, n_rb_alloc=7, mcs=9, ndi=1, tpc=1, cyclic_shift=0, cqi_request=0)
    dl_1a = DC.pack_1a(dict(flag_1a=1, distributed=0, rb_start=10, n_rb_alloc=5, mcs=4, harq=2, ndi=0, rv=0, tpc=1), 25)
    dl_1 = pack_1(dict(ra_type=0, ra=0b1010000000001, mcs=11, harq=1, ndi=1, rv=0, tpc=0), 25, capi)            # RBGs 0, 2 and 12: 2 + 2 + 1 PRBs
    dl_2a = pack_2x(dict(ra_type=0, ra=0b0000000000110, tpc=0, harq=0, swap=0, tb=[dict(mcs=5, ndi=0, rv=0), dict(mcs=6, ndi=1, rv=1)], precoding=0), 25, 2, "2A", capi)
    X, Y = 0x1111, 0x2222

    def plan(g, sf, n_cce, put):
        if g > 2:
            return
        used = set()

        def at(rnti, L):
            c = [c for c in SR.search_space(rnti, sf, n_cce, L) if not used & set(range(c, c + L))][0]
            used.update(range(c, c + L))
            return c
        put(X, 2, at(X, 2), 0, "a", dl_1a if g != 1 else pack_0(up, 25, capi))
        put(Y, 4, at(Y, 4), 1 if g != 2 else 2, "b", dl_1 if g != 2 else dl_2a)

    tfg, cfi, planted = SC.crafted(case, plan=plan)
    o, _, _ = SC.twin_record(H, capi, case, tfg, cfi)
    rows = {r["subframe"]: r for r in o.load(25)}
    assert set(rows) == {g for g in range(6) if o.sf[g].cfi} and o.rntis() == {X: 3, Y: 3}
    assert [(rows[g]["dl_grants"], rows[g]["ul_grants"], rows[g]["dl_prb"], rows[g]["ul_prb"], rows[g]["rntis"]) for g in (0, 1, 2)] == [
        (2, 0, 5 + 5, 0, [X, Y]), (1, 1, 5, 7, [X, Y]), (2, 0, 5 + 4, 0, [X, Y])]
    assert all((rows[g]["dl_grants"], rows[g]["ul_grants"], rows[g]["rntis"]) == (0, 0, []) for g in rows if g > 2)
    assert rows[0]["cce_used"] >= 6 and rows[0]["n_cce"] == o.sf[0].n_cce


# ---------------------------------------------------------------- sanitizers
def test_stand_alone_program_under_address_and_undefined_sanitizers(H, capi, tmp_path):
    """the same source with its own main, built with -fsanitize=address,undefined: a clean exit, and the record the library form gives"""
    if SC.stale(SC.SAN):
        subprocess.check_call(PC.HIPCC + ["-O1", "-g", "-DPDCCH_SCAN_HOST_MAIN", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                                          "-fno-sanitize-recover=undefined", "-o", SC.SAN, SC.TWIN_SRC])
    runs = [(SC.CASES[1], None), (SC.CASES[7], None), (SC.CASES[2], np.full((84, 180), np.nan + 0j))]
    for case, grid in runs:
        tfg, cfi, _ = SC.crafted(case)
        tfg = tfg if grid is None else grid
        n_id, cp, ports, n_rb = case[:4]
        cfg = SC.make_cfg(capi, case)
        cfi72 = np.concatenate([cfi, np.zeros(72, np.int32)])[:72].astype(np.int32)
        path = tmp_path / "grid.bin"
        with open(path, "wb") as f:
            f.write(np.array([tfg.shape[0], PR.n_symb_of(cp), n_rb, n_id, cp, ports, SC.dl_mask_of(case), 0], np.int32).tobytes() + PC.jump_tables(n_rb)[:32].tobytes() +
                    bytes(cfg) + cfi72.tobytes() + np.ascontiguousarray(tfg, np.complex128).tobytes())
        r = subprocess.run([SC.SAN, str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
        v = r.stdout.split()
        o, _, _ = SC.twin_record(H, capi, case, tfg, cfi)
        assert [int(x) for x in v[:10]] == [o.n_sf, o.n_read, o.n_accepted, o.n_si, o.n_paging, o.n_ra, o.n_ue, o.n_rnti, o.n_msg, o.n_dropped]
        per = [x for m in o.listed() for x in (m["subframe"], m["L"], m["cce"], m["size_index"], m["bits"], m["rnti"], m["flags"], m["n_repeat"], m["n_err"], m["n_obs"], m["quality"])]
        assert [float(x) for x in v[10:]] == [float(x) for x in per]
