"""Distributed allocations and format 1C on the CPU: the host twin (tests/host/pdsch_dvrb_host.cpp: pdsch.h compiled for the host, the code
k_pdsch_plan and k_pdsch_llr run) against the numpy statement of the rule (tests/pdsch_dvrb_ref.py, written from include/lcs.h) and
the package's own Python (capi.dvrb_prb, capi.dci_1c_fields) -- the properties that pin a rule written from memory of the standard,
the 1C payloads, the set-based element lists, the whole record on crafted grids, and the stage with the setting off."""
import ctypes as C

import numpy as np
import pytest

import pcfich_ref as PR
import pdsch_cases as SC
import pdsch_dvrb_cases as VC
import pdsch_dvrb_ref as VR
import pdsch_ref as SR
from conftest import load_pkg


@pytest.fixture(scope="module")
def H():
    return VC.load_twin(load_pkg().capi)


@pytest.fixture(scope="module")
def H0():
    return SC.load_twin(load_pkg().capi)


def test_layouts(H):
    capi = load_pkg().capi
    assert H.pdsch_dvrb_host_alloc_bytes() == C.sizeof(capi.PdschAlloc) == 256 and H.pdsch_dvrb_host_alloc_cfg_bytes() == C.sizeof(capi.PdschAllocCfg) == 16


def test_map_properties_for_every_bandwidth(H):
    """what pins the map: a permutation per slot, the two PRBs of a VRB N_gap apart, N_VRB <= n_rb; twin = numpy = capi"""
    capi = load_pkg().capi
    out = np.zeros(5, np.int32)
    n_checked = 0
    for n_rb in range(6, 111):
        for gap in (0, 1):
            if gap and n_rb < 50:
                assert VR.gaps(n_rb)[1] is None and capi.dvrb_gap(n_rb)[1] is None
                continue
            z = VR.sizes(n_rb, gap)
            H.pdsch_dvrb_host_params(n_rb, gap, SC._ip(out))
            assert tuple(out) == (z["n_gap"], z["n_vrb"], z["unit"], z["n_row"], z["n_null"]), (n_rb, gap)
            assert capi.dvrb_sizes(n_rb, gap) == z and capi.dvrb_gap(n_rb)[gap] == z["n_gap"]
            assert 0 < z["n_vrb"] <= n_rb and z["n_vrb"] % 2 == 0
            maps = [[VR.prb_of(n_rb, gap, v, s) for v in range(z["n_vrb"])] for s in (0, 1)]
            for s in (0, 1):
                assert len(set(maps[s])) == z["n_vrb"] and min(maps[s]) >= 0 and max(maps[s]) < n_rb, (n_rb, gap, s)
                assert maps[s] == [H.pdsch_dvrb_host_prb(n_rb, gap, v, s) for v in range(z["n_vrb"])] == [capi.dvrb_prb(n_rb, gap, v, s) for v in range(z["n_vrb"])]
                assert maps[s] == [VR.prb_of(n_rb, gap, v, s + 2) for v in range(z["n_vrb"])]
            assert all(abs(a - b) == z["n_gap"] for a, b in zip(*maps)), (n_rb, gap)
            n_checked += 1
    assert n_checked == 105 + 61
    assert [VR.prb_of(25, 0, v, 0) for v in range(8)] == [0, 6, 12, 18, 1, 7, 13, 19]
    assert [VR.sizes(n, 0)["n_null"] for n in (6, 15, 25)] == [2, 2, 0]


def test_sizes_of_format_1c(H):
    pkg = load_pkg()
    assert [H.pdsch_dvrb_host_tbs_1c(i) for i in range(32)] == VR.TBS_1C == [pkg.capi.tbs_1c(i) for i in range(32)]
    assert all(t + 24 in pkg.synth.TURBO_K for t in VR.TBS_1C)
    for n_rb in (6, 15, 25, 50, 75, 100):
        assert H.pdsch_dvrb_host_1c_bits(n_rb) == VR.size_1c(n_rb) == pkg.capi.dci_common_sizes(n_rb)[1], n_rb
        assert pkg.capi.dci_1c_riv_bits(n_rb) == VR.riv_bits_1c(n_rb)


@pytest.mark.parametrize("n_rb", [6, 15, 25, 50, 100])
def test_format_1c_write_read_round_trip(H, n_rb):
    """every valid (gap, start, length, I_TBS): the generator's writer and the reference's agree, and the three readers return the fields"""
    pkg = load_pkg()
    out = np.zeros(7, np.int32)
    step = VR.n_step_of(n_rb)
    n_done = 0
    for gap in ((0, 1) if n_rb >= 50 else (0,)):
        n = VR.sizes(n_rb, gap)["n_vrb"] // step
        seen = set()
        for S in range(n):
            for L in range(1, n - S + 1):
                for i_tbs in range(32):
                    bits = VR.pack_1c(gap, step * S, step * L, i_tbs, n_rb)
                    if i_tbs in (0, 31):
                        assert bits == pkg.synth.dci_1c_payload(dict(gap=gap, rb_start=step * S, n_prb=step * L, i_tbs=i_tbs), n_rb)
                    assert len(bits) == pkg.capi.dci_common_sizes(n_rb)[1]
                    v = sum(b << t for t, b in enumerate(bits))
                    H.pdsch_dvrb_host_1c(v, n_rb, SC._ip(out))
                    f = VR.fields_1c(v, n_rb)
                    assert f["riv_ok"] and (f["gap"], f["rb_start"], f["n_prb"], f["i_tbs"]) == (gap, step * S, step * L, i_tbs)
                    assert tuple(out) == (f["gap"], f["riv"], 1, f["rb_start"], f["n_prb"], f["i_tbs"], step)
                    if i_tbs in (0, 31):
                        c = pkg.capi.dci_1c_fields(bits, n_rb)
                        assert (c["gap"], c["riv"], c["riv_ok"], c["rb_start"], c["n_rb_alloc"], c["i_tbs"], c["tbs"]) == \
                               (gap, f["riv"], True, step * S, step * L, i_tbs, VR.TBS_1C[i_tbs])
                    n_done += 1
                seen.add(f["riv"])
        assert seen == set(range(n * (n + 1) // 2))          # the valid RIVs are exactly those below N' (N' + 1) / 2
        for riv in range(n * (n + 1) // 2, 1 << VR.riv_bits_1c(n_rb)):
            v = sum(b << t for t, b in enumerate(VR.pack_1c(gap, 0, step, 5, n_rb, riv=riv)))
            H.pdsch_dvrb_host_1c(v, n_rb, SC._ip(out))
            f = VR.fields_1c(v, n_rb)
            assert not f["riv_ok"] and tuple(out) == (gap, riv, 0, f["rb_start"], f["n_prb"], 5, step) and not pkg.capi.dci_1c_fields(v, n_rb)["riv_ok"]
    assert n_done >= 32 * 6


def test_assumed_redundancy_version(H):
    capi = load_pkg().capi
    for kind in (1, 2, 4):
        for sfn0 in (-1, 0, 5, 6, 1023):
            for w in (0, 1, 5, 10, 15, 20, 40):
                for g in range(0, 40):
                    want = VR.rv_1c(kind, g, sfn0, w)
                    assert H.pdsch_dvrb_host_1c_rv(kind, g, sfn0, w) == want, (kind, sfn0, w, g)
                    if kind != 1 or sfn0 < 0 or (w in (0, 15) and not (g % 10 == 5 and (sfn0 + g // 10) % 2 == 0)):
                        assert want == 0
    assert [VR.rv_1c(1, 5 + 20 * i, 0, 0) for i in range(4)] == [capi.sib1_rv(2 * i) for i in range(4)] == [0, 2, 3, 1]


def test_elements_over_sets_against_brute_force(H):
    """the kernel's rank -> (l, k) over a per-slot set of resource blocks against the brute force: every CRS pattern, both CP types,
    PBCH / PSS / SSS subframes, the central cut through half a resource block at odd n_rb, both gaps"""
    lk = np.zeros(2 * 12 * 110 * 14, np.int32)
    n_cases = 0
    for n_id, cp, ports, n_rb in ((0, 1, 1, 6), (1, 2, 2, 6), (68, 1, 4, 6), (5, 1, 1, 15), (141, 2, 2, 15), (256, 1, 4, 15), (9, 1, 2, 25), (503, 2, 4, 25), (4, 1, 1, 50),
                                  (2, 1, 4, 50), (7, 1, 2, 75)):
        for gap in ((0, 1) if n_rb >= 50 else (0,)):
            nv, unit = VR.sizes(n_rb, gap)["n_vrb"], VR.sizes(n_rb, gap)["unit"]
            for sf in (0, 3, 5):
                for tdd in (0, 1):
                    for n_ctrl in (1, 4):
                        for s, n in ((0, nv), (0, 1), (nv - 1, 1), (nv // 2 - 1, 2), (1, nv - 1), (max(unit - 3, 0), min(6, nv - max(unit - 3, 0)))):
                            want = VR.elements(n_id, cp, ports, n_rb, sf, n_ctrl, gap, s, n, bool(tdd))
                            got = H.pdsch_dvrb_host_elements(n_rb, ports, PR.n_symb_of(cp), n_id, sf, tdd, n_ctrl, gap, s, n, SC._ip(lk), lk.size // 2)
                            assert got == len(want) and [tuple(v) for v in lk[:2 * got].reshape(-1, 2)] == want, (n_id, cp, ports, n_rb, gap, sf, tdd, n_ctrl, s, n)
                            n_cases += 1
    assert n_cases > 900


def test_crafted_plans_hold_what_they_claim():
    """the crafted grids carry every kind of grant the rule distinguishes"""
    for case in VC.CASES:
        _, _, planted = VC.crafted(case)
        n_rb, tdd = case[3], VC.tdd_of(case)
        by_g = {}
        for p in planted:
            by_g.setdefault(p["g"], []).append(p)
        kinds = {(p["format"], p["distributed"], SR.kind_of(p["rnti"])) for p in planted}
        if not tdd:         # (the TDD table leaves subframes 0, 1, 4, 5, 6, 9 of the plan: the FDD case of the same bandwidth, ports and CP holds every kind)
            assert {("1a", 1, 1), ("1a", 1, 2), ("1a", 1, 4), ("1c", 1, 1), ("1c", 1, 2), ("1a", 0, 1)} <= kinds, VC.case_id(case)
            assert by_g[VC.BEYOND_SF][0]["bits"] is None or n_rb == 6
        if not tdd and n_rb > 6:          # (the control region of 6 resource blocks holds one candidate)
            assert len(by_g[VC.TWO_SF]) == 2 and {p["i"] for p in by_g[VC.TWO_SF]} == {0, 1} and ("1c", 1, 4) in kinds
        if not tdd:
            assert by_g[VC.RIV_SF][0]["riv"] is not None and by_g[VC.ROWS_SF][0]["bits"] is None
        if n_rb == 15:      # through the centre in subframes 0 and 5: columns 54 .. 125, which cut resource blocks 4 and 10 in half
            for g in (0, 5):
                lists = VR.prb_lists(n_rb, 0, by_g[g][0]["rb_start"], by_g[g][0]["n_prb"])
                assert all({4, 10} <= set(x) for x in lists)
        if n_rb == 50:
            assert by_g[8][0]["gap"] == 1 and by_g[9][0]["gap"] == 1 and by_g[9][0]["rb_start"] < 18 < by_g[9][0]["rb_start"] + by_g[9][0]["n_prb"]
        assert any(p["format"] == "1c" and SR.kind_of(p["rnti"]) == 1 and p["rv"] != 0 for p in planted), VC.case_id(case)


@pytest.mark.parametrize("setting", sorted(VC.SETTINGS))
@pytest.mark.parametrize("case", VC.CASES, ids=VC.case_id)
def test_record_against_numpy(H, case, setting):
    """fields, status, iterations, payload and last_alloc equal; soft bits to 1e-12 of the block's largest (the stage's bar on the
    CPU); no numpy decision within 1e-9 of a tie; every planted block decoded to its bytes where the assumed rv is the sent one"""
    capi = load_pkg().capi
    tfg, cfi, planted = VC.crafted(case)
    blocks = VC.reference(case, setting)
    pdc = SC.pdcch_twin_record(capi, case, tfg, cfi)
    rec, allocs, llr = VC.twin_record(H, capi, case, tfg, pdc, setting, want_soft=True)
    assert all(b["margin"] > 1e-9 for b in blocks), [b["margin"] for b in blocks]
    n, excused = SC.assert_blocks_against_numpy(rec, blocks, VC.case_id(case))
    assert excused == 0 and n >= len(planted)         # (beyond the planted: a noise candidate whose CRC lands on a followed RNTI, as numpy finds it too)
    assert allocs == [b["alloc"] for b in blocks]
    for b, slot in zip(blocks, VC.slots_of(blocks)):
        if "llr" in b:
            G = len(b["llr"])
            assert G == 2 * b["n_re"] and np.abs(llr[slot, :G] - b["llr"]).max() <= 1e-12 * np.abs(b["llr"]).max(), (VC.case_id(case), b["subframe"])
    st = [0] * 10
    for b in blocks:
        st[b["status"]] += 1
    assert list(rec.n_status) == st and rec.n_ok == st[1] and rec.n_overflow == 0 and st[SR.STATUS["distributed"]] == 0
    got = {(x["subframe"], x["rnti"]): x for x in rec.blocks()}     # (a DCI sent on eight CCEs is found on their first four too: the slot may be lower)
    n_ok = 0
    for p in planted:
        x = got[(p["g"], p["rnti"])]
        assert (x["mcs"], x["rnti"]) == (p["mcs"], p["rnti"]) and (p["riv"] is not None or (x["rb_start"], x["n_prb"]) == (p["rb_start"], p["n_prb"]))
        if p["riv"] is not None or (p["g"] == VC.BEYOND_SF and p["bits"] is None and not VC.tdd_of(case)):
            assert x["status"] == "bad_alloc" and x["bytes"] == b""
        elif p["g"] == VC.ROWS_SF:
            assert x["status"] == "rows"
        elif p["bits"] is None:
            assert x["status"] == "special"
        elif setting == "sfn" or p["format"] == "1a" or p["rv"] == 0:
            assert x["status"] == "ok" and x["rv"] == p["rv"] and x["bytes"] == np.packbits(p["bits"]).tobytes(), (VC.case_id(case), p["g"], x["status"])
            n_ok += 1
        else:                   # a 1C SI grant sent with rv != 0 and read as rv 0: a wrong assumption shows as crc
            assert x["status"] == "crc" and x["rv"] == 0
    assert n_ok >= (3 if VC.tdd_of(case) else 8)


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_setting_off_leaves_the_record_as_it_was(H, H0, case):
    """zeros, and a setting whose flags are zero: the record of the stage's own nine grids, byte for byte the stage's twin's"""
    capi = load_pkg().capi
    tfg, cfi, _ = SC.crafted(case)
    pdc = SC.pdcch_twin_record(capi, case, tfg, cfi)
    want = SC.twin_record(H0, capi, case, tfg, pdc)
    _, blocks = SC.reference(case)
    assert SC.assert_blocks_against_numpy(want, blocks, SC.case_id(case))[1] == 0
    for setting in ((0, 0, 0), (0, 6, 10)):
        rec, allocs = VC.twin_record(H, capi, case, tfg, pdc, setting)
        assert bytes(rec) == bytes(want)
        for a, b in zip(allocs, blocks):
            dist = b["status"] == SR.STATUS["distributed"]
            assert (a["format"], a["distributed"], a["n_step"]) == ("1a", int(dist), 1)
            inside = not dist and b["rb_start"] + b["n_prb"] <= case[3]
            assert a["prb"] == ([list(range(b["rb_start"], b["rb_start"] + b["n_prb"]))] * 2 if inside else [[], []])
