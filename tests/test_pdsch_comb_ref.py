"""The numpy statement of the rule that combines redundancy versions (tests/pdsch_comb_ref.py) on the scenarios of
tests/pdsch_comb_cases.py: the conditions on the inputs that the other tests of the stage rely on, and what the rule gives on each."""
import numpy as np
import pytest

import pdsch_comb_cases as CC
import pdsch_comb_ref as CR
import pdsch_ref as SR
from conftest import load_pkg

OK, CRC = SR.STATUS["ok"], SR.STATUS["crc"]


def planted_payload(sc, msg):
    _, _, planted = CC.crafted(sc)
    p = next(p for p in planted if p["msg"] == msg and p["bits"] is not None)
    return SR.payload_bytes(np.concatenate([np.zeros(0, np.uint8), p["bits"]]), 0, p["tbs"])


def groups(sc):
    return CC.reference(sc)[2]["groups"]


def test_sib1_rv():
    capi = load_pkg().capi
    assert [capi.sib1_rv(sfn) for sfn in range(0, 16, 2)] == [0, 2, 3, 1, 0, 2, 3, 1] and capi.sib1_rv(1023) == capi.sib1_rv(1022) == 1


@pytest.mark.parametrize("name", ["more-info-than-coded", "more-info-than-coded-forced"])
def test_more_information_than_coded_bits(name):
    """tbs 296 (K = 320) on one resource block of 6 (tbs 208, K = 232, forced, with the extended CP and two ports): G < K in every
    transmission.  Each member alone ends crc; the sum decodes to the planted bits.  Sent with rv 0, 1, 0, not 0, 2, 3: see
    test_parity_only_transmission_is_a_false_ok"""
    sc = CC.by_name(name)
    _, blocks, comb = CC.reference(sc)
    assert len(blocks) == 3 and all(b["status"] == CRC and b["n_iter"] == 8 and 2 * b["n_re"] < b["K"] for b in blocks)
    (g,) = comb["groups"]
    assert g["members"] == [0, 1, 2] and g["status"] == CR.STATUS["ok"] and 1 <= g["n_iter"] <= 8 and g["margin"] > 1e-9
    assert np.array_equal(g["payload"], planted_payload(sc, "a")) and g["rv_mask"] == 3


def test_rate_one_with_the_sib1_redundancy_versions():
    """the issue's first case with its rv 0, 2, 3 at the (tbs, n_prb) at which the numpy rule meets both conditions: tbs 488 (K = 512) on
    two resource blocks of 15, G = 528 -- 1.03 coded bits per bit of the code block; tbs 296 on one resource block does not (below)"""
    sc = CC.by_name("rate-one-rv023")
    _, blocks, comb = CC.reference(sc)
    assert [(b["rv"], b["status"], b["n_iter"], b["K"], 2 * b["n_re"]) for b in blocks] == [(0, CRC, 8, 512, 528), (2, CRC, 8, 512, 528), (3, CRC, 8, 512, 528)]
    (g,) = comb["groups"]
    assert g["members"] == [0, 1, 2] and g["status"] == CR.STATUS["ok"] and g["rv_mask"] == 0b1101 and np.array_equal(g["payload"], planted_payload(sc, "a"))


def test_parity_only_transmission_is_a_false_ok():
    """The issue's first case as it states it -- tbs 296 on one resource block, rv 0, 2, 3 -- does not meet "each member alone ends
    crc": a transmission with rv 2 or 3 and G well below K holds parity bits only, and none that the known first and last states of
    the trellis reach.  The stage's decoder then has a zero (rv 2) or never negative posterior, decides all zeros, and CRC24A of zeros
    is zero: status ok after one iteration, with a zero payload.  The rule takes such a block for a member that decoded.  Pinned here
    as a property of the input, so that a change of it is seen: on the grid, and on the decoder alone at three sizes, where rv 2 with
    G = K / 2 ends so at either noise level, while with G = K - 1 both rv 2 and rv 3 reach enough of the trellis to end crc."""
    sc = CC.by_name("more-info-rv023")
    _, blocks, comb = CC.reference(sc)
    assert [(b["rv"], b["status"], b["n_iter"]) for b in blocks] == [(0, CRC, 8), (2, OK, 1), (3, OK, 1)]
    assert not blocks[1]["payload"].any() and not blocks[2]["payload"].any() and all(2 * b["n_re"] < b["K"] for b in blocks)
    (g,) = comb["groups"]
    assert (g["status"], g["n_ok_members"], g["n_same"]) == (CR.STATUS["member"], 2, 2) and not g["payload"].any()
    synth = load_pkg().synth
    rng = np.random.default_rng(1)
    for tbs in (144, 296, 1480):
        K, F = SR.block_size(tbs)
        for rv, n_e, sigma, want in ((2, K // 2, 0.1, OK), (2, K // 2, 2.0, OK), (2, K - 1, 0.1, CRC), (3, K - 1, 0.1, CRC)):
            a = rng.integers(0, 2, tbs).astype(np.uint8)
            c = np.concatenate([np.zeros(F, np.uint8), a, synth.crc24a(a)])
            llr = (1 - 2.0 * synth.turbo_ratematch(synth.turbo_encode(c), n_e, rv, F)) + sigma * rng.standard_normal(n_e)
            r = SR.turbo_decode(SR.derm(llr, K, F, rv), K, F, 8)
            assert r["status"] == want and (want == CRC or (r["n_iter"] == 1 and not r["bits"].any())), (tbs, rv, n_e, sigma, r["status"], r["n_iter"])


def test_one_block_over_different_grants():
    """tbs 256 as (column 0, mcs 8) and (column 1, mcs 6), other allocations, one across the PSS / SSS columns, rv 0 / 2 / 3: the
    noise fails every member, the sum decodes"""
    sc = CC.by_name("different-grants")
    _, blocks, comb = CC.reference(sc)
    assert [(b["mcs"], b["rv"], b["n_prb"], b["status"], b["tbs"]) for b in blocks] == [(8, 0, 2, CRC, 256), (6, 2, 3, CRC, 256), (8, 3, 2, CRC, 256)]
    assert len({b["n_re"] for b in blocks}) == 2
    (g,) = comb["groups"]
    assert g["status"] == CR.STATUS["ok"] and g["n_iter"] >= 1 and g["rv_mask"] == 0b1101 and np.array_equal(g["payload"], planted_payload(sc, "a"))


def test_a_member_that_decodes_alone():
    sc = CC.by_name("member-decodes")
    _, blocks, comb = CC.reference(sc)
    assert [b["status"] for b in blocks] == [OK, CRC, OK]
    (g,) = comb["groups"]
    assert (g["status"], g["n_iter"], g["n_ok_members"], g["n_same"]) == (CR.STATUS["member"], 0, 2, 2) and np.array_equal(g["payload"], planted_payload(sc, "a"))


def test_changed_content():
    (g,) = groups(CC.by_name("changed-content-ok"))
    assert (g["status"], g["n_ok_members"], g["n_same"]) == (CR.STATUS["member"], 2, 1)
    assert np.array_equal(g["payload"], planted_payload(CC.by_name("changed-content-ok"), "a"))
    (g,) = groups(CC.by_name("changed-content-crc"))
    assert (g["status"], g["n_iter"], g["n_ok_members"], g["n_same"]) == (CR.STATUS["crc"], 8, 0, 0)


@pytest.mark.parametrize("name", ["parity", "parity-tdd"])
def test_parity(name):
    sc = CC.by_name(name)
    ga, gb = groups(sc)
    assert ga["members"] == list(range(0, len(ga["members"]) * 2, 2)) and gb["members"] == [m + 1 for m in ga["members"]]
    assert ga["status"] == gb["status"] == CR.STATUS["ok"]
    assert np.array_equal(ga["payload"], planted_payload(sc, "a")) and np.array_equal(gb["payload"], planted_payload(sc, "b"))


def test_rule_2():
    assert groups(CC.by_name("window-off")) == []
    a, c, b = groups(CC.by_name("window-20"))
    assert (a["members"], a["rule"], a["status"]) == ([0, 2], 2, CR.STATUS["ok"]) and np.array_equal(a["payload"], planted_payload(CC.by_name("window-20"), "a"))
    assert (c["members"], c["status"], c["tbs"]) == ([1], CR.STATUS["member"], 104)
    assert (b["members"], b["status"], b["n_iter"]) == ([3], CR.STATUS["crc"], 0)
    (g,) = groups(CC.by_name("window-no-sib1"))
    assert (g["members"], g["rule"], g["status"]) == ([0, 1, 2], 2, CR.STATUS["ok"])


def test_never_members():
    sc = CC.by_name("never-members")
    _, blocks, comb = CC.reference(sc)
    assert [(b["kind"], b["status"]) for b in blocks] == [(2, CRC), (4, CRC), (1, 7), (1, 3), (1, 4), (1, CRC)]
    (g,) = comb["groups"]
    assert g["members"] == [5] and g["status"] == CR.STATUS["crc"] and g["n_iter"] == 0 and np.array_equal(g["payload"], blocks[5]["payload"])
    _, blocks, comb = CC.reference(CC.by_name("rows"))
    assert [b["status"] for b in blocks] == [CRC, 5] and [g["members"] for g in comb["groups"]] == [[0]]


def test_limits():
    a, b = groups(CC.by_name("fifth-member"))
    assert a["members"] == [0, 1, 2, 3] and b["members"] == [4, 5] and a["status"] == b["status"] == CR.STATUS["ok"]
    assert np.array_equal(a["payload"], b["payload"])
    comb = CC.reference(CC.by_name("ninth-group"))[2]
    assert [g["members"] for g in comb["groups"]] == [[i] for i in range(8)] and comb["n_overflow"] == 2


def test_a_sum_that_is_silent():
    _, blocks, comb = CC.reference(CC.by_name("silent-sum"))
    assert [b["status"] for b in blocks] == [CRC, CRC] and np.array_equal(blocks[0]["llr"], -blocks[1]["llr"])
    (g,) = comb["groups"]
    assert (g["status"], g["n_iter"]) == (CR.STATUS["silent"], 0) and not g["payload"].any()


def test_no_decision_near_a_tie():
    """what the twin and the device are held to numpy on: no posterior of a decoded group, and of no block, within 1e-9 of zero"""
    for sc in CC.SCENARIOS:
        _, blocks, comb = CC.reference(sc)
        assert all(g["margin"] > 1e-9 for g in comb["groups"]), sc["name"]
        assert all(b["margin"] > 1e-9 for b in blocks), sc["name"]


def test_grouping_on_lists():
    """the grouping alone, on block lists written out by hand"""
    B = lambda sf, tbs, st=CRC, kind=1: dict(subframe=sf, tbs=tbs, status=st, kind=kind)
    bl = [B(5, 100), B(5, 100), B(15, 100), B(25, 100), B(25, 200), B(45, 100), B(45, 100), B(45, 100, 7), B(55, 100, CRC, 2)]
    assert CR.grouping(bl) == [(1, [0, 1, 3, 5]), (1, [2]), (1, [4]), (1, [6])]
    assert CR.grouping(bl, sib1=False) == [] and CR.grouping(bl, 61, sib1=False) == [(2, [0, 1, 2, 3]), (2, [4]), (2, [5, 6])]
    bl = [B(3, 100), B(4, 50), B(22, 100), B(23, 100), B(25, 100), B(42, 100)]
    assert CR.grouping(bl, 20) == [(2, [0, 2]), (2, [1]), (2, [3, 5]), (1, [4])]
    assert CR.grouping(bl, 1) == [(2, [0]), (2, [1]), (2, [2]), (2, [3]), (1, [4]), (2, [5])]
