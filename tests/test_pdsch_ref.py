"""The numpy statement of the PDSCH rule (tests/pdsch_ref.py) and the generator (synth) against each other and against what is pinned
elsewhere, on the CPU: code, rate matching and decoder round trips, the two number tables, the reference bits, the windowed rule
against the full-block decoder on the crafted cases, and the SIB1 reader against its writer."""
import numpy as np
import pytest

import pcfich_ref as PR
import pdsch_cases as SC
import pdsch_ref as SR
from conftest import load_pkg


def _block(rng, K, F):
    synth = load_pkg().synth
    a = rng.integers(0, 2, K - F - 24).astype(np.uint8)
    c = np.concatenate([np.zeros(F, np.uint8), a, synth.crc24a(a)])
    return a, c, synth.turbo_encode(c)


@pytest.mark.parametrize("K,F", [(40, 0), (64, 0), (64, 8), (512, 0), (528, 0), (528, 10), (2240, 0), (2240, 40)])
def test_round_trip_every_rv(K, F):
    """encoder -> rate matching -> de-rate-matching -> decoder, every rv, with fewer and with more bits than the circular buffer holds"""
    synth = load_pkg().synth
    rng = np.random.default_rng(K + F)
    a, c, d = _block(rng, K, F)
    n_w = 3 * (K + 4) - 2 * F
    for rv in range(4):
        for E in (2 * n_w // 3 & ~1, 2 * n_w + 6):
            e = synth.turbo_ratematch(d, E, rv, F)
            llr = (1 - 2.0 * e) + 0.3 * rng.standard_normal(E)
            res = SR.turbo_decode(SR.derm(llr, K, F, rv), K, F)
            assert res["status"] == 1 and np.array_equal(res["bits"], c), (K, F, rv, E, res["n_iter"])
            assert np.array_equal(SR.payload_bytes(res["bits"], F, len(a))[:(len(a) + 7) // 8], np.packbits(np.concatenate([a, np.zeros(-len(a) % 8, np.uint8)])))


def test_derm_is_the_inverse_of_rate_matching():
    synth = load_pkg().synth
    for K, F, rv, E in ((40, 0, 0, 200), (104, 8, 3, 100), (528, 0, 2, 1000)):
        idx = np.arange(3 * (K + 4)).reshape(3, K + 4)
        e = synth.turbo_ratematch(idx, E, rv, F)
        val = np.random.default_rng(E).standard_normal(E)
        want = np.zeros(3 * (K + 4))
        for i in range(E):
            want[e[i]] = want[e[i]] + val[i]
        assert np.array_equal(SR.derm(val, K, F, rv).reshape(-1), want)
        nulls = set(range(F)) | set(range(K + 4, K + 4 + F))
        assert not nulls & set(e.tolist())


def test_all_interleavers_are_permutations():
    synth = load_pkg().synth
    assert len(synth.TURBO_K) == 127 and synth.TURBO_K[0] == 40 and synth.TURBO_K[-1] == 2240
    for K in synth.TURBO_K:
        assert np.array_equal(np.sort(synth.turbo_interleaver(K)), np.arange(K)), K


def test_every_tbs_plus_24_is_a_block_size():
    pkg = load_pkg()
    for tpc in (0, 1):
        sizes = [pkg.capi.tbs_1a(m, tpc) for m in range(27)]
        assert sizes == sorted(sizes) and all(t + 24 in pkg.synth.TURBO_K for t in sizes)
        assert all(SR.block_size(t)[1] == 0 for t in sizes)


def test_crc24a_detects_and_is_linear():
    synth = load_pkg().synth
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 2, 100).astype(np.uint8), rng.integers(0, 2, 100).astype(np.uint8)
    assert np.array_equal(synth.crc24a(a) ^ synth.crc24a(b), synth.crc24a(a ^ b))
    assert SR.crc24a_int(np.concatenate([a, synth.crc24a(a)])) == 0
    one = np.zeros(1, np.uint8) + 1
    assert int("".join(map(str, synth.crc24a(one))), 2) == 0x864CFB


def test_reference_bits_are_the_pinned_ones():
    """the reference signals this file's receiver reads are the PCFICH's, which the measurement pins to the oracle; the scrambling bits
    it reads (synth._pn, pinned with the PBCH) are those the product's own path makes -- c_init, the jumps by 1600 and by 160 2^b
    clocks, the chunks -- over the largest allocation's 33600 bits and at the chunk boundaries"""
    pkg = load_pkg()
    for n_id, cp, n_rb in ((7, 1, 25), (503, 2, 6)):
        for slot in (0, 11):
            for sym in (0, 1, PR.n_symb_of(cp) - 3):
                assert np.array_equal(PR.rs_row(n_id, cp, n_rb, slot, sym), pkg.synth._crs_wide(n_id, slot, sym, cp == 1, n_rb))
    H = SC.load_twin(pkg.capi)
    for rnti, sf, n_id, n_bits in ((0xFFFF, 5, 141, 33600), (0xFFFE, 0, 0, 161), (60, 9, 503, 160 * 129), (1, 3, 7, 1)):
        c_init = H.pdsch_host_c_init(rnti, sf, n_id)
        assert c_init == rnti * 16384 + sf * 512 + n_id
        n_chunk = -(-n_bits // 160)
        words = np.zeros(5 * n_chunk, np.uint32)
        H.pdsch_host_scramble(c_init, n_chunk, SC._up(SC.jump_tables(25)), SC._up(words))
        bits = ((words[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).reshape(-1)[:n_bits]
        assert np.array_equal(bits, SR.scrambling(rnti, sf, n_id, n_bits)), (rnti, sf, n_id)


def test_elements_agree_with_the_generator():
    synth = load_pkg().synth
    for n_id, cp, ports, n_rb, sf, n_ctrl, s, n, tdd in ((7, 1, 2, 25, 0, 2, 0, 25, False), (68, 1, 4, 6, 5, 3, 1, 4, False), (0, 2, 1, 15, 0, 1, 5, 6, True),
                                                         (329, 1, 1, 15, 5, 3, 0, 15, True), (2, 2, 4, 6, 3, 4, 0, 6, False)):
        assert SR.elements(n_id, cp, ports, n_rb, sf, n_ctrl, s, n, tdd) == synth.pdsch_elements(n_id, n_rb, ports, cp == 1, sf, n_ctrl, s, n, tdd)


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_windowed_rule_decodes_what_the_full_block_decodes(case):
    """every block of every crafted case through the full-block decoder; it decodes at least every block that was sent at a code
    rate K / G of 3/4 or less (at 20 dB a QPSK element carries nearly two bits, and a rate-3/4 turbo code needs about 6 dB: the
    blocks the plan means to be decodable, at least four per case), and the windowed rule decodes all it decodes"""
    _, _, planted = SC.crafted(case)
    _, blocks = SC.reference(case)
    sent = {(p["g"], p["rnti"], p["rb_start"], p["n_prb"]) for p in planted if p["bits"] is not None and not p["silent"]}
    n = want = 0
    for b in blocks:
        if "d" not in b:
            continue
        full = SR.turbo_decode(b["d"], b["K"], b["F"], 8, win=b["K"])
        meant = (b["subframe"], b["rnti"], b["rb_start"], b["n_prb"]) in sent and 4 * b["K"] <= 3 * 2 * b["n_re"]
        want += meant
        if meant:
            assert full["status"] == 1, (SC.case_id(case), b["subframe"], b["K"])
        if full["status"] == 1:
            n += 1
            assert b["status"] == 1, (SC.case_id(case), b["subframe"], b["K"])
    print(SC.case_id(case), n, want)
    assert n >= want >= 4


def test_crafted_cases_have_no_block_near_a_tie():
    """the host and device comparisons excuse a block whose posterior comes within 1e-9 of zero: the cases are chosen to have none"""
    for case in SC.CASES:
        _, blocks = SC.reference(case)
        assert all(b["margin"] > 1e-9 for b in blocks), SC.case_id(case)


def test_crafted_cases_cover_the_plan():
    seen = set()
    for case in SC.CASES:
        _, _, planted = SC.crafted(case)
        _, blocks = SC.reference(case)
        by = {(b["subframe"], b["rnti"], b["rb_start"], b["n_prb"]): b for b in blocks}      # (a DCI sent at L = 8 is found at L = 4 first)
        for p in planted:
            b = by.get((p["g"], p["rnti"], p["rb_start"], p["n_prb"]))
            assert b is not None, (SC.case_id(case), p["g"])
            seen.add(b["status"])
            if p["bits"] is not None and not p["silent"] and 3 * (p["tbs"] + 28) <= 2 * b["n_re"]:
                assert b["status"] == 1 and np.array_equal(b["payload"], SR.payload_bytes(p["bits"], 0, p["tbs"])), (SC.case_id(case), p["g"], b["status"])
    assert {1, 2, 3, 4, 5, 6, 7} <= seen


def test_sib1_reader_reads_its_writer():
    pkg = load_pkg()
    for f in (SC.SIB1, dict(SC.SIB1, tdd=(2, 7), p_max=None, barred=True, plmns=[("310", "410", False)], csg=True, csg_id=12345, q_rx_lev_min_offset=3)):
        bits = pkg.synth.sib1_message(f)
        assert pkg.capi.sib1_fields(np.packbits(bits).tobytes()) == f and pkg.capi.sib1_fields(bits) == f
        assert pkg.capi.sib1_fields(bits[:40]) is None
    assert pkg.capi.sib1_fields(bytes([0x00] * 30)) is None          # c1: systemInformation, not SIB1
