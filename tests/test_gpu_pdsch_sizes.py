"""GPU tests of the PDSCH stage at the sizes tests/test_gpu_pdsch.py does not reach (k_pdsch_llr, k_pdsch_dec; the inputs and what they
are for: tests/pdsch_cases.py, settled on the CPU by tests/test_pdsch_sizes_host.py).

lcs_turbo_decode at all 127 block sizes, with and without fillers, against the host twin: every number of lanes, every length of the
last window, the wave's boundary from both sides (K = 2048 against 2112), blocks that run out of iterations.  The stage with forced
grants at K = 2048 .. 2240 and with up to 63 fillers on a 25 resource block grid: the device's de-rate-matching over rank tables of
those sizes, punctured and wrapped, at every rv.  The stage on grids of 100, 75 and 50 resource blocks: k_pdsch_llr beyond 25 resource
blocks, the scrambling sequence's jump for bit 7 of the chunk number and the jump table the product builds for it."""
import collections
import json

import numpy as np
import pytest

import pdcch_cases as DC
import pdsch_cases as SC
import test_gpu_pdsch as TG
from conftest import load_pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def S(pkg):
    s = pkg.Searcher(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def H(pkg):
    return SC.load_twin(pkg.capi)


def worst_soft_bit(S, blocks):
    """the largest difference between the last call's soft bits and numpy's, relative to the block's largest"""
    worst, per_sf = 0.0, {}
    for b in blocks:
        u = per_sf.get(b["subframe"], 0)
        per_sf[b["subframe"]] = u + 1
        if "llr" in b:
            llr = S.pdsch_last_soft(b["subframe"], u, len(b["llr"]))
            worst = max(worst, np.abs(llr - b["llr"]).max() / max(np.abs(b["llr"]).max(), 1e-300))
    return worst


def test_turbo_decode_every_size(S):
    """decisions, iterations and outcome equal the twin's at every size (the kernel is bit-equal to it and numpy's posteriors stay
    4e-6 clear of zero: nothing is excused); a decoded block is the encoded one; decodes of three iterations and more, in which the
    metrics traded between windows and between the two waves decide the result, are seen in every class of K mod 32 and at the three
    sizes of the second wave"""
    blocks, twin = SC.size_blocks(), SC.size_blocks_twin()
    hist, slow, sizes = collections.Counter(), set(), set()
    for b, (tb, tn, ts) in zip(blocks, twin):
        bits, n_iter, ok = S.turbo_decode(b["d"], b["K"], b["F"], b["max_iter"])
        assert (n_iter, ok) == (tn, ts == 1) and np.array_equal(bits, tb), (b["K"], b["F"], b["sigma"], b["max_iter"], n_iter, ok, tn, ts, int((bits != tb).sum()))
        if ok:
            assert np.array_equal(bits, b["c"]), (b["K"], b["F"])
        hist[n_iter] += 1
        sizes.add(b["K"])
        if ok and n_iter >= 3:
            slow.add(b["K"])
    assert len(sizes) == 127 and len(blocks) == 271
    assert {K % 32 for K in slow} == {0, 8, 16, 24} and slow >= {2112, 2176, 2240}, sorted(slow)
    print("pdsch_sizes", json.dumps(dict(test="turbo_decode_every_size", blocks=len(blocks), iterations=dict(sorted(hist.items())), sizes_with_three_and_more=len(slow))))


def test_forced_grants_at_the_large_sizes(pkg, S, H):
    """SC.LARGE_PLAN in two calls of four forced grants: the record byte-equal to the twin's, every field numpy's, the soft bits to
    1e-9 of the block's largest, every planted block back with its bytes"""
    case, tfg, calls, planted = SC.large_forced()
    n_rb = case[3]
    cell, cfg = TG._case_cell(pkg, case), DC.make_cfg(pkg.capi, SC.pdcch_case(case))
    worst, iters = 0.0, []
    for call in (0, 1):
        ps = SC.make_cfg(pkg.capi, forced=calls[call])
        got, pdc = S.pdsch(cell, tfg, n_rb, 0x3FF, cfg, ps, want_pdcch=True)
        twin = SC.twin_record(H, pkg.capi, case, tfg, pdc, cfg=ps)
        assert bytes(got) == bytes(twin), (call, [(b["K"], b["F"], b["n_iter"], b["status"]) for b in got.blocks()], [(b["n_iter"], b["status"]) for b in twin.blocks()])
        blocks = SC.large_forced_reference(call)
        assert SC.assert_blocks_against_numpy(got, blocks, "call %d" % call) == (4, 0)
        rel = worst_soft_bit(S, blocks)
        print("call", call, "worst soft bit %.2e" % rel)
        assert rel <= 1e-9, (call, rel)
        worst = max(worst, rel)
        by = {(g[0], g[2]): bits for g, bits in zip(calls[call], planted[call])}
        for b in got.blocks():
            assert b["crc_ok"] and b["bytes"] == np.packbits(by[(b["subframe"], b["rb_start"])]).tobytes(), (b["subframe"], b["K"], b["F"], b["status"], b["n_iter"])
        assert {(b["K"], b["F"], b["rv"]) for b in got.blocks()} == {p[4:7] for p in SC.LARGE_PLAN if p[0] == call}
        iters += [b["n_iter"] for b in got.blocks()]
    assert max(iters) >= 2
    print("pdsch_sizes", json.dumps(dict(test="forced_grants_at_the_large_sizes", iterations=dict(sorted(collections.Counter(iters).items())), worst_soft_bit=worst)))


@pytest.mark.parametrize("case", SC.WIDE_CASES, ids=SC.case_id)
def test_stage_on_wide_grids(pkg, S, H, case):
    """tests/test_gpu_pdsch.py's test on the crafted grids, on those of 100, 75 and 50 resource blocks"""
    TG.test_stage_against_numpy_and_the_host_twin_on_crafted_grids(pkg, S, H, case)
    _, blocks = SC.reference(case)                  # (the record's fields are these: asserted above)
    worst = worst_soft_bit(S, blocks)
    assert worst <= 1e-9
    print("pdsch_sizes", json.dumps(dict(test="stage_on_wide_grids", case=SC.case_id(case), iterations=dict(sorted(collections.Counter(b["n_iter"] for b in blocks).items())),
                                         largest_G=max(2 * b["n_re"] for b in blocks), worst_soft_bit=worst)))
