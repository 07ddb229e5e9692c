"""GPU test of the PBCH soft path between the channel estimate and the Viterbi decoder (lcs_pbch_soft: k_chan_est in the
PBCH-rows-only form that decode_mib uses, then pbch_llr_wave and pbch_decode_wave for one forced candidate) against the oracle's
orc_pbch_soft, on every case of tests/pbch_cases.py and all twelve candidates -- the mismatched ones too: their soft values are as
deterministic as the right one's.

Per element that is no edge (pbch_ref: an exponent argument within 1e-6 of the point where e^{-x} rounds to zero):
|e_est - oracle| and |d_est - oracle| within pbch_ref's allowance, 1e-9 (|l| + median |e_est|) plus two units in the last place of
every subnormal likelihood sum seen through the logarithm; LLRs whose four likelihoods all underflow are exactly 0.0; the decoded
bits and the CRC flag equal the oracle's; decode_mib's record equals the oracle's in every integer field.  The allowance comes from
the reference alone (tests/test_pbch_ref.py asserts the regime counts and the edge cap without a GPU).

Observed |difference| / allowance on an MI355X, the worst over all cases per regime: LINEAR 2.4e-5, EXACT 9.8e-6, SUBNORMAL 6.6e-4,
CLIPPED 2.0e-5, ZERO 0 (exactly equal), d_est 5.2e-5; no element is an edge."""
import numpy as np
import pytest

import pbch_cases as PC
import pbch_ref as PB
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


def lcs_cell(pkg, cell):
    """the oracle's record as the product's (the same layout: tests/test_tables_abi.py)"""
    return pkg.LcsCell.from_buffer_copy(bytes(cell))


WORST = {}


@pytest.mark.parametrize("name", PC.NAMES)
def test_soft_values_of_every_candidate_against_the_oracle(pkg, S, name):
    cell, tfg = PC.grid(name)
    oe, od, oc, ook, orec = PC.oracle_soft(name)
    c = lcs_cell(pkg, cell)
    worst = {}
    for k, (g, p) in enumerate(PB.CANDIDATES):
        e, d, bits, ok = S.pbch_soft(c, tfg, g, p)
        assert e.shape == oe[k].shape
        if name not in PC.INTEGERS_ONLY:
            w = PC.compare(e, d, name, k)
            for a, b in w["worst"].items():
                worst[a] = max(worst.get(a, 0.0), b)
        assert np.array_equal(bits, oc[k]), (name, g, p, bits, oc[k])
        assert ok == bool(ook[k]), (name, g, p)
    print(name, {a: f"{b:.2g}" for a, b in worst.items()})
    for a, b in worst.items():
        WORST[a] = max(WORST.get(a, 0.0), b)
    got = S.decode_mib(c, tfg)
    assert PC.cell_fields(got) == PC.cell_fields(orec), (name, got, orec)
    assert got.ind == orec.ind
    if name in ("noise-free", "pbch-rows-zero"):      # several candidates pass: the first in the reference's order wins
        assert ook.sum() > 1 and (got.n_ports, got.n_rb_dl, got.sfn) == (1, 6, 0)


def test_worst_ratio_per_regime_is_reported():
    print("worst |difference| / allowance per regime:", {a: f"{b:.3g}" for a, b in WORST.items()})
    assert all(b <= 1.0 for b in WORST.values())


def test_refusals(pkg, S):
    cell, tfg = PC.grid("id7-cp1-tx2-g3")
    c = lcs_cell(pkg, cell)
    S.pbch_soft(c, tfg, 3, 4)
    for g, p in ((-1, 1), (4, 1)):                       # a frame_timing_guess outside 0 .. 3
        with pytest.raises(pkg.SearcherError):
            S.pbch_soft(c, tfg, g, p)
    for p in (0, 3, 8):                                  # n_ports outside {1, 2, 4}
        with pytest.raises(pkg.SearcherError):
            S.pbch_soft(c, tfg, 0, p)
    with pytest.raises(pkg.SearcherError):               # what decode_mib refuses: not the cell's full grid ...
        S.pbch_soft(c, tfg[:-1], 0, 1)
    with pytest.raises(pkg.SearcherError):
        S.decode_mib(c, tfg[:-1])
    for field, value in (("cp_type", 0), ("n_id_1", -1), ("n_id_2", -1)):      # ... an unknown CP type, no identity
        bad = lcs_cell(pkg, cell)
        setattr(bad, field, value)
        with pytest.raises(pkg.SearcherError):
            S.pbch_soft(bad, tfg, 0, 1)
        with pytest.raises(pkg.SearcherError):
            S.decode_mib(bad, tfg)
    # the context is as usable as before
    assert PC.cell_fields(S.decode_mib(c, tfg)) == PC.cell_fields(PC.oracle_soft("id7-cp1-tx2-g3")[4])
