"""The crafted peak-search cases (tests/peak_cases.py) on the CPU: the oracle (src/searcher.cpp:422-510 restated in C) and the
table's plain numpy model return the same records for every case, and every premise the GPU tests
(tests/test_gpu_peak_search_cases.py) rest on holds -- checked against the oracle alone, no GPU."""
import numpy as np
import pytest

import oracle as O
import peak_cases as P
from conftest import golden, iq_u8_to_capbuf

FS = 1.92e6


@pytest.fixture(scope="module")
def seed():
    """the seed buffer of the GPU tests: two combining windows of the recorded capture"""
    g = golden("capbuf_0000")
    cap, fc = iq_u8_to_capbuf(g["iq_u8"])[:19600], float(g["fc"][0])
    O.set_legacy(False)
    ro = O.xcorr_pss(cap, P.F_SET, P.DS, fc, fc, FS)
    assert ro["n_comb_xc"] == P.N_COMB
    ro["single"].setflags(write=False)
    return ro["single"], fc


def _run(case, single, fc):
    Z = P.z_of(case["sp"])
    pow64 = case["pow32"].astype(np.float64)
    trace = []
    m = P.model(pow64, case["frq"], Z, case["f"], single, P.DS, trace=trace)
    o = O.peak_search(pow64, case["frq"], Z, case["f"], fc, fc, single, P.DS)
    return m, [(c.n_id_2, c.ind, c.freq, c.pss_pow) for c in o], trace


def test_case_table_is_complete():
    assert tuple(c["name"] for c in P.cases()) == P.NAMES
    for c in P.cases():
        assert c["pow32"].shape == (3, P.N) and c["pow32"].dtype == np.float32 and (c["pow32"] >= 0).all()
        assert c["frq"].shape == (3, P.N) and c["frq"].min() >= 0 and c["frq"].max() < P.N_F
        assert c["sp"].shape == (P.N,) and (c["sp"] > 0).all() and c["f"].size == P.N_F


@pytest.mark.parametrize("name", P.NAMES)
def test_oracle_equals_model_and_premises_hold(seed, name):
    single, fc = seed
    case = P.case(name)
    m, o, trace = _run(case, single, fc)
    assert o == m                                        # record by record, every field equal
    assert len(o) <= 102                                 # LCS_MAX_PEAKS = 104 is never reached
    pos = [(r, c) for r, c, _, _, passed in trace if passed]
    assert len(pos) == len(o) and len(trace) == len(o) + 1 and not trace[-1][4]
    # what the case was built to show
    if "n_peaks" in case:
        assert len(o) == case["n_peaks"]
    if "positions" in case:
        assert pos == [tuple(rc) for rc in case["positions"]]
    for rc in case.get("vanish", ()):
        assert rc not in pos and case["pow32"][rc] > 0
    # no global maximum of any iteration within Z_MARGIN of its column's threshold
    worst = min(abs(p - z) / z for _, _, p, z, _ in trace)
    assert worst >= P.Z_MARGIN, f"{name}: a maximum lies {worst:.3e} (relative) from its Z_th1, margin {P.Z_MARGIN:.0e}"
    if case.get("exact_margin"):                         # the planted margin, rounded away from Z to the next float32
        assert worst <= P.Z_MARGIN + 2.0 ** -23, worst
        assert any(passed and (p - z) / z <= P.Z_MARGIN + 2.0 ** -23 for _, _, p, z, passed in trace)
        assert (trace[-1][3] - trace[-1][2]) / trace[-1][3] <= P.Z_MARGIN + 2.0 ** -23
    # the middle share (hypotheses 2..4) sees peaks on both sides of both of its edges
    if len(o) >= 5:
        fi = {int(case["frq"][rc]) for rc in pos}
        assert fi & {0, 1} and fi & {2, 3, 4} and fi & {5, 6}, (name, sorted(fi))
        assert any(2 <= int(case["frq"][rc]) <= 4 and rec[1] >= 0 for rc, rec in zip(pos, o)), name      # ... and refines one of its own


def test_refinement_margin_in_the_seed(seed):
    """At every peak of every case the best two of the refinement's candidates in the oracle's xc_incoherent_single differ by more
    than REFINE_MARGIN: the GPU's values are within 1e-5 of the oracle's (the standing bar), so the refined index cannot flip."""
    single, fc = seed
    worst, where, n = np.inf, None, 0
    for case in P.cases():
        _, _, trace = _run(case, single, fc)
        for r, c, _, _, passed in trace:
            cand = P.refine_candidates(c)
            if not passed or not cand:
                continue
            v = np.sort(single[r, cand, int(case["frq"][r, c])].astype(np.float64))[::-1]
            n += 1
            if (v[0] - v[1]) / v[0] < worst:
                worst, where = (v[0] - v[1]) / v[0], (case["name"], r, c)
    assert n > 500
    assert worst > P.REFINE_MARGIN, f"worst margin of the best two candidates {worst:.3e} at {where} (over {n} peaks), needed {P.REFINE_MARGIN:.0e}"
    print(f"refinement: worst relative margin of the best two candidates {worst:.3e} at {where}, {n} peaks")


def test_z_margin_is_100_times_the_bound_on_chi2cdf_inv():
    """tests/test_tables_abi.py: the library's chi2cdf_inv is within 1e-9 k of the oracle's."""
    k = 2 * P.N_COMB * (2 * P.DS + 1)
    r = O.chi2cdf_inv(1 - 1e-12, k)
    assert P.Z_MARGIN >= 100 * (1e-9 * k / r), (r, k)


def test_floor_pairs_stay_on_their_sides():
    for p in P.FLOOR_PEAKS:
        lo, hi = P.floor_pair(np.float32(p))
        assert lo.dtype == np.float32 and hi.dtype == np.float32 and np.nextafter(lo, np.float32(1)) == hi
        for t in (np.nextafter(P.FLOOR, 0), P.FLOOR, np.nextafter(P.FLOOR, 1)):
            assert float(lo) < float(np.float32(p)) * t <= float(hi)


def test_no_float32_peak_has_a_representable_floor():
    """`< thresh` against `<= thresh` can only differ where p * 10^-1.2, rounded to double, is a float32: over every float32
    mantissa (powers of two scale exactly in the normal range) and the three doubles a pow() may return, there is no such p -- so
    the floor cases hold no exact pair."""
    m = np.arange(2 ** 23, 2 ** 24, dtype=np.float64)
    for t in (np.nextafter(P.FLOOR, 0), P.FLOOR, np.nextafter(P.FLOOR, 1)):
        prod = m * t
        assert not (prod.astype(np.float32).astype(np.float64) == prod).any()


def test_pack_is_the_word_layout():
    """(float bits << 32) | (0xFFFFFFFF - frq): non-negative words ordered like (pow, -frq)"""
    c = P.case("random_0")
    words, meta = P.pack(c["pow32"], c["frq"], c["sp"])
    assert words.dtype == np.int64 and words.shape == (3 * P.N,) and (words >= 0).all()
    assert np.array_equal((words >> 32).astype(np.uint32).view(np.float32).reshape(3, P.N), c["pow32"])
    assert np.array_equal(0xFFFFFFFF - (words & 0xFFFFFFFF), c["frq"].reshape(-1))
    assert meta.shape == (P.N + 1,) and meta[-1] == P.N_COMB and np.array_equal(meta[:-1], c["sp"])
    a, b = P.pack(np.float32([1.5, 1.5, 2.0]), np.int32([3, 4, 0]), c["sp"])[0], None
    assert a[0] > a[1] and a[2] > a[0]


@pytest.mark.parametrize("ds", [0, 1, 2, 3])
def test_model_equals_oracle_on_crafted_single_every_arm(ds):
    """the stage kernel's run: an eight-level xc_incoherent_single (exact ties inside the window: the first wins) and every
    ds_comb_arm of 0..3, whose wrap quirk the cells at columns 0..3 and 9596..9599 of these cases meet"""
    single = P.crafted_single()
    cols = set()
    for name in ("dense", "dense_low", "edges", "ties", "cancel_274", "random_3"):
        case = P.case(name)
        Z = P.z_of(case["sp"])
        pow64 = case["pow32"].astype(np.float64)
        trace = []
        m = P.model(pow64, case["frq"], Z, case["f"], single, ds, trace=trace)
        o = O.peak_search(pow64, case["frq"], Z, case["f"], 1e9, 1e9, single, ds)
        assert [(c.n_id_2, c.ind, c.freq, c.pss_pow) for c in o] == m
        cols |= {c for _, c, _, _, passed in trace if passed}
        for (r, c, _, _, passed), rec in zip(trace, m):
            assert (rec[1] == -1) == (c < ds)
    assert cols >= {0, 1, 2, 3, 9596, 9597, 9598, 9599}
