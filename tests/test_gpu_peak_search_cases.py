"""The fused chain's peak search (k_peak_search_reg: the 3 x 9600 working copy in registers) on crafted arrays.

Every product path runs that kernel on the output of a real correlation only: a handful of peaks, no two equal floats.  Here the
cases of tests/peak_cases.py are put in front of it through the split entry points: lcs_foe_partial on a short seed buffer leaves
the packed (pow, frq) words and the meta vector in the caller's tensors, the test overwrites both with a case's arrays, and
lcs_foe_finish (k_foe_unpack -> k_peak_search_reg) returns the peak list, which must EQUAL the oracle's -- under three shares of
the hypotheses, because the refinement of `ind` reads this rank's slice of xc_incoherent_single (the seed's) by local index.
The premises (no maximum within 1e-6 of its threshold, refinement candidates 1e-4 apart in the seed) are checked on the CPU by
tests/test_peak_cases_host.py; nothing here is compared with a tolerance."""

import numpy as np
import pytest

import oracle as O
import peak_cases as P
from conftest import golden, iq_u8_to_capbuf, load_pkg

pytestmark = pytest.mark.gpu
FS = 1.92e6


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def S(pkg):
    s = pkg.Searcher(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def seed():
    """two combining windows of the recorded dongle capture (int8 kernel) and the oracle's xc_incoherent_single of them"""
    g = golden("capbuf_0000")
    cap, fc = iq_u8_to_capbuf(g["iq_u8"])[:19600], float(g["fc"][0])
    O.set_legacy(False)
    ro = O.xcorr_pss(cap, P.F_SET, P.DS, fc, fc, FS)
    assert ro["n_comb_xc"] == P.N_COMB
    return cap, fc, ro["single"]


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch.empty(3 * P.N, dtype=torch.int64, device="cuda"), torch.empty(P.N + 1, dtype=torch.float64, device="cuda")


def _inject(S, dev, seed, share, pow32, frq, sp):
    """lcs_foe_partial on the seed, the case's arrays over what it left, lcs_foe_finish -> the peak list"""
    import torch
    words, meta = dev
    cap, fc, _ = seed
    S.foe_partial(cap, P.F_SET, share[0], share[1], fc, fc, FS, words.data_ptr(), meta.data_ptr())
    assert S.last_xcorr_info()[0] == "k_xcorr_i8x3"
    w, m = P.pack(pow32, frq, sp)
    words.copy_(torch.from_numpy(w))
    meta.copy_(torch.from_numpy(m))
    torch.cuda.synchronize()
    return S.foe_finish(words.data_ptr(), meta.data_ptr(), P.F_SET)[2]


_expected_cache = {}


def _expected(case, seed):
    """the oracle's list on the seed's xc_incoherent_single, with each peak's (row, column) and hypothesis index"""
    if case["name"] not in _expected_cache:
        _, fc, single = seed
        Z = P.z_of(case["sp"])
        pow64 = case["pow32"].astype(np.float64)
        o = O.peak_search(pow64, case["frq"], Z, case["f"], fc, fc, single, P.DS)
        trace = []
        P.model(pow64, case["frq"], Z, case["f"], single, P.DS, trace=trace)
        pos = [(r, c) for r, c, _, _, passed in trace if passed]
        assert len(pos) == len(o)
        _expected_cache[case["name"]] = [(c.n_id_2, c.ind, c.freq, c.pss_pow, rc, int(case["frq"][rc])) for c, rc in zip(o, pos)]
    return _expected_cache[case["name"]]


def _check(peaks, case, seed, share):
    exp = _expected(case, seed)
    fc = seed[1]
    first, count = share
    got = [(p.n_id_2, p.ind, p.freq, p.pss_pow, p.reserved) for p in peaks]
    want = []
    for n_id_2, ind, freq, pss_pow, rc, fi in exp:
        mine = first <= fi < first + count
        assert rc[0] == n_id_2 and pss_pow == float(case["pow32"][rc]) and freq == P.F_SET[fi]
        want.append((n_id_2, ind if mine else -1, freq, float(case["pow32"][rc]), 0 if mine else 1))
    assert got == want, f"{case['name']} share {share}: {len(got)} peaks, expected {len(want)}; first difference at " \
                        f"{next((k for k, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))}"
    assert all(p.fc_requested == fc and p.fc_programmed == fc and p.n_id_1 == -1 for p in peaks)


@pytest.mark.parametrize("share", P.SHARES, ids=["owns_nothing", "owns_everything", "owns_the_middle"])
@pytest.mark.parametrize("name", P.NAMES)
def test_fused_peak_search_equals_oracle(S, dev, seed, name, share):
    case = P.case(name)
    peaks = _inject(S, dev, seed, share, case["pow32"], case["frq"], case["sp"])
    _check(peaks, case, seed, share)
    if share[1] == 0:
        assert all(p.ind == -1 and p.reserved == 1 for p in peaks)
    if share[1] == P.N_F:
        assert all(p.reserved == 0 for p in peaks)


def test_middle_share_meets_both_kinds_of_peak(seed):
    """(the table's premise, on the lists the test above compares: owned and foreign peaks, refined ones among the owned)"""
    for name in ("dense", "dense_low", "plateau", "ties") + tuple(f"cancel_{c}" for c in P.CANCEL_COLS):
        exp = _expected(P.case(name), seed)
        assert any(2 <= e[5] <= 4 and e[1] >= 0 for e in exp) and any(e[5] < 2 for e in exp) and any(e[5] > 4 for e in exp), name


@pytest.mark.parametrize("ds", [0, 1, 2, 3])
def test_stage_kernel_on_the_same_table(S, ds):
    """k_peak_search (lcs_peak_search) on every case, with a crafted xc_incoherent_single of eight levels -- exact ties inside the
    refinement's window, the first wins -- and every ds_comb_arm: cells at columns 0..3 and 9596..9599 meet the uint16 wrap quirk
    (ind = -1 where column < ds_comb_arm) and the wrap past 9599."""
    single = P.crafted_single()
    key = lambda cells: [(c.n_id_2, c.ind, c.freq, c.pss_pow) for c in cells]
    for case in P.cases():
        Z = P.z_of(case["sp"])
        pow64 = case["pow32"].astype(np.float64)
        got = S.peak_search(pow64, case["frq"], Z, case["f"], 1e9, 1e9, single, ds)
        exp = O.peak_search(pow64, case["frq"], Z, case["f"], 1e9, 1e9, single, ds)
        assert key(got) == key(exp), (case["name"], ds)


def test_bounded_loop_reports_overflow_and_the_context_goes_on(S, pkg, dev, seed):
    """Z_th1 = 0 everywhere over an all-zero array: the reference's loop never ends; the device's is bounded and lcs_foe_finish
    returns LCS_ERR_OVERFLOW (include/lcs.h).  The next case on the same context gives its normal answer."""
    zero = np.zeros((3, P.N), np.float32)
    with pytest.raises(pkg.SearcherError, match="LCS_ERR_OVERFLOW"):
        _inject(S, dev, seed, (0, P.N_F), zero, np.zeros((3, P.N), np.int32), np.zeros(P.N))
    case = P.case("dense")
    _check(_inject(S, dev, seed, (0, P.N_F), case["pow32"], case["frq"], case["sp"]), case, seed, (0, P.N_F))


def test_finish_without_partial_is_refused(S, pkg, dev, seed):
    words, meta = dev
    case = P.case("ties")
    _inject(S, dev, seed, (2, 3), case["pow32"], case["frq"], case["sp"])
    with pytest.raises(pkg.SearcherError, match="lcs_foe_finish needs the lcs_foe_partial call of the same buffer first"):
        S.foe_finish(words.data_ptr(), meta.data_ptr(), P.F_SET)          # the pending result was used up
    _check(_inject(S, dev, seed, (2, 3), case["pow32"], case["frq"], case["sp"]), case, seed, (2, 3))
