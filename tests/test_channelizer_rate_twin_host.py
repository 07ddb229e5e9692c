"""The rational channelizer's tile arithmetic pinned on the CPU over its whole rate domain: every coprime up / down with
2 <= up < down <= 128 and down <= 16 up, 4696 pairs.  tests/host/chan_rate_host.cpp walks a workgroup of channelizer_rate.hip the way
the kernel does -- staging with the odd LDS stride, four waves, their tiles, the k-steps, one v_mfma_f32_32x32x2_f32 as a 64-lane
loop (lane l holds A[row l & 31][k l >> 5] and B[k l >> 5][col l & 31]; register v holds row (v & 3) + 8 (v >> 2) + 4 (l >> 5), column
l & 31; fp32, one fma per k), the guards, the phase rotation, the stores -- and takes every index from the __host__ __device__
helpers of channelizer.h that the kernels and the launcher call themselves.  Here that twin is compared with independent statements
of the contract: closed forms in integers (a), the float64 restatement tests/chan_rate_ref.py where fp32 is exact (b) and at the
project's standing bar where it rounds (c), and the rule for non-finite samples of include/lcs.h.  The GPU leg is
tests/test_gpu_channelizer_rate.py, at the corners of the domain.

What these tests catch was tried once, on two mutations of the shared helpers in a scratch copy of the tree (twin rebuilt, (a)
and (b) run, nothing of it committed):
  * s_q off by one for one residue (cr_sq returns ceil(q D / U) + 1 for q = 1): (a) FAILED at the first pair, 2/3, in the read
    offsets -- the tiles of residue 1 read one sample behind the closed form's -- and (b) FAILED at 2/3 on the first carrier, at
    the odd outputs (residue 1), the even ones equal;
  * the two A rows of a carrier swapped (cr_table_value: ri == 0 <-> ri != 0): (a) FAILED at 2/3 in the table comparison, from
    lane 0 of the first group on, and (b) FAILED at 2/3 on the first carrier at every output: re and im exchanged.
Both mutations are caught by (a) and by (b), each on its own."""
import numpy as np
import pytest

import chan_rate_ref as RR
import chan_rate_twin as T
import chan_ref as R
from conftest import load_pkg

RTOL = 1e-5          # fp32-class arrays against a double oracle: the project's standing bar (tests/test_gpu_channelizer_rate.py)
FS_OUT = 1.92e6
QUARTER = [0, 1 << 62, (1 << 64) - (1 << 62), 1 << 63]      # steps of the carriers at 0, fs_in / 4, -fs_in / 4, fs_in / 2
TURNS = [0, 1, 3, 2]                                        # ... as quarter turns per sample


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def test_the_domain_is_4696_pairs():
    assert len(T.PAIRS) == 4696 and len(set(T.PAIRS)) == 4696
    assert all(p in T.PAIRS for p in T.MARKETED) and all((u, d) in T.PAIRS for u, d, _ in T.CORNERS)


def _expected_table(U, D, G, taps, n_ch):
    """A in lane order from the contract: carrier k is the rows [g_re, -g_im] / [g_im, g_re] over kk = 2 j + c,
    g[j] = U taps[q D + Tg-1 - (s_q + j) U] exp(-i (pi / 2) turns_k j) where that tap exists, 0 where it does not"""
    Tg, n_rb = 16 * D, (n_ch + 15) // 16
    q, j = np.arange(U)[:, None], np.arange(4 * G)[None, :]
    t = q * D + Tg - 1 - (-(-q * D // U) + j) * U
    assert t.max() <= Tg - 1
    h = np.where(t >= 0, U * taps[np.maximum(t, 0)].astype(np.float64), 0.0)                   # [q][j]
    turns = np.array([TURNS[k % 4] for k in range(n_ch)] + [0] * (16 * n_rb - n_ch))[:, None]
    live = (np.arange(16 * n_rb) < n_ch)[:, None, None]
    qt = (turns * j) % 4                                                                       # [ch][j]
    g_re = live * h[None] * np.array([1.0, 0.0, -1.0, 0.0])[qt][:, None, :]                    # [ch][q][j]
    g_im = live * h[None] * np.array([0.0, -1.0, 0.0, 1.0])[qt][:, None, :]
    A = np.stack([np.stack([g_re, -g_im]), np.stack([g_im, g_re])])                            # [ri][c][ch][q][j]
    A = A.reshape(2, 2, n_rb, 16, U, G, 4).transpose(2, 4, 5, 1, 3, 0, 6)                      # [rb][q][s4][c][ch of rb][ri][i]
    return t, A.reshape(n_rb, U, G, 64, 4)


def test_geometry_invariants_over_the_whole_domain():
    """(a) pure integers, all 4696 pairs."""
    n_ch = 17
    by_ni, lds_max = {}, (0, None)
    for U, D in T.PAIRS:
        G, NI, xrows, lds = T.geometry(U, D)
        Tg, S = 16 * D, 2 * D + 1
        by_ni[NI] = by_ni.get(NI, 0) + 1
        lds_max = max(lds_max, (lds, (U, D)))
        assert 1 <= NI <= 4 and lds == 4 * xrows * S and lds <= T.CR_LDS_MAX, (U, D)
        assert 4 * (G - 1) < -(-Tg // U) <= 4 * G, (U, D)
        # the staging map: sample idx -> row idx / D, position idx % D, (re, im) side by side; never the pad float of a row
        st = T.stage_offsets(U, D)
        idx = np.arange(xrows * D)
        assert np.array_equal(st, (idx // D) * S + 2 * (idx % D)), (U, D)
        written = np.zeros(xrows * S, bool)
        written[st] = True
        written[st + 1] = True
        assert written.sum() == 2 * xrows * D and not written[2 * D::S].any(), (U, D)
        # every read: lane l at k-step j of tile t (residue t % U, column block t / U) reads component l >> 5 of the sample
        # (32 (t / U) + (l & 31)) D + s_q + j of the staged range -- a float the staging loop wrote
        got = T.read_offsets(U, D)
        tl = np.arange(U * NI)
        it, q = tl // U, tl % U
        sq = -(-q * D // U)
        n = ((32 * it)[:, None, None] + np.arange(32)[None, None, :]) * D + sq[:, None, None] + np.arange(4 * G)[None, :, None]
        assert n.max() < xrows * D, (U, D, int(n.max()), xrows * D)
        want = np.concatenate([st[n], st[n] + 1], axis=2)
        assert np.array_equal(got, want), (U, D, np.argwhere(got != want)[:4])
        assert got.min() >= 0 and got.max() < xrows * S and written[got].all(), (U, D)
        # the table: per residue the taps t = q D + Tg-1 - (s_q + j) U, 0 <= t < Tg, one slot each, zeros behind them; together the
        # residues hold every tap once
        taps = np.arange(1, Tg + 1, dtype=np.float32)
        st64 = np.array([QUARTER[k % 4] for k in range(n_ch)], np.uint64)
        t, want_tab = _expected_table(U, D, G, taps, n_ch)
        assert (t[:, 0] > Tg - 1 - U).all() and (np.diff(t, axis=1) == -U).all(), (U, D)
        assert np.array_equal(np.sort(t[t >= 0]), np.arange(Tg)), (U, D)
        got_tab = T.table(st64, taps, U, D)
        assert np.array_equal(got_tab, want_tab), (U, D, np.argwhere(got_tab != want_tab)[:4])
        assert np.count_nonzero(got_tab[0, :, :, 0, :]) == Tg, (U, D)      # lane 0: g_re of carrier 0 (shift 0)
        # the stores of a launch: one full workgroup, a second nearly empty one, a partial residue cycle; 16 carriers and one
        n_out = 32 * NI * U + U + 1
        cnt, outside = T.store_census(U, D, n_ch, n_out)
        assert outside == 0 and (cnt == 1).all(), (U, D, outside, np.argwhere(cnt != 1)[:4])
    # the census of the launcher's rule (derived from the launcher as it stood when these tests were written: a change of the rule
    # must re-derive them deliberately)
    assert [by_ni.get(k, 0) for k in (1, 2, 3, 4)] == [3563, 842, 156, 135], by_ni
    assert lds_max == (49140, (31, 94)), lds_max


def _raw_s8(rng, n_in):
    q = rng.integers(-127, 128, 2 * n_in).astype(np.int8)
    return q, (q[0::2].astype(np.float64) + 1j * q[1::2].astype(np.float64)) / 128.0


def test_twin_equals_the_contract_bit_for_bit_where_fp32_is_exact():
    """(b) all 4696 pairs.  Integer taps in [-8, 8], raw s8 samples k / 128, carriers at 0, fs_in / 4, -fs_in / 4, fs_in / 2: every tap
    phase and output phase is a multiple of a quarter turn, every product and partial sum an integer / 128 of magnitude at most
    U * 8 * 127 * ceil(16 D / U) <= 2 193 544 < 2^24: fp32 is exact in any order, and the twin must EQUAL the float64 restatement of
    x (-i)^n, x i^n, x (-1)^n at shift 0 (exact in float64 as well).  The quarter-turn carriers exercise the -g_im / g_im slots of A."""
    worst = max(U * 8 * 127 * -(-16 * D // U) for U, D in T.PAIRS)
    assert worst == 2193544 and worst < 2 ** 24
    rng = np.random.default_rng(4696)
    st = np.array(QUARTER, np.uint64)
    rot = np.array([[1, 1, 1, 1], [1, -1j, -1, 1j], [1, 1j, -1, -1j], [1, -1, 1, -1]])      # exp(-2 pi i df / fs_in n), n mod 4
    for U, D in T.PAIRS:
        NI = T.geometry(U, D)[1]
        n_out = 32 * NI * U + U + 1
        n_in = RR.n_in_min(n_out, U, D)
        fs_in = FS_OUT * D / U
        assert [T.step(f, fs_in) for f in (0.0, 0.25 * fs_in, -0.25 * fs_in, 0.5 * fs_in)] == QUARTER
        taps = rng.integers(-8, 9, 16 * D).astype(np.float64)
        q, x = _raw_s8(rng, n_in)
        got = T.run(q, "s8", n_in, U, D, st, taps, n_out)
        n4 = np.arange(n_in) % 4
        for k in range(4):
            want = RR.channelize_rate_ref(x * rot[k][n4], fs_in, U, D, [0.0], n_out, taps=taps)[0]
            assert np.array_equal(got[k].astype(np.complex128), want), (U, D, k, np.flatnonzero(got[k] != want)[:6])


def _subset():
    """the corner pairs, the six marketed rates and 200 seeded draws of the rest, each in all three formats"""
    named = [(u, d) for u, d, _ in T.CORNERS] + T.MARKETED
    rest = [p for p in T.PAIRS if p not in named]
    pick = np.random.default_rng(200).choice(len(rest), 200, replace=False)
    return [(u, d, f) for u, d in named + [rest[i] for i in sorted(pick)] for f in ("s8", "s16", "c64")]


def test_twin_meets_the_standing_bar_with_the_library_taps_on_noise(pkg):
    """(c) the library's own filter (lcs_channelizer_proto, as float like the launcher hands it over), noise and tones, the 17 carriers of
    the GPU tests: max|y - y_ref| / max|y_ref| per channel against the float64 restatement, at the GPU tests' bar."""
    cases = _subset()
    assert len(cases) == 3 * 216 and {f for _, _, f in cases} == {"s8", "s16", "c64"}
    worst = {}
    for U, D, fmt in cases:
        n_out = T.corner_n_out(U, D)
        n_in, fs_in = RR.n_in_min(n_out, U, D), FS_OUT * D / U
        shifts = T.shifts17(fs_in)
        q, xq = R.quantise(T.noise_and_tones(1000 * D + U + len(fmt), n_in, fs_in), fmt)
        ref = RR.channelize_rate_ref(xq, fs_in, U, D, shifts, n_out)
        y = T.run(q, fmt, n_in, U, D, T.steps(shifts, fs_in), pkg.channelizer_proto(D), n_out)
        ratios = [float(np.abs(y[k] - ref[k]).max() / np.abs(ref[k]).max()) for k in range(17)]
        worst[fmt] = max(worst.get(fmt, 0.0), max(ratios))
        assert max(ratios) <= RTOL, (U, D, fmt, ratios)
    print("rational channelizer, host twin, worst max|y - y_ref| / max|y_ref| per format:", {f: f"{v:.3e}" for f, v in worst.items()})


def test_a_non_finite_sample_spoils_its_padded_windows_only(pkg):
    """include/lcs.h, lcs_channelize_rational: outputs whose padded window [s, s + 4 G) does not hold the sample are finite and within
    the bar; outputs whose taps meet it are non-finite; the (at most 4) positions between are unconstrained."""
    x, n_in, fs_in, shifts, n_out, clean, dirty = T.nonfinite_case()
    with np.errstate(invalid="ignore", over="ignore"):
        ref = RR.channelize_rate_ref(x.astype(np.complex128), fs_in, 3, 4, shifts, n_out)
    assert np.isfinite(ref[:, ~dirty]).all()
    y = T.run(x, "c64", n_in, 3, 4, T.steps(shifts, fs_in), pkg.channelizer_proto(4), n_out)
    T.check_nonfinite(y, ref, clean, dirty, RTOL)
