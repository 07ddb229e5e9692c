"""Near-ties of the frequency arg-max, by the hundred.

xc_incoherent_collapsed_frq is an integer output of the reference and must be EQUAL, on top of correlation kernels that are ~1e-6
accurate: positions whose best two hypotheses lie within lcs_frq_tie_eps() are listed by k_collapse* and recomputed in the
reference's arithmetic by k_frq_repair.  The suite's ordinary inputs hold next to no near-ties (0-3 positions of
28 800 per buffer on the 5 kHz grids), so "0 differing indices" there says little about the repair.  A dense frequency raster -- 31
hypotheses 100 Hz or 50 Hz apart -- makes adjacent hypotheses almost equal around every maximum: hundreds of genuine, non-duplicate
near-ties per buffer, a few exact ties and three-way ties among them, far below the bound on the repair's work.

Per case: (v) the ORACLE's output holds the near-ties (checked first: an input that lost them fails instead of passing vacuously);
(i) every index equals the oracle's; (ii) at every position the oracle shows within eps / 4 the collapsed power is the oracle's
float bit for bit (the repair rewrites it); (iii) the library listed at least as many positions as the oracle shows within eps / 4
(the factor 4 leaves room for the GPU's own value error of up to eps / 2 on either value); (iv) no listed position was left
unrepaired.  With the listing switched off (LCS_FRQ_TIE_EPS = 0 in a scratch build) these inputs give 6-7 differing indices per correlation
kernel (0 for k_single_exact), all at oracle margins <= 2.5e-7: the assertions (i) and (iii) fail."""
import os

import numpy as np
import pytest

import oracle as O
from conftest import golden, iq_u8_to_capbuf, load_pkg
from test_gpu_pss import _check_frq, _check_tie_premise

pytestmark = pytest.mark.gpu
FS = 1.92e6
N_CAP = 153600
STEPS = (100.0, 50.0)
NAMES = ("capbuf_0000", "noise", "planted")


def raster(step):
    return (np.arange(31) - 15) * step + 35e3


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def S(pkg):
    s = pkg.Searcher(0)
    yield s
    s.close()


@pytest.fixture(scope="module", autouse=True)
def _threads():
    O.set_legacy(False)
    O.set_threads(min(16, os.cpu_count() or 1))


def make_buffers(pkg):
    """The recorded capture, the seeded noise buffer of test_gpu_pss.py, and a synthetic buffer with three planted cells (near-ties
    at or above Z_th1 -- where a wrong index would become a wrong peak -- are counted per raster; the recorded capture has them too)."""
    g = golden("capbuf_0000")
    fc = float(g["fc"][0])
    noise = np.clip(np.rint(np.random.default_rng(17).normal(127.0, 14.0, g["iq_u8"].size)), 0, 255).astype(np.uint8)
    planted, _ = pkg.synth.make_capbuf(1717, fc, [dict(n_id_1=12, n_id_2=0, f_off=35.02e3), dict(n_id_1=150, n_id_2=2, f_off=34.1e3, gain_db=-5),
                                                  dict(n_id_1=77, n_id_2=1, f_off=36.33e3, gain_db=-9, cp_normal=False)], 4.0)
    return fc, [g["iq_u8"], noise, planted]


def tie_stats(ro, eps):
    """From the oracle's arrays alone: the relative margin between the best two hypotheses of every position, and the counts."""
    inc = np.sort(ro["incoherent"].astype(np.float64), axis=2)
    a, b, c = inc[..., -1], inc[..., -2], inc[..., -3]
    m = (a - b) / a
    return dict(margin=m, lt_1e6=int((m < 1e-6).sum()), lt_2e6=int((m < 2e-6).sum()), lt_4e6=int((m < 4e-6).sum()), exact=int((m == 0).sum()),
                three=int(((a - c) / a < 4e-6).sum()), quarter=m < eps / 4, above_z=int(((m < eps) & (ro["pow"] >= O.z_th1(ro["sp_incoherent"], ro["n_comb_xc"])[None, :])).sum()))


@pytest.fixture(scope="module")
def cases(pkg):
    """{step: (f, fc, [u8 buffers], [oracle outputs], [tie statistics])} with the precondition (v) asserted on the oracle's output."""
    eps = pkg.frq_tie_eps()
    fc, bufs = make_buffers(pkg)
    out = {}
    for step in STEPS:
        f = raster(step)
        ros = [O.xcorr_pss(iq_u8_to_capbuf(b), f, 2, fc, fc, FS) for b in bufs]
        sts = [tie_stats(ro, eps) for ro in ros]
        for name, st in zip(NAMES, sts):
            print(f"[oracle] {name} step {step:.0f} Hz: margin < 1e-6: {st['lt_1e6']}, < 2e-6: {st['lt_2e6']}, < 4e-6: {st['lt_4e6']}, exact ties {st['exact']}, "
                  f"three within 4e-6: {st['three']}, within eps/4: {int(st['quarter'].sum())}, near-ties at or above Z_th1: {st['above_z']}")
            assert st["lt_2e6"] >= 30, (name, step, st["lt_2e6"])
        assert sum(st["three"] + st["exact"] for st in sts) >= 1, step
        assert sum(st["above_z"] for st in sts) >= 1, "some near-tie must sit where a peak can come from"
        out[step] = (f, fc, bufs, ros, sts)
    return out


def _assert_case(r_pow, r_frq, ro, st, listed, left, tag, pow_scale=1.0):
    _check_frq(r_frq, ro, tag)                                                       # (i)
    q = st["quarter"]
    same = (r_pow * pow_scale)[q] == ro["pow"][q]                                    # (ii) (a power-of-two scale is exact)
    assert same.all(), f"{tag}: collapsed power differs from the oracle's float at {int((~same).sum())} of {int(q.sum())} repaired positions"
    assert listed >= int(q.sum()), f"{tag}: {listed} positions listed, the oracle shows {int(q.sum())} within eps/4"      # (iii)
    assert left == 0, f"{tag}: {left} of {listed} listed positions left unrepaired"   # (iv)
    print(f"[ties] {tag}: listed {listed} (oracle within eps/4: {int(q.sum())}, within 4e-6: {st['lt_4e6']}), unrepaired {left}")


@pytest.mark.parametrize("step", STEPS)
def test_dense_raster_batches_as_bytes_and_as_floats(S, pkg, cases, step):
    import torch
    f, fc, bufs, ros, sts = cases[step]
    fcs = np.full(len(bufs), fc)
    d8 = torch.from_numpy(np.ascontiguousarray(np.stack(bufs))).cuda()
    d32 = torch.from_numpy(np.stack([iq_u8_to_capbuf(b).astype(np.complex64) for b in bufs])).cuda()
    for fmt, dptr, kernel in ((pkg.FMT_IQ_U8, d8.data_ptr(), "k_xcorr_i8x3"), (pkg.FMT_C64, d32.data_ptr(), "k_xcorr_f16x3")):
        S.search_batch(dptr, fmt, len(bufs), N_CAP, f, fcs, fcs, FS, pkg.STAGE_PSS, max_cells_per_buf=64)
        assert S.last_xcorr_info()[0] == kernel
        listed, left = S.last_frq_repair_stats()
        assert listed >= sum(int(st["quarter"].sum()) for st in sts), (listed, kernel)      # (iii) for the batch as a whole
        for b, name in enumerate(NAMES):
            r = S.batch_readback(b, f.size)
            tag = f"{name} step {step:.0f} Hz [{kernel}]"
            err = np.abs(r["single"].astype(np.float64) - ros[b]["single"]) / ros[b]["single"]
            _check_tie_premise(S, {"single": err.max()}, tag)
            _assert_case(r["pow"], r["frq"], ros[b], sts[b], listed, left, tag)


@pytest.mark.parametrize("step", STEPS)
def test_dense_raster_host_calls_int8_and_fp32(S, pkg, cases, step):
    f, fc, bufs, ros, sts = cases[step]
    for b, name in enumerate(NAMES):
        cap = iq_u8_to_capbuf(bufs[b])
        for scale, kernel in ((1.0, "k_xcorr_i8x3"), (0.5, "k_xcorr_mfma_blk")):
            r = S.xcorr_pss(scale * cap, f, 2, fc, fc, FS)
            assert S.last_xcorr_info()[0].startswith(kernel), S.last_xcorr_info()
            tag = f"{name} step {step:.0f} Hz host x {scale} [{S.last_xcorr_info()[0]}]"
            k = 1.0 / (scale * scale)
            errs = {a: (np.abs(k * r[a].astype(np.float64) - ros[b][a]) / ros[b][a]).max() for a in ("single", "incoherent")}
            _check_tie_premise(S, errs, tag)
            listed, left = S.last_frq_repair_stats()
            _assert_case(r["pow"], r["frq"], ros[b], sts[b], listed, left, tag, pow_scale=k)


def test_dense_raster_on_a_one_window_buffer(S, pkg):
    """k_single_exact (one combining window): 9600 + 136 + 137 + 100 samples of the recorded capture on the 50 Hz raster."""
    g = golden("capbuf_0000")
    fc = float(g["fc"][0])
    cap = iq_u8_to_capbuf(g["iq_u8"])[:9600 + 136 + 137 + 100]
    f = raster(50.0)
    eps = pkg.frq_tie_eps()
    ro = O.xcorr_pss(cap, f, 2, fc, fc, FS)
    st = tie_stats(ro, eps)
    print(f"[oracle] one window, step 50 Hz: margin < 1e-6: {st['lt_1e6']}, < 2e-6: {st['lt_2e6']}, < 4e-6: {st['lt_4e6']}, exact {st['exact']}, three {st['three']}")
    assert st["lt_2e6"] >= 30
    r = S.xcorr_pss(cap, f, 2, fc, fc, FS)
    assert r["n_comb_xc"] == 1 and S.last_xcorr_info()[0] == "k_single_exact"
    errs = {a: (np.abs(r[a].astype(np.float64) - ro[a]) / ro[a]).max() for a in ("single", "incoherent")}
    _check_tie_premise(S, errs, "one window, step 50 Hz")
    listed, left = S.last_frq_repair_stats()
    _assert_case(r["pow"], r["frq"], ro, st, listed, left, "one window, step 50 Hz [k_single_exact]")


@pytest.mark.parametrize("step", STEPS)
def test_dense_raster_split_over_two_contexts(pkg, cases, step):
    """The hypothesis-split path: 31 hypotheses as 16 + 15 over two contexts of one GPU, MAX of the packed words standing in for the
    all-reduce; the near-ties between the shares (every maximum that falls on hypotheses 15 | 16) are settled by lcs_foe_contend /
    _resolve.  The planted buffer: the peak list is the oracle's as well."""
    import torch
    f, fc, bufs, ros, sts = cases[step]
    shares = [(0, 16), (16, 15)]
    ctxs = [pkg.Searcher(0) for _ in shares]
    try:
        for b, name in enumerate(NAMES):
            cap = iq_u8_to_capbuf(bufs[b])
            words = [torch.empty(3 * 9600, dtype=torch.int64, device="cuda") for _ in ctxs]
            meta = [torch.empty(9601, dtype=torch.float64, device="cuda") for _ in ctxs]
            for S_, (a, n), w, m in zip(ctxs, shares, words, meta):
                S_.foe_partial(cap, f, a, n, fc, fc, FS, w.data_ptr(), m.data_ptr())
            red = torch.stack(words).max(dim=0).values
            w2 = [torch.empty(3 * 9600, dtype=torch.int64, device="cuda") for _ in ctxs]
            listed = left = 0
            for S_, x in zip(ctxs, w2):
                S_.foe_contend(f, red.data_ptr(), x.data_ptr())
                li, le = S_.last_frq_repair_stats()
                listed, left = listed + li, left + le
            red2 = torch.stack(w2).max(dim=0).values
            ctxs[0].foe_resolve(red.data_ptr(), red2.data_ptr())
            pw, fq = pkg.sweep.unpack_pow_frq(red.cpu().numpy().reshape(3, 9600))
            # (iii): a position within eps/4 is listed by the rank that owns its runner-up or, on the winner's rank, its own second
            _assert_case(pw, fq, ros[b], sts[b], listed, left, f"{name} step {step:.0f} Hz split 16 + 15")
            zo = O.z_th1(ros[b]["sp_incoherent"], ros[b]["n_comb_xc"])
            po = O.peak_search(ros[b]["pow"], ros[b]["frq"], zo, f, fc, fc, ros[b]["single"], 2)
            # every rank returns the whole peak list; a peak's refined `ind` only from the rank that owns its hypothesis (-1 elsewhere, lcs.h)
            lists = [S_.foe_finish(red.data_ptr(), meta[0].data_ptr(), f)[2] for S_ in ctxs]
            for pk in lists:
                assert [(p.n_id_2, p.freq) for p in pk] == [(p.n_id_2, p.freq) for p in po], name
            for k, p in enumerate(po):
                assert sorted(pk[k].ind for pk in lists) == [-1, p.ind], (name, k)
    finally:
        for S_ in ctxs:
            S_.close()


# ---- the repair at the circular edge of the 9600 positions, and the remote winner's window starts ----------------------------
# k_frq_repair stages the samples of the lags on one side of the wrap and reads the others straight from memory; on the split
# path a rank recomputes a winner it does not own from window starts it forms itself (lcs_win_start).  The dense rasters above
# list no position within the arm of 0 or 9599 (checked on the oracle's output), so one crafted buffer does: two cells whose PSS
# correlation peaks sit on positions 0 (PSS 0) and 9599 (PSS 1), three hypotheses of which the last two are the same frequency --
# an exact tie at every position they win, the peaks and their +- arm neighbours far above Z_th1 (the list is crowded, so only
# such positions are recomputed).
EDGE_F = np.array([30e3, 35e3, 35e3])
EDGE_AT = ((0, 0), (1, 9599))      # (PSS, position of its peak)


@pytest.fixture(scope="module")
def edge_case(pkg):
    fc = 739e6
    iq, _ = pkg.synth.make_capbuf(4242, fc, [dict(n_id_1=25, n_id_2=0, f_off=35e3, t0=823.0), dict(n_id_1=101, n_id_2=1, f_off=35e3, t0=10424.0)])
    cap = iq_u8_to_capbuf(iq)
    ro = O.xcorr_pss(cap, EDGE_F, 2, fc, fc, FS)
    z = O.z_th1(ro["sp_incoherent"], ro["n_comb_xc"])
    where = []
    for t, p in EDGE_AT:
        assert int(np.argmax(ro["single"][t, :, 1])) == p, "the crafted peak moved"
        for d in range(-2, 3):
            i = (p + d) % 9600
            # the position is an exact tie of the duplicated hypotheses, won by the first, and can become a peak: it is listed AND repaired
            assert ro["incoherent"][t, i, 1] == ro["incoherent"][t, i, 2] > ro["incoherent"][t, i, 0] and ro["frq"][t, i] == 1
            assert ro["pow"][t, i] > 2 * z[i]
            where.append((t, i))
    return fc, cap, ro, where


def _assert_edge(pw, fq, ro, where, tag):
    for t, i in where:
        assert fq[t, i] == ro["frq"][t, i], f"{tag}: frq[{t}][{i}] = {fq[t, i]}, the oracle's {ro['frq'][t, i]}"
        assert pw[t, i] == ro["pow"][t, i], f"{tag}: pow[{t}][{i}] = {pw[t, i]!r} is not the oracle's float {ro['pow'][t, i]!r}"


def test_repair_at_the_circular_edge(S, edge_case):
    fc, cap, ro, where = edge_case
    r = S.xcorr_pss(cap, EDGE_F, 2, fc, fc, FS)
    assert S.last_xcorr_info()[0] == "k_xcorr_i8x3"
    listed, left = S.last_frq_repair_stats()
    assert listed > 32 * 64 and 0 < left < listed, (listed, left)      # crowded: bounded work, yet some positions were recomputed
    _assert_edge(r["pow"], r["frq"], ro, where, "edge")


def test_remote_winner_at_the_circular_edge(pkg, edge_case):
    """The same buffer with the hypotheses split 2 + 1 over two contexts: the second rank owns only the duplicate, so wherever it
    contends the global winner (hypothesis 1) is remote and its window starts are formed by the contending rank."""
    import torch
    fc, cap, ro, where = edge_case
    shares = [(0, 2), (2, 1)]
    ctxs = [pkg.Searcher(0) for _ in shares]
    try:
        words = [torch.empty(3 * 9600, dtype=torch.int64, device="cuda") for _ in ctxs]
        meta = [torch.empty(9601, dtype=torch.float64, device="cuda") for _ in ctxs]
        for S_, (a, n), w, m in zip(ctxs, shares, words, meta):
            S_.foe_partial(cap, EDGE_F, a, n, fc, fc, FS, w.data_ptr(), m.data_ptr())
        red = torch.stack(words).max(dim=0).values
        w2 = [torch.empty(3 * 9600, dtype=torch.int64, device="cuda") for _ in ctxs]
        for S_, x in zip(ctxs, w2):
            S_.foe_contend(EDGE_F, red.data_ptr(), x.data_ptr())
        assert ctxs[1].last_frq_repair_stats()[0] > 0, "the rank that owns only the duplicate contends"
        red2 = torch.stack(w2).max(dim=0).values
        ctxs[0].foe_resolve(red.data_ptr(), red2.data_ptr())
        pw, fq = pkg.sweep.unpack_pow_frq(red.cpu().numpy().reshape(3, 9600))
        _assert_edge(pw, fq, ro, where, "edge, split 2 + 1")
    finally:
        for S_ in ctxs:
            S_.close()
