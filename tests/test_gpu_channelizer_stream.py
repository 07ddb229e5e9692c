"""The channelizer's continuous form on the GPU (lcs_chan_stream_open / _count / _push / _close, sweep.WidebandFeed): after any
sequence of pushes the outputs handed out are, bit for bit, those of ONE lcs_channelize_rational call on everything pushed."""
import numpy as np
import pytest

import chan_rate_ref as RR
import chan_rate_twin as T
import chan_ref as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu

RTOL = 1e-5          # fp32-class arrays against a double oracle: the project's standing bar (tests/test_gpu_pss.py)
FS_OUT = 1.92e6
BYTES = {"c64": 8, "s16": 4, "s8": 2}


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def _fmt(pkg, name):
    return {"c64": pkg.FMT_C64, "s8": pkg.FMT_IQ_S8, "s16": pkg.FMT_IQ_S16}[name]


def count(N, U, D):
    """M(N) of include/lcs.h"""
    return 0 if N * U < 16 * D else (N * U - 16 * D) // D + 1


def corner(U, D):
    """two full workgroups and a partial column of outputs (256 columns per workgroup at up == 1), the stream no longer than they need"""
    NI = 8 if U == 1 else T.geometry(U, D)[1]
    n_out = 2 * (32 * NI * U) + U + 1
    n_in = RR.n_in_min(n_out, U, D)
    assert count(n_in, U, D) == n_out
    return n_out, n_in


def one_shot(s, d_in, fmt, n_in, fs_in, U, D, shifts, n_out):
    import torch
    out = torch.zeros((len(shifts), n_out), dtype=torch.complex64, device="cuda")
    s.channelize_rational(d_in.data_ptr(), fmt, n_in, fs_in, U, D, shifts, out.data_ptr(), n_out)
    s.sync()
    return out


def push_all(s, d_in, sample_bytes, chunks, U, D, out, n_start=0, filled=0):
    """push the chunks one behind the other from sample n_start on, the outputs one behind the other into out[n_ch][n_out] from column
    `filled` on; every push's (n_emit, m_first) is M(N)'s.  -> [(n_emit, m_first)]"""
    n_out, N, got = out.shape[1], n_start, []
    for n in chunks:
        assert s.chan_stream_count(n) == count(N + n, U, D) - count(N, U, D)
        n_emit, m_first = s.chan_stream_push(d_in.data_ptr() + N * sample_bytes, n, out.data_ptr() + 8 * filled, n_out, n_out - filled)
        assert (m_first, n_emit) == (count(N, U, D), count(N + n, U, D) - count(N, U, D)), (N, n, m_first, n_emit)
        assert m_first == filled
        N, filled = N + n, filled + n_emit
        got.append((n_emit, m_first))
    return got


def chunkings(U, D, n_in, seed):
    rng = np.random.default_rng(seed)
    L = -(-16 * D // U)                       # the first output needs L samples
    rand = []
    while sum(rand) < n_in:
        rand.append(min(int(rng.integers(1, 3 * D + 1)), n_in - sum(rand)))
    short = [max(1, (L - 1) // 5)] * 5        # together shorter than the filter
    return {"one": [n_in],
            "ones_across_a_window": [L - 3] + [1] * (2 * D + 8) + [n_in - (L - 3) - (2 * D + 8)],
            "all_of_down": [D] * (n_in // D) + ([n_in % D] if n_in % D else []),
            "random": rand,
            "short_start": short + [n_in - sum(short)]}


CASES = [(1, 2, "s8"), (1, 16, "s16"), (1, 16, "c64"), (2, 3, "s8"), (3, 4, "s8"), (3, 4, "s16"), (3, 4, "c64"), (12, 125, "s8"), (12, 125, "s16"),
         (12, 125, "c64"), (127, 128, "s16"), (31, 94, "c64"), (3, 47, "s16")]


@pytest.mark.parametrize("U,D,fmt", CASES)
def test_chunked_equals_one_shot(pkg, U, D, fmt):
    """17 carriers, every chunking of chunkings(): torch.equal on the bytes.  31/94 is the LDS maximum, 3/47 has NI held by the cap."""
    import torch
    n_out, n_in = corner(U, D)
    fs_in = FS_OUT * D / U
    shifts = T.shifts17(fs_in)
    q, _ = R.quantise(T.noise_and_tones(100 * D + U + len(fmt), n_in, fs_in), fmt)
    d_in = torch.from_numpy(q).cuda()
    with pkg.Searcher(0) as s:
        whole = one_shot(s, d_in, _fmt(pkg, fmt), n_in, fs_in, U, D, shifts, n_out)
        assert float(whole.abs().max()) > 0
        for name, chunks in chunkings(U, D, n_in, 7 * D + U).items():
            assert sum(chunks) == n_in and min(chunks) >= 1, name
            out = torch.full((17, n_out), float("nan"), dtype=torch.complex64, device="cuda")
            s.chan_stream_open(_fmt(pkg, fmt), fs_in, U, D, shifts)
            got = push_all(s, d_in, BYTES[fmt], chunks, U, D, out)
            s.sync()
            s.chan_stream_close()
            if name == "short_start":
                assert [g[0] for g in got[:5]] == [0] * 5 and got[5][1] == 0 and got[5][0] == n_out
            assert sum(g[0] for g in got) == n_out
            assert torch.equal(out.view(torch.int64), whole.view(torch.int64)), (name, torch.nonzero(out.view(torch.int64) != whole.view(torch.int64))[:4].tolist())


@pytest.mark.parametrize("fmt", ["s8", "s16", "c64"])
def test_chunked_arrays_match_the_double_reference(pkg, fmt):
    """the stream against the definition (tests/chan_rate_ref.py), not only against the sibling kernel: 12/125, seeded chunks"""
    import torch
    U, D = 12, 125
    n_out, n_in = corner(U, D)
    fs_in = FS_OUT * D / U
    shifts = T.shifts17(fs_in)
    q, xq = R.quantise(T.noise_and_tones(31 + len(fmt), n_in, fs_in), fmt)
    ref = RR.channelize_rate_ref(xq, fs_in, U, D, shifts, n_out)
    d_in = torch.from_numpy(q).cuda()
    out = torch.zeros((17, n_out), dtype=torch.complex64, device="cuda")
    with pkg.Searcher(0) as s:
        s.chan_stream_open(_fmt(pkg, fmt), fs_in, U, D, shifts)
        push_all(s, d_in, BYTES[fmt], chunkings(U, D, n_in, 5)["random"], U, D, out)
        s.sync()
    y = out.cpu().numpy()
    ratios = [float(np.abs(y[k] - ref[k]).max() / np.abs(ref[k]).max()) for k in range(17)]
    print(f"channelizer stream {fmt} 12/125: worst max|y - y_ref| / max|y_ref| per channel = {max(ratios):.3e}")
    assert max(ratios) <= RTOL, ratios


@pytest.mark.parametrize("n_ch", [1, 15, 16, 31, 33])
def test_a_push_writes_its_outputs_and_nothing_else(pkg, n_ch):
    """2/3, s8: every push goes to the same place of a tensor of n_ch + 1 rows, row_stride = out_cap + 5, from an address that is 8-byte
    but not 16-byte aligned; after every push every cell outside [k][0 .. n_emit) still holds the sentinel."""
    import torch
    U, D = 2, 3
    n_out, n_in = corner(U, D)
    fs_in = FS_OUT * D / U
    shifts = np.resize(T.shifts17(fs_in), n_ch)
    q, _ = R.quantise(T.noise_and_tones(23 + n_ch, n_in, fs_in), "s8")
    d_in = torch.from_numpy(q).cuda()
    sentinel = complex(-7.25, 1234.5)
    chunks = [5, 19, 1, 300, 2, n_in - 327 - 64, 64]
    out_cap = max(count(sum(chunks[:k + 1]), U, D) - count(sum(chunks[:k]), U, D) for k in range(len(chunks)))
    stride = out_cap + 5
    with pkg.Searcher(0) as s:
        whole = one_shot(s, d_in, pkg.FMT_IQ_S8, n_in, fs_in, U, D, shifts, n_out).cpu().numpy()
        flat = torch.empty(1 + (n_ch + 1) * stride, dtype=torch.complex64, device="cuda")
        assert (flat.data_ptr() + 8) % 16 == 8
        s.chan_stream_open(pkg.FMT_IQ_S8, fs_in, U, D, shifts)
        N = 0
        for n in chunks:
            flat.fill_(sentinel)
            torch.cuda.synchronize()
            n_emit, m_first = s.chan_stream_push(d_in.data_ptr() + 2 * N, n, flat.data_ptr() + 8, stride, out_cap)
            s.sync()
            N += n
            h = flat.cpu().numpy()
            assert h[0] == np.complex64(sentinel)
            body = h[1:].reshape(n_ch + 1, stride)
            assert body[:n_ch, :n_emit].tobytes() == whole[:, m_first:m_first + n_emit].tobytes(), (n, m_first, n_emit)
            assert (body[:n_ch, n_emit:] == np.complex64(sentinel)).all() and (body[n_ch] == np.complex64(sentinel)).all(), (n, m_first, n_emit)
        assert m_first + n_emit == n_out


@pytest.mark.parametrize("U,D", [(1, 16), (12, 125)])
def test_long_stream_in_64_uneven_pushes(pkg, U, D):
    import torch
    n_in = 1 << 21
    n_out = count(n_in, U, D)
    fs_in = FS_OUT * D / U
    shifts = np.array([1234567.8, -0.45 * fs_in])
    rng = np.random.default_rng(64 + D)
    q = rng.integers(-128, 128, 2 * n_in).astype(np.int8)
    cuts = np.sort(rng.choice(np.arange(1, n_in), 63, replace=False))
    chunks = np.diff(np.concatenate([[0], cuts, [n_in]])).tolist()
    d_in = torch.from_numpy(q).cuda()
    out = torch.zeros((2, n_out), dtype=torch.complex64, device="cuda")
    with pkg.Searcher(0) as s:
        whole = one_shot(s, d_in, pkg.FMT_IQ_S8, n_in, fs_in, U, D, shifts, n_out)
        s.chan_stream_open(pkg.FMT_IQ_S8, fs_in, U, D, shifts)
        push_all(s, d_in, 2, chunks, U, D, out)
        s.sync()
    assert len(chunks) == 64 and torch.equal(out.view(torch.int64), whole.view(torch.int64))


def test_a_refused_push_leaves_the_stream_intact(pkg):
    import torch
    U, D = 3, 4
    n_out, n_in = corner(U, D)
    fs_in = FS_OUT * D / U
    shifts = T.shifts17(fs_in)
    q, _ = R.quantise(T.noise_and_tones(9, n_in, fs_in), "s16")
    d_in = torch.from_numpy(q).cuda()
    out = torch.zeros((17, n_out), dtype=torch.complex64, device="cuda")
    a, b = 200, 311
    with pkg.Searcher(0) as s:
        whole = one_shot(s, d_in, pkg.FMT_IQ_S16, n_in, fs_in, U, D, shifts, n_out)
        s.chan_stream_open(pkg.FMT_IQ_S16, fs_in, U, D, shifts)
        (f0, _), = push_all(s, d_in, 4, [a], U, D, out)
        need = s.chan_stream_count(b)
        assert need == count(a + b, U, D) - count(a, U, D) > 1
        with pytest.raises(pkg.SearcherError, match="lcs_chan_stream_push: out_cap < n_emit"):
            s.chan_stream_push(d_in.data_ptr() + 4 * a, b, out.data_ptr() + 8 * f0, n_out, need - 1)
        with pytest.raises(pkg.SearcherError, match="row_stride < out_cap"):
            s.chan_stream_push(d_in.data_ptr() + 4 * a, b, out.data_ptr() + 8 * f0, need - 1, need)
        with pytest.raises(pkg.SearcherError, match="d_out is not 8-byte aligned"):
            s.chan_stream_push(d_in.data_ptr() + 4 * a, b, out.data_ptr() + 8 * f0 + 4, n_out, need)
        with pytest.raises(pkg.SearcherError, match="already open"):
            s.chan_stream_open(pkg.FMT_IQ_S16, fs_in, U, D, shifts)
        assert s.chan_stream_count(b) == need
        push_all(s, d_in, 4, [b, n_in - a - b], U, D, out, n_start=a, filled=f0)
        s.sync()
        s.chan_stream_close()
        with pytest.raises(pkg.SearcherError, match="no channelizer stream is open"):
            s.chan_stream_count(1)
    assert torch.equal(out.view(torch.int64), whole.view(torch.int64))


def test_one_shot_calls_and_the_stream_share_a_context(pkg):
    """with a stream open at 12/125, a one-shot call at 3/4 on the same context gives the bytes of a fresh context; the stream goes on
    bit-exactly behind it; close and reopen with other carriers at another rate works"""
    import torch
    U, D = 12, 125
    n_out, n_in = corner(U, D)
    fs_in = FS_OUT * D / U
    shifts = T.shifts17(fs_in)
    q, _ = R.quantise(T.noise_and_tones(77, n_in, fs_in), "s16")
    d_in = torch.from_numpy(q).cuda()
    n_out2, n_in2 = corner(3, 4)
    fs2, shifts2 = FS_OUT * 4 / 3, np.array([0.0, 250e3, -1.0e6])
    q2, _ = R.quantise(T.noise_and_tones(78, n_in2, fs2), "s8")
    d_in2 = torch.from_numpy(q2).cuda()
    with pkg.Searcher(0) as fresh:
        whole = one_shot(fresh, d_in, pkg.FMT_IQ_S16, n_in, fs_in, U, D, shifts, n_out)
    with pkg.Searcher(0) as fresh:
        other = one_shot(fresh, d_in2, pkg.FMT_IQ_S8, n_in2, fs2, 3, 4, shifts2, n_out2)
    out = torch.zeros((17, n_out), dtype=torch.complex64, device="cuda")
    with pkg.Searcher(0) as s:
        s.chan_stream_open(pkg.FMT_IQ_S16, fs_in, U, D, shifts)
        half = n_in // 2 + 3
        got = push_all(s, d_in, 4, [1000, half - 1000], U, D, out)
        between = one_shot(s, d_in2, pkg.FMT_IQ_S8, n_in2, fs2, 3, 4, shifts2, n_out2)
        assert torch.equal(between.view(torch.int64), other.view(torch.int64))
        push_all(s, d_in, 4, [n_in - half], U, D, out, n_start=half, filled=sum(g[0] for g in got))
        s.sync()
        assert torch.equal(out.view(torch.int64), whole.view(torch.int64))
        s.chan_stream_close()
        out2 = torch.zeros((3, n_out2), dtype=torch.complex64, device="cuda")
        s.chan_stream_open(pkg.FMT_IQ_S8, fs2, 3, 4, shifts2)
        push_all(s, d_in2, 2, [n_in2 // 3, n_in2 - n_in2 // 3], 3, 4, out2)
        s.sync()
        assert torch.equal(out2.view(torch.int64), other.view(torch.int64))


def test_a_non_finite_sample_spoils_its_windows_only(pkg):
    """include/lcs.h: 3/4, c64, one Inf in mid-stream, seeded chunks.  Outputs whose taps meet the sample are non-finite; outputs whose
    padded window does not hold it -- the zone the header leaves untouched -- are finite and equal the one-shot call's bit for bit."""
    import torch
    x, n_in, fs_in, shifts, n_out, clean, dirty = T.nonfinite_case()
    assert count(n_in, 3, 4) == n_out
    d_in = torch.from_numpy(x).cuda()
    out = torch.zeros((17, n_out), dtype=torch.complex64, device="cuda")
    with pkg.Searcher(0) as s:
        whole = one_shot(s, d_in, pkg.FMT_C64, n_in, fs_in, 3, 4, shifts, n_out).cpu().numpy()
        s.chan_stream_open(pkg.FMT_C64, fs_in, 3, 4, shifts)
        push_all(s, d_in, 8, chunkings(3, 4, n_in, 34)["random"], 3, 4, out)
        s.sync()
    y = out.cpu().numpy()
    assert np.isfinite(y[:, clean]).all() and not np.isfinite(y[:, dirty]).any()
    assert y[:, clean].tobytes() == whole[:, clean].tobytes()
    assert not (np.isfinite(whole) & ~np.isfinite(y)).any()      # the stream may be finite where the one-shot call is not, never the reverse


def test_wideband_feed_searches_a_20_msps_stream_like_the_one_shot_path(pkg):
    """The 20 Msps s16 capture of tests/test_gpu_channelizer_rate.py through sweep.WidebandFeed in uneven transfer buffers; n_cap =
    153584 is one output short of what the capture gives, so its last buffer straddles the capture boundary and is split there."""
    import torch
    iq, _, _ = RR.wbr_capture(pkg)
    d = torch.from_numpy(iq).cuda()
    n_in, fs_in, U, D, n_cap = iq.size // 2, RR.WBR_FS_IN, RR.WBR["up"], RR.WBR["down"], RR.WBR["n_out"]
    carriers = RR.wbr_carriers()
    assert count(n_in, U, D) == n_cap + 1
    rng = np.random.default_rng(20)
    cuts = np.sort(rng.choice(np.arange(1, n_in - 50), 9, replace=False))
    chunks = np.diff(np.concatenate([[0], cuts, [n_in]])).tolist()
    with pkg.Searcher(0) as s:
        whole = one_shot(s, d, pkg.FMT_IQ_S16, n_in, fs_in, U, D, carriers - RR.WBR["fc_centre"], n_cap)
        want = s.search_batch(whole.data_ptr(), pkg.FMT_C64, len(carriers), n_cap, RR.WBR_GRID, carriers, carriers, FS_OUT, pkg.STAGE_FULL, 16)
        done, N = [], 0
        with pkg.sweep.WidebandFeed(s, pkg.FMT_IQ_S16, fs_in, (U, D), RR.WBR["fc_centre"], carriers, RR.WBR_GRID, n_cap=n_cap) as feed:
            for k, n in enumerate(chunks):
                got = feed.push(d.data_ptr() + 4 * N, n)
                N += n
                assert (len(got) == 1) == (k == len(chunks) - 1), (k, len(got))
                done += got
            s.sync()
            assert feed.cur == 1 and feed.filled == 1
            assert torch.equal(feed.bufs[0].view(torch.int64), whole.view(torch.int64))
    assert len(done) == 1 and len(done[0]) == len(carriers)
    assert sum(len(c) for c in want) == len(RR.WBR_PLACED)
    for a, b in zip(done[0], want):
        assert [(R.cell_key(c), c.pss_pow, c.freq_superfine, c.frame_start) for c in a] == [(R.cell_key(c), c.pss_pow, c.freq_superfine, c.frame_start) for c in b]
