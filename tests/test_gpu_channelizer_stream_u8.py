"""8-bit captures from the channelizer stream on the GPU (lcs_chan_stream_open_u8 / _count_u8 / _push_u8, sweep.WidebandFeed(out="u8")):
every capture of every carrier is lcs_channelize_u8's rule applied to the floats the float stream hands out for the same samples --
gains EQUAL, bytes EQUAL, no rounding band: the floats are the same bits, 2^e * y is exact, and the one thing computed differently,
the capture's power (fp32 in blocks on the GPU, float64 here), decides e only through 4^e P / 2's side of 16^2 and 32^2, which every
test that compares with the rule asserts to lie 1 % or more away (tests/chan_stream_u8_cases.py chooses the amplitudes and seeds for
that on the CPU; tests/test_channelizer_stream_u8_host.py checks them there).  n_cap = corner(U, D)[0] is odd where up is even (12/125);
the captures of 1, 5 and 4099 outputs are odd at the other rates."""
import numpy as np
import pytest

import chan_rate_ref as RR
import chan_rate_twin as T
import chan_ref as R
import chan_stream_u8_cases as S
from conftest import load_pkg

pytestmark = pytest.mark.gpu

FS_OUT = 1.92e6
_shared = {}


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def _fmt(pkg, name):
    return {"c64": pkg.FMT_C64, "s8": pkg.FMT_IQ_S8, "s16": pkg.FMT_IQ_S16}[name]


def float_stream(pkg, case, chunks=None):
    """the floats of the same samples: a float stream on a context of its own (one push, or the given chunks) -> complex64 [n_ch][M(n_in)]"""
    import torch
    n_ch, n_out = len(case["shifts"]), S.count(case["n_in"], case["up"], case["down"])
    d_in = torch.from_numpy(np.array(case["q"])).cuda()
    out = torch.zeros((n_ch, n_out), dtype=torch.complex64, device="cuda")
    N = filled = 0
    with pkg.Searcher(0) as s:
        s.chan_stream_open(_fmt(pkg, case["fmt"]), case["fs_in"], case["up"], case["down"], case["shifts"])
        for n in chunks or [case["n_in"]]:
            n_emit, m_first = s.chan_stream_push(d_in.data_ptr() + N * S.BYTES[case["fmt"]], n, out.data_ptr() + 8 * filled, n_out, n_out - filled)
            assert m_first == filled
            N, filled = N + n, filled + n_emit
        s.sync()
    assert (N, filled) == (case["n_in"], n_out)
    return out.cpu().numpy()


def expected(pkg, key, case):
    """(codes [n_caps][n_ch][n_cap][2], gains [n_caps][n_ch]) by the rule from the float stream's outputs, the premise asserted for every
    capture and carrier; computed once per stream and shared"""
    if key not in _shared:
        y = float_stream(pkg, case)
        codes, gain, v = S.rule(y, case["n_cap"])
        assert codes.shape[0] == case["n_caps"] and np.isfinite(v).all() and (v > 0).all(), key
        assert S.margin(v) >= S.MARGIN, (key, S.margin(v))
        for a in (y, codes, gain):
            a.setflags(write=False)
        _shared[key] = (codes, gain, y)
    return _shared[key]


class Arena:
    """Where a test's pushes write: every push gets a 16-byte aligned place of its own behind the last one's captures, in a byte tensor
    full of a sentinel; gains go to row cap_first of [n_caps][n_ch]."""
    SENTINEL = 0xA5

    def __init__(self, n_caps, n_ch, n_cap):
        import torch
        self.n_caps, self.n_ch, self.n_cap, self.cap_bytes = n_caps, n_ch, n_cap, 2 * n_ch * n_cap
        self.buf = torch.full((n_caps * self.cap_bytes + 16 * (n_caps + 1),), self.SENTINEL, dtype=torch.uint8, device="cuda")
        self.gain = torch.full((n_caps, n_ch), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert self.buf.data_ptr() % 16 == 0
        self.pos, self.at, self.done = 0, [], 0

    def push(self, s, d_ptr, n):
        room = self.n_caps - self.done
        n_done, cap_first = s.chan_stream_push_u8(d_ptr, n, self.buf.data_ptr() + self.pos, self.gain[self.done].data_ptr() if room else 0, room)
        assert cap_first == self.done, (cap_first, self.done)
        self.at += [self.pos + j * self.cap_bytes for j in range(n_done)]
        self.pos = (self.pos + n_done * self.cap_bytes + 15) // 16 * 16
        self.done += n_done
        return n_done

    def result(self):
        """-> (codes [n_caps][n_ch][n_cap][2], gains [n_caps][n_ch]); every byte outside the captures still holds the sentinel"""
        h = self.buf.cpu().numpy()
        assert len(self.at) == self.n_caps
        codes = np.stack([h[a:a + self.cap_bytes].reshape(self.n_ch, self.n_cap, 2) for a in self.at])
        mask = np.ones(h.size, bool)
        for a in self.at:
            mask[a:a + self.cap_bytes] = False
        assert (h[mask] == self.SENTINEL).all()
        return codes, self.gain.cpu().numpy()


def run_u8(pkg, case, chunks, s=None, between=None):
    """the stream pushed as the given chunks -> (codes, gains); every push's (n_done, cap_first) and count_u8 are the closed forms"""
    import torch
    U, D, n_cap, sb = case["up"], case["down"], case["n_cap"], S.BYTES[case["fmt"]]
    d_in = torch.from_numpy(np.array(case["q"])).cuda()
    arena = Arena(case["n_caps"], len(case["shifts"]), n_cap)
    own = s is None
    s = pkg.Searcher(0) if own else s
    try:
        s.chan_stream_open_u8(_fmt(pkg, case["fmt"]), case["fs_in"], U, D, case["shifts"], n_cap)
        N = 0
        for k, n in enumerate(chunks):
            want = S.count(N + n, U, D) // n_cap - S.count(N, U, D) // n_cap
            assert s.chan_stream_count_u8(n) == want and s.chan_stream_count(n) == S.count(N + n, U, D) - S.count(N, U, D)
            assert arena.push(s, d_in.data_ptr() + N * sb, n) == want, (k, N, n)
            N += n
            if between:
                between(k, s, d_in, N)
        s.sync()
        s.chan_stream_close()
    finally:
        if own:
            s.close()
    return arena.result()


def assert_equal(got, want, what):
    codes, gain = got
    assert np.array_equal(gain, want[1]), (what, np.argwhere(gain != want[1])[:5].tolist())
    assert np.array_equal(codes, want[0]), (what, np.argwhere(codes != want[0])[:5].tolist())


CUTS = ["one", "ones_across_a_window", "all_of_down", "random", "short_start"]


@pytest.mark.parametrize("cut", CUTS)
@pytest.mark.parametrize("U,D,fmt", S.CASES)
def test_captures_follow_the_rule_exactly(pkg, U, D, fmt, cut):
    """17 carriers, three captures and half of a fourth.  Gains EQUAL, bytes EQUAL; the burst on carrier BURST_CH reaches both clamps."""
    case = S.stream_case(U, D, fmt)
    want = expected(pkg, (U, D, fmt), case)
    chunks = S.chunkings(U, D, case["n_in"], 7 * D + U)[cut]
    assert sum(chunks) == case["n_in"] and min(chunks) >= 1
    got = run_u8(pkg, case, chunks)
    assert_equal(got, want, (U, D, fmt, cut))
    b = got[0][1, S.BURST_CH]
    assert (b == 0).any() and (b == 255).any()


@pytest.mark.parametrize("U,D,fmt", S.CASES)
def test_any_cut_and_any_run_give_the_same_bytes(pkg, U, D, fmt):
    """no premise: bytes and gains of all five cuts are torch.equal, and a second run of one of them too"""
    import torch
    case = S.stream_case(U, D, fmt)
    cuts = S.chunkings(U, D, case["n_in"], 7 * D + U)
    runs = [run_u8(pkg, case, cuts[c]) for c in CUTS] + [run_u8(pkg, case, cuts["random"])]
    a = [torch.from_numpy(r[0]) for r in runs], [torch.from_numpy(r[1]) for r in runs]
    for k in range(1, len(runs)):
        assert torch.equal(a[0][0], a[0][k]) and torch.equal(a[1][0], a[1][k]), (U, D, fmt, k)


@pytest.mark.parametrize("U,D,fmt", S.CASES)
def test_capture_0_is_the_one_shot_8_bit_call(pkg, U, D, fmt):
    """capture 0 of a stream equals channelize_u8 with n_out = n_cap on the first cs_need(n_cap) samples: bytes and gains EQUAL under the
    premise (the one-shot call sums the power in its matrix-core kernel's epilogue, in another order)"""
    import torch
    case = S.stream_case(U, D, fmt)
    want = expected(pkg, (U, D, fmt), case)
    n_cap, n_in = case["n_cap"], S.need(case["n_cap"], U, D)
    d_in = torch.from_numpy(np.array(case["q"])).cuda()
    out = torch.zeros((17, n_cap, 2), dtype=torch.uint8, device="cuda")
    with pkg.Searcher(0) as s:
        gain = s.channelize_u8(d_in.data_ptr(), _fmt(pkg, fmt), n_in, case["fs_in"], U, D, case["shifts"], out.data_ptr(), n_cap, want_gain=True)
        s.sync()
        with pytest.raises(pkg.SearcherError, match="too short"):
            s.channelize_u8(d_in.data_ptr(), _fmt(pkg, fmt), n_in - 1, case["fs_in"], U, D, case["shifts"], out.data_ptr(), n_cap)
    assert np.array_equal(gain.cpu().numpy(), want[1][0]) and np.array_equal(out.cpu().numpy(), want[0][0])


@pytest.mark.parametrize("name", [n for n in S.SIMPLE if n.startswith("nine_")])
def test_one_push_completes_nine_captures(pkg, name):
    """12/125 and 1/16; n_cap = 5 and 1 (rows at any even address), n_cap = 8 (every row of d_out on a 16-byte boundary): one chunk that
    completes 9 captures into a d_out of 16 slots; slots 9..15 and their gains keep their sentinel"""
    import torch
    case = S.simple_case(name)
    want = expected(pkg, name, case)
    n_cap, n_ch = case["n_cap"], 17
    d_in = torch.from_numpy(np.array(case["q"])).cuda()
    out = torch.full((16, n_ch, n_cap, 2), 0xA5, dtype=torch.uint8, device="cuda")
    gain = torch.full((16, n_ch), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert out.data_ptr() % 16 == 0
    with pkg.Searcher(0) as s:
        s.chan_stream_open_u8(_fmt(pkg, case["fmt"]), case["fs_in"], case["up"], case["down"], case["shifts"], n_cap)
        assert s.chan_stream_count_u8(case["n_in"]) == 9 and s.chan_stream_count_u8(case["n_in"] - 1) == 8
        assert s.chan_stream_push_u8(d_in.data_ptr(), case["n_in"], out.data_ptr(), gain.data_ptr(), 16) == (9, 0)
        s.sync()
    h, g = out.cpu().numpy(), gain.cpu().numpy()
    assert (h[9:] == 0xA5).all() and (g[9:] == -1.0).all()
    assert_equal((h[:9], g[:9]), want, name)


@pytest.mark.parametrize("n_ch", [1, 15, 16, 31, 33])
def test_a_push_writes_its_captures_and_nothing_else(pkg, n_ch):
    """2/3, s8, n_cap odd: d_out has three slots and one capture completes.  The sentinel in slots 1 and 2 -- slot 1 starts with the row
    behind the last carrier's -- and in d_gain[1..2] is intact; a push that completes nothing writes nothing."""
    import torch
    base = S.simple_case("guard_2_3")
    case = dict(base, shifts=base["shifts"][:n_ch])
    full = expected(pkg, "guard_2_3", base)
    n_cap = case["n_cap"]
    assert n_cap % 2 == 1
    d_in = torch.from_numpy(np.array(case["q"])).cuda()
    out = torch.full((3, n_ch, n_cap, 2), 0xA5, dtype=torch.uint8, device="cuda")
    gain = torch.full((3, n_ch), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    first = case["n_in"] - 7
    with pkg.Searcher(0) as s:
        s.chan_stream_open_u8(pkg.FMT_IQ_S8, case["fs_in"], 2, 3, case["shifts"], n_cap)
        assert s.chan_stream_push_u8(d_in.data_ptr(), first, out.data_ptr(), gain.data_ptr(), 3) == (0, 0)
        s.sync()
        assert (out.cpu().numpy() == 0xA5).all() and (gain.cpu().numpy() == -1.0).all()
        assert s.chan_stream_push_u8(d_in.data_ptr() + 2 * first, 7, out.data_ptr(), gain.data_ptr(), 3) == (1, 0)
        s.sync()
    h, g = out.cpu().numpy(), gain.cpu().numpy()
    assert (h[1:] == 0xA5).all() and (g[1:] == -1.0).all()
    assert_equal((h[:1], g[:1]), (full[0][:, :n_ch], full[1][:, :n_ch]), n_ch)


def test_refused_calls_leave_the_stream_intact(pkg):
    import torch
    U, D, fmt = 3, 4, "s8"
    case = S.stream_case(U, D, fmt)
    want = expected(pkg, (U, D, fmt), case)
    n_cap, n_in = case["n_cap"], case["n_in"]
    a = S.need(n_cap, U, D) - 5                       # five samples short of capture 0
    b = S.need(2 * n_cap, U, D) - a                   # ... and a chunk that completes captures 0 and 1
    d_in = torch.from_numpy(np.array(case["q"])).cuda()
    arena = Arena(3, 17, n_cap)
    small = torch.zeros(64, dtype=torch.complex64, device="cuda")
    with pkg.Searcher(0) as s:
        with pytest.raises(pkg.SearcherError, match="lcs_chan_stream_open_u8: n_cap < 1"):
            s.chan_stream_open_u8(pkg.FMT_IQ_S8, case["fs_in"], U, D, case["shifts"], 0)
        with pytest.raises(pkg.SearcherError, match="no channelizer stream is open"):
            s.chan_stream_count_u8(1)
        s.chan_stream_open(pkg.FMT_IQ_S8, case["fs_in"], U, D, case["shifts"])
        with pytest.raises(pkg.SearcherError, match="lcs_chan_stream_push_u8: the stream hands out floats"):
            s.chan_stream_push_u8(d_in.data_ptr(), 8, arena.buf.data_ptr(), 0, 3)
        with pytest.raises(pkg.SearcherError, match="lcs_chan_stream_count_u8: the stream hands out floats"):
            s.chan_stream_count_u8(8)
        assert s.chan_stream_push(d_in.data_ptr(), 8, small.data_ptr(), 64, 64) == (0, 0)      # the float stream is where it was
        s.chan_stream_close()
        s.chan_stream_open_u8(pkg.FMT_IQ_S8, case["fs_in"], U, D, case["shifts"], n_cap)
        assert arena.push(s, d_in.data_ptr(), a) == 0
        assert s.chan_stream_count_u8(b) == 2
        with pytest.raises(pkg.SearcherError, match="lcs_chan_stream_push_u8: cap_room < n_done"):
            s.chan_stream_push_u8(d_in.data_ptr() + 2 * a, b, arena.buf.data_ptr(), 0, 1)
        with pytest.raises(pkg.SearcherError, match="d_out is not 16-byte aligned"):
            s.chan_stream_push_u8(d_in.data_ptr() + 2 * a, b, arena.buf.data_ptr() + 8, 0, 3)
        with pytest.raises(pkg.SearcherError, match="lcs_chan_stream_push: the stream hands out 8-bit captures"):
            s.chan_stream_push(d_in.data_ptr() + 2 * a, b, small.data_ptr(), 64, 64)
        with pytest.raises(pkg.SearcherError, match="already open"):
            s.chan_stream_open_u8(pkg.FMT_IQ_S8, case["fs_in"], U, D, case["shifts"], n_cap)
        with pytest.raises(pkg.SearcherError, match="already open"):
            s.chan_stream_open(pkg.FMT_IQ_S8, case["fs_in"], U, D, case["shifts"])
        assert s.chan_stream_count_u8(b) == 2 and s.chan_stream_count(b) == S.count(a + b, U, D) - S.count(a, U, D)
        assert arena.push(s, d_in.data_ptr() + 2 * a, b) == 2
        assert arena.push(s, d_in.data_ptr() + 2 * (a + b), n_in - a - b) == 1
        s.sync()
        s.chan_stream_close()
        with pytest.raises(pkg.SearcherError, match="no channelizer stream is open"):
            s.chan_stream_push_u8(d_in.data_ptr(), 8, arena.buf.data_ptr(), 0, 3)
    assert_equal(arena.result(), want, "after the refusals")


def test_one_shot_calls_and_the_stream_share_a_context(pkg):
    """with a stream of 8-bit captures open at 12/125, channelize_u8 at 3/4 on the same context between two pushes gives the bytes of a
    fresh context, and the stream ends as an undisturbed one"""
    import torch
    U, D, fmt = 12, 125, "s16"
    case = S.stream_case(U, D, fmt)
    want = expected(pkg, (U, D, fmt), case)
    other = S.stream_case(3, 4, "s8")
    n2, n_in2 = other["n_cap"], S.need(other["n_cap"], 3, 4)
    d2 = torch.from_numpy(np.array(other["q"])).cuda()

    def one_shot(s):
        out = torch.zeros((17, n2, 2), dtype=torch.uint8, device="cuda")
        g = s.channelize_u8(d2.data_ptr(), pkg.FMT_IQ_S8, n_in2, other["fs_in"], 3, 4, other["shifts"], out.data_ptr(), n2, want_gain=True)
        s.sync()
        return out.cpu().numpy(), g.cpu().numpy()

    with pkg.Searcher(0) as fresh:
        alone = one_shot(fresh)
    seen = []
    half = case["n_in"] // 2 + 3
    got = run_u8(pkg, case, [1000, half - 1000, case["n_in"] - half], between=lambda k, s, d_in, N: seen.append(one_shot(s)) if k == 1 else None)
    assert len(seen) == 1 and np.array_equal(seen[0][0], alone[0]) and np.array_equal(seen[0][1], alone[1])
    assert_equal(got, want, "around a one-shot call")


def test_an_all_zero_capture_has_gain_1_and_code_127(pkg):
    import torch
    U, D, n_cap = 12, 125, 781
    n_in = S.need(2 * n_cap, U, D)
    fs_in = FS_OUT * D / U
    case = dict(q=np.zeros(2 * n_in, np.int16), n_in=n_in, fs_in=fs_in, shifts=T.shifts17(fs_in), n_cap=n_cap, n_caps=2, up=U, down=D, fmt="s16")
    codes, gain = run_u8(pkg, case, [n_in // 3, n_in - n_in // 3])
    assert (codes == 127).all() and (gain == 1.0).all()


def test_an_inf_sample_spoils_its_capture_only(pkg):
    """T.nonfinite_case: 3/4, c64, captures of n_out // 3.  The capture that holds the Inf has gain 1 and code 127 exactly where the float
    stream's output is not finite; the captures beside it follow the rule.  Both streams are cut alike: which of the outputs whose
    padded window holds the Inf are spoilt depends on the cut (include/lcs.h)."""
    x, n_in, fs_in, shifts, n_out, clean, dirty = T.nonfinite_case(S.NONFINITE_SEED)
    n_cap = n_out // 3
    case = dict(q=x, n_in=n_in, fs_in=fs_in, shifts=shifts, n_cap=n_cap, n_caps=3, up=3, down=4, fmt="c64")
    chunks = S.chunkings(3, 4, n_in, 34)["random"]
    y = float_stream(pkg, case, chunks)
    bad = ~np.isfinite(y)
    hit = sorted(set((np.argwhere(bad)[:, 1] // n_cap).tolist()))
    assert hit == [1] and bad[:, dirty].all() and not bad[:, clean].any()
    with np.errstate(invalid="ignore", over="ignore"):
        codes_ref, gain_ref, v = S.rule(y, n_cap)
    assert S.margin(v[[0, 2]]) >= S.MARGIN and (gain_ref[1] == 1.0).all()
    codes, gain = run_u8(pkg, case, chunks)
    assert_equal((codes, gain), (codes_ref, gain_ref), "with an Inf sample")
    b1 = bad[:, n_cap:2 * n_cap]
    assert (gain[1] == 1.0).all() and (codes[1][b1] == 127).all()


def test_long_stream_in_64_uneven_pushes(pkg):
    """2^21 s16 samples at 12/125, n_cap = 4099 (odd): 49 captures of 17 carriers, every one against the rule"""
    case = S.long_case()
    want = expected(pkg, "long", case)
    rng = np.random.default_rng(64 + 125)
    cuts = np.sort(rng.choice(np.arange(1, case["n_in"]), 63, replace=False))
    chunks = np.diff(np.concatenate([[0], cuts, [case["n_in"]]])).tolist()
    assert len(chunks) == 64 and case["n_caps"] == 49
    assert_equal(run_u8(pkg, case, chunks), want, "long stream")


def test_wideband_feed_u8_searches_a_20_msps_stream_on_the_int8_kernel(pkg):
    """The 20 Msps s16 capture of tests/test_gpu_channelizer_rate.py through sweep.WidebandFeed(out="u8") in ten uneven transfer buffers,
    n_cap = 153584: one capture, complete on the last push.  Bytes and gains equal channelize_u8 on the whole capture; the cells equal
    search_batch on those bytes field for field."""
    import torch
    iq, _, _ = RR.wbr_capture(pkg)
    d = torch.from_numpy(iq).cuda()
    n_in, fs_in, U, D, n_cap = iq.size // 2, RR.WBR_FS_IN, RR.WBR["up"], RR.WBR["down"], RR.WBR["n_out"]
    carriers = RR.wbr_carriers()
    assert S.count(n_in, U, D) == n_cap + 1
    rng = np.random.default_rng(20)
    cuts = np.sort(rng.choice(np.arange(1, n_in - 50), 9, replace=False))
    chunks = np.diff(np.concatenate([[0], cuts, [n_in]])).tolist()
    fields = lambda c: (R.cell_key(c), c.pss_pow, c.freq_superfine, c.frame_start, c.fc_requested, c.freq, c.freq_fine, c.ind)
    with pkg.Searcher(0) as s:
        whole = torch.zeros((len(carriers), n_cap, 2), dtype=torch.uint8, device="cuda")
        gain = s.channelize_u8(d.data_ptr(), pkg.FMT_IQ_S16, n_in, fs_in, U, D, carriers - RR.WBR["fc_centre"], whole.data_ptr(), n_cap, want_gain=True)
        want = s.search_batch(whole.data_ptr(), pkg.FMT_IQ_U8, len(carriers), n_cap, RR.WBR_GRID, carriers, carriers, FS_OUT, pkg.STAGE_FULL, 16)
        done, N = [], 0
        with pkg.sweep.WidebandFeed(s, pkg.FMT_IQ_S16, fs_in, (U, D), RR.WBR["fc_centre"], carriers, RR.WBR_GRID, n_cap=n_cap, out="u8") as feed:
            assert feed.gains is None
            for k, n in enumerate(chunks):
                got = feed.push(d.data_ptr() + 4 * N, n)
                N += n
                assert (len(got) == 1) == (k == len(chunks) - 1), (k, len(got))
                done += got
            assert s.last_xcorr_info()[0] == "k_xcorr_i8x3"
            s.sync()
            assert feed.cur == 1 and feed.bufs[0].dtype == torch.uint8 and feed.gains.dtype == torch.float32
            assert torch.equal(feed.bufs[0], whole) and torch.equal(feed.gains, gain)
            on_one_scale = pkg.sweep.records_with_gain(done[0], feed.gains)
    assert len(done) == 1 and len(done[0]) == len(carriers)
    assert sum(len(c) for c in done[0]) == len(RR.WBR_PLACED)
    for a, b in zip(done[0], want):
        assert [fields(c) for c in a] == [fields(c) for c in b]
    g = gain.cpu().numpy().astype(np.float64)
    for k, cells in enumerate(on_one_scale):
        assert [c["pss_pow"] for c in cells] == [c.pss_pow / g[k] ** 2 for c in done[0][k]]
