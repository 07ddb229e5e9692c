"""The rational channelizer on the GPU (lcs_channelize_rational) against its float64 restatement (tests/chan_rate_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import chan_rate_ref as RR
import chan_rate_twin as T
import chan_ref as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu

RTOL = 1e-5          # fp32-class arrays against a double oracle: the project's standing bar (tests/test_gpu_pss.py)
FS_OUT = 1.92e6


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def _fmt(pkg, name):
    return {"c64": pkg.FMT_C64, "s8": pkg.FMT_IQ_S8, "s16": pkg.FMT_IQ_S16}[name]


_noise_and_tones, _shifts17 = T.noise_and_tones, T.shifts17      # the signal and the 17 carriers the host twin's tests share


def _run(s, q, fmt, n_in, fs_in, up, down, shifts, n_out):
    import torch
    d_in = torch.from_numpy(q).cuda()
    d_out = torch.zeros((len(shifts), n_out), dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    s.channelize_rational(d_in.data_ptr(), fmt, n_in, fs_in, up, down, shifts, d_out.data_ptr(), n_out)
    s.sync()
    return d_out.cpu().numpy()


def _worst(y, ref):
    return [float(np.abs(y[k] - ref[k]).max() / np.abs(ref[k]).max()) for k in range(len(ref))]


RATES = [(12, 125, f) for f in ("s8", "s16", "c64")] + [(3, 4, f) for f in ("s8", "s16", "c64")] + [(24, 125, "s16"), (8, 25, "s16"), (15, 16, "s16"),
                                                                                                  (96, 125, "s16")]


@pytest.mark.parametrize("up,down,fmt", RATES)
def test_arrays_match_the_double_reference(pkg, up, down, fmt):
    fs_in, n_out = FS_OUT * down / up, 4099
    n_in = RR.n_in_min(n_out, up, down)          # exactly what "valid" mode needs: the last window ends on the last sample
    shifts = _shifts17(fs_in)
    assert shifts.size == 17 and np.abs(shifts).max() <= 0.5 * fs_in
    q, xq = R.quantise(_noise_and_tones(100 * down + up + len(fmt), n_in, fs_in), fmt)
    ref = RR.channelize_rate_ref(xq, fs_in, up, down, shifts, n_out)
    with pkg.Searcher(0) as s:
        y = _run(s, q, _fmt(pkg, fmt), n_in, fs_in, up, down, shifts, n_out)
        assert s.last_channelize_ms() > 0
    ratios = _worst(y, ref)
    print(f"rational channelizer {fmt} {up}/{down}: worst max|y - y_ref| / max|y_ref| per channel = {max(ratios):.3e}")
    assert max(ratios) <= RTOL, ratios


def test_a_call_smaller_than_one_residue_cycle(pkg):
    up, down, n_out = 12, 125, 5
    fs_in, n_in = 20e6, RR.n_in_min(5, 12, 125)
    shifts = np.array([1234567.8])
    q, xq = R.quantise(_noise_and_tones(5, n_in, fs_in), "s16")
    ref = RR.channelize_rate_ref(xq, fs_in, up, down, shifts, n_out)
    with pkg.Searcher(0) as s:
        y = _run(s, q, pkg.FMT_IQ_S16, n_in, fs_in, up, down, shifts, n_out)
    ratios = _worst(y, ref)
    print(f"rational channelizer, n_out = 5, one carrier: {max(ratios):.3e}")
    assert max(ratios) <= RTOL, ratios


def _against_twin(pkg, y, q, fmt, n_in, fs_in, up, down, shifts, n_out, ref):
    """max|gpu - twin| / max|ref| per channel, the worst: the kernel against its walk on the CPU (tests/host/chan_rate_host.cpp) -- the
    same indices, tables built in the same arithmetic, one fma per k.  A figure to read, not a bound: how the matrix core rounds
    inside one instruction is not something this project has measured."""
    tw = T.run(q, fmt, n_in, up, down, T.steps(shifts, fs_in), pkg.channelizer_proto(down), n_out)
    return max(float(np.abs(y[k] - tw[k]).max() / np.abs(ref[k]).max()) for k in range(len(ref)))


@pytest.mark.parametrize("up,down,fmt", T.CORNERS)
def test_corners_of_the_rate_domain(pkg, up, down, fmt):
    """The pairs at which the launcher's bookkeeping is at an edge (tests/chan_rate_twin.py: CORNERS), each with one full workgroup, a
    second nearly empty one and a partial residue cycle: n_out = 32 NI up + up + 1, the capture no longer than that needs."""
    n_out = T.corner_n_out(up, down)
    fs_in, n_in = FS_OUT * down / up, RR.n_in_min(n_out, up, down)
    shifts = _shifts17(fs_in)
    q, xq = R.quantise(_noise_and_tones(100 * down + up + len(fmt), n_in, fs_in), fmt)
    ref = RR.channelize_rate_ref(xq, fs_in, up, down, shifts, n_out)
    with pkg.Searcher(0) as s:
        y = _run(s, q, _fmt(pkg, fmt), n_in, fs_in, up, down, shifts, n_out)
    ratios = _worst(y, ref)
    print(f"rational channelizer corner {fmt} {up}/{down} n_out={n_out}: worst max|y - y_ref| / max|y_ref| per channel = {max(ratios):.3e}; "
          f"max|gpu - twin| / max|y_ref| = {_against_twin(pkg, y, q, fmt, n_in, fs_in, up, down, shifts, n_out, ref):.3e}")
    assert max(ratios) <= RTOL, ratios


@pytest.mark.parametrize("n_ch", [1, 15, 16, 31, 33])
def test_carrier_counts_around_a_block_of_16_write_nothing_else(pkg, n_ch):
    """2/3, s8: a carrier count below, at and above whole blocks of 16 carriers.  The output is the contiguous [n_ch][n_out] head of a
    tensor of n_ch + 1 rows of n_out + 4: everything behind it -- a guard row and the guard columns -- keeps its sentinel."""
    import torch
    up, down = 2, 3
    n_out = T.corner_n_out(up, down)
    fs_in, n_in = FS_OUT * down / up, RR.n_in_min(n_out, up, down)
    shifts = np.resize(_shifts17(fs_in), n_ch)
    q, xq = R.quantise(_noise_and_tones(23 + n_ch, n_in, fs_in), "s8")
    ref = RR.channelize_rate_ref(xq, fs_in, up, down, shifts, n_out)
    d_in = torch.from_numpy(q).cuda()
    sentinel = complex(-7.25, 1234.5)
    d_out = torch.full((n_ch + 1, n_out + 4), sentinel, dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    with pkg.Searcher(0) as s:
        s.channelize_rational(d_in.data_ptr(), pkg.FMT_IQ_S8, n_in, fs_in, up, down, shifts, d_out.data_ptr(), n_out)
        s.sync()
    flat = d_out.cpu().numpy().reshape(-1)
    y, guard = flat[:n_ch * n_out].reshape(n_ch, n_out), flat[n_ch * n_out:]
    assert guard.size == n_out + 4 * (n_ch + 1) and (guard == np.complex64(sentinel)).all(), np.flatnonzero(guard != np.complex64(sentinel))[:8]
    ratios = _worst(y, ref)
    print(f"rational channelizer s8 2/3, {n_ch} carriers: worst ratio = {max(ratios):.3e}; "
          f"max|gpu - twin| / max|y_ref| = {_against_twin(pkg, y, q, 's8', n_in, fs_in, up, down, shifts, n_out, ref):.3e}")
    assert max(ratios) <= RTOL, ratios


@pytest.mark.parametrize("n_out", [1, 126])
def test_fewer_outputs_than_residues(pkg, n_out):
    """127/128 with n_out = 1 and n_out = up - 1: most tiles of the only workgroup have no output at all."""
    up, down = 127, 128
    fs_in, n_in = FS_OUT * down / up, RR.n_in_min(n_out, up, down)
    shifts = _shifts17(fs_in)
    q, xq = R.quantise(_noise_and_tones(127 + n_out, n_in, fs_in), "s16")
    ref = RR.channelize_rate_ref(xq, fs_in, up, down, shifts, n_out)
    with pkg.Searcher(0) as s:
        y = _run(s, q, pkg.FMT_IQ_S16, n_in, fs_in, up, down, shifts, n_out)
    ratios = _worst(y, ref)
    print(f"rational channelizer s16 127/128, n_out = {n_out}: worst ratio = {max(ratios):.3e}; "
          f"max|gpu - twin| / max|y_ref| = {_against_twin(pkg, y, q, 's16', n_in, fs_in, up, down, shifts, n_out, ref):.3e}")
    assert max(ratios) <= RTOL, ratios


def test_a_non_finite_sample_spoils_its_padded_windows_only(pkg):
    """include/lcs.h, lcs_channelize_rational: 3/4, c64, one Inf in mid-capture.  Outputs whose padded window [s, s + 4 G) does not hold
    the sample are finite and within the bar; outputs whose taps meet it are non-finite; the positions between are unconstrained
    (0 * Inf at a zero tap).  The host twin meets the same rule in tests/test_channelizer_rate_twin_host.py."""
    x, n_in, fs_in, shifts, n_out, clean, dirty = T.nonfinite_case()
    with np.errstate(invalid="ignore", over="ignore"):
        ref = RR.channelize_rate_ref(x.astype(np.complex128), fs_in, 3, 4, shifts, n_out)
    with pkg.Searcher(0) as s:
        y = _run(s, x, pkg.FMT_C64, n_in, fs_in, 3, 4, shifts, n_out)
    worst = T.check_nonfinite(y, ref, clean, dirty, RTOL)
    print(f"rational channelizer c64 3/4 with one Inf sample: worst ratio over the {int(clean.sum())} clean outputs = {worst:.3e}")


def test_full_length_capture_keeps_its_phase_to_the_last_sample(pkg):
    """80 ms at 20 Msps: sample 1.6 M.  An fp32 phase (or an fp32 running product) is wrong by radians there."""
    up, down, n_out, tail = 12, 125, 153584, 2048
    fs_in, n_in = 20e6, 1600000
    shifts = np.array([1234567.8, -8.9e6, 100e3, 0.45 * fs_in])
    q, xq = R.quantise(_noise_and_tones(7, n_in, fs_in), "s16")
    ref = RR.channelize_rate_ref(xq, fs_in, up, down, shifts, tail, m_first=n_out - tail)
    with pkg.Searcher(0) as s:
        y = _run(s, q, pkg.FMT_IQ_S16, n_in, fs_in, up, down, shifts, n_out)[:, n_out - tail:]
    ratios = _worst(y, ref)
    print(f"rational channelizer full length: worst ratio over the last {tail} outputs = {max(ratios):.3e}")
    assert max(ratios) <= RTOL, ratios


def test_up_1_is_the_integer_channelizer_byte_for_byte(pkg):
    import torch
    D, n_out = 8, 4099
    fs_in, n_in = D * FS_OUT, (n_out - 1) * D + 16 * D
    shifts = _shifts17(fs_in)
    q, _ = R.quantise(_noise_and_tones(81, n_in, fs_in), "s16")
    d_in = torch.from_numpy(q).cuda()
    outs = [torch.zeros((17, n_out), dtype=torch.complex64, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    with pkg.Searcher(0) as s:
        s.channelize(d_in.data_ptr(), pkg.FMT_IQ_S16, n_in, fs_in, D, shifts, outs[0].data_ptr(), n_out)
        s.channelize_rational(d_in.data_ptr(), pkg.FMT_IQ_S16, n_in, fs_in, 1, D, shifts, outs[1].data_ptr(), n_out)
        s.sync()
    a, b = (o.cpu().numpy() for o in outs)
    assert np.abs(a).max() > 0
    assert a.tobytes() == b.tobytes()


def test_bad_arguments_are_refused_and_leave_the_context_usable(pkg):
    import torch
    up, down, n_out, n_ch = 3, 4, 512, 3
    fs_in, n_in = FS_OUT * down / up, RR.n_in_min(512, 3, 4)
    q, xq = R.quantise(_noise_and_tones(3, n_in, fs_in), "s16")
    d_in = torch.from_numpy(q).cuda()
    d_out = torch.zeros((n_ch, n_out + 4), dtype=torch.complex64, device="cuda")
    shifts = np.array([0.0, 250e3, -1.0e6])
    L = pkg.capi.load()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    with pkg.Searcher(0) as s:
        good = dict(wide=d_in.data_ptr(), fmt=pkg.FMT_IQ_S16, n_in=n_in, fs=fs_in, up=up, down=down, f=shifts, n_ch=n_ch, out=d_out.data_ptr(), n_out=n_out)

        def call(**kw):
            a = dict(good, **kw)
            f = a["f"]
            return L.lcs_channelize_rational(s._h, C.c_void_p(a["wide"]), a["fmt"], a["n_in"], a["fs"], a["up"], a["down"],
                                             dp(f) if f is not None else None, a["n_ch"], C.c_void_p(a["out"]), a["n_out"])

        cases = dict(rate_25_16=dict(up=25, down=16), rate_1_17=dict(up=1, down=17), rate_1_129=dict(up=1, down=129), rate_6_8=dict(up=6, down=8),
                     rate_4_4=dict(up=4, down=4), rate_7_113=dict(up=7, down=113), up_0=dict(up=0), short_capture=dict(n_in=n_in - 1),
                     shift_beyond_nyquist=dict(f=np.array([0.0, 0.5 * fs_in + 1.0, 0.0])), unknown_fmt=dict(fmt=pkg.FMT_IQ_U8),
                     misaligned_out=dict(out=d_out.data_ptr() + 8), null_wide=dict(wide=None), null_shift=dict(f=None), null_out=dict(out=None),
                     no_channel=dict(n_ch=0))
        for name, kw in cases.items():
            assert call(**kw) == -2, name
            assert L.lcs_last_error(s._h).decode().strip(), name
            assert call() == 0, f"a valid call after {name}"
        assert L.lcs_channelize_rational(None, C.c_void_p(good["wide"]), good["fmt"], n_in, fs_in, up, down, dp(shifts), n_ch, C.c_void_p(good["out"]),
                                         n_out) == -2
        s.sync()
        y = d_out.cpu().numpy().reshape(-1)[:n_ch * n_out].reshape(n_ch, n_out)
        ref = RR.channelize_rate_ref(xq, fs_in, up, down, shifts, n_out)
        assert max(_worst(y, ref)) <= RTOL


def test_contexts_give_the_channelizer_memory_back(pkg):
    """Twelve create / channelize_rational (different rates, ~2000 carriers) / destroy cycles return the device's free memory to where
    it started, after tests/test_gpu_channelizer.py.  The filter bank a context grows is 2 MB (3/4) to 73 MB (96/125)."""
    import torch
    n_out = 256
    rates = ((12, 125), (3, 4), (24, 125), (8, 25), (15, 16), (96, 125))
    n_max = max(RR.n_in_min(n_out, u, d) for u, d in rates)
    q, _ = R.quantise(_noise_and_tones(11, n_max, 20e6), "s16")
    d_in = torch.from_numpy(q).cuda()
    d_out = torch.zeros((2100, n_out), dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()

    def one(k):
        (up, down), n_ch = rates[k % 6], 2000 + 7 * k
        fs_in = FS_OUT * down / up
        with pkg.Searcher(0) as s:
            s.channelize_rational(d_in.data_ptr(), pkg.FMT_IQ_S16, n_max, fs_in, up, down, np.linspace(-0.4, 0.4, n_ch - 900) * fs_in, d_out.data_ptr(), n_out)
            s.channelize_rational(d_in.data_ptr(), pkg.FMT_IQ_S16, n_max, fs_in, up, down, np.linspace(-0.4, 0.4, n_ch) * fs_in, d_out.data_ptr(), n_out)
            s.sync()

    one(0)                                  # first use pays for one-off allocations of the runtime itself
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for k in range(1, 13):
        one(k)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert abs(free1 - free0) < 16 << 20, (free0, free1)


@pytest.fixture(scope="module")
def wbr(pkg):
    """The 20 Msps capture of tests/test_channelizer_rate_host.py (tests/chan_rate_ref.py: WBR), on the device."""
    import torch
    iq, x, _ = RR.wbr_capture(pkg)
    return dict(iq=iq, x=x, d=torch.from_numpy(iq).cuda(), n_in=iq.size // 2, fs_in=RR.WBR_FS_IN, up=RR.WBR["up"], down=RR.WBR["down"],
                n_out=RR.WBR["n_out"], carriers=RR.wbr_carriers())


def test_band_search_from_one_20_msps_capture_matches_the_oracle(pkg, wbr):
    """sweep.search_wideband(rate=(12, 125)) on the capture, against the oracle's chain on the float64 channelizer's output, carrier by
    carrier.  n_out is left to search_wideband: the most the capture holds."""
    import oracle as O
    O.set_threads(min(8, __import__("os").cpu_count() or 1))
    ref = RR.channelize_rate_ref(wbr["x"], wbr["fs_in"], wbr["up"], wbr["down"], wbr["carriers"] - RR.WBR["fc_centre"], wbr["n_out"],
                                 taps=pkg.channelizer_proto(wbr["down"]))
    with pkg.Searcher(0) as s:
        got = pkg.sweep.search_wideband(s, wbr["d"].data_ptr(), pkg.FMT_IQ_S16, wbr["n_in"], wbr["fs_in"], 0, RR.WBR["fc_centre"], wbr["carriers"],
                                        RR.WBR_GRID, chunk=2, rate=(wbr["up"], wbr["down"]))      # two chunks: the buffer is reused
    n_planted = len(RR.WBR_PLACED)
    assert RR.WBR_GRID.size == 5
    for k, fc in enumerate(wbr["carriers"]):
        want, _ = O.search_capbuf(ref[k], RR.WBR_GRID, fc, fc, FS_OUT)
        assert [R.cell_key(c) for c in got[k]] == [R.cell_key(c) for c in want], fc
        for a, b in zip(got[k], want):
            assert abs(a.freq_superfine - b.freq_superfine) < 1e-3, (fc, a.freq_superfine, b.freq_superfine)
        assert (len(got[k]) == 1) if k < n_planted else (got[k] == []), (fc, got[k])
    ids = [got[k][0].n_id_cell() for k in range(n_planted)]
    assert ids == [cells[0]["n_id_2"] + 3 * cells[0]["n_id_1"] for _, cells in RR.WBR_PLACED]


def test_a_batch_enqueued_behind_the_rational_channelizer_is_ordered_behind_it(pkg, wbr):
    """channelize_rational immediately followed by batch_enqueue on the same context, no sync between: records byte-identical to the
    same two calls with a sync between them."""
    import torch
    n_ch = len(wbr["carriers"])
    recs = []
    for with_sync in (True, False):
        buf = torch.zeros((n_ch, wbr["n_out"]), dtype=torch.complex64, device="cuda")
        torch.cuda.synchronize()
        with pkg.Searcher(0) as s:
            s.channelize_rational(wbr["d"].data_ptr(), pkg.FMT_IQ_S16, wbr["n_in"], wbr["fs_in"], wbr["up"], wbr["down"],
                                  wbr["carriers"] - RR.WBR["fc_centre"], buf.data_ptr(), wbr["n_out"])
            if with_sync:
                s.sync()
            s.batch_enqueue(buf.data_ptr(), pkg.FMT_C64, n_ch, wbr["n_out"], RR.WBR_GRID, wbr["carriers"], wbr["carriers"], FS_OUT, pkg.STAGE_FULL)
            rec, cnt = s.batch_collect_raw(n_ch)
        recs.append((rec.tobytes(), cnt.tobytes(), int(cnt.sum())))
    assert recs[0][2] == len(RR.WBR_PLACED)
    assert recs[0][0] == recs[1][0] and recs[0][1] == recs[1][1]
