"""The wideband channelizer on the GPU (lcs_channelize) against its float64 restatement (tests/chan_ref.py)."""
import ctypes as C

import numpy as np
import pytest

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


def _noise_and_tones(seed, n_in, fs_in):
    rng = np.random.default_rng(seed)
    x = 0.1 * (rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in))
    n = np.arange(n_in, dtype=np.float64)
    for f, a in ((0.013e6, 0.2), (-0.31e6, 0.15), (0.21 * fs_in, 0.25), (-0.449 * fs_in, 0.2)):
        x += a * np.exp(2j * np.pi * (f / fs_in) * n + 1j * rng.uniform(0, 2 * np.pi))
    return x


def _run(pkg, s, q, fmt, n_in, fs_in, D, shifts, n_out):
    import torch
    d_in = torch.from_numpy(q).cuda()
    d_out = torch.zeros((len(shifts), n_out), dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    s.channelize(d_in.data_ptr(), fmt, n_in, fs_in, D, shifts, d_out.data_ptr(), n_out)
    s.sync()
    return d_out.cpu().numpy()


def _arrays_match(pkg, fmt, D, n_out):
    fs_in = D * FS_OUT
    n_in = (n_out - 1) * D + 16 * D          # exactly what "valid" mode needs: the last window ends on the last sample
    shifts = np.array([0.0, 100e3, -100e3, 1234567.8, -987654.3, 0.45 * fs_in, -0.45 * fs_in, 0.5 * fs_in, 333333.3])
    q, xq = R.quantise(_noise_and_tones(100 * D + len(fmt), n_in, fs_in), fmt)
    ref = R.channelize_ref(xq, fs_in, D, shifts, n_out)
    with pkg.Searcher(0) as s:
        y = _run(pkg, s, q, _fmt(pkg, fmt), n_in, fs_in, D, shifts, n_out)
        assert s.last_channelize_ms() > 0
    ratios = [float(np.abs(y[k] - ref[k]).max() / np.abs(ref[k]).max()) for k in range(len(shifts))]
    print(f"channelizer {fmt} D={D} n_out={n_out}: worst max|y - y_ref| / max|y_ref| per channel = {max(ratios):.3e}")
    assert max(ratios) <= RTOL, ratios


@pytest.mark.parametrize("D", [2, 8, 16])
@pytest.mark.parametrize("fmt", ["s8", "s16", "c64"])
def test_arrays_match_the_double_reference(pkg, fmt, D):
    _arrays_match(pkg, fmt, D, 4096)


@pytest.mark.parametrize("D", range(2, 17))
def test_every_decimation_matches_the_double_reference(pkg, D):
    """s16, every D the integer kernel takes, one workgroup of 256 outputs plus one output."""
    _arrays_match(pkg, "s16", D, 257)


def test_full_length_capture_keeps_its_phase_to_the_last_sample(pkg):
    """80 ms at 30.72 Msps: sample 2.4 M.  An fp32 phase (or an fp32 running product) is wrong by radians there."""
    D, n_out, tail = 16, 153584, 2048
    fs_in, n_in = D * FS_OUT, 153600 * D
    shifts = np.array([1234567.8, -13.7e6, 100e3, 0.45 * fs_in])
    q, xq = R.quantise(_noise_and_tones(7, n_in, fs_in), "s16")
    ref = R.channelize_ref(xq, fs_in, D, shifts, tail, m_first=n_out - tail)
    with pkg.Searcher(0) as s:
        y = _run(pkg, s, q, pkg.FMT_IQ_S16, n_in, fs_in, D, shifts, n_out)[:, n_out - tail:]
    ratios = [float(np.abs(y[k] - ref[k]).max() / np.abs(ref[k]).max()) for k in range(len(shifts))]
    print(f"channelizer full length: worst ratio over the last {tail} outputs = {max(ratios):.3e}")
    assert max(ratios) <= RTOL, ratios


def test_bad_arguments_are_refused_and_leave_the_context_usable(pkg):
    import torch
    D, n_out, n_ch = 4, 512, 3
    fs_in, n_in = D * FS_OUT, (512 - 1) * 4 + 64
    q, xq = R.quantise(_noise_and_tones(3, n_in, fs_in), "s16")
    d_in = torch.from_numpy(q).cuda()
    d_out = torch.zeros((n_ch, n_out + 4), dtype=torch.complex64, device="cuda")
    shifts = np.array([0.0, 250e3, -1.0e6])
    L = pkg.capi.load()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    with pkg.Searcher(0) as s:
        good = dict(wide=d_in.data_ptr(), fmt=pkg.FMT_IQ_S16, n_in=n_in, fs=fs_in, D=D, f=shifts, n_ch=n_ch, out=d_out.data_ptr(), n_out=n_out)

        def call(**kw):
            a = dict(good, **kw)
            f = a["f"]
            return L.lcs_channelize(s._h, C.c_void_p(a["wide"]), a["fmt"], a["n_in"], a["fs"], a["D"], dp(f) if f is not None else None, a["n_ch"],
                                    C.c_void_p(a["out"]), a["n_out"])

        cases = dict(null_wide=dict(wide=None), null_shift=dict(f=None), null_out=dict(out=None), decim_1=dict(D=1), decim_17=dict(D=17),
                     no_channel=dict(n_ch=0), short_capture=dict(n_in=n_in - 1), shift_beyond_nyquist=dict(f=np.array([0.0, 0.5 * fs_in + 1.0, 0.0])),
                     negative_shift_beyond=dict(f=np.array([-0.51 * fs_in, 0.0, 0.0])), unknown_fmt=dict(fmt=pkg.FMT_IQ_U8), unknown_fmt_9=dict(fmt=9),
                     misaligned_out=dict(out=d_out.data_ptr() + 8))
        for name, kw in cases.items():
            assert call(**kw) == -2, name
            assert L.lcs_last_error(s._h).decode().strip(), name
            assert call() == 0, f"a valid call after {name}"
        assert L.lcs_channelize(None, C.c_void_p(good["wide"]), good["fmt"], n_in, fs_in, D, dp(shifts), n_ch, C.c_void_p(good["out"]), n_out) == -2
        s.sync()
        y = d_out.cpu().numpy().reshape(-1)[:n_ch * n_out].reshape(n_ch, n_out)
        ref = R.channelize_ref(xq, fs_in, D, shifts, n_out)
        assert max(np.abs(y[k] - ref[k]).max() / np.abs(ref[k]).max() for k in range(n_ch)) <= RTOL


def test_contexts_give_the_channelizer_memory_back(pkg):
    """Twelve create / channelize (different n_ch, D) / destroy cycles return the device's free memory to where it started, in the manner
    of tests/test_gpu_world8.py::test_contexts_give_their_memory_back.  ~2000 carriers: the filter bank a context grows is 1 MB (D = 2)
    to 8 MB (D = 16), 46 MB over the twelve cycles if it stayed behind."""
    import torch
    n_out = 256
    x = _noise_and_tones(11, (n_out - 1) * 16 + 256, 16 * FS_OUT)
    q, _ = R.quantise(x, "s16")
    d_in = torch.from_numpy(q).cuda()
    d_out = torch.zeros((2100, n_out), dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()

    def one(k):
        D, n_ch = (2, 3, 5, 8, 12, 16)[k % 6], 2000 + 7 * k
        with pkg.Searcher(0) as s:
            s.channelize(d_in.data_ptr(), pkg.FMT_IQ_S16, x.size, D * FS_OUT, D, np.linspace(-0.4, 0.4, n_ch - 900) * D * FS_OUT, d_out.data_ptr(), n_out)
            s.channelize(d_in.data_ptr(), pkg.FMT_IQ_S16, x.size, D * FS_OUT, D, np.linspace(-0.4, 0.4, n_ch) * D * FS_OUT, d_out.data_ptr(), n_out)
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
def wb(pkg):
    """The wideband capture of tests/test_channelizer_host.py (tests/chan_ref.py: WB), on the device."""
    import torch
    iq, x, _ = R.wb_capture(pkg)
    return dict(iq=iq, x=x, d=torch.from_numpy(iq).cuda(), n_in=iq.size // 2, fs_in=R.WB["decim"] * FS_OUT, D=R.WB["decim"], n_out=R.WB["n_out"],
                carriers=R.wb_carriers())


def test_band_search_from_one_wideband_capture_matches_the_oracle(pkg, wb):
    """sweep.search_wideband on the capture, against the oracle's chain on the float64 channelizer's output, carrier by carrier."""
    import oracle as O
    O.set_threads(min(8, __import__("os").cpu_count() or 1))
    ref = R.channelize_ref(wb["x"], wb["fs_in"], wb["D"], wb["carriers"] - R.WB["fc_centre"], wb["n_out"], taps=pkg.channelizer_taps(wb["D"]))
    with pkg.Searcher(0) as s:
        got = pkg.sweep.search_wideband(s, wb["d"].data_ptr(), pkg.FMT_IQ_S16, wb["n_in"], wb["fs_in"], wb["D"], R.WB["fc_centre"], wb["carriers"],
                                        R.WB_GRID, n_out=wb["n_out"], chunk=4)      # two chunks: the buffer is reused
    n_planted = len(R.WB_PLACED)
    for k, fc in enumerate(wb["carriers"]):
        want, _ = O.search_capbuf(ref[k], R.WB_GRID, fc, fc, FS_OUT)
        assert [R.cell_key(c) for c in got[k]] == [R.cell_key(c) for c in want], fc
        for a, b in zip(got[k], want):
            assert abs(a.freq_superfine - b.freq_superfine) < 1e-3, (fc, a.freq_superfine, b.freq_superfine)
        assert (len(got[k]) == 1) if k < n_planted else (got[k] == []), (fc, got[k])
    ids = [got[k][0].n_id_cell() for k in range(n_planted)]
    assert ids == [cells[0]["n_id_2"] + 3 * cells[0]["n_id_1"] for _, cells in R.WB_PLACED]


def test_a_batch_enqueued_behind_the_channelizer_is_ordered_behind_it(pkg, wb):
    """channelize immediately followed by batch_enqueue on the same context, no sync between: records byte-identical to the same
    two calls with a sync between them."""
    import torch
    n_ch = len(wb["carriers"])
    recs = []
    for with_sync in (True, False):
        buf = torch.zeros((n_ch, wb["n_out"]), dtype=torch.complex64, device="cuda")
        torch.cuda.synchronize()
        with pkg.Searcher(0) as s:
            s.channelize(wb["d"].data_ptr(), pkg.FMT_IQ_S16, wb["n_in"], wb["fs_in"], wb["D"], wb["carriers"] - R.WB["fc_centre"], buf.data_ptr(), wb["n_out"])
            if with_sync:
                s.sync()
            s.batch_enqueue(buf.data_ptr(), pkg.FMT_C64, n_ch, wb["n_out"], R.WB_GRID, wb["carriers"], wb["carriers"], FS_OUT, pkg.STAGE_FULL)
            rec, cnt = s.batch_collect_raw(n_ch)
        recs.append((rec.tobytes(), cnt.tobytes(), int(cnt.sum())))
    assert recs[0][2] == len(R.WB_PLACED)
    assert recs[0][0] == recs[1][0] and recs[0][1] == recs[1][1]
