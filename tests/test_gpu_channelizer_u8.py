"""The 8-bit channelizer output on the GPU (lcs_channelize_u8) against the numpy restatement of its rule (tests/chan_u8_ref.py) on
the float64 channelizers' output.  A code may differ from the reference's by one only inside the ROUNDING BAND: where the
reference's scaled value 2^e * component lies within 1e-5 * max|2^e y_ref| -- the channelizer's standing bound on its float outputs
-- of a half-integer, where that error may carry it across a rounding boundary.  Everywhere else the codes, and every gain, are EQUAL.

What the band rests on, and where it is thin: with the carriers 60 dB apart the fp32 sums of the quietest carriers carry the rounding
noise of the loud tones in the same capture.  The CPU walk of the kernels' arithmetic (tests/chan_rate_twin.py, one fma per k) puts the
float outputs of the three quietest carriers at up to 3.1e-5 (decim 16, s16), 3.8e-5 (decim 16, c64) and 4.4e-5 (12/125) of their own
maximum, above the 1e-5 the band is derived from, and at or below 4.4e-6 everywhere else; the bytes it predicts for all nine array cases
have no difference outside the band.  None of this has run on a GPU yet."""
import ctypes as C
import os

import numpy as np
import pytest

import chan_rate_twin as T
import chan_ref as R
import chan_u8_cases as K
import chan_u8_ref as U
from conftest import load_pkg

pytestmark = pytest.mark.gpu

FS_OUT = 1.92e6


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def _fmt(pkg, name):
    return {"c64": pkg.FMT_C64, "s8": pkg.FMT_IQ_S8, "s16": pkg.FMT_IQ_S16}[name]


def _run(pkg, s, case, n_ch=None):
    """-> (codes uint8 [n_ch][n_out][2], gains float32 [n_ch])"""
    import torch
    f = case["shifts"] if n_ch is None else case["shifts"][:n_ch]
    d_in = torch.from_numpy(np.array(case["q"])).cuda()
    d_out = torch.full((len(f), case["n_out"], 2), 99, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gain = s.channelize_u8(d_in.data_ptr(), _fmt(pkg, case["fmt"]), case["n_in"], case["fs_in"], case["up"], case["down"], f, d_out.data_ptr(),
                           case["n_out"], want_gain=True)
    s.sync()
    return d_out.cpu().numpy(), gain.cpu().numpy()


def _compare(codes, gain, case, what):
    """gains equal; codes equal outside the rounding band, within one inside it.  Prints the share of in-band components that differed."""
    n_ch = codes.shape[0]
    assert np.array_equal(gain.astype(np.float64), case["gain"][:n_ch]), (what, gain, case["gain"])
    ref, z = case["codes"][:n_ch], case["z"][:n_ch]
    finite = np.isfinite(z)
    band = U.rounding_band(np.where(finite, z, 0.0)) & finite
    diff = codes.astype(np.int32) - ref.astype(np.int32)
    n_band, n_diff = int(band.sum()), int((diff != 0).sum())
    print(f"{what}: {n_band} of {band.size} components in the rounding band, {n_diff} of them differ from the reference "
          f"({100.0 * n_diff / max(n_band, 1):.1f} %)")
    assert not (diff[~band] != 0).any(), (what, np.argwhere((diff != 0) & ~band)[:5])
    assert np.abs(diff[band]).max(initial=0) <= 1, what


def _premises(case, what):
    share, margin = K.premises(case)
    assert share < 0.01 and margin >= 0.01, (what, share, margin)
    e = np.log2(case["gain"])
    assert len(set(e)) >= 2, (what, e)


@pytest.mark.parametrize("D,fmt", K.INTEGER)
def test_integer_form_matches_the_reference(pkg, D, fmt):
    """n_out = 257: two workgroups along the outputs, so two power partials per carrier; 17 carriers: two carrier blocks."""
    case = K.arrays_case(1, D, fmt, 257)
    _premises(case, (D, fmt))
    if fmt == "c64":
        assert np.log2(case["gain"]).min() < 0      # the capture scaled by 2^10 needs negative exponents
    with pkg.Searcher(0) as s:
        codes, gain = _run(pkg, s, case)
        assert s.last_channelize_ms() > 0
    _compare(codes, gain, case, f"u8 channelizer {fmt} D={D}")


@pytest.mark.parametrize("up,down", K.RATIONAL)
def test_rational_form_matches_the_reference(pkg, up, down):
    """n_out = 32 NI up + up + 1: one full workgroup, a second nearly empty one, a partial residue cycle."""
    case = K.arrays_case(up, down, "s16", T.corner_n_out(up, down))
    _premises(case, (up, down))
    with pkg.Searcher(0) as s:
        codes, gain = _run(pkg, s, case)
    _compare(codes, gain, case, f"u8 channelizer s16 {up}/{down} n_out={case['n_out']}")


def test_a_burst_clamps_where_the_reference_clamps(pkg):
    case = K.burst_case()
    ref, z = case["codes"], case["z"]
    assert (ref == 0).sum() >= 4 and (ref == 255).sum() >= 4 and np.abs(z).max() > 4 * 128
    delta = 1e-5 * np.abs(z).max()
    assert not (np.abs(z - 128.5) <= delta).any() and not (np.abs(z + 127.5) <= delta).any()      # no value sits on a clamp's edge
    with pkg.Searcher(0) as s:
        codes, gain = _run(pkg, s, case)
    _compare(codes, gain, case, "u8 channelizer burst")
    assert np.array_equal(codes == 0, ref == 0) and np.array_equal(codes == 255, ref == 255)


def test_zero_capture_gives_code_127_and_gain_1(pkg):
    n_out = 257
    case = dict(q=np.zeros(2 * K.n_in_for(n_out, 1, 4), np.int16), n_in=K.n_in_for(n_out, 1, 4), fs_in=4 * FS_OUT, shifts=np.array([0.0, 3e5, -1.1e6]),
                n_out=n_out, up=1, down=4, fmt="s16")
    with pkg.Searcher(0) as s:
        codes, gain = _run(pkg, s, case)
    assert (codes == 127).all() and (gain == 1.0).all()


def test_an_inf_sample_gives_gain_1_and_code_127_where_the_output_is_not_finite(pkg):
    D, n_out, n0 = 2, 257, 200
    fs_in, n_in = D * FS_OUT, K.n_in_for(n_out, 1, D)
    rng = np.random.default_rng(12)
    x = (40.0 * (rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in))).astype(np.complex64)
    x[n0] = np.inf
    f = np.array([0.0, 4.1e5])
    with np.errstate(invalid="ignore", over="ignore"):
        codes_ref, gain_ref, z, y = U.channelize_u8_ref(x.astype(np.complex128), fs_in, 1, D, f, n_out)
    m = np.arange(n_out)
    holds = (m * D <= n0) & (n0 <= m * D + 16 * D - 1)                      # the outputs whose window holds the sample
    assert np.array_equal(~np.isfinite(y), np.broadcast_to(holds, y.shape)) and (gain_ref == 1.0).all()
    case = dict(q=x, n_in=n_in, fs_in=fs_in, shifts=f, n_out=n_out, up=1, down=D, fmt="c64", codes=codes_ref, gain=gain_ref, z=z)
    with pkg.Searcher(0) as s:
        codes, gain = _run(pkg, s, case)
    assert (gain == 1.0).all()
    assert (codes[:, holds] == 127).all()
    _compare(codes, gain, case, "u8 channelizer with an Inf sample")
    assert len(np.unique(codes[:, ~holds])) > 50                            # the finite outputs are coded at gain 1


@pytest.mark.parametrize("n_ch", [1, 16, 31])
def test_odd_rows_and_carrier_counts_write_nothing_else(pkg, n_ch):
    """n_out = 257 is odd: the rows are only 2-byte aligned.  (a) One call for all carriers into the middle of a byte tensor: 32
    guard bytes in front, a guard row and 32 more bytes behind keep their sentinel, and every byte between is the reference's.
    (b) Every carrier on its own into a row with 16 guard bytes in front of and behind it: every guard keeps its sentinel."""
    import torch
    base = K.arrays_case(1, 16, "s16", 257)
    n_out, row = base["n_out"], 2 * base["n_out"]
    f = np.resize(base["shifts"], n_ch)
    d_in = torch.from_numpy(np.array(base["q"])).cuda()
    whole = torch.full((32 + (n_ch + 1) * row + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    slot = 16 + (row + 15) // 16 * 16 + 16                                  # guard, the row rounded up to 16 bytes, guard
    rows = torch.full((n_ch * slot,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pkg.Searcher(0) as s:
        s.channelize_u8(d_in.data_ptr(), pkg.FMT_IQ_S16, base["n_in"], base["fs_in"], 1, 16, f, whole.data_ptr() + 32, n_out)
        for k in range(n_ch):
            s.channelize_u8(d_in.data_ptr(), pkg.FMT_IQ_S16, base["n_in"], base["fs_in"], 1, 16, f[k:k + 1], rows.data_ptr() + k * slot + 16, n_out)
        s.sync()
    w, r = whole.cpu().numpy(), rows.cpu().numpy().reshape(n_ch, slot)
    assert (w[:32] == 0xA5).all() and (w[32 + n_ch * row:] == 0xA5).all()
    assert (r[:, :16] == 0xA5).all() and (r[:, 16 + row:] == 0xA5).all()
    idx = np.resize(np.arange(K.N_CH), n_ch)
    ref = dict(codes=base["codes"][idx], gain=base["gain"][idx], z=base["z"][idx])
    _compare(w[32:32 + n_ch * row].reshape(n_ch, n_out, 2), ref["gain"].astype(np.float32), ref, f"u8 channelizer, {n_ch} odd rows")
    _compare(r[:, 16:16 + row].reshape(n_ch, n_out, 2), ref["gain"].astype(np.float32), ref, f"u8 channelizer, {n_ch} rows on their own")


@pytest.mark.parametrize("up,down", [(1, 16), (3, 4)])
def test_two_calls_give_the_same_bytes(pkg, up, down):
    case = K.arrays_case(up, down, "s16", 257 if up == 1 else T.corner_n_out(up, down))
    with pkg.Searcher(0) as s:
        a = _run(pkg, s, case)
        b = _run(pkg, s, case)
    with pkg.Searcher(0) as s:
        c = _run(pkg, s, case)
    for o in (b, c):
        assert a[0].tobytes() == o[0].tobytes() and a[1].tobytes() == o[1].tobytes()


def test_bad_arguments_are_refused_and_leave_the_context_usable(pkg):
    import torch
    case = K.arrays_case(1, 16, "s16", 257)
    n_out, n_ch = case["n_out"], 3
    d_in = torch.from_numpy(np.array(case["q"])).cuda()
    d_out = torch.zeros((n_ch * 2 * n_out + 64,), dtype=torch.uint8, device="cuda")
    shifts = np.ascontiguousarray(case["shifts"][:n_ch])
    n_in_r = K.n_in_for(n_out, 3, 4)                    # the rational calls read less of the same capture than it holds
    L = pkg.capi.load()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    with pkg.Searcher(0) as s:
        good = dict(wide=d_in.data_ptr(), fmt=pkg.FMT_IQ_S16, n_in=case["n_in"], fs=case["fs_in"], up=1, down=16, n_ch=n_ch, out=d_out.data_ptr(), n_out=n_out)

        def call(**kw):
            a = dict(good, **kw)
            return L.lcs_channelize_u8(s._h, C.c_void_p(a["wide"]), a["fmt"], a["n_in"], a["fs"], a["up"], a["down"], dp(shifts), a["n_ch"],
                                       C.c_void_p(a["out"]), a["n_out"], None)

        cases = dict(null_out=dict(out=None), misaligned_out=dict(out=d_out.data_ptr() + 8), up_equals_down=dict(up=4, down=4), up_above_down=dict(up=5, down=4),
                     ratio_above_16=dict(up=1, down=17), ratio_above_16_rational=dict(up=3, down=49), short_capture=dict(n_in=case["n_in"] - 1),
                     short_capture_rational=dict(up=3, down=4, n_in=n_in_r - 1), no_channel=dict(n_ch=0), u8_as_input=dict(fmt=pkg.FMT_IQ_U8))
        for name, kw in cases.items():
            assert call(**kw) == -2, name
            assert L.lcs_last_error(s._h).decode().strip(), name
            assert call() == 0, f"a valid call after {name}"
        assert call(up=3, down=4, n_in=n_in_r) == 0
        assert call() == 0
        s.sync()
        codes = d_out.cpu().numpy()[:n_ch * 2 * n_out].reshape(n_ch, n_out, 2)
    _compare(codes, case["gain"][:n_ch].astype(np.float32), case, "u8 channelizer after the refusals")


def test_contexts_give_the_u8_channelizer_memory_back(pkg):
    """Twelve create / channelize_u8 (different n_ch, rates) / destroy cycles return the device's free memory to where it started, as
    tests/test_gpu_channelizer.py::test_contexts_give_the_channelizer_memory_back.  ~2000 carriers: the float scratch a context grows
    is 4 MB, its filter bank 1 to 8 MB -- some 100 MB over the twelve cycles if they stayed behind."""
    import torch
    n_out = 256
    case = K.arrays_case(1, 16, "s16", 257)
    d_in = torch.from_numpy(np.array(case["q"])).cuda()
    d_out = torch.zeros((2100, n_out, 2), dtype=torch.uint8, device="cuda")
    n_in = case["n_in"]
    torch.cuda.synchronize()

    def one(k):
        (up, down), n_ch = ((1, 2), (1, 3), (3, 4), (1, 8), (5, 12), (1, 16))[k % 6], 2000 + 7 * k
        assert n_in >= K.n_in_for(n_out, up, down)
        fs_in = FS_OUT * down / up
        with pkg.Searcher(0) as s:
            s.channelize_u8(d_in.data_ptr(), pkg.FMT_IQ_S16, n_in, fs_in, up, down, np.linspace(-0.4, 0.4, n_ch - 900) * fs_in, d_out.data_ptr(), n_out)
            s.channelize_u8(d_in.data_ptr(), pkg.FMT_IQ_S16, n_in, fs_in, up, down, np.linspace(-0.4, 0.4, n_ch) * fs_in, d_out.data_ptr(), n_out, want_gain=True)
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
    """The wideband capture of tests/test_gpu_channelizer.py (tests/chan_ref.py: WB) on the device, and the reference bytes of its
    carriers: chan_u8_ref on the float64 channelizer's output."""
    import torch
    iq, x, _ = R.wb_capture(pkg)
    w = dict(iq=iq, d=torch.from_numpy(iq).cuda(), n_in=iq.size // 2, fs_in=R.WB["decim"] * FS_OUT, D=R.WB["decim"], n_out=R.WB["n_out"],
             carriers=R.wb_carriers())
    y = R.channelize_ref(x, w["fs_in"], w["D"], w["carriers"] - R.WB["fc_centre"], w["n_out"], taps=pkg.channelizer_taps(w["D"]))
    w["codes_ref"], w["gain_ref"], _ = U.quantise_ref(y)
    return w


def _capbuf(codes):
    """bytes [n_out][2] -> the complex128 capture they stand for, the dongle convention (u8 - 127) / 128"""
    c = codes.astype(np.float64)
    return (c[:, 0] - 127.0) / 128.0 + 1j * ((c[:, 1] - 127.0) / 128.0)


def test_band_search_on_bytes_takes_the_int8_route_and_matches_the_oracle(pkg, wb):
    import oracle as O
    import torch
    O.set_threads(min(8, os.cpu_count() or 1))
    n_ch = len(wb["carriers"])
    own = torch.zeros((n_ch, wb["n_out"], 2), dtype=torch.uint8, device="cuda")
    with pkg.Searcher(0) as s:
        got = pkg.sweep.search_wideband(s, wb["d"].data_ptr(), pkg.FMT_IQ_S16, wb["n_in"], wb["fs_in"], wb["D"], R.WB["fc_centre"], wb["carriers"],
                                        R.WB_GRID, n_out=wb["n_out"], chunk=4, out="u8")      # two chunks: the buffer is reused
        assert s.last_xcorr_info()[0] == "k_xcorr_i8x3"
        gain = s.channelize_u8(wb["d"].data_ptr(), pkg.FMT_IQ_S16, wb["n_in"], wb["fs_in"], 1, wb["D"], wb["carriers"] - R.WB["fc_centre"],
                               own.data_ptr(), wb["n_out"], want_gain=True)
        s.sync()
    own = own.cpu().numpy()
    assert np.array_equal(gain.cpu().numpy().astype(np.float64), wb["gain_ref"])
    n_planted = len(R.WB_PLACED)
    for k, fc in enumerate(wb["carriers"]):
        want, _ = O.search_capbuf(_capbuf(wb["codes_ref"][k]), R.WB_GRID, fc, fc, FS_OUT)        # the chain on the REFERENCE bytes
        mine, _ = O.search_capbuf(_capbuf(own[k]), R.WB_GRID, fc, fc, FS_OUT)                    # ... and on the GPU's own
        assert [R.cell_key(c) for c in got[k]] == [R.cell_key(c) for c in want], fc
        assert [R.cell_key(c) for c in got[k]] == [R.cell_key(c) for c in mine], fc
        for a, b in zip(got[k], mine):
            assert abs(a.freq_superfine - b.freq_superfine) < 1e-3, (fc, a.freq_superfine, b.freq_superfine)
        assert (len(got[k]) == 1) if k < n_planted else (got[k] == []), (fc, got[k])
    ids = [got[k][0].n_id_cell() for k in range(n_planted)]
    assert ids == [cells[0]["n_id_2"] + 3 * cells[0]["n_id_1"] for _, cells in R.WB_PLACED]


def test_a_batch_enqueued_behind_channelize_u8_is_ordered_behind_it(pkg, wb):
    """channelize_u8 immediately followed by batch_enqueue on the same context, no sync between: records byte-identical to the same
    two calls with a sync between them."""
    import torch
    n_ch = len(wb["carriers"])
    recs = []
    for with_sync in (True, False):
        buf = torch.zeros((n_ch, wb["n_out"], 2), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with pkg.Searcher(0) as s:
            s.channelize_u8(wb["d"].data_ptr(), pkg.FMT_IQ_S16, wb["n_in"], wb["fs_in"], 1, wb["D"], wb["carriers"] - R.WB["fc_centre"], buf.data_ptr(),
                            wb["n_out"])
            if with_sync:
                s.sync()
            s.batch_enqueue(buf.data_ptr(), pkg.FMT_IQ_U8, n_ch, wb["n_out"], R.WB_GRID, wb["carriers"], wb["carriers"], FS_OUT, pkg.STAGE_FULL)
            rec, cnt = s.batch_collect_raw(n_ch)
        recs.append((rec.tobytes(), cnt.tobytes(), int(cnt.sum())))
    assert recs[0][2] == len(R.WB_PLACED)
    assert recs[0][0] == recs[1][0] and recs[0][1] == recs[1][1]
