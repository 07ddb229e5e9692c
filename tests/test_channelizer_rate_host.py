"""CPU-side checks of the rational channelizer: its float64 restatement (tests/chan_rate_ref.py) against the integer one on a
zero-stuffed capture, its filter (lcs_channelizer_proto) against the rule of include/lcs.h, and the 20 Msps fixture
(synth.make_wideband_rate) through the restatement and the oracle's searcher."""
import ctypes as C
import math

import numpy as np
import pytest

import chan_rate_ref as RR
import chan_ref as R
import oracle as O
from conftest import load_pkg

FS_OUT = 1.92e6


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.mark.parametrize("up,down", [(12, 125), (15, 16), (3, 4)])
def test_reference_is_the_integer_reference_on_the_zero_stuffed_capture(up, down):
    """up * channelize_ref(x zero-stuffed by up, zero-padded to (n_out-1) down + Tg, up fs_in, down) = channelize_rate_ref(x)."""
    n_out, Tg = 2048, 16 * down
    fs_in = FS_OUT * down / up
    n_in = RR.n_in_min(n_out, up, down)
    rng = np.random.default_rng(1000 * up + down)
    x = rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in)
    shifts = np.array([0.0, 100e3, -0.31 * fs_in, 0.5 * fs_in, 1234567.8 * fs_in / 20e6])
    xu = np.zeros((n_out - 1) * down + Tg, np.complex128)
    xu[np.arange(n_in) * up] = x
    want = up * R.channelize_ref(xu, fs_in * up, down, shifts, n_out)
    got = RR.channelize_rate_ref(x, fs_in, up, down, shifts, n_out)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{up}/{down}: rational reference against the zero-stuffed integer reference: {err:.3e}")
    assert err <= 1e-10
    # a later range of outputs is the same numbers (m_first only moves the window)
    tail = RR.channelize_rate_ref(x, fs_in, up, down, shifts, 301, m_first=n_out - 301)
    assert np.abs(tail - got[:, n_out - 301:]).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("down", [4, 5, 16, 25, 125, 128])
def test_proto_follows_the_rule_and_meets_the_filter_spec_at_the_fine_rate(pkg, down):
    g = pkg.channelizer_proto(down)
    assert g.shape == (16 * down,)
    assert np.abs(g - R.taps_ref(down)).max() <= 1e-15
    # sum 1: every tap is a double divided by the taps' running double sum -- that sum is off by at most Tg roundings of
    # sum|g|, each quotient by half an ulp more -- and fsum adds nothing of its own
    assert abs(math.fsum(g) - 1.0) <= (16 * down + 1) * 2.0 ** -53 * np.abs(g).sum()
    n_fft = 1 << 18
    H = np.abs(np.fft.fft(g, n_fft))
    f = np.fft.fftfreq(n_fft, 1.0 / (down * FS_OUT))
    pb = 20 * np.log10(H[np.abs(f) <= 0.66e6])
    sb = 20 * np.log10(np.maximum(H[np.abs(f) >= 1.26e6], 1e-300))
    print(f"down={down}: passband ripple {pb.max() - pb.min():.4f} dB, stopband {sb.max():.2f} dB")
    assert pb.max() - pb.min() <= 0.005
    assert sb.max() <= -78.0


def test_proto_refuses_bad_arguments(pkg):
    L = pkg.capi.load()
    buf = np.zeros(16 * 129)
    dp = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert L.lcs_channelizer_proto(1, dp) == -2
    assert L.lcs_channelizer_proto(129, dp) == -2
    assert L.lcs_channelizer_proto(125, None) == -2
    assert L.lcs_channelizer_proto(125, dp) == 0
    with pytest.raises(pkg.SearcherError):
        pkg.channelizer_proto(1)
    with pytest.raises(pkg.SearcherError):
        pkg.channelizer_proto(129)


def test_make_wideband_rate_picks_a_narrowband_length_it_can_stuff(pkg):
    s = pkg.synth
    cell = [(740.0e6, [dict(n_id_1=3, n_id_2=0, cp_normal=True, n_ports=1, n_rb_dl=25, f_off=0.0, gain_db=0.0)])]
    iq, _ = s.make_wideband_rate(1, 740.0e6, 15, 16, cell, 10.0, pkg.FMT_IQ_S8, n_in=5000)      # 15 does not divide every length
    assert iq.dtype == np.int8 and iq.size == 2 * 5000
    x, _ = s.make_wideband_rate(1, 740.0e6, 3, 4, cell, 10.0, pkg.FMT_C64, n_in=4001)
    assert x.dtype == np.complex64 and x.size == 4001
    with pytest.raises(ValueError):
        s.make_wideband_rate(1, 740.0e6, 6, 8, cell)
    with pytest.raises(ValueError):
        s.make_wideband_rate(1, 740.0e6, 5, 4, cell)


def test_rate_fixture_is_sound_without_a_gpu(pkg):
    """make_wideband_rate at 12/125 (20 Msps, s16; tests/chan_rate_ref.py: WBR) through channelize_rate_ref, then the oracle's full
    chain per carrier on a three-point grid around the planted offset: every planted identity is decoded on its carrier, nothing on
    the empty carrier and nothing on the carrier 1.92 MHz above the cell that is 40 dB stronger than the noise (its alias)."""
    O.set_threads(min(8, __import__("os").cpu_count() or 1))
    iq, x, truth = RR.wbr_capture(pkg)
    up, down, n_out = RR.WBR["up"], RR.WBR["down"], RR.WBR["n_out"]
    assert iq.dtype == np.int16 and iq.size == 2 * 1600000 and np.abs(iq).max() < 32767      # the AGC leaves headroom
    assert x.size >= RR.n_in_min(n_out, up, down)
    assert [c for c, _ in truth] == [c for c, _ in RR.WBR_PLACED]
    carriers = RR.wbr_carriers()
    y = RR.channelize_rate_ref(x, RR.WBR_FS_IN, up, down, carriers - RR.WBR["fc_centre"], n_out, taps=pkg.channelizer_proto(down))
    planted = {c: cells[0] for c, cells in RR.WBR_PLACED}
    for k, fc in enumerate(carriers):
        cd = planted.get(fc)
        f0 = 5e3 * round(cd["f_off"] / 5e3) if cd else 0.0
        cells, _ = O.search_capbuf(y[k], f0 + np.array([-5e3, 0.0, 5e3]), fc, fc, FS_OUT)
        got = sorted((c.n_id_cell(), c.cp_type, c.n_ports, c.n_rb_dl) for c in cells)
        if cd:
            assert got == [(cd["n_id_2"] + 3 * cd["n_id_1"], 1 if cd["cp_normal"] else 2, cd["n_ports"], cd["n_rb_dl"])], (fc, got)
            assert abs(cells[0].freq_superfine - cd["f_off"]) < 50.0, (fc, cells[0].freq_superfine)
        else:
            assert got == [], (fc, got)
