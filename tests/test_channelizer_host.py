"""CPU-side checks of the wideband channelizer: its filter (lcs_channelizer_taps) against the rule of include/lcs.h, and the
wideband fixture (synth.make_wideband) through the float64 restatement of the channelizer and the oracle's searcher."""
import ctypes as C

import numpy as np
import pytest

import chan_ref as R
import oracle as O
from conftest import load_pkg

FS_OUT = 1.92e6


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.mark.parametrize("D", [2, 3, 4, 8, 10, 16])
def test_taps_follow_the_rule_and_meet_the_filter_spec(pkg, D):
    h = pkg.channelizer_taps(D)
    assert h.shape == (16 * D,)
    assert np.abs(h - R.taps_ref(D)).max() <= 1e-15
    assert abs(h.sum() - 1.0) <= 1e-15
    n_fft = 1 << 18
    H = np.abs(np.fft.fft(h, n_fft))
    f = np.fft.fftfreq(n_fft, 1.0 / (D * FS_OUT))
    pb = 20 * np.log10(H[np.abs(f) <= 0.66e6])
    sb = 20 * np.log10(np.maximum(H[np.abs(f) >= 1.26e6], 1e-300))
    print(f"D={D}: passband ripple {pb.max() - pb.min():.4f} dB, stopband {sb.max():.2f} dB")
    assert pb.max() - pb.min() <= 0.005
    assert sb.max() <= (-71.0 if D == 2 else -75.0 if D == 3 else -78.0)


def test_taps_refuse_bad_arguments(pkg):
    L = pkg.capi.load()
    buf = np.zeros(16 * 17)
    dp = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert L.lcs_channelizer_taps(1, dp) == -2
    assert L.lcs_channelizer_taps(17, dp) == -2
    assert L.lcs_channelizer_taps(8, None) == -2
    assert L.lcs_channelizer_taps(8, dp) == 0
    with pytest.raises(pkg.SearcherError):
        pkg.channelizer_taps(1)


def test_wideband_fixture_is_sound_without_a_gpu(pkg):
    """make_wideband at D = 8, s16 (tests/chan_ref.py: WB) through channelize_ref, then the oracle's full chain per carrier on a
    three-point grid around the planted offset: every planted identity is decoded on its carrier, nothing on the empty carriers
    and nothing on the carrier 1.92 MHz above the cell that is 40 dB stronger than the noise (its alias)."""
    O.set_threads(min(8, __import__("os").cpu_count() or 1))
    iq, x, truth = R.wb_capture(pkg)
    D, n_out = R.WB["decim"], R.WB["n_out"]
    assert iq.dtype == np.int16 and iq.size == 2 * 153600 * D and np.abs(iq).max() < 32767      # the AGC leaves headroom
    assert [c for c, _ in truth] == [c for c, _ in R.WB_PLACED]
    carriers = R.wb_carriers()
    y = R.channelize_ref(x, D * FS_OUT, D, carriers - R.WB["fc_centre"], n_out, taps=pkg.channelizer_taps(D))
    planted = {c: cells[0] for c, cells in R.WB_PLACED}
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
