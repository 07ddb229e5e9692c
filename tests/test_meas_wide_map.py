"""The timing map of sweep.measure_wideband (sweep.map_frame_start), on the CPU alone.

A noise-free single-path cell of synth.make_wideband_cell in a 30.72 Msps capture (K = 16) is channelized by the channelizer's numpy
twin (tests/chan_ref.py) both ways: decim 16 for the search and decim 16 / R for the measurement, R in {2, 8}.  The cell's true frame
start in the search buffer follows from the generator (the wide sample of the frame boundary read through the filter's centre,
include/lcs.h: lcs_channelize); the map takes it into the measurement buffer.  Both buffers are measured by the numpy rule
(tests/meas_wide_ref.py) and the residual timing read from arg A_0, -arg n_fft / (2 pi 6) samples: the wide one must be the narrow
one's times R.  A half-input-sample error in the map is 0.5 / D_m measurement samples: 0.25 at D_m = 2 (R = 8).

Measured here with the correct map: |t_wide - R t_narrow| = 2.4e-3 (R = 2) and 2.11e-2 (R = 8) measurement-rate samples.  The wide
residual itself is 1e-3 and 1e-4; what is left is the narrow one (2e-3 to 3e-3 samples at 1.92 Msps, the search filter's droop over
the 72 subcarriers read as a slope) times R.  The bar is twice the larger, 0.042 -- below the ceiling of 0.1 --, and a map that is
half a capture sample off misses it at both rates: by 0.0625 at D_m = 8 and by 0.25 at D_m = 2."""
import numpy as np
import pytest

import chan_ref as CR
import meas_wide_ref as WR
from conftest import load_pkg

FS = 1.92e6
K = 16
FC_CENTRE = 2.0e9
CARRIER = FC_CENTRE + 0.7e6
T0 = 19000.25                  # nominal 1.92 Msps samples into the frame at the capture's first sample
N_NB = 28800                   # 15 ms
BAR = 0.042


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def narrow_and_capture(pkg):
    out = {}
    for R in (2, 8):
        cell = dict(n_id_1=77, n_id_2=1, n_ports=1, t0=T0, port_gains=[1.0], sfn0=4)
        x, truth, _ = pkg.synth.make_wideband_cell(3, FC_CENTRE, K, [(CARRIER, R, WR.MAX_RB_OF_R[R], cell)], snr_db=None, n_in=N_NB * K)
        x = x.astype(np.complex128)
        out[R] = x
    return out


def _timings(pkg, x, R, shift_wide=0.0):
    """-> (narrow residual timing in 1.92 Msps samples, wide residual timing in measurement-rate samples); shift_wide: an error planted
    in the map, in samples of the capture"""
    fs_in, D_s, D_m = FS * K, K, K // R
    n_id, n_rb = 77 * 3 + 1, WR.MAX_RB_OF_R[R]
    nb = CR.channelize_ref(x, fs_in, D_s, [CARRIER - FC_CENTRE], (x.size - 16 * D_s) // D_s + 1)[0]
    wb = CR.channelize_ref(x, fs_in, D_m, [CARRIER - FC_CENTRE], (x.size - 16 * D_m) // D_m + 1)[0]
    # the frame boundary behind the capture's start lies (19200 - T0) nominal samples in: that wide sample, read through the search filter
    wide = (19200.0 - T0) * K
    fs_search = (wide - (16 * D_s - 1) / 2) / D_s
    fs_meas = pkg.sweep.map_frame_start(fs_search, D_s, D_m) + shift_wide / D_m
    assert abs((fs_meas - shift_wide / D_m) * D_m + (16 * D_m - 1) / 2 - wide) < 1e-6
    n_ofdm = 40                # 20 reference rows from the frame boundary on
    rn = WR.measure_capture(nb, n_id, 1, 1, fs_search, 0.0, CARRIER, CARRIER, FS, 128, 6, n_ofdm)
    rw = WR.measure_capture(wb, n_id, 1, 1, fs_meas, 0.0, CARRIER, CARRIER, FS * R, 128 * R, n_rb, n_ofdm)
    assert rn["status"] == 0 and rw["status"] == 0
    return WR.timing_of(rn["A"][0], 128), WR.timing_of(rw["A"][0], 128 * R), rn, rw


@pytest.mark.parametrize("R", [2, 8])
def test_mapped_frame_start_keeps_the_residual_timing(pkg, narrow_and_capture, R):
    x = narrow_and_capture[R]
    tn, tw, rn, rw = _timings(pkg, x, R)
    print("R = %d: narrow residual %.4f samples, wide %.4f = %.4f narrow samples; |t_w - R t_n| = %.2e" % (R, tn, tw, tw / R, abs(tw - R * tn)))
    assert abs(tw - R * tn) <= BAR
    # both see the same cell: a bin of the 128 R-point grid holds R times the power of a bin at 1.92 Msps (the units are the buffer's
    # power per sample, and the same signal fills 1 / R of the bins)
    assert abs(WR.db(rw["rsrp_rb"][0][rw["n_rb"] // 2] / (R * rn["rsrp"][0]))) < 0.05
    # half a sample of the capture in the map shows as 0.5 / D_m measurement samples, either way, and the bar catches it
    for half in (0.5, -0.5):
        _, tw_bad, _, _ = _timings(pkg, x, R, half)
        print("   map off by %+.1f capture samples: t_w - R t_n = %+.4f (0.5 / D_m = %.4f)" % (half, tw_bad - R * tn, 0.5 * R / K))
        assert abs((tw_bad - R * tn) - half * R / K) <= BAR and abs(tw_bad - R * tn) > BAR


def test_map_is_the_filters_centres(pkg):
    m = pkg.sweep.map_frame_start
    assert m(100.0, 16, 16) == 100.0
    assert m(100.0, 16, 2) == (100.0 * 16 + 127.5 - 15.5) / 2
    assert m(100.0, 16, 1) == 100.0 * 16 + 127.5
    assert m(0.0, 8, 4) == (63.5 - 31.5) / 4
    assert [pkg.sweep.meas_rate(n) for n in (6, 7, 15, 16, 25, 26, 50, 51, 75, 100)] == [1, 2, 2, 4, 4, 8, 8, 16, 16, 16]
    with pytest.raises(ValueError):
        pkg.sweep.meas_rate(101)
