"""The numpy restatement of the full-bandwidth measurement (tests/meas_wide_ref.py) held to what is known independently of it:
the oracle's extract_tfg and the narrow rule at R = 1, the Gold sequence, the generator's powers on clean waveforms, a two-path
channel's |H(f)|^2, and a planted SNR.  CPU only: np.fft for the grid, the sums as written."""
import os

import numpy as np
import pytest

import cell_meas_ref as MR
import meas_wide_ref as WR
import oracle as O
import tdd_config_ref as TR
from conftest import load_pkg

FS = 1.92e6
FC = 739e6


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def golden_cell(capbuf_0000):
    """the strongest cell of the golden capture, as the oracle's chain finds it"""
    cap, fc = capbuf_0000
    O.set_legacy(False)
    O.set_threads(min(16, os.cpu_count() or 1))
    cells, _ = O.search_capbuf(cap, np.array([30e3, 35e3, 40e3]), fc, fc, FS)
    assert len(cells) >= 1
    return cells[0]


# ---------------------------------------------------------------- (a) R = 1, n_rb = 6 is extract_tfg and the narrow rule
def test_at_128_points_the_grid_is_extract_tfg_and_the_record_the_narrow_rule(capbuf_0000, golden_cell):
    cap, fc = capbuf_0000
    c = golden_cell
    tfg_o, ts_o = O.extract_tfg(c, cap, fc, fc, FS)
    n_ofdm = tfg_o.shape[0]
    tfg_w, ts_w = WR.grid(cap, c.frame_start, c.freq_fine, c.cp_type, fc, fc, FS, 128, 6, n_ofdm)
    assert np.array_equal(ts_w, ts_o)
    err = np.abs(tfg_w - tfg_o).max() / np.abs(tfg_o).max()
    print("wide grid against the oracle's extract_tfg: %.2e of the largest magnitude" % err)
    assert err <= 1e-10
    n_id = c.n_id_2 + 3 * c.n_id_1
    for mask, ports in ((0x3FF, c.n_ports), (0x021, 1)):
        ref = MR.measure(n_id, c.cp_type, tfg_w, mask, ports)
        got = WR.measure(n_id, c.cp_type, tfg_w, 6, 128, mask, ports)
        assert (got["status"], got["n_rows"], got["n_ports"], got["dl_mask"]) == (ref["status"], ref["n_rows"], ref["n_ports"], ref["dl_mask"]) and ref["status"] == 0
        s, n = ref["sums"], ref["n_rows"]
        for p in range(ref["n_ports"]):
            unit = s["E"][p] / (12 * n)
            assert abs(got["A"][p] - ref["A"][p]) <= 1e-9 * s["scale"]["A"][p]
            assert abs(got["rsrp"][p] - ref["rsrp"][p]) <= 1e-9 * unit and abs(got["noise"][p] - ref["noise"][p]) <= 1e-9 * unit
        assert abs(got["rssi"] - ref["rssi"]) <= 1e-9 * ref["rssi"] and abs(got["rsrq"] - ref["rsrq"]) <= 1e-9 * 6 * (s["E"][0] / (12 * n)) / ref["rssi"]
        # the profile adds up: the RBs' powers are the row's power
        assert abs(got["rssi_rb"].sum() - got["rssi"]) <= 1e-12 * got["rssi"]


# ---------------------------------------------------------------- (b) the reference sequence
def test_reference_sequence_of_n_rb(pkg):
    pn = pkg.synth._pn
    for n_id, cp in ((0, 1), (301, 2), (503, 1)):
        n = TR.n_symb_of(cp)
        rs6, sh6 = WR.rs_wide(n_id, cp, 6)
        rs100, sh100 = WR.rs_wide(n_id, cp, 100)
        rs_o, sh_o = O.rs_dl(n_id, cp)
        for slot in range(20):
            for j, sym in enumerate((0, n - 3)):
                b = 2 * slot + j
                # six resource blocks: the generator's twelve, the oracle's RS_DL row and its shifts, bit for bit
                assert rs6[b].tobytes() == np.ascontiguousarray(pkg.synth._crs(n_id, slot, sym, cp == 1)).tobytes()
                assert rs6[b].tobytes() == np.ascontiguousarray(rs_o[slot * n + sym]).tobytes()
                assert list(sh6[b]) == [int(sh_o[slot * n + sym, 0]), int(sh_o[slot * n + sym, 1])] == list(sh100[b])
                # a hundred: m = 0 is r(10), m = 199 is r(209), straight from the Gold sequence; the centre twelve are the 6 RB sequence
                c_init = (1 << 10) * (7 * (slot + 1) + sym + 1) * (2 * n_id + 1) + 2 * n_id + (1 if cp == 1 else 0)
                c = pn(c_init, 440).astype(np.float64)
                for m, mp in ((0, 10), (199, 209)):
                    assert rs100[b][m] == ((1 - 2 * c[2 * mp]) + 1j * (1 - 2 * c[2 * mp + 1])) / np.sqrt(2.0)
                assert rs100[b][94:106].tobytes() == rs6[b].tobytes()
        for n_rb in (15, 25, 50, 75):
            assert WR.rs_wide(n_id, cp, n_rb)[0][:, n_rb - 6:n_rb + 6].tobytes() == rs6.tobytes()


# ---------------------------------------------------------------- (c) clean waveforms: the generator's powers
PAD = 1000            # samples in front of the frame boundary: frame_start


def _clean(pkg, R, n_rb, gains, cp_normal=True, seed=0):
    w = pkg.synth.cell_waveform_wide(3, 41, 2, R, n_rb, cp_normal, n_ports=len(gains), rng=np.random.default_rng(seed), port_gains=gains)
    return np.concatenate([np.zeros(PAD, np.complex128), w])


@pytest.mark.parametrize("R,n_rb", [(2, 15), (16, 100)])
def test_clean_waveform_gives_the_generators_power_flat_over_the_resource_blocks(pkg, R, n_rb):
    gains = np.array([0.9 * np.exp(0.7j), 1.1 * np.exp(-2.1j)])
    cap = _clean(pkg, R, n_rb, gains)
    rec = WR.measure_capture(cap, 41 * 3 + 2, 1, 2, float(PAD), 0.0, FC, FC, FS * R, 128 * R, n_rb, 280)
    assert rec["status"] == 0 and rec["n_rows"] == 80
    for p in range(2):
        want = abs(gains[p]) ** 2 / 2                    # unit reference elements times port_gains / sqrt(n_ports)
        assert abs(rec["rsrp"][p] - want) <= 1e-9 * want
        assert abs(rec["noise"][p]) <= 1e-9 * rec["rsrp"][p]
        assert np.abs(rec["rsrp_rb"][p] - want).max() <= 1e-9 * want
        # zero timing error: the pair products are real
        assert abs(WR.timing_of(rec["A"][p], 128 * R)) <= 1e-9


# ---------------------------------------------------------------- (d) a two-path channel: the profile follows |H(f)|^2
def test_profile_follows_a_two_path_channel(pkg):
    """A static channel 1 + a delta(t - d), d = 2 samples at R = 4 (0.26 us, the CP is 36): H(k) = 1 + a exp(-2 pi j k d / N) on
    subcarrier k.  Noise-free, rsrp_rb[0][i] n_ports / |g_0|^2 = |sum_r z_r| / n_rows with z_r = H(k_r) conj(H(k_r + 6)), k_r the first
    reference subcarrier of the RB in row r.  The allowed deviation from X = |H(c_i)|^2 at the RB's centre c_i, from the rule:
      * |d|H|^2 / dk| = |2 a sin(theta) 2 pi d / N| <= 4 pi a d / N =: s, and both reference elements lie within 5.5 subcarriers of the
        centre, so each |H|^2 is within delta = 5.5 s of X and so is their geometric mean |z_r|;
      * |d arg H / dk| <= (2 pi d / N) a / (1 - a) =: g, so every z_r lies within an angle 6 g of the real axis and
        |sum z_r| >= cos(6 g) sum |z_r|.
    Hence  (X - delta) cos(6 g) <= value <= X + delta:  the bar is delta + X (1 - cos(6 g)), 0.14 to 0.16 here against a profile that
    swings between 0.25 and 2.25."""
    R, n_rb, d, a, N = 4, 25, 2, 0.5, 512
    g0 = 0.8 * np.exp(1.3j)
    w = _clean(pkg, R, n_rb, np.array([g0]))
    cap = w.copy()
    cap[d:] += a * w[:-d]
    rec = WR.measure_capture(cap, 41 * 3 + 2, 1, 1, float(PAD), 0.0, FC, FC, FS * R, N, n_rb, 280)
    assert rec["status"] == 0
    centre = 12 * np.arange(n_rb) + 5.5 - 6 * n_rb            # in columns; the column's subcarrier number skips 0
    k = np.where(centre < 0, centre, centre + 1)
    X = np.abs(1 + a * np.exp(-2j * np.pi * k * d / N)) ** 2
    s, g = 4 * np.pi * a * d / N, (2 * np.pi * d / N) * a / (1 - a)
    bar = 5.5 * s + X * (1 - np.cos(6 * g))
    got = rec["rsrp_rb"][0] / abs(g0) ** 2
    print("two-path profile: worst deviation %.3f, bar %.3f .. %.3f, profile %.2f .. %.2f" % (np.abs(got - X).max(), bar.min(), bar.max(), X.min(), X.max()))
    assert np.all(np.abs(got - X) <= bar) and X.max() - X.min() > 1.5


# ---------------------------------------------------------------- (e) a planted SNR
SNR_DB = 10.0
SINR_BAR_DB = 2 * 0.32       # twice the worst |sinr_db[0] - SNR_DB| of this reference over seeds 0 .. 19 at this shape (measured: 0.319 dB, seed 8)


def sinr_case(pkg, seed):
    """(R, n_rb) = (2, 15), two frames, two ports, complex white noise SNR_DB below port 0's reference elements"""
    gains = np.array([1.0 * np.exp(0.4j), 0.8 * np.exp(2.0j)])
    cap = _clean(pkg, 2, 15, gains, seed=seed)
    rng = np.random.default_rng(5000 + seed)
    sigma2 = (abs(gains[0]) ** 2 / 2) / 10 ** (SNR_DB / 10)
    cap = cap + np.sqrt(sigma2 / 2) * (rng.standard_normal(cap.size) + 1j * rng.standard_normal(cap.size))
    rec = WR.measure_capture(cap, 41 * 3 + 2, 1, 2, float(PAD), 0.0, FC, FC, FS * 2, 256, 15, 280)
    return WR.db(WR.sinr(rec, 0))


@pytest.mark.parametrize("seed", [0, 8, 19])
def test_sinr_recovers_the_planted_snr(pkg, seed):
    """bound: SINR_BAR_DB, twice the worst deviation of this numpy reference over 20 seeds at the test's shape, measured on the CPU
    as max(abs(sinr_case(pkg, s) - SNR_DB) for s in range(20)): 0.319 dB (seed 8; the median is 0.07 dB) -> 0.64 dB"""
    v = sinr_case(pkg, seed)
    print("seed %d: sinr_db[0] = %.3f for a planted %.1f dB" % (seed, v, SNR_DB))
    assert abs(v - SNR_DB) <= SINR_BAR_DB
