"""The reference of the unwrapped frequency estimate (tests/pss_coarse_ref.py) on planted TDD cells, on the CPU.

On the reference's 5 kHz hypothesis grid the residual of a cell reaches +- 2500 Hz; the native PSS/SSS estimate of a TDD cell is
unambiguous within +- 2330 Hz (normal CP) / +- 2000 Hz (extended) only, and a cell whose estimate aliased does not decode.  The
PSS-only coarse estimate picks the period.  Peaks come from the oracle, SSS detection and the native estimate from the numpy
restatement in TDD mode (tests/sss_duplex_ref.py), everything behind them from the oracle.

A decision n is RIGHT when it is the whole number of periods between the native estimate and the planted offset:
n_true = rint((f_off - native) / period), which is unambiguous while the native estimate's own error stays below half a period
(its standard deviation is tens of Hz at these SNRs)."""
import os

import numpy as np
import pytest

import oracle as O
import pss_coarse_ref as PC
import sss_duplex_ref as R
import foe_unwrap_cases as K
from conftest import iq_u8_to_capbuf, load_pkg

FS, FC, TDD = K.FS, K.FC, K.TDD


@pytest.fixture(scope="module", autouse=True)
def _oracle_mode():
    O.set_legacy(False)
    O.set_threads(min(16, os.cpu_count() or 1))


@pytest.mark.parametrize("name, snr, cp_normal, f_off, n, native_ok", K.CRAFTED, ids=[c[0] for c in K.CRAFTED])
def test_crafted_cells_on_the_5_khz_grid(name, snr, cp_normal, f_off, n, native_ok):
    r = K.crafted_ref(snr, cp_normal, f_off, mib=True)
    cz, nat, unw = r["coarse"], r["native"], r["unwrapped"]
    period = cz["fs"] / cz["dist"]
    print(name, "hypothesis", r["peak"].freq, "native", nat.freq_fine, "coarse", cz["f_coarse"] + r["peak"].freq, "n", r["n"], "unwrapped", unw.freq_fine)
    assert cz["dist"] == (412 if cp_normal else 480) and period == FS * ((FC - r["peak"].freq) / FC) / cz["dist"]
    assert r["n"] == n
    assert r["n"] == int(np.rint((f_off - nat.freq_fine) / period)), "the decision is the true number of periods"
    assert abs(cz["f_coarse"] + r["peak"].freq - f_off) < period / 2
    if n == 0:
        assert unw.freq_fine == nat.freq_fine, "n = 0 hands the native double on"
    else:
        assert unw.freq_fine == nat.freq_fine + n * period
    if snr >= 10:
        assert abs(unw.freq_fine - f_off) < 100.0, unw.freq_fine
    # the MIB in both modes
    assert (r["mib_native"] is not None) == native_ok
    c = r["mib_unwrapped"]
    assert c is not None, "the cell does not decode with the unwrapped estimate"
    assert (c.n_id_1, c.n_id_2, c.cp_type, c.n_ports, c.n_rb_dl) == (77, 2, 1 if cp_normal else 2, 2, 25)
    assert abs(c.freq_superfine - f_off) < 100.0, c.freq_superfine
    if native_ok:
        assert bytes(r["mib_native"]) == bytes(c), "where nothing aliased the two modes give the same record"


def test_the_cases_the_issue_names_fail_natively():
    fails = {c[0] for c in K.CRAFTED if not c[5]}
    assert {"10 dB normal +2400", "10 dB extended +2400", "10 dB extended -2300"} <= fails


def test_decision_rule_edges():
    fs, dist = FS, 412
    period = fs / dist
    for q, n in ((0.49, 0), (-0.49, 0), (0.51, 1), (-0.51, -1), (1.6, 1), (-1.6, -1), (0.0, 0)):
        native = 1234.5
        f_coarse = (native - 1000.0) + q * period
        assert PC.unwrap_n(native, 1000.0, f_coarse, fs, dist) == n, q
        got = PC.unwrap(native, 1000.0, f_coarse, fs, dist)
        assert got == (native if n == 0 else native + n * period)
    assert PC.unwrap_n(0.0, 0.0, 3000.0, fs, dist, ok=False) == 0
    assert PC.unwrap_n(0.0, 0.0, float("nan"), fs, dist) == 0
    assert not PC.usable(0j, 5) and not PC.usable(complex(np.nan, 1.0), 5) and not PC.usable(1 + 1j, 0) and PC.usable(1e-300 + 0j, 1)


# ---------------------------------------------------------------- a population
CHANNELS = (None, "EPA", "EVA", "ETU")
SEEDS = range(100, 148)


def _draw(seed):
    """seed -> (cell keys, snr): residual uniform in +- 2500 Hz (the first number of the seed's generator), SNR -3 .. 10 dB, random
    identity and timing, the seven uplink-downlink configurations and no channel / EPA / EVA / ETU in turn, every third cell with
    the extended CP"""
    rng = np.random.default_rng(seed)
    f_off = float(rng.uniform(-2500.0, 2500.0))
    snr = float(rng.uniform(-3.0, 10.0))
    cell = dict(n_id_1=int(rng.integers(0, 168)), n_id_2=int(rng.integers(0, 3)), cp_normal=bool(seed % 3 != 2), n_ports=2, n_rb_dl=25,
                f_off=f_off, t0=float(rng.uniform(0.0, 19200.0)), tdd=(seed % 7, 9), channel=CHANNELS[seed % 4])
    return cell, snr


def test_population_draws_cover_the_ground():
    """a property of the draws alone: enough of them lie outside the native estimate's range, on either side"""
    out = [c["f_off"] for c, _ in map(_draw, SEEDS) if abs(c["f_off"]) > (2330.0 if c["cp_normal"] else 2000.0)]
    assert len(out) >= 8 and min(out) < 0 < max(out), out
    assert {c["tdd"][0] for c, _ in map(_draw, SEEDS)} == set(range(7)) and {c["channel"] for c, _ in map(_draw, SEEDS)} == set(CHANNELS)


def test_population_has_no_wrong_decision():
    synth = load_pkg().synth
    detected = nonzero = 0
    wrong, worst = [], 0.0
    for seed in SEEDS:
        cell, snr = _draw(seed)
        cap = iq_u8_to_capbuf(synth.make_capbuf(seed, FC, [cell], snr_db=snr, quantise=True)[0])
        peaks = [p for p in R.oracle_peaks(cap, K.GRID5, FC, FC, FS) if p.n_id_2 == cell["n_id_2"]]
        if not peaks:
            continue
        det, _ = R.sss_detect(R.oracle_cell(peaks[0]), cap, 3.0, FC, FC, FS, TDD)
        if (det.n_id_1, det.cp_type) != (cell["n_id_1"], 1 if cell["cp_normal"] else 2):
            continue
        detected += 1
        out, n, cz = PC.pss_sss_foe(det, cap, FC, FC, FS, TDD)
        native = R.pss_sss_foe(det, cap, FC, FC, FS, TDD).freq_fine
        period = cz["fs"] / cz["dist"]
        n_true = int(np.rint((cell["f_off"] - native) / period))
        worst = max(worst, abs(cz["f_coarse"] + det.freq - cell["f_off"]))
        nonzero += n != 0
        if n != n_true:
            wrong.append((seed, n, n_true, native, cz["f_coarse"], cell["f_off"]))
    print("draws", len(SEEDS), "detected", detected, "n != 0", nonzero, "wrong", wrong, "worst coarse error %.0f Hz" % worst)
    assert len(SEEDS) >= 48 and detected >= len(SEEDS) - 6      # (a cell at -3 dB behind an ETU channel may be missed)
    assert not wrong, wrong
    assert nonzero >= 8
