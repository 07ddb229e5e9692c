"""The numpy restatement of the uplink-downlink configuration rule (tests/tdd_config_ref.py) on grids whose answer is known by
construction, and on planted TDD cells recovered through the CPU chain.

Crafted grids: RS_DL times a smooth channel plus data and noise on the downlink rows of a chosen configuration and DwPTS length,
random QPSK of 1.5 times the amplitude (or nothing) on the others.  A subframe with CRS reads T = 1 within the noise; one without
reads 0 within 2.25 / sqrt(11 rows-in-the-subframe) ~ 0.14 rms for the QPSK uplink, so every decision sits several sigma from 1/2
and the asserted clearance of 0.05 is a property of the seeds used, checked, not a tuned bar."""
import os

import numpy as np
import pytest

import oracle as O
import tdd_config_ref as TR
import tdd_config_cases as K


@pytest.fixture(scope="module", autouse=True)
def _oracle_mode():
    O.set_legacy(False)
    O.set_threads(min(16, os.cpu_count() or 1))


def _full(cp):
    return 854 if cp == 1 else 732


def test_tables():
    assert [TR.dwpts_rows(d, 1) for d in (3, 5, 6, 8, 9, 10, 11, 12)] == [1, 2, 2, 3, 3, 3, 3, 4]
    assert [TR.dwpts_rows(d, 2) for d in (3, 5, 6, 8, 9, 10, 11, 12)] == [1, 2, 2, 3, 3, 4, 4, 4]
    assert len(TR.ref_rows(854, 1)) == len(TR.ref_rows(732, 2)) == 244
    # a 61-subframe grid: 7 occurrences of subframe 0, 6 of the others, in each of the 4 rows
    _, N, _ = TR.bins(5, 1, np.zeros((854, 72), np.complex128))
    assert (N[0] == 7).all() and (N[1:] == 6).all()


@pytest.mark.parametrize("cp", [1, 2], ids=["normal CP", "extended CP"])
@pytest.mark.parametrize("cfg", range(7))
def test_every_configuration_and_dwpts_class(cfg, cp):
    for rows in (1, 2, 3, 4):
        n_id = 100 + 6 * cfg + rows
        g = TR.crafted_grid(n_id, cp, TR.SUBFRAMES[cfg], TR.DWPTS_OF_ROWS[cp][rows], _full(cp), seed=10 * cfg + rows, n_ports=1 + 3 * (rows % 2),
                            uplink="qpsk" if rows != 3 else "none")
        e = TR.estimate(n_id, cp, g)
        print(cfg, cp, rows, "margin %.3f clearance %.3f" % (e["margin"], TR.clearance(e)))
        assert (e["ul_dl_config"], e["dwpts_rs_rows"]) == (cfg, rows)
        assert TR.clearance(e) >= 0.05
        assert np.all(np.abs(e["T"][[0, 5]] - 1) < 0.1)
    # the longer DwPTS of a class read the same class
    for dwpts in ((10, 11) if cp == 1 else (9,)):
        g = TR.crafted_grid(33, cp, TR.SUBFRAMES[cfg], dwpts, _full(cp), seed=77 + dwpts)
        assert TR.estimate(33, cp, g)["dwpts_rs_rows"] == 3


@pytest.mark.parametrize("cp", [1, 2], ids=["normal CP", "extended CP"])
def test_grids_that_get_no_number(cp):
    # a pattern outside the table: downlink in subframes 3 and 7 only
    g = TR.crafted_grid(7, cp, "DSUDUDSDUU", 9, _full(cp), seed=1)
    e = TR.estimate(7, cp, g)
    assert e["ul_dl_config"] == -1 and e["dwpts_rs_rows"] == -1 and e["margin"] > 0.05
    # CRS in subframe 2 (an FDD frame, say): no number although (3, 4, 7, 8, 9) = DDDDD is configuration 5's pattern
    e = TR.estimate(7, cp, TR.crafted_grid(7, cp, "DDDDDDDDDD", 9, _full(cp), seed=2))
    assert e["ul_dl_config"] == -1 and np.all(e["T"] > 0.9)
    # all zero: ref is zero
    e = TR.estimate(7, cp, np.zeros((_full(cp), 72), np.complex128))
    assert (e["ul_dl_config"], e["dwpts_rs_rows"], e["margin"]) == (-1, -1, 0.0)
    # a NaN in a downlink row poisons ref, one in an uplink row its own T
    n = TR.n_symb_of(cp)
    for row in (0, 4 * n):
        g = TR.crafted_grid(7, cp, TR.SUBFRAMES[1], 9, _full(cp), seed=3)
        g[row, 30:36] = np.nan      # six neighbours: one of them is a reference subcarrier whatever the shift
        e = TR.estimate(7, cp, g)
        assert (e["ul_dl_config"], e["dwpts_rs_rows"], e["margin"]) == (-1, -1, 0.0)


@pytest.mark.parametrize("cp, n_ofdm", [(1, 280), (2, 240), (1, 283), (1, 285), (2, 245), (2, 500), (1, 854), (2, 732)])
def test_short_and_partial_grids(cp, n_ofdm):
    n = TR.n_symb_of(cp)
    for cfg, rows in ((1, 3), (3, 1), (6, 4)):
        g = TR.crafted_grid(200 + cfg, cp, TR.SUBFRAMES[cfg], TR.DWPTS_OF_ROWS[cp][rows], n_ofdm, seed=n_ofdm + cfg, snr_db=20.0, uplink_gain=1.0)
        e = TR.estimate(200 + cfg, cp, g)
        assert e["N"].sum() == len(TR.ref_rows(n_ofdm, cp)) == 2 * (n_ofdm // n) + (n_ofdm % n > 0) + (n_ofdm % n > n - 3)
        print(cp, n_ofdm, cfg, "margin %.3f clearance %.3f" % (e["margin"], TR.clearance(e)))
        assert (e["ul_dl_config"], e["dwpts_rs_rows"]) == (cfg, rows)


def test_rule_is_the_same_on_the_compensated_grid():
    """a common phase per row and a phase ramp over the subcarriers change no decision and move T by rounding only"""
    g = TR.crafted_grid(91, 1, TR.SUBFRAMES[2], 10, 854, seed=5)
    k = np.arange(72)
    rot = np.exp(2j * np.pi * 0.0071 * np.arange(854))[:, None] * np.exp(-2j * np.pi * 0.4 * (k - 35.5) / 128)[None, :]
    a, b = TR.estimate(91, 1, g), TR.estimate(91, 1, g * rot)
    assert (a["ul_dl_config"], a["dwpts_rs_rows"]) == (b["ul_dl_config"], b["dwpts_rs_rows"]) == (2, 3)
    assert np.abs(a["T"] - b["T"]).max() < 1e-12 and np.abs(a["R"] - b["R"]).max() < 1e-12


@pytest.mark.parametrize("b", range(len(K.BUFFERS)))
def test_planted_cells_name_their_configuration(b):
    want = K.planted(b)
    got = {c.n_id_2 + 3 * c.n_id_1: (c, e) for c, _, e in K.recovered(b)}
    assert set(want) <= set(got), "a planted cell did not decode"
    for n_id, (cfg, rows, cp) in want.items():
        c, e = got[n_id]
        print("buffer", b, "cell", n_id, "config", e["ul_dl_config"], "rows", e["dwpts_rs_rows"], "margin %.3f" % e["margin"], "T", np.round(e["T"], 2),
              "R", np.round(e["R"], 2))
        assert c.cp_type == cp
        assert e["margin"] >= 0.1, "the planted cases are chosen to sit clear of the threshold"
        assert e["ul_dl_config"] == cfg
        assert e["dwpts_rs_rows"] == rows
