"""The cell measurement rule itself (include/lcs.h: lcs_set_cell_meas), in its numpy restatement (tests/cell_meas_ref.py), on the
CPU: does it measure what it says?  Crafted grids with a planted truth, and planted cells through the oracle chain
(tests/cell_meas_cases.py, tests/tdd_config_cases.py)."""
import os

import numpy as np
import pytest

import cell_meas_cases as CS
import cell_meas_ref as MR
import oracle as O
import tdd_config_cases as K


@pytest.fixture(scope="module", autouse=True)
def _oracle_mode():
    O.set_legacy(False)
    O.set_threads(min(16, os.cpu_count() or 1))


def test_flat_crafted_grids_give_the_planted_power_and_noise():
    """854 / 732 rows at 15 dB, every subframe downlink, no amplitude ripple: rsrp within 2 % of the planted power per reference
    element, noise within 15 % of the planted variance (measured: 0.6 % and 5.3 % at worst over ports 0 and 1; the noise estimate
    averages 12 n_rows = 3432 / 3420 squared magnitudes beside a signal 30 times as strong), rssi within 1 % of the expected row power."""
    for n_id, cp, n_ofdm in ((233, 1, 854), (9, 2, 732)):
        tfg, truth = CS.crafted(n_id, cp, "DDDDDDDDDD", 0, n_ofdm, seed=3, snr_db=15.0, n_ports=2, flat=True)
        m = MR.measure(n_id, cp, tfg, 0x3FF, 2)
        assert m["status"] == 0 and m["n_ports"] == 2 and m["n_rows"] == len(MR.TR.ref_rows(n_ofdm, cp))
        e_r, e_n = np.abs(m["rsrp"] / truth["rs_power"][:2] - 1), np.abs(m["noise"] / truth["noise_var"] - 1)
        print(n_id, "rsrp error", e_r, "noise error", e_n, "rssi error", m["rssi"] / truth["row_power"] - 1)
        assert e_r.max() <= 0.02 and e_n.max() <= 0.15
        assert abs(m["rssi"] / truth["row_power"] - 1) <= 0.01
        assert abs(m["rsrq"] - 6 * m["rsrp"][0] / m["rssi"]) <= 1e-15
        # one port: port 1's reference elements are empty, port 0 reads the same
        tfg1, truth1 = CS.crafted(n_id, cp, "DDDDDDDDDD", 0, n_ofdm, seed=3, snr_db=15.0, n_ports=1, flat=True)
        m1 = MR.measure(n_id, cp, tfg1, 0x3FF, 1)
        assert m1["n_ports"] == 1 and abs(m1["rsrp"][0] / truth1["rs_power"][0] - 1) <= 0.02 and m1["rsrp"][1] == 0 == m1["noise"][1]


def test_the_rule_reads_noise_high_on_a_selective_channel():
    """what the rule is not: with the crafted 25 % amplitude ripple over the 72 subcarriers at 25 dB the channel's change over 6
    subcarriers lands in `noise` (measured: 2.3 to 2.6 times the planted variance); rsrp stays within the ripple's mean power"""
    tfg, truth = CS.crafted(233, 1, "DDDDDDDDDD", 0, 854, seed=3, snr_db=25.0, n_ports=2, flat=False)
    m = MR.measure(233, 1, tfg, 0x3FF, 2)
    ratio = m["noise"] / truth["noise_var"]
    print("noise / planted", ratio)
    assert np.all(ratio > 1.5) and np.all(ratio < 4.0)
    assert np.all(np.abs(m["rsrp"] / (truth["rs_power"][:2] * (1 + 0.25 ** 2 / 2)) - 1) < 0.03)


def test_sinr_follows_the_planted_snr_on_the_oracle_chain():
    """the four FDD buffers of one cell at 15 / 8 / 2 / -3 dB: port 0's SINR in dB lies in [snr - 2.0, snr + 0.5] and is strictly
    increasing with the planted SNR (measured: 14.33, 7.33, 1.19, -4.22 dB; 10 log10 rsrq -11.4, -12.0, -13.7, -16.7)"""
    got = []
    for b, snr in enumerate(CS.SNR_SERIES):
        rec = CS.recovered(b)
        assert [c.n_id_2 + 3 * c.n_id_1 for c, _, _ in rec] == [233]
        c, tfg, _ = rec[0]
        m = MR.measure(233, c.cp_type, tfg, 0x3FF, c.n_ports)
        assert m["status"] == 0 and m["n_ports"] == 2
        got.append(MR.db(MR.sinr(m)))
        print(snr, "SINR %.2f dB, RSRQ %.1f dB" % (got[-1], MR.db(m["rsrq"])))
        assert snr - 2.0 <= got[-1] <= snr + 0.5
    assert all(a > b for a, b in zip(got, got[1:]))


def test_raw_and_compensated_grid_agree():
    """a row's frequency correction is a common phase and the timing correction turns every neighbour product by one angle: rsrp
    within 5e-3 relative between the oracle's raw grid and its tfoec-compensated one (measured: 1.1e-3 at worst), rssi within 1e-12;
    beside it the ratio of noise[p] to the reference's own chan_est noise power, printed and not asserted (measured: 1.17 to 1.22)"""
    n = 0
    for b in range(len(CS.BUFFERS)):
        for c, tfg, tfgc in CS.recovered(b):
            n_id = c.n_id_2 + 3 * c.n_id_1
            raw, comp = MR.measure(n_id, c.cp_type, tfg, 0x3FF, c.n_ports), MR.measure(n_id, c.cp_type, tfgc, 0x3FF, c.n_ports)
            assert raw["status"] == comp["status"] == 0
            P = raw["n_ports"]
            ratio = [raw["noise"][p] / O.chan_est(c, tfgc, p)[1] for p in range(P)]
            print(b, n_id, "rsrp raw / compensated - 1:", raw["rsrp"][:P] / comp["rsrp"][:P] - 1, "noise / chan_est np:", ratio)
            assert np.all(np.abs(raw["rsrp"][:P] / comp["rsrp"][:P] - 1) <= 5e-3)
            assert abs(raw["rssi"] / comp["rssi"] - 1) <= 1e-12
            n += 1
    assert n == 7      # every planted cell decodes: four single cells, two of the two-cell buffer, the 4-port cell through EPA


def test_tdd_configuration_mask_and_subframes_0_and_5_agree():
    """the TDD buffers: the rule with tdd_dl_mask(planted configuration) and with 0x021 -- both give a number, and rsrp[0] agrees
    within 15 % (measured spread: 0 to 3.5 %, the two EPA buffers 0.5 % and 0.2 %; configuration 0 has no subframe beyond 0 and 5,
    so its two masks are one)"""
    seen = set()
    for b in range(len(K.BUFFERS)):
        for c, tfg, _ in K.recovered(b):
            n_id = c.n_id_2 + 3 * c.n_id_1
            if n_id not in K.planted(b):
                continue
            cfg = K.planted(b)[n_id][0]
            a, d = MR.measure(n_id, c.cp_type, tfg, MR.tdd_dl_mask(cfg), c.n_ports), MR.measure(n_id, c.cp_type, tfg, 0x021, c.n_ports)
            assert a["status"] == d["status"] == 0 and a["n_rows"] >= d["n_rows"] == 52
            print(b, n_id, cfg, a["n_rows"], "rsrp ratio %.4f" % (a["rsrp"][0] / d["rsrp"][0]), "SINR %.2f / %.2f dB" % (MR.db(MR.sinr(a)), MR.db(MR.sinr(d))))
            assert abs(a["rsrp"][0] / d["rsrp"][0] - 1) <= 0.15
            seen.add(cfg)
    assert seen == set(range(7))
