"""The numpy restatement of sss_detect / pss_sss_foe (tests/sss_duplex_ref.py) is the reference of the TDD tests.  It earns that
standing here: with the FDD geometry it must equal the CPU oracle -- every estimate and likelihood to 1e-12 of the array's
largest magnitude (both sides are fp64; the summation order and the FFT differ), the decisions exactly, frame_start to 1e-9
samples and freq_fine to 1e-6 Hz (three orders inside the bars the GPU stages are held to)."""
import os

import numpy as np
import pytest

import oracle as O
import sss_duplex_ref as R
from conftest import golden, iq_u8_to_capbuf, load_pkg

FS = 1.92e6
FC = 739e6
ARRAYS = ("h1_np", "h2_np", "h1_nrm", "h2_nrm", "h1_ext", "h2_ext", "ll_nrm", "ll_ext")


@pytest.fixture(scope="module", autouse=True)
def _oracle_mode():
    O.set_legacy(False)
    O.set_threads(min(16, os.cpu_count() or 1))


def _peaks(cap, f, fc):
    r = O.xcorr_pss(cap, f, 2, fc, fc, FS)
    return O.peak_search(r["pow"], r["frq"], O.z_th1(r["sp_incoherent"], r["n_comb_xc"]), f, fc, fc, r["single"], 2)


def _same_as_oracle(cell, cap, fc):
    co, do = O.sss_detect(cell, cap, 3.0, fc, fc, FS)
    cr, dr = R.sss_detect(cell, cap, 3.0, fc, fc, FS, R.GEO["fdd"])
    for k in ARRAYS:
        err = np.abs(dr[k] - do[k]).max() / np.abs(do[k]).max()
        assert err <= 1e-12, (k, err)
    assert (cr.n_id_1, cr.cp_type) == (co.n_id_1, co.cp_type)
    if co.n_id_1 < 0:
        assert np.isnan(cr.frame_start) and np.isnan(co.frame_start)
        return co
    assert abs(cr.frame_start - co.frame_start) < 1e-9, (cr.frame_start, co.frame_start)
    fo = O.pss_sss_foe(co, cap, fc, fc, FS)
    fr = R.pss_sss_foe(co, cap, fc, fc, FS, R.GEO["fdd"])
    assert abs(fr.freq_fine - fo.freq_fine) < 1e-6, (fr.freq_fine, fo.freq_fine)
    return co


def test_fdd_restatement_equals_oracle_on_golden_capture():
    cap = iq_u8_to_capbuf(golden("capbuf_0000")["iq_u8"])
    peaks = _peaks(cap, np.array([30e3, 35e3, 40e3]), FC)
    assert len(peaks) >= 2
    found = [c.n_id_cell() for c in (_same_as_oracle(p, cap, FC) for p in peaks) if c.n_id_1 >= 0]
    assert 277 in found and 271 in found


@pytest.mark.parametrize("cp_normal, t0", [(True, 5000.0), (False, 12345.0),
                                           (True, 832.0 - 107),                 # the buffer starts t0 samples into a frame: PSS DFT window at sample 107, peak at ~100 -- the room rule moves it
                                           (False, 9600.0 + 832 - 47)])
def test_fdd_restatement_equals_oracle_on_synthetic(cp_normal, t0):
    pkg = load_pkg()
    cell = dict(n_id_1=101, n_id_2=1, cp_normal=cp_normal, n_ports=2, f_off=700.0, t0=t0, sfn0=321)
    cap, _ = pkg.synth.make_capbuf(11, FC, [cell], snr_db=5.0, quantise=False, n_cap=57600)
    peaks = [p for p in _peaks(cap, np.array([-5e3, 0.0, 5e3]), FC) if p.n_id_2 == 1]
    assert peaks
    if t0 in (832.0 - 107, 9600.0 + 832 - 47):
        assert peaks[0].ind + 9 < 162, peaks[0].ind
    c = _same_as_oracle(peaks[0], cap, FC)
    assert (c.n_id_1, c.cp_type) == (101, 1 if cp_normal else 2)


def test_tdd_table_is_the_issue_s():
    t = R.GEO["tdd"]
    assert t["sss_back"] == (412, 480) and t["room"] == 482 and t["pss_in_frame"] == (2204, 2272) and t["sss_in_frame"] == (1792, 1792)
    f = R.GEO["fdd"]
    assert f["sss_back"] == (137, 160) and f["room"] == 162 and f["pss_in_frame"] == (832, 832) and f["sss_in_frame"] == (695, 672)
