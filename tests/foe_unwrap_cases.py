"""The crafted TDD cells on the reference's 5 kHz hypothesis grid that the unwrap tests share (test_pss_coarse_ref.py,
test_foe_coarse_host.py, test_gpu_foe_unwrap.py): one cell at a residual of up to 2.4 kHz, where the native PSS/SSS estimate of a
TDD cell aliases by a period of 4660 Hz (normal CP) / 4000 Hz (extended).  Not a test module."""
from __future__ import annotations

import numpy as np

import pss_coarse_ref as PC
import sss_duplex_ref as R
from conftest import iq_u8_to_capbuf, load_pkg

FS = 1.92e6
FC = 1.9e9
GRID5 = np.array([-5e3, 0.0, 5e3])
TDD = R.GEO["tdd"]
BASE = dict(n_id_1=77, n_id_2=2, n_ports=2, n_rb_dl=25, sfn0=500, t0=6000.0, tdd=(2, 10))

# (id, snr_db, cp_normal, f_off, n the rule must decide, does the cell decode natively)
CRAFTED = [
    ("10 dB normal +2400", 10.0, True, 2400.0, +1, False),
    ("10 dB normal -2300", 10.0, True, -2300.0, 0, True),
    ("10 dB extended +2400", 10.0, False, 2400.0, +1, False),
    ("10 dB extended -2300", 10.0, False, -2300.0, -1, False),
    ("0 dB normal -2300", 0.0, True, -2300.0, -1, False),
    ("-6 dB extended +2400", -6.0, False, 2400.0, -1, False),      # the peak search lands on the 5 kHz hypothesis there
    ("10 dB normal -1000", 10.0, True, -1000.0, 0, True),
    ("10 dB extended +300", 10.0, False, 300.0, 0, True),
    ("0 dB normal +1700", 0.0, True, 1700.0, 0, True),
    ("-6 dB extended -1000", -6.0, False, -1000.0, 0, True),
]

_u8, _ref = {}, {}


def crafted_cell(cp_normal, f_off):
    return dict(BASE, cp_normal=cp_normal, f_off=f_off)


def crafted_u8(snr, cp_normal, f_off, n_cap=153600):
    key = (snr, cp_normal, f_off, n_cap)
    if key not in _u8:
        _u8[key] = load_pkg().synth.make_capbuf(5, FC, [crafted_cell(cp_normal, f_off)], snr_db=snr, quantise=True, n_cap=n_cap)[0]
    return _u8[key]


def crafted_ref(snr, cp_normal, f_off, mib=False):
    """The reference chain on one crafted buffer, computed once: the oracle's peaks, the first of the planted n_id_2 through SSS
    detection, the native estimate and the rule; with mib also the whole chain natively and unwrapped.
    -> dict(cap, peaks, peak, detected, native (cell), n, coarse, unwrapped (cell) [, mib_native, mib_unwrapped])"""
    key = (snr, cp_normal, f_off)
    if key not in _ref:
        cap = iq_u8_to_capbuf(crafted_u8(snr, cp_normal, f_off))
        peaks = R.oracle_peaks(cap, GRID5, FC, FC, FS)
        mine = [p for p in peaks if p.n_id_2 == BASE["n_id_2"]]
        assert mine, "no PSS peak of the planted cell"
        pk = mine[0]
        det, _ = R.sss_detect(R.oracle_cell(pk), cap, 3.0, FC, FC, FS, TDD)
        assert (det.n_id_1, det.cp_type) == (BASE["n_id_1"], 1 if cp_normal else 2), "SSS detection survives the residual"
        native = R.pss_sss_foe(det, cap, FC, FC, FS, TDD)
        unwrapped, n, cz = PC.pss_sss_foe(det, cap, FC, FC, FS, TDD)
        _ref[key] = dict(cap=cap, peaks=peaks, peak=pk, detected=det, native=native, n=n, coarse=cz, unwrapped=unwrapped)
    r = _ref[key]
    if mib and "mib_native" not in r:
        r["mib_native"] = PC.per_peak(r["peak"], r["cap"], FC, FC, FS, TDD, unwrap_on=False)
        r["mib_unwrapped"] = PC.per_peak(r["peak"], r["cap"], FC, FC, FS, TDD, unwrap_on=True)
    return r
