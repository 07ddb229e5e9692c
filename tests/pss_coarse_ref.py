"""numpy restatement of the PSS-only coarse frequency estimate and of the rule that unwraps pss_sss_foe with it
(include/lcs.h: lcs_set_foe_unwrap), on top of sss_duplex_ref.foe_geometry:

  P_k      = round(first_sss + k step) + dist + 2                       k = 0 .. n_sss - 1
  z_k[t]   = capbuf[P_k + t] cis(-2 pi cell.freq / fs t) conj(p[t])     t = 0 .. 127, p = oracle.pss_td(n_id_2)[9:137]
  A_k, B_k = the sums of z_k over t < 64 and t >= 64;  C = sum_k conj(A_k) B_k (occurrence order, unweighted)
  f_coarse = atan2(C.im, C.re) / (2 pi) fs / 64                         relative to cell.freq
  n        = clamp(rint((f_coarse - (native - cell.freq)) / (fs / dist)), -1, +1); 0 if n_sss = 0 or C is zero or not finite
  freq_fine = native if n = 0 (the same double), native + n fs / dist otherwise

Not a test module; imported by test_pss_coarse_ref.py, test_foe_coarse_host.py, test_gpu_foe_unwrap.py and tools/bench_tdd_grid.py."""
from __future__ import annotations

import numpy as np

import sss_duplex_ref as R

O = R.O
_T128 = np.arange(128, dtype=np.float64)
_tab = {}


def pss_useful(n_id_2):
    """the 128 samples of the time-domain PSS behind its 9-sample cyclic prefix"""
    if n_id_2 not in _tab:
        _tab[n_id_2] = np.asarray(O.pss_td(n_id_2), np.complex128)[9:137].copy()
    return _tab[n_id_2]


def windows(cell, capbuf, fc_requested, fc_programmed, fs_programmed, geo):
    """-> (z [n_occ][128], fs, dist): the rotated, template-multiplied PSS windows of every occurrence pss_sss_foe uses"""
    cap = np.ascontiguousarray(capbuf, np.complex128)
    k_factor, dist, first, _, step, n_sss = R.foe_geometry(cell, cap.size, fc_requested, fc_programmed, fs_programmed, geo)
    n_sss = max(0, min(n_sss, R.MAX_HF))
    fs = fs_programmed * k_factor
    kph = np.pi * (-cell.freq) / (fs / 2)
    rot = np.cos(kph * _T128) + 1j * np.sin(kph * _T128)
    cp = np.conj(pss_useful(cell.n_id_2))
    z = np.zeros((n_sss, 128), np.complex128)
    for k in range(n_sss):
        z[k] = R._mid128(cap, R._round_i(first + k * step) + dist + 2) * rot * cp
    return z, fs, dist


def halves(z):
    """-> (A [n_occ], B [n_occ])"""
    return z[:, :64].sum(axis=1), z[:, 64:].sum(axis=1)


def coarse_hz(C, fs):
    return float(np.arctan2(C.imag, C.real) / (2 * np.pi) * fs / 64)


def coarse(cell, capbuf, fc_requested, fc_programmed, fs_programmed, geo=R.GEO["fdd"]):
    """-> dict(f_coarse, C, n_occ, A, B, fs, dist, scale = sum_k |A_k| |B_k|, what C's error is measured against)"""
    z, fs, dist = windows(cell, capbuf, fc_requested, fc_programmed, fs_programmed, geo)
    A, B = halves(z)
    C = 0j
    for k in range(z.shape[0]):
        C = C + np.conj(A[k]) * B[k]
    return dict(f_coarse=coarse_hz(C, fs), C=complex(C), n_occ=z.shape[0], A=A, B=B, z=z, fs=fs, dist=dist,
                scale=float((np.abs(A) * np.abs(B)).sum()))


def usable(C, n_occ):
    return bool(n_occ > 0 and np.isfinite(C.real) and np.isfinite(C.imag) and C != 0)


def unwrap_n(native, freq, f_coarse, fs, dist, ok=True):
    x = (f_coarse - (native - freq)) / (fs / dist)
    if not ok or np.isnan(x):
        return 0
    return int(min(1.0, max(-1.0, np.rint(x))))


def unwrap(native, freq, f_coarse, fs, dist, ok=True):
    n = unwrap_n(native, freq, f_coarse, fs, dist, ok)
    return native if n == 0 else native + n * (fs / dist)


def pss_sss_foe(cell, capbuf, fc_requested, fc_programmed, fs_programmed, geo=R.GEO["fdd"], unwrap_on=True):
    """sss_duplex_ref.pss_sss_foe followed by the rule -> (cell_out, n, dict of coarse())"""
    out = R.pss_sss_foe(cell, capbuf, fc_requested, fc_programmed, fs_programmed, geo)
    c = coarse(cell, capbuf, fc_requested, fc_programmed, fs_programmed, geo)
    if not unwrap_on:
        return out, 0, c
    ok = usable(c["C"], c["n_occ"])
    n = unwrap_n(out.freq_fine, cell.freq, c["f_coarse"], c["fs"], c["dist"], ok)
    out.freq_fine = unwrap(out.freq_fine, cell.freq, c["f_coarse"], c["fs"], c["dist"], ok)
    return out, n, c


# ---- the chain of sss_duplex_ref with the rule behind pss_sss_foe -----------------------------------------------------
def per_peak(peak, capbuf, fc_requested, fc_programmed, fs_programmed, geo, unwrap_on=True, info=None):
    """as sss_duplex_ref.per_peak; info (a dict) receives n and the cell behind SSS detection"""
    c, _ = R.sss_detect(R.oracle_cell(peak), capbuf, 3.0, fc_requested, fc_programmed, fs_programmed, geo)
    if c.n_id_1 == -1:
        return None
    c, n, cz = pss_sss_foe(c, capbuf, fc_requested, fc_programmed, fs_programmed, geo, unwrap_on)
    if info is not None:
        info.update(n=n, f_coarse=cz["f_coarse"], freq_fine=c.freq_fine, detected=R._copy(c))
    tfg, ts = O.extract_tfg(c, capbuf, fc_requested, fc_programmed, fs_programmed)
    c, tfgc, _ = O.tfoec(c, tfg, ts, fc_requested, fc_programmed)
    c = O.decode_mib(c, tfgc)
    return None if c.n_rb_dl == -1 else c


def search_peaks(peaks, capbuf, fc_requested, fc_programmed, fs_programmed, geo, unwrap_on=True):
    cells = (per_peak(p, capbuf, fc_requested, fc_programmed, fs_programmed, geo, unwrap_on) for p in peaks)
    return [c for c in cells if c is not None]
