"""numpy restatement of the two stages that depend on the duplex mode: sss_detect (sss_detect_getce_sss, sss_detect_ml and the
decision, ref src/searcher.cpp:533-761) and pss_sss_foe (:767-850), with the positions of the synchronisation signals as a
parameter (GEO: the table of include/lcs.h at lcs_set_duplex).

The CPU oracle is FDD only.  This module earns its standing as the TDD reference by being pinned to the oracle in FDD
(tests/test_sss_duplex_ref.py: every estimate and likelihood to 1e-12 relative, the decisions equal); in TDD only the window
positions and the frame arithmetic differ, and those are the entries of GEO.  Everything behind the two stages (extract_tfg,
tfoec, chan_est, decode_mib) takes a cell record and is checked against the oracle itself.

Not a test module; imported by test_sss_duplex_ref.py, test_synth_tdd.py, test_gpu_tdd.py and tools/parity_population.py."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle as O  # noqa: E402

FS_LTE = 30720000.0
CP_NORMAL, CP_EXTENDED = 1, 2
MAX_HF = 20
# index 0: normal CP, 1: extended CP.  Samples at 1.92 Msps.
GEO = {
    "fdd": dict(sss_back=(128 + 9, 128 + 32),                # PSS DFT window start minus SSS DFT window start
                room=162,                                    # peak_loc + 9 below this: the peak moves one half frame right
                pss_in_frame=(960 - 128, 960 - 128),         # PSS DFT window start inside the frame
                frame_from="ind",                            # frame_start reads cell.ind (the C++ reference) ...
                sss_in_frame=(960 - 128 - 9 - 128, 960 - 128 - 32 - 128)),
    "tdd": dict(sss_back=(3 * 128 + 10 + 9 + 9, 3 * 160),
                room=2 + 3 * 160,
                pss_in_frame=(1920 + 138 + 137 + 9, 1920 + 2 * 160 + 32),
                frame_from="peak_loc",                       # ... or the peak behind the room rule (Matlab/sss_detect.m)
                sss_in_frame=(1920 - 128, 1920 - 128)),
}

_tab = {}


def _pss_fd(n_id_2):
    if ("p", n_id_2) not in _tab:
        _tab[("p", n_id_2)] = np.asarray(O.pss_fd(n_id_2), np.complex128)
    return _tab[("p", n_id_2)]


def _sss_try(n_id_2):
    """[168][2][62]: sss_fd(n_id_1, n_id_2, slot 0 | 10)"""
    if ("s", n_id_2) not in _tab:
        _tab[("s", n_id_2)] = np.array([[np.asarray(O.sss_fd(t, n_id_2, s), np.float64) for s in (0, 10)] for t in range(168)])
    return _tab[("s", n_id_2)]


def _round_i(x):
    return int(np.rint(x))


def _floor_i(x):
    return int(np.floor(x))


def _range_len(first, incr, last):            # ref src/itpp_ext.cpp:97-109
    s1 = np.sign(last - first)
    s2 = np.sign(incr)
    return _floor_i((last - first) / incr) + 1 if s1 * s2 >= 0 else 0


def _wrap(x, sm, lg):
    k, n = x - sm, lg - sm
    return (k if n == 0 else k - n * _floor_i(k / n)) + sm


def _mid128(cap, start):
    start = int(start)
    if start >= 0 and start + 128 <= cap.size:
        return cap[start:start + 128]
    j = start + np.arange(128)
    ok = (j >= 0) & (j < cap.size)
    return np.where(ok, cap[np.clip(j, 0, cap.size - 1)], 0)


_T128 = np.arange(128, dtype=np.float64)


def extract_psss(w, foc_freq, fs):
    """ref :516-530: fshift, rotate left by 2, 128-point DFT / sqrt(128), the 62 PSS / SSS bins"""
    k = np.pi * foc_freq / (fs / 2)
    a = w * (np.cos(k * _T128) + 1j * np.sin(k * _T128))
    o = np.fft.fft(np.roll(a, -2)) / np.sqrt(128.0)
    return np.concatenate([o[97:128], o[1:32]])


def _chan(e, n_id_2):
    """h_raw, h_sm (13-tap mean, :584-588), noise power (:591)"""
    h_raw = e * np.conj(_pss_fd(n_id_2))
    h_sm = np.empty(62, np.complex128)
    for t in range(62):
        lt, rt = max(t - 6, 0), min(t + 6, 61)
        h_sm[t] = h_raw[lt:rt + 1].sum() / (rt - lt + 1)
    d = h_sm - h_raw
    return h_raw, h_sm, float(np.sum(d.real ** 2 + d.imag ** 2) / 62)


def _copy(cell):
    return type(cell).from_buffer_copy(cell)


def sss_geometry(cell, n_cap, fc_requested, fc_programmed, geo):
    peak_loc = float(cell.ind)
    k_factor = (fc_requested - cell.freq) / fc_programmed
    if peak_loc + 9 < geo["room"]:
        peak_loc += 9600 * k_factor
    n_pss = min(_range_len(peak_loc, k_factor * 9600, float(n_cap) - 125 - 9), MAX_HF)
    return peak_loc, k_factor, n_pss


def sss_detect(cell, capbuf, thresh2_n_sigma, fc_requested, fc_programmed, fs_programmed, geo=GEO["fdd"]):
    """-> (cell_out, dict of the reference's "only used for testing" arrays, as oracle.sss_detect returns them)"""
    cap = np.ascontiguousarray(capbuf, np.complex128)
    peak_loc, k_factor, n_pss = sss_geometry(cell, cap.size, fc_requested, fc_programmed, geo)
    out = _copy(cell)
    if n_pss < 1:
        raise RuntimeError("no PSS occurrence in range")
    fs = fs_programmed * k_factor
    h_sm, pss_np, nrm_raw, ext_raw = [], [], [], []
    for k in range(n_pss):
        pss_dft = _round_i(peak_loc + k * (k_factor * 9600)) + 9 - 2
        _, sm, npw = _chan(extract_psss(_mid128(cap, pss_dft), -cell.freq, fs), cell.n_id_2)
        h_sm.append(sm)
        pss_np.append(npw)
        ext_raw.append(extract_psss(_mid128(cap, pss_dft - geo["sss_back"][1]), -cell.freq, fs))
        nrm_raw.append(extract_psss(_mid128(cap, pss_dft - geo["sss_back"][0]), -cell.freq, fs))
    np12, nrm12, ext12 = np.empty(124), np.empty(124, np.complex128), np.empty(124, np.complex128)
    for h in range(2):            # even / odd occurrences (:618-631)
        s = np.zeros(62)
        sn, se = np.zeros(62, np.complex128), np.zeros(62, np.complex128)
        for k in range(h, n_pss, 2):
            s = s + np.abs(h_sm[k]) ** 2 * (1.0 / pss_np[k])
            w = np.conj(h_sm[k]) * (1.0 / pss_np[k])
            sn = sn + w * nrm_raw[k]
            se = se + w * ext_raw[k]
        np_est = 1 / (1 + s)
        np12[62 * h:62 * h + 62], nrm12[62 * h:62 * h + 62], ext12[62 * h:62 * h + 62] = np_est, sn * np_est, se * np_est
    # ML over 168 x {12, 21} x {nrm, ext} (:636-693)
    tr = _sss_try(cell.n_id_2)
    t12 = np.concatenate([tr[:, 0], tr[:, 1]], axis=1)      # [168][124]
    t21 = np.concatenate([tr[:, 1], tr[:, 0]], axis=1)

    def ml(est, tries):
        acc = (np.conj(est)[None, :] * tries).sum(axis=1)
        rot = np.exp(-1j * np.angle(acc))
        diff = tries * rot[:, None] - est[None, :]
        return -(diff.real ** 2 / np12[None, :]).sum(axis=1) - (diff.imag ** 2 / np12[None, :]).sum(axis=1)

    ll_nrm = np.stack([ml(nrm12, t12), ml(nrm12, t21)], axis=1)      # [168][2]
    ll_ext = np.stack([ml(ext12, t12), ml(ext12, t21)], axis=1)
    # decision (:719-758)
    ext = 0 if ll_nrm.max() > ll_ext.max() else 1
    ll = ll_ext if ext else ll_nrm
    base = peak_loc if geo["frame_from"] == "peak_loc" else float(cell.ind)
    frame_start = base + (9 - 2 - geo["pss_in_frame"][ext]) * 16 / FS_LTE * fs_programmed * k_factor
    if ll[:, 0].max() > ll[:, 1].max():
        col = 0
    else:
        col = 1
        frame_start = frame_start + 9600 * k_factor * 16 / FS_LTE * fs_programmed * k_factor      # quirk Q3
    frame_start = _wrap(frame_start, -0.5, (2 * 9600.0 - 0.5) * 16 / FS_LTE * fs_programmed * k_factor)
    n_id_1_est = int(np.argmax(ll[:, col]))
    lik_final = ll[n_id_1_est, col]
    L = np.concatenate([ll_nrm.T.reshape(-1), ll_ext.T.reshape(-1)])
    lik_mean = L.sum() / 672
    lik_var = ((L * L).sum() - L.sum() ** 2 / 672) / 671
    if lik_final >= lik_mean + lik_var ** 0.5 * thresh2_n_sigma:
        out.n_id_1, out.cp_type, out.frame_start = n_id_1_est, (CP_EXTENDED if ext else CP_NORMAL), frame_start
    d = dict(h1_np=np12[:62].copy(), h2_np=np12[62:].copy(), h1_nrm=nrm12[:62].copy(), h2_nrm=nrm12[62:].copy(),
             h1_ext=ext12[:62].copy(), h2_ext=ext12[62:].copy(), ll_nrm=ll_nrm, ll_ext=ll_ext)
    return out, d


def foe_geometry(cell, n_cap, fc_requested, fc_programmed, fs_programmed, geo):
    k_factor = (fc_requested - cell.freq) / fc_programmed
    if cell.cp_type == CP_NORMAL:
        dist = _round_i(geo["sss_back"][0] * 16 / FS_LTE * fs_programmed * k_factor) & 0xFFFF
        first = cell.frame_start + geo["sss_in_frame"][0] * 16 / FS_LTE * fs_programmed * k_factor
    elif cell.cp_type == CP_EXTENDED:
        dist = _round_i(geo["sss_back"][1] * k_factor) & 0xFFFF      # quirk Q4
        first = cell.frame_start + geo["sss_in_frame"][1] * 16 / FS_LTE * fs_programmed * k_factor
    else:
        raise RuntimeError("pss_sss_foe needs a CP type")
    first = _wrap(first, -0.5, 9600 * 2 - 0.5)
    if first - 9600 * k_factor > -0.5:
        first -= 9600 * k_factor
        sn = 10
    else:
        sn = 0
    step = 9600 * 16 / FS_LTE * fs_programmed * k_factor
    n_sss = _range_len(first, step, float(int(n_cap) - 127 - dist - 100))
    return k_factor, dist, first, sn, step, n_sss


def pss_sss_foe(cell, capbuf, fc_requested, fc_programmed, fs_programmed, geo=GEO["fdd"]):
    cap = np.ascontiguousarray(capbuf, np.complex128)
    k_factor, dist, first, sn, step, n_sss = foe_geometry(cell, cap.size, fc_requested, fc_programmed, fs_programmed, geo)
    out = _copy(cell)
    fs = fs_programmed * k_factor
    sn = (1 - sn // 10) * 10
    M = 0j
    ph = np.pi * (-cell.freq)
    ph = ph / (FS_LTE / 16 / 2)
    ph = ph * float(-dist)
    ph = np.cos(ph) + 1j * np.sin(ph)
    for k in range(n_sss):
        sn = (1 - sn // 10) * 10
        sss_dft = _round_i(first + k * step)
        h_raw, h_sm, pss_np = _chan(extract_psss(_mid128(cap, sss_dft + dist), -cell.freq, fs), cell.n_id_2)
        e = extract_psss(_mid128(cap, sss_dft), -cell.freq, fs)
        sss_raw = e * ph * np.asarray(O.sss_fd(cell.n_id_1, cell.n_id_2, sn), np.float64)
        a2 = np.abs(h_sm) ** 2
        w = a2 * (1.0 / (2 * a2 * pss_np + pss_np * pss_np))
        M = M + (np.conj(sss_raw) * h_raw * w).sum()
    out.freq_fine = cell.freq + np.angle(M) / (2 * np.pi) / (1 / (fs_programmed * k_factor) * dist)
    return out


# ---- the chain of src/CellSearch.cpp:484-558 with the two stages above and the oracle for everything else ----------
def oracle_cell(c):
    """any cell record (the oracle's or the library's) as an oracle Cell"""
    o = O.new_cell()
    for k, _ in O.Cell._fields_:
        if hasattr(c, k):
            setattr(o, k, getattr(c, k))
    return o


def per_peak(peak, capbuf, fc_requested, fc_programmed, fs_programmed, geo):
    """One peak_search record through sss_detect .. decode_mib -> the decoded cell, or None where the reference's loop drops it"""
    c, _ = sss_detect(oracle_cell(peak), capbuf, 3.0, fc_requested, fc_programmed, fs_programmed, geo)
    if c.n_id_1 == -1:
        return None
    c = pss_sss_foe(c, capbuf, fc_requested, fc_programmed, fs_programmed, geo)
    tfg, ts = O.extract_tfg(c, capbuf, fc_requested, fc_programmed, fs_programmed)
    c, tfgc, _ = O.tfoec(c, tfg, ts, fc_requested, fc_programmed)
    c = O.decode_mib(c, tfgc)
    return None if c.n_rb_dl == -1 else c


def oracle_peaks(capbuf, f_search_set, fc_requested, fc_programmed, fs_programmed):
    f = np.ascontiguousarray(f_search_set, np.float64)
    r = O.xcorr_pss(capbuf, f, 2, fc_requested, fc_programmed, fs_programmed)
    Z = O.z_th1(r["sp_incoherent"], r["n_comb_xc"])
    return O.peak_search(r["pow"], r["frq"], Z, f, fc_requested, fc_programmed, r["single"], 2)


def search_peaks(peaks, capbuf, fc_requested, fc_programmed, fs_programmed, geo):
    cells = (per_peak(p, capbuf, fc_requested, fc_programmed, fs_programmed, geo) for p in peaks)
    return [c for c in cells if c is not None]
