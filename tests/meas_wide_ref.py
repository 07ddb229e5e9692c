"""numpy restatement of the full-bandwidth cell measurement (include/lcs.h: lcs_meas_wide_info; the product's form is
lte-cell-scanner_amd/csrc/cell_meas_wide.h and tfg_wide.hip), the reference of every test of that rule.

positions(): extract_tfg's walk (ref src/searcher.cpp:875-920) with the caller's rate.  grid(): np.fft of the frequency-corrected
n_fft samples at round_i of every location, / sqrt(n_fft), the 12 n_rb columns concat(dft.right(6 n_rb), dft.mid(1, 6 n_rb)), late-
compensated.  rs_wide(): 36.211 6.10.1.1 for N_RB = n_rb from the Gold sequence (lcs_table_lte_pn, a CPU table).  sums() / finish():
the sums as written, over port 0's reference rows under the mask."""
import functools

import numpy as np

import tdd_config_ref as TR
from conftest import load_pkg

FS_LTE = 30720000.0
MAX_RB = 100
MAX_RB_OF_R = {1: 6, 2: 15, 4: 25, 8: 50, 16: 100}


@functools.lru_cache(maxsize=None)
def rs_wide(n_id_cell, cp_type, n_rb):
    """-> (rs [40][2 n_rb] complex, shift [40][2] int32) by bin b = 2 slot + (symbol != 0): r(m'), m' = m + 110 - n_rb, and the first
    subcarriers of ports 0 and 1"""
    pn = load_pkg().synth._pn
    n = TR.n_symb_of(cp_type)
    rs = np.zeros((40, 2 * n_rb), np.complex128)
    sh = np.zeros((40, 2), np.int32)
    m = np.arange(2 * n_rb) + 110 - n_rb
    for slot in range(20):
        for j, sym in enumerate((0, n - 3)):
            c_init = (1 << 10) * (7 * (slot + 1) + sym + 1) * (2 * n_id_cell + 1) + 2 * n_id_cell + (1 if cp_type == 1 else 0)
            c = pn(c_init, 440).astype(np.float64)
            rs[2 * slot + j] = ((1 - 2 * c[2 * m]) + 1j * (1 - 2 * c[2 * m + 1])) / np.sqrt(2.0)
            v = (0, 3) if sym == 0 else (3, 0)
            sh[2 * slot + j] = [(v[0] + n_id_cell) % 6, (v[1] + n_id_cell) % 6]
    return rs, sh


def positions(frame_start, freq_fine, cp_type, fc_requested, fc_programmed, fs_programmed, n_ofdm):
    """-> (ts [n_ofdm]: the ideal location of every row, kk: the frequency correction's half turns per sample)"""
    k_factor = (fc_requested - freq_fine) / fc_programmed
    lead = 10 if cp_type == 1 else 32
    loc = frame_start + lead * 16 / FS_LTE * fs_programmed * k_factor
    if loc - .01 * fs_programmed * k_factor > -0.5:
        loc = loc - .01 * fs_programmed * k_factor
    ts = np.empty(n_ofdm)
    sym = 0
    for t in range(n_ofdm):
        ts[t] = loc
        if cp_type != 1:
            loc += (128 + 32) * 16 / FS_LTE * fs_programmed * k_factor
        else:
            loc += ((128 + 10) if sym == 6 else (128 + 9)) * 16 / FS_LTE * fs_programmed * k_factor
            sym = (sym + 1) % 7
    return ts, (-freq_fine) / ((fs_programmed * k_factor) / 2)


def grid(cap, frame_start, freq_fine, cp_type, fc_requested, fc_programmed, fs_programmed, n_fft, n_rb, n_ofdm, rows=None):
    """-> (tfg [n_ofdm][12 n_rb], ts [n_ofdm]); rows: compute only these (the others stay zero)"""
    cap = np.asarray(cap, np.complex128)
    ts, kk = positions(frame_start, freq_fine, cp_type, fc_requested, fc_programmed, fs_programmed, n_ofdm)
    half = 6 * n_rb
    cn = np.concatenate([np.arange(-half, 0), np.arange(1, half + 1)]).astype(np.float64)
    tfg = np.zeros((n_ofdm, 12 * n_rb), np.complex128)
    for t in (range(n_ofdm) if rows is None else rows):
        loc = int(np.rint(ts[t]))
        assert loc >= 0 and loc + n_fft <= cap.size, (t, loc, cap.size)
        ph = kk * np.arange(loc, loc + n_fft, dtype=np.float64)
        ph = ph - 2.0 * np.round(ph / 2.0)                 # exact: the phase in half turns, reduced to [-1, 1]
        X = np.fft.fft(cap[loc:loc + n_fft] * np.exp(1j * np.pi * ph)) / np.sqrt(float(n_fft))
        late = float(loc) - ts[t]
        tfg[t] = np.concatenate([X[n_fft - half:], X[1:half + 1]]) * np.exp(-2j * np.pi * late / n_fft * cn)
    return tfg, ts


def ports_measured(n_ports):
    return 2 if n_ports >= 2 else 1


def sums(n_id_cell, cp_type, tfg, n_rb, dl_mask, n_ports):
    """-> dict(A [2], E [2], W, B [2][n_rb], Wrb [n_rb], n_rows, scale = dict(A [2], B [2][n_rb]: the sums of |h| |h'|; E, W, Wrb: themselves))"""
    tfg = np.asarray(tfg, np.complex128)
    assert tfg.shape[1] == 12 * n_rb
    rs, sh = rs_wide(n_id_cell, cp_type, n_rb)
    P, N = ports_measured(n_ports), 2 * n_rb
    A, E, S = np.zeros(2, np.complex128), np.zeros(2), np.zeros(2)
    B, SB, Wrb = np.zeros((2, n_rb), np.complex128), np.zeros((2, n_rb)), np.zeros(n_rb)
    W, n_rows = 0.0, 0
    with np.errstate(all="ignore"):
        for r, slot, sym, s, j in TR.ref_rows(tfg.shape[0], cp_type):
            if not (dl_mask >> s) & 1:
                continue
            n_rows += 1
            b = 2 * slot + (sym != 0)
            p2 = tfg[r].real ** 2 + tfg[r].imag ** 2
            W += float(np.sum(p2))
            Wrb += p2.reshape(n_rb, 12).sum(axis=1)
            for p in range(P):
                h = tfg[r, int(sh[b, p]) + 6 * np.arange(N)] * np.conj(rs[b])
                pr = h[:-1] * np.conj(h[1:])
                A[p] += np.sum(pr)
                E[p] += float(np.sum(h.real ** 2 + h.imag ** 2))
                S[p] += float(np.sum(np.abs(h[:-1]) * np.abs(h[1:])))
                B[p] += pr[0::2]
                SB[p] += (np.abs(h[:-1]) * np.abs(h[1:]))[0::2]
    return dict(A=A, E=E, W=W, B=B, Wrb=Wrb, n_rows=n_rows, scale=dict(A=S, B=SB, E=E.copy(), W=W, Wrb=Wrb.copy()))


def finish(s, n_rb, n_fft, n_ports, dl_mask):
    P, n, N = ports_measured(n_ports), s["n_rows"], 2 * n_rb
    out = dict(status=-1, n_rows=n, n_ports=P, dl_mask=dl_mask, n_rb=n_rb, n_fft=n_fft, rsrp=np.zeros(2), noise=np.zeros(2), rssi=0.0, rsrq=0.0,
               A=np.zeros(2, np.complex128), rsrp_rb=np.zeros((2, n_rb)), rssi_rb=np.zeros(n_rb))
    if n == 0:
        return out
    with np.errstate(all="ignore"):
        rssi = s["W"] / n
        rsrp = np.abs(s["A"]) / ((N - 1) * n)
        noise = s["E"] / (N * n) - rsrp
        rsrq = n_rb * rsrp[0] / rssi if rssi > 0 else np.nan
    if not (rssi > 0 and np.all(np.isfinite([rssi, rsrq])) and np.all(np.isfinite(rsrp)) and np.all(np.isfinite(noise)) and np.all(np.isfinite(s["A"]))):
        return out
    out.update(status=0, rsrp=rsrp, noise=noise, rssi=float(rssi), rsrq=float(rsrq), A=s["A"].copy(), rsrp_rb=np.abs(s["B"]) / n, rssi_rb=s["Wrb"] / n)
    return out


def measure(n_id_cell, cp_type, tfg, n_rb, n_fft, dl_mask=0x3FF, n_ports=1):
    """the rule on a grid -> finish()'s dict with `sums` added"""
    s = sums(n_id_cell, cp_type, tfg, n_rb, dl_mask, n_ports)
    out = finish(s, n_rb, n_fft, n_ports, dl_mask)
    out["sums"] = s
    return out


def measure_capture(cap, n_id_cell, cp_type, n_ports, frame_start, freq_fine, fc_requested, fc_programmed, fs_programmed, n_fft, n_rb, n_ofdm, dl_mask=0x3FF):
    """the whole stage: port 0's reference rows of the grid, then the rule"""
    rows = [r[0] for r in TR.ref_rows(n_ofdm, cp_type)]
    tfg, _ = grid(cap, frame_start, freq_fine, cp_type, fc_requested, fc_programmed, fs_programmed, n_fft, n_rb, n_ofdm, rows)
    return measure(n_id_cell, cp_type, tfg, n_rb, n_fft, dl_mask, n_ports)


def sinr(rec, p=0):
    return float(rec["rsrp"][p] / rec["noise"][p]) if rec["noise"][p] > 0 else float("inf")


def db(x):
    return 10 * np.log10(x)


def timing_of(a, n_fft):
    """the residual timing a pair-product sum A stands for, in samples: -arg(A) n_fft / (2 pi 6)"""
    return -np.angle(a) * n_fft / (2 * np.pi * 6)


def assert_record_close(rec, ref, tol, what=""):
    """rec: an object with the fields of lcs_meas_wide_info (capi.CellMeasWide); ref: measure()'s dict.  Integers exact; A_p and B_p[i]
    within tol of their scales (the sums of |h| |h'|); rsrp, noise within tol of E_p / (2 n_rb n_rows), rssi and rssi_rb of themselves,
    rsrq of n_rb times that unit over rssi; rsrp_rb[p][i] within tol of its scale / n_rows; entries beyond n_rb are zero.  Returns the
    worst error seen in units of tol's reference."""
    ints = lambda r, g: (g(r, "status"), g(r, "n_rows"), g(r, "n_ports"), g(r, "dl_mask"), g(r, "n_rb"), g(r, "n_fft"))
    assert ints(rec, getattr) == ints(ref, lambda r, k: r[k]), (what, ints(rec, getattr), ints(ref, lambda r, k: r[k]))
    n_rb = ref["n_rb"]
    full_rb = np.array([list(rec._rsrp_rb[0]), list(rec._rsrp_rb[1])]), np.array(list(rec._rssi_rb))
    assert not full_rb[0][:, n_rb:].any() and not full_rb[1][n_rb:].any(), what
    worst = 0.0
    if ref["status"] != 0:
        assert list(rec.rsrp) + list(rec.noise) + [rec.rssi, rec.rsrq] + list(rec.a_re_im) == [0.0] * 10 and not full_rb[0].any() and not full_rb[1].any(), what
        return worst
    s, n, N = ref["sums"], ref["n_rows"], 2 * n_rb
    for p in range(2):
        a = complex(rec.a_re_im[2 * p], rec.a_re_im[2 * p + 1])
        if p >= ref["n_ports"]:
            assert a == 0 and rec.rsrp[p] == 0 and rec.noise[p] == 0 and not full_rb[0][p].any(), what
            continue
        unit = s["E"][p] / (N * n)
        e = [abs(a - ref["A"][p]) / s["scale"]["A"][p], abs(rec.rsrp[p] - ref["rsrp"][p]) / unit, abs(rec.noise[p] - ref["noise"][p]) / unit,
             float(np.max(np.abs(full_rb[0][p, :n_rb] - ref["rsrp_rb"][p]) / (s["scale"]["B"][p] / n)))]
        worst = max([worst] + e)
        assert max(e) <= tol, (what, p, e)
    e = [abs(rec.rssi - ref["rssi"]) / ref["rssi"], abs(rec.rsrq - ref["rsrq"]) / (n_rb * (s["E"][0] / (N * n)) / ref["rssi"]),
         float(np.max(np.abs(full_rb[1][:n_rb] - ref["rssi_rb"]) / ref["rssi_rb"]))]
    worst = max([worst] + e)
    assert max(e) <= tol, (what, e)
    return worst
