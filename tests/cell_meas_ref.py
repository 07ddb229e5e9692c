"""numpy restatement of the cell measurement rule (include/lcs.h: lcs_set_cell_meas; the product's form is
lte-cell-scanner_amd/csrc/cell_meas.h), the reference of every test of that rule.

The rule reads port 0's reference rows of a grid tfg[n_ofdm][72] whose row 0 is slot 0 symbol 0 of a frame, those whose subframe has
its bit in the 10-bit dl_mask; ports 0 and 1 share these rows and the row's RS_DL sequence.  Per used row and port p
  h_m = tfg[r][shift_p + 6 m] conj(rs[m]);  a_p = sum_{m<11} h_m conj(h_{m+1});  e_p = sum_m |h_m|^2;  w = sum_k |tfg[r][k]|^2
and over the n_rows used rows A_p, E_p, W:
  rsrp[p] = |A_p| / (11 n_rows), noise[p] = E_p / (12 n_rows) - rsrp[p], rssi = W / n_rows, rsrq = 6 rsrp[0] / rssi.
RS_DL comes from the oracle (tdd_config_ref._rs)."""
import numpy as np

import tdd_config_ref as TR

NOT_MEASURED = -2
NAMES = ("A0", "A1", "E0", "E1", "W")


def tdd_dl_mask(cfg):
    """the D subframes of configuration cfg as a mask, special subframes excluded; -1 for anything else"""
    if not 0 <= cfg < len(TR.SUBFRAMES):
        return -1
    return sum(1 << s for s, k in enumerate(TR.SUBFRAMES[cfg]) if k == "D")


def ports_measured(n_ports):
    return 2 if n_ports >= 2 else 1


def sums(n_id_cell, cp_type, tfg, dl_mask, n_ports):
    """-> dict(A [2] complex, E [2], W, n_rows, scale = dict(A [2]: sum |h_m| |h_{m+1}|, E [2], W: the sums themselves, all terms
    being non-negative): what a sum's rounding is measured against)"""
    tfg = np.asarray(tfg, np.complex128)
    rs, sh = TR._rs(n_id_cell, cp_type)
    n = TR.n_symb_of(cp_type)
    P = ports_measured(n_ports)
    A, E, S = np.zeros(2, np.complex128), np.zeros(2), np.zeros(2)
    W, n_rows = 0.0, 0
    with np.errstate(all="ignore"):
        for r, slot, sym, s, j in TR.ref_rows(tfg.shape[0], cp_type):
            if not (dl_mask >> s) & 1:
                continue
            n_rows += 1
            row20 = slot * n + sym
            W += float(np.sum(tfg[r].real ** 2 + tfg[r].imag ** 2))
            for p in range(P):
                h = tfg[r, int(sh[row20, p]) + 6 * np.arange(12)] * np.conj(rs[row20])
                A[p] += np.sum(h[:11] * np.conj(h[1:]))
                E[p] += float(np.sum(h.real ** 2 + h.imag ** 2))
                S[p] += float(np.sum(np.abs(h[:11]) * np.abs(h[1:])))
    return dict(A=A, E=E, W=W, n_rows=n_rows, scale=dict(A=S, E=E.copy(), W=W))


def finish(s, n_ports, dl_mask):
    """the record from the sums -> dict(status, n_rows, n_ports, dl_mask, rsrp [2], noise [2], rssi, rsrq, A [2])"""
    P, n = ports_measured(n_ports), s["n_rows"]
    out = dict(status=-1, n_rows=n, n_ports=P, dl_mask=dl_mask, rsrp=np.zeros(2), noise=np.zeros(2), rssi=0.0, rsrq=0.0, A=np.zeros(2, np.complex128))
    if n == 0:
        return out
    with np.errstate(all="ignore"):
        rssi = s["W"] / n
        rsrp = np.abs(s["A"]) / (11 * n)
        noise = s["E"] / (12 * n) - rsrp
        rsrq = 6 * rsrp[0] / rssi if rssi > 0 else np.nan
    if not (rssi > 0 and np.all(np.isfinite([rssi, rsrq])) and np.all(np.isfinite(rsrp)) and np.all(np.isfinite(noise)) and np.all(np.isfinite(s["A"]))):
        return out
    out.update(status=0, rsrp=rsrp, noise=noise, rssi=float(rssi), rsrq=float(rsrq), A=s["A"].copy())
    return out


def measure(n_id_cell, cp_type, tfg, dl_mask=0x3FF, n_ports=1):
    """the whole rule -> finish()'s dict with `sums` (the dict of sums()) added"""
    s = sums(n_id_cell, cp_type, tfg, dl_mask, n_ports)
    out = finish(s, n_ports, dl_mask)
    out["sums"] = s
    return out


def sinr(rec, p=0):
    """rsrp[p] / noise[p], inf where noise <= 0"""
    return float(rec["rsrp"][p] / rec["noise"][p]) if rec["noise"][p] > 0 else float("inf")


def db(x):
    return 10 * np.log10(x)


def assert_record_close(rec, ref, tol, what=""):
    """rec: an object with the fields of lcs_meas_info (capi.CellMeas); ref: measure()'s dict.  Integers exact; the sums A_p within tol
    of their scale; the derived fields within tol relative to E_p / (12 n_rows) (rsrp, noise; rsrq as 6 times that over rssi) or to rssi.
    Returns the worst error seen, in units of tol's reference."""
    assert (rec.status, rec.n_rows, rec.n_ports, rec.dl_mask) == (ref["status"], ref["n_rows"], ref["n_ports"], ref["dl_mask"]), \
        (what, (rec.status, rec.n_rows, rec.n_ports, rec.dl_mask), (ref["status"], ref["n_rows"], ref["n_ports"], ref["dl_mask"]))
    worst = 0.0
    if ref["status"] != 0:
        assert list(rec.rsrp) + list(rec.noise) + [rec.rssi, rec.rsrq] + list(rec.a_re_im) == [0.0] * 10, what
        return worst
    s, n = ref["sums"], ref["n_rows"]
    for p in range(2):
        a = complex(rec.a_re_im[2 * p], rec.a_re_im[2 * p + 1])
        if p >= ref["n_ports"]:
            assert a == 0 and rec.rsrp[p] == 0 and rec.noise[p] == 0, what
            continue
        e_a = abs(a - ref["A"][p]) / s["scale"]["A"][p]
        unit = s["E"][p] / (12 * n)
        e_r, e_n = abs(rec.rsrp[p] - ref["rsrp"][p]) / unit, abs(rec.noise[p] - ref["noise"][p]) / unit
        worst = max(worst, e_a, e_r, e_n)
        assert e_a <= tol and e_r <= tol and e_n <= tol, (what, p, e_a, e_r, e_n)
    e_s, e_q = abs(rec.rssi - ref["rssi"]) / ref["rssi"], abs(rec.rsrq - ref["rsrq"]) / (6 * (s["E"][0] / (12 * n)) / ref["rssi"])
    worst = max(worst, e_s, e_q)
    assert e_s <= tol and e_q <= tol, (what, e_s, e_q)
    return worst
