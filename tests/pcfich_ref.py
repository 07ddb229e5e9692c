"""numpy statement of the PCFICH rule (include/lcs.h: lcs_pcfich_info), written from 36.211 6.7 / 36.212 5.3.4 and the rule's text,
not from the product's header: the reference of every test of that stage.

A grid tfg[n_ofdm][12 n_rb] whose row 0 is symbol 0 of slot 0 of a frame.  Grid subframe g starts at row 2 g n_symb and is subframe
g mod 10.  columns(): 36.211 6.7.4.  rs_row() / shifts(): 36.211 6.10.1.1-2 for N_RB = n_rb.  channel(): least squares on the port's
reference row, linear between the two reference elements around a column, the outer line beyond the first and the last.
decode(): combining (one port; SFBC on pairs; SFBC-FSTD with ports (0, 2), (1, 3)), descrambling, the three codewords."""
import functools

import numpy as np

from conftest import load_pkg

BANDWIDTHS = (6, 15, 25, 50, 75, 100)
# 36.212 table 5.3.4-1
CODEWORDS = np.array([[0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1],
                      [1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0],
                      [1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1]])


def n_symb_of(cp_type):
    return 7 if cp_type == 1 else 6


def ports_of(n_ports):
    return n_ports if n_ports in (1, 2, 4) else 1


def n_sf_of(n_ofdm, cp_type):
    return -(-n_ofdm // (2 * n_symb_of(cp_type))) if n_ofdm > 0 else 0


def columns(n_id_cell, n_rb):
    """the 16 columns of symbol 0, in mapping order: z(i) on the resource-element group represented by k = kbar + floor(i N_RB / 2)
    N_sc / 2 (mod N_RB N_sc), kbar = (N_sc / 2) (N_ID mod 2 N_RB); a group of symbol 0 is six columns of which the two with
    k = N_ID (mod 3) are kept for reference signals"""
    kbar = 6 * (n_id_cell % (2 * n_rb))
    out = []
    for i in range(4):
        k0 = (kbar + (i * n_rb // 2) * 6) % (12 * n_rb)
        out += [k for k in range(k0, k0 + 6) if k % 3 != n_id_cell % 3]
    return np.array(out)


@functools.lru_cache(maxsize=None)
def rs_row(n_id_cell, cp_type, n_rb, slot, sym):
    """r(m'), m' = m + 110 - n_rb, m < 2 n_rb, of that slot and symbol"""
    pn = load_pkg().synth._pn
    c_init = (1 << 10) * (7 * (slot + 1) + sym + 1) * (2 * n_id_cell + 1) + 2 * n_id_cell + (1 if cp_type == 1 else 0)
    c = pn(c_init, 440).astype(np.float64)
    m = np.arange(2 * n_rb) + 110 - n_rb
    return ((1 - 2 * c[2 * m]) + 1j * (1 - 2 * c[2 * m + 1])) / np.sqrt(2.0)


def shift_of(port, n_id_cell, slot):
    """the first subcarrier of the port's reference elements in the first symbol that carries them (symbol 0: ports 0, 1; symbol 1:
    ports 2, 3): (v + v_shift) mod 6 with v = 0, 3, 3 (n_s mod 2), 3 + 3 (n_s mod 2)"""
    v = (0, 3, 3 * (slot & 1), 3 + 3 * (slot & 1))[port]
    return (v + n_id_cell) % 6


def channel(row, rs, shift, cols):
    """the port's channel at the columns cols from its reference row"""
    n = rs.size
    pos = shift + 6 * np.arange(n)
    h = row[pos] * np.conj(rs)
    m0 = np.clip(np.floor_divide(cols - shift, 6), 0, n - 2)
    t = (cols - pos[m0]) / 6.0
    return h[m0] + (h[m0 + 1] - h[m0]) * t


@functools.lru_cache(maxsize=None)
def scrambling(n_id_cell, sf):
    return load_pkg().synth._pn((sf + 1) * (2 * n_id_cell + 1) * 512 + n_id_cell, 32).astype(np.int64)


def decode_subframe(tfg, g, n_id_cell, cp_type, n_ports, n_rb):
    """-> (cfi, corr [3], margin) of grid subframe g; (0, zeros, 0) where the sum of |b| is zero or not finite"""
    P, n = ports_of(n_ports), n_symb_of(cp_type)
    r0, sf = 2 * g * n, g % 10
    cols = columns(n_id_cell, n_rb)
    y = tfg[r0, cols]
    with np.errstate(all="ignore"):
        h = {}
        for p in range(P):
            sym = 0 if p < 2 else 1
            h[p] = channel(tfg[r0 + sym], rs_row(n_id_cell, cp_type, n_rb, 2 * sf, sym), shift_of(p, n_id_cell, 2 * sf), cols)
        s = np.zeros(16, np.complex128)
        if P == 1:
            s = np.conj(h[0]) * y
        else:
            for u in range(8):
                a, b = ((u & 1), (u & 1) + 2) if P == 4 else (0, 1)
                e0, e1 = 2 * u, 2 * u + 1
                s[e0] = np.conj(h[a][e0]) * y[e0] + h[b][e1] * np.conj(y[e1])
                s[e1] = np.conj(h[a][e1]) * y[e1] - h[b][e0] * np.conj(y[e0])
        bits = np.empty(32)
        bits[0::2], bits[1::2] = s.real, s.imag
        bits = bits * (1 - 2 * scrambling(n_id_cell, sf))
        den = np.sum(np.abs(bits))
        num = (1 - 2 * CODEWORDS) @ bits
    if not (den > 0 and np.isfinite(den) and np.all(np.isfinite(num))):
        return 0, np.zeros(3), 0.0
    corr = num / den
    best = int(np.argmax(corr))                     # the lowest index on a tie
    return best + 1, corr, float(corr[best] - np.max(np.delete(corr, best)))


def decode(tfg, n_id_cell, cp_type, n_ports, n_rb, dl_mask=0x3FF):
    """the rule on a grid -> dict with the fields of lcs_pcfich_info (arrays cut to n_sf)"""
    tfg = np.asarray(tfg, np.complex128)
    assert tfg.shape[1] == 12 * n_rb and n_rb in BANDWIDTHS
    P, n, n_ofdm = ports_of(n_ports), n_symb_of(cp_type), tfg.shape[0]
    n_sf = n_sf_of(n_ofdm, cp_type)
    cfi, corr, margin = np.zeros(n_sf, np.int32), np.zeros((n_sf, 3)), np.zeros(n_sf)
    for g in range(n_sf):
        r0 = 2 * g * n
        if not (dl_mask >> (g % 10)) & 1 or r0 >= n_ofdm or (P == 4 and r0 + 1 >= n_ofdm):
            continue
        cfi[g], corr[g], margin[g] = decode_subframe(tfg, g, n_id_cell, cp_type, n_ports, n_rb)
    dec = cfi > 0
    n_ctrl = cfi[dec] + (1 if n_rb <= 10 else 0)
    return dict(n_sf=n_sf, n_decoded=int(dec.sum()), n_cfi=[int((cfi == c).sum()) for c in (1, 2, 3)], dl_mask=dl_mask, n_rb=n_rb, n_ports=P,
                mean_n_ctrl_sym=float(n_ctrl.sum()) / int(dec.sum()) if dec.any() else 0.0, min_margin=float(margin[dec].min()) if dec.any() else 0.0,
                cfi=cfi, corr=corr, margin=margin)


def assert_record_close(rec, ref, tol, what=""):
    """rec: capi.PcfichInfo; ref: decode()'s dict.  Integers and decisions equal, corr and margin within tol (they are ratios of order
    one), the summary from the same decisions; the entries beyond n_sf are zero.  Returns the worst difference."""
    ints = lambda r, g: (g(r, "n_sf"), g(r, "n_decoded"), list(g(r, "n_cfi")), g(r, "dl_mask"), g(r, "n_rb"), g(r, "n_ports"))
    assert ints(rec, getattr) == ints(ref, lambda r, k: r[k]), (what, ints(rec, getattr), ints(ref, lambda r, k: r[k]))
    n = ref["n_sf"]
    assert not np.ctypeslib.as_array(rec._cfi)[n:].any() and not np.ctypeslib.as_array(rec._corr)[n:].any() and not np.ctypeslib.as_array(rec._margin)[n:].any(), what
    assert np.array_equal(rec.cfi, ref["cfi"]), (what, rec.cfi, ref["cfi"])
    worst = max(float(np.abs(rec.corr - ref["corr"]).max()), float(np.abs(rec.margin - ref["margin"]).max()), abs(rec.min_margin - ref["min_margin"]))
    assert worst <= tol, (what, worst)
    assert abs(rec.mean_n_ctrl_sym - ref["mean_n_ctrl_sym"]) <= 1e-15 * 4, what
    assert np.array_equal(rec.n_ctrl_sym, np.where(ref["cfi"] > 0, ref["cfi"] + (1 if ref["n_rb"] <= 10 else 0), 0)), what
    return worst
