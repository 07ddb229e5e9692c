"""numpy statement of the blind-search rule (include/lcs.h: lcs_pdcch_scan_info), written from the rule's text and from 36.211 6.8,
36.212 5.1.3.1 / 5.1.4.2 and 36.213 9.1.1, not from the product's header: the reference of every test of that stage.  Layout, planting,
channel and combining are tests/pdcch_ref.py's; the soft bits are the same arithmetic over every quadruplet of the subframe.

The decoder is written state by state (predecessors 2 j and 2 j + 1 of state j + 32 b), without the product's lane map, and for a
whole batch of candidates at once.  It is integer arithmetic after the quantisation, so the product must equal it bit for bit; the
only excuse is a decode where some 127 d / m lies within 1e-9 of a half-integer (near_half)."""
import functools

import numpy as np

import pcfich_ref as PR
import pdcch_ref as DR
from conftest import load_pkg

MAX_CCE, MAX_MSG = 88, 1024
LEVELS = (1, 2, 4, 8)
M_OF = {1: 6, 2: 6, 4: 2, 8: 2}
_J = np.arange(32)
_SGN = 1 - 2 * ((np.arange(8)[:, None] >> np.arange(3)[None, :]) & 1)          # word -> +-1 per generator


def candidates(n_cce):
    """[(L, first CCE)] by L ascending, then c"""
    return [(L, c) for L in LEVELS for c in range(0, n_cce - L + 1, L)]


def rate_ok(K, L):
    return 4 * K <= 3 * 72 * L


def search_space(rnti, sf, n_cce, L):
    y = rnti
    for _ in range(sf + 1):
        y = (39827 * y) % 65537
    n = n_cce // L
    return [L * ((y + m) % n) for m in range(M_OF[L])] if n else []


def in_space(rnti, sf, n_cce, L, cce):
    return 0x003D <= rnti <= 0xFFF3 and cce in search_space(rnti, sf, n_cce, L)


def soft_bits(tfg, g, n_id, cp_type, ports, n_rb, lay):
    """the 72 N_CCE soft bits of grid subframe g: pdcch_ref.soft_bits over every quadruplet"""
    n, row0, sf = lay["n_reg"], 2 * g * PR.n_symb_of(cp_type), g % 10
    q = DR.quad_of_reg(n, n_id)
    reg_of_quad = np.empty(n, np.int64)
    reg_of_quad[q] = np.arange(n)
    n_q = 9 * lay["n_cce"]
    s = np.zeros(4 * n_q, np.complex128)
    h_rows = {p: (tfg[row0 + (0 if p < 2 else 1)], PR.rs_row(n_id, cp_type, n_rb, 2 * sf, 0 if p < 2 else 1), PR.shift_of(p, n_id, 2 * sf)) for p in range(ports)}
    for u in range(n_q):
        k, l = lay["order"][reg_of_quad[u]]
        cols = np.array(DR.reg_columns(k, l, n_id, ports, cp_type))
        y = tfg[row0 + l, cols]
        h = {p: PR.channel(*h_rows[p], cols) for p in range(ports)}
        if ports == 1:
            s[4 * u:4 * u + 4] = np.conj(h[0]) * y
            continue
        for pair in range(2):
            a, b = (pair, pair + 2) if ports == 4 else (0, 1)
            e0, e1 = 2 * pair, 2 * pair + 1
            s[4 * u + e0] = np.conj(h[a][e0]) * y[e0] + h[b][e1] * np.conj(y[e1])
            s[4 * u + e1] = np.conj(h[a][e1]) * y[e1] - h[b][e0] * np.conj(y[e0])
    llr = np.empty(8 * n_q)
    llr[0::2], llr[1::2] = s.real, s.imag
    return llr * (1 - 2 * DR.scrambling(n_id, sf, 8 * n_q))


def wava(q, passes=3, odd_on_tie=False):
    """q [n][3][K] integers -> (bits [n][K], end state [n], traced start state [n])"""
    n, _, K = q.shape
    pm = np.zeros((n, 64), np.int64)
    dec = np.zeros((K, n, 64), bool)
    for _ in range(passes):
        for t in range(K):
            bm = -(q[:, :, t] @ _SGN.T)                                  # [n][8]
            new = np.empty_like(pm)
            for b in range(2):
                m0 = pm[:, 2 * _J] + bm[:, DR._WORD[b, 2 * _J]]
                m1 = pm[:, 2 * _J + 1] + bm[:, DR._WORD[b, 2 * _J + 1]]
                take = (m1 <= m0) if odd_on_tie else (m1 < m0)
                new[:, _J + 32 * b] = np.where(take, m1, m0)
                dec[t][:, _J + 32 * b] = take
            pm = new
    end = np.argmin(pm, axis=1)
    s, bits, rows = end.copy(), np.zeros((n, K), np.int64), np.arange(n)
    for t in range(K - 1, -1, -1):
        bits[:, t] = (s >> 5) & 1
        s = ((s << 1) & 63) | dec[t][rows, s]
    return bits, end, s


def encode_tailbite(bits):
    """bits [n][K] -> coded [n][3][K] (36.212 5.1.3.1: the register starts with the last six bits)"""
    n, K = bits.shape
    out = np.zeros((n, 3, K), np.int64)
    for j, gen in enumerate(DR._G):
        for i in range(7):
            if (gen >> (6 - i)) & 1:
                out[:, j, :] ^= np.roll(bits, i, axis=1)
    return out


def crc16_rows(bits):
    crc = np.zeros(bits.shape[0], np.int64)
    for i in range(bits.shape[1]):
        msb = ((crc >> 15) & 1) ^ bits[:, i]
        crc = ((crc << 1) & 0xFFFF) ^ (0x1021 * msb)
    return crc


def decode_batch(cl, L, A, passes=3, odd_on_tie=False, truncate=False):
    """cl [n][72 L] soft bits of n candidates of level L -> list of dicts (None: zero entry): bits (int), bitsK, rnti_x, tb_ok, n_obs,
    n_err, quality, silent, near_half"""
    K = A + 16
    n = cl.shape[0]
    if not rate_ok(K, L) or n == 0:
        return [None] * n
    lists = DR.derm_lists(K, 72 * L)
    d = np.zeros((n, 3 * K))
    for b, p in enumerate(lists):
        for t in p:                                  # ascending position, one addition at a time: the rule's order
            d[:, b] = d[:, b] + cl[:, t]
    finite = np.isfinite(d).all(axis=1)
    m = np.abs(np.where(np.isfinite(d), d, 0.0)).max(axis=1)
    live = finite & (m > 0)
    with np.errstate(all="ignore"):
        x = (127.0 * d) / np.where(live, m, 1.0)[:, None]
    x = np.where(live[:, None], x, 0.0)
    q = (np.trunc(x) if truncate else np.rint(x)).astype(np.int64)
    near = np.abs(np.abs(x - np.floor(x)) - 0.5).min(axis=1) <= 1e-9
    bits, end, start = wava(q.reshape(n, 3, K), passes, odd_on_tie)
    c = encode_tailbite(bits).reshape(n, 3 * K)
    num, den = (q * (1 - 2 * c)).sum(axis=1), np.abs(q).sum(axis=1)
    n_obs = (q != 0).sum(axis=1)
    n_err = ((q != 0) & ((q < 0) != (c != 0))).sum(axis=1)
    par = sum(bits[:, A + t] << (15 - t) for t in range(16))
    rnti = crc16_rows(bits[:, :A]) ^ par
    out = []
    for i in range(n):
        if not finite[i]:
            out.append(None)
        elif not live[i]:
            out.append(dict(bits=0, rnti_x=0, tb_ok=False, n_obs=0, n_err=0, quality=0.0, silent=True, near_half=False))
        else:
            out.append(dict(bits=sum(int(v) << t for t, v in enumerate(bits[i, :A])), rnti_x=int(rnti[i]), tb_ok=bool(end[i] == start[i]), n_obs=int(n_obs[i]),
                            n_err=int(n_err[i]), quality=float(num[i]) / float(den[i]), silent=False, near_half=bool(near[i])))
    return out


def kind_of(rnti):
    return 1 if rnti == 0xFFFF else 2 if rnti == 0xFFFE else 4 if 1 <= rnti <= 60 else 0


def receive(tfg, n_id, cp_type, n_ports, n_rb, cfi, dur, res, sizes, min_quality, min_repeat=2, dl_mask=0x3FF, rnti_mask=7, mi=None, msg_cap=MAX_MSG, **mutant):
    """the rule on a grid with the CFI of every subframe given -> dict: n_sf, sf [g] = dict(cfi, n_reg, n_cce, n_cand, n_common, n_ue,
    cce_mask), llr {g}, dec {(g, candidate index, size index): dict with flags, n_repeat, L, cce}, msg (list of keys, in order, cut to
    msg_cap), n_dropped and the head's counts"""
    tfg = np.asarray(tfg, np.complex128)
    P, n_sf = PR.ports_of(n_ports), PR.n_sf_of(tfg.shape[0], cp_type)
    out = dict(n_sf=n_sf, sf=[dict(cfi=0, n_reg=0, n_cce=0, n_cand=0, n_common=0, n_ue=0, cce_mask=[0, 0, 0]) for _ in range(n_sf)], llr={}, dec={})
    for g in range(n_sf):
        c = int(cfi[g])
        if not DR.is_read(g, tfg.shape[0], cp_type, n_rb, dl_mask, dur, mi is not None) or not 1 <= c <= 3:
            continue
        lay = DR.layout(n_id, cp_type, P, n_rb, c, dur, res, 1 if mi is None else mi[g % 10])
        if lay is None or lay["n_cce"] == 0:
            continue
        n_cce = lay["n_cce"]
        assert n_cce <= MAX_CCE
        cand = candidates(n_cce)
        out["sf"][g].update(cfi=c, n_reg=lay["n_reg"], n_cce=n_cce, n_cand=len(cand))
        with np.errstate(all="ignore"):
            llr = out["llr"][g] = soft_bits(tfg, g, n_id, cp_type, P, n_rb, lay)
            for L in LEVELS:
                idx = [i for i, (l, _) in enumerate(cand) if l == L]
                cl = np.array([llr[72 * cand[i][1]:72 * (cand[i][1] + L)] for i in idx]).reshape(len(idx), 72 * L)
                for si, A in enumerate(sizes):
                    for i, d in zip(idx, decode_batch(cl, L, A, **mutant)):
                        cce = cand[i][1]
                        if d is None:
                            d = dict(bits=0, rnti_x=0, tb_ok=False, n_obs=0, n_err=0, quality=0.0, silent=False, near_half=False, flags=0)
                        else:
                            common = bool(kind_of(d["rnti_x"]) & rnti_mask) and L >= 4 and cce < 16 and not d["silent"]
                            d["flags"] = 1 if d["silent"] else 1 | (8 if d["tb_ok"] else 0) | (4 if in_space(d["rnti_x"], g % 10, n_cce, L, cce) else 0) | (18 if common else 0)
                        out["dec"][(g, i, si)] = dict(d, L=L, cce=cce, n_repeat=0)
    hit = lambda d: bool(d["flags"] & 4) and d["quality"] >= min_quality
    seen = {}
    for (g, i, si), d in out["dec"].items():
        if hit(d):
            seen.setdefault(d["rnti_x"], set()).add(g)
    msg, acc = [], []
    for key in sorted(out["dec"]):
        d = out["dec"][key]
        common = bool(d["flags"] & 2)
        if hit(d):
            d["n_repeat"] = len(seen[d["rnti_x"]])
            if d["n_repeat"] >= min_repeat:
                d["flags"] |= 2
        if d["flags"] & 2:
            acc.append(d)
            s = out["sf"][key[0]]
            s["n_common" if common else "n_ue"] += 1
            for c in range(d["cce"], d["cce"] + d["L"]):
                s["cce_mask"][c >> 5] |= 1 << (c & 31)
        if hit(d) or common:
            msg.append(key)
    ue = [d for d in acc if not d["flags"] & 16]
    out.update(msg=msg[:msg_cap], n_msg=min(len(msg), msg_cap), n_dropped=max(len(msg) - msg_cap, 0), n_read=sum(1 for s in out["sf"] if s["cfi"]), n_accepted=len(acc),
               n_si=sum(d["rnti_x"] == 0xFFFF for d in acc), n_paging=sum(d["rnti_x"] == 0xFFFE for d in acc), n_ra=sum(1 <= d["rnti_x"] <= 60 for d in acc),
               n_ue=len(ue), n_rnti=len({d["rnti_x"] for d in ue}))
    return out
