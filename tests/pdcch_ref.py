"""numpy statement of the PDCCH common-search-space rule (include/lcs.h: lcs_pdcch_info), transmit and receive side, written from
36.211 6.2.4 / 6.8 / 6.9.3, 36.212 5.1.4.2 / 5.3.3, 36.213 9.1.1 and the rule's text, not from the product's header or tables: the
reference of every test of that stage.  Grid, subframes, reference signals, channel and combining as tests/pcfich_ref.py.

What is pinned to the reference project elsewhere: the Gold bits, CRC + encoder + rate matching (test_pdcch_ref.py).  What rests on
this file's reading of the standard alone: the PHICH's REG positions, the quadruplet interleaver and shift, the search space."""
import functools

import numpy as np

import pcfich_ref as PR
from conftest import load_pkg

PERM = [1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31, 0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30]
NG = {1: (1, 6), 2: (1, 2), 3: (1, 1), 4: (2, 1)}          # phich_resource -> Ng as a fraction
N_QUAD, N_LLR, SLOTS = 144, 1152, 6
SLOT_CAND = [(4, 0), (4, 4), (4, 8), (4, 12), (8, 0), (8, 8)]


def n_ctrl_of(cfi, n_rb):
    return cfi + (1 if n_rb <= 10 else 0)


def regs_per_rb(l, ports, cp_type):
    if l == 0:
        return 2
    if l == 1:
        return 2 if ports == 4 else 3
    if l == 2:
        return 3
    return 3 if cp_type == 1 else 2


def symbol_regs(l, n_rb, ports, cp_type):
    per = regs_per_rb(l, ports, cp_type)
    return [12 * n + (12 // per) * j for n in range(n_rb) for j in range(per)]


def reg_columns(k, l, n_id, ports, cp_type):
    if regs_per_rb(l, ports, cp_type) == 3:
        return [k, k + 1, k + 2, k + 3]
    return [c for c in range(k, k + 6) if c % 3 != n_id % 3]


def phich_units(res, n_rb, mi=1):
    num, den = NG[res]
    return mi * -(-(num * n_rb) // (8 * den))


@functools.lru_cache(maxsize=None)
def layout(n_id, cp_type, ports, n_rb, cfi, dur, res, mi=1):
    """-> dict(pcfich, phich, order: lists of (k', l'); n_reg, n_cce), or None where the rule refuses (extended duration with fewer
    than three control symbols; PHICH units that collide)"""
    n_ctrl = n_ctrl_of(cfi, n_rb)
    if dur == 2 and n_ctrl < 3:
        return None
    pcf = [((6 * (n_id % (2 * n_rb)) + 6 * (i * n_rb // 2)) % (12 * n_rb), 0) for i in range(4)]
    left = {l: [k for k in symbol_regs(l, n_rb, ports, cp_type) if (k, l) not in pcf] for l in range(n_ctrl)}
    phich = []
    for m in range(phich_units(res, n_rb, mi)):
        for i in range(3):
            l = i if dur == 2 else 0
            n_l, n_0 = len(left[l]), len(left[0])
            phich.append((left[l][(n_id * n_l // n_0 + m + i * n_l // 3) % n_l], l))
    if len(set(phich)) != len(phich):
        return None
    taken = set(phich)
    order = sorted((k, l) for l in range(n_ctrl) for k in left[l] if (k, l) not in taken)
    return dict(pcfich=pcf, phich=phich, order=order, n_reg=len(order), n_cce=len(order) // 9)


def n_reg_closed_form(cp_type, ports, n_rb, cfi, res, mi=1):
    return sum(regs_per_rb(l, ports, cp_type) for l in range(n_ctrl_of(cfi, n_rb))) * n_rb - 4 - 3 * phich_units(res, n_rb, mi)


def interleave(n):
    """the order in which n quadruplets leave the sub-block interleaver"""
    rows = -(-n // 32)
    m = np.concatenate([np.full(32 * rows - n, -1), np.arange(n)]).reshape(rows, 32)
    out = np.concatenate([m[:, PERM[c]] for c in range(32)])
    return out[out >= 0]


def quad_of_reg(n, n_id):
    """q[i]: the quadruplet of the multiplexed stream that REG i of the order carries"""
    return interleave(n)[(np.arange(n) + n_id) % n]


def candidates(n_cce):
    """the slots that exist: [(slot, L, first CCE)]"""
    out = []
    for s, (L, cce) in enumerate(SLOT_CAND):
        m = s if L == 4 else s - 4
        if m < min(4 if L == 4 else 2, n_cce // L):
            out.append((s, L, cce))
    return out


@functools.lru_cache(maxsize=None)
def scrambling(n_id, sf, n):
    return load_pkg().synth._pn(sf * 512 + n_id, n).astype(np.int64)


@functools.lru_cache(maxsize=None)
def derm_lists(K, E):
    """for coded bit s K + t the ascending positions among the E rate-matched bits that carry it (synth.conv_ratematch run on indices)"""
    idx = load_pkg().synth.conv_ratematch(np.arange(3 * K, dtype=np.uint8).reshape(3, K), E).astype(np.int64)
    return [np.flatnonzero(idx == b) for b in range(3 * K)]


def crc16_int(bits):
    crc = 0
    for b in bits:
        msb = ((crc >> 15) & 1) ^ int(b)
        crc = (crc << 1) & 0xFFFF
        if msb:
            crc ^= 0x1021
    return crc


def dci_codeword(payload, rnti, L):
    """the 72 L bits of a DCI: payload + (CRC-16 ^ RNTI, MSB first), tail-biting code, rate matching (synth's encoders, which the
    PBCH tests pin to the oracle)"""
    synth = load_pkg().synth
    a = np.asarray(payload, np.uint8)
    par = crc16_int(a) ^ int(rnti)
    c = np.concatenate([a, np.array([(par >> (15 - t)) & 1 for t in range(16)], np.uint8)])
    return synth.conv_ratematch(synth.conv_encode_tailbite(c), 72 * L)


# ------------------------------------------------------------------ transmit: onto a grid
def plant(tfg, g, n_id, cp_type, ports, n_rb, cfi, dur, res, dcis, chan, fill=0.0, rng=None, mi=1):
    """puts the PDCCH of grid subframe g on tfg: dcis = [dict(rnti, bits, L, cce)]; every resource element of the PDCCH's REGs is
    overwritten (silent where no CCE is used; `fill`: that share of the unused CCEs gets random bits); chan(port, row, cols) is the
    channel.  Returns the layout."""
    synth = load_pkg().synth
    lay = layout(n_id, cp_type, ports, n_rb, cfi, dur, res, mi)
    n, n_cce = lay["n_reg"], lay["n_cce"]
    stream, used = np.zeros(8 * n, np.int64), np.zeros(n, bool)
    for d in dcis:
        L, cce = d["L"], d["cce"]
        assert cce + L <= n_cce and not used[9 * cce:9 * (cce + L)].any()
        stream[72 * cce:72 * (cce + L)] = dci_codeword(d["bits"], d["rnti"], L)
        used[9 * cce:9 * (cce + L)] = True
    for cce in range(n_cce):
        if fill > 0 and not used[9 * cce] and rng.random() < fill:
            stream[72 * cce:72 * (cce + 1)] = rng.integers(0, 2, 72)
            used[9 * cce:9 * (cce + 1)] = True
    b = stream ^ scrambling(n_id, g % 10, 8 * n)
    z = (((1 - 2.0 * b[0::2]) + 1j * (1 - 2.0 * b[1::2])) / np.sqrt(2.0)).reshape(n, 4) * used[:, None]
    q = quad_of_reg(n, n_id)
    row0 = 2 * g * PR.n_symb_of(cp_type)
    for i, (k, l) in enumerate(lay["order"]):
        cols = np.array(reg_columns(k, l, n_id, ports, cp_type))
        x = synth._tx_diversity(z[q[i]], ports)
        tfg[row0 + l, cols] = sum(x[p] * chan(p, row0 + l, cols) for p in range(ports))
    return lay


# ------------------------------------------------------------------ receive
def soft_bits(tfg, g, n_id, cp_type, ports, n_rb, lay):
    """the 1152 soft bits of grid subframe g (zeros beyond 9 N_CCE quadruplets)"""
    n, row0, sf = lay["n_reg"], 2 * g * PR.n_symb_of(cp_type), g % 10
    q = quad_of_reg(n, n_id)
    reg_of_quad = np.empty(n, np.int64)
    reg_of_quad[q] = np.arange(n)
    n_q = min(N_QUAD, 9 * lay["n_cce"])
    s = np.zeros(4 * N_QUAD, np.complex128)
    h_rows = {p: (tfg[row0 + (0 if p < 2 else 1)], PR.rs_row(n_id, cp_type, n_rb, 2 * sf, 0 if p < 2 else 1), PR.shift_of(p, n_id, 2 * sf)) for p in range(ports)}
    for u in range(n_q):
        k, l = lay["order"][reg_of_quad[u]]
        cols = np.array(reg_columns(k, l, n_id, ports, cp_type))
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
    llr = np.empty(N_LLR)
    llr[0::2], llr[1::2] = s.real, s.imag
    return llr * (1 - 2 * scrambling(n_id, sf, N_LLR))


_G = (0o133, 0o171, 0o165)
_WORD = np.array([[sum((bin(((b << 6) | p) & _G[j]).count("1") & 1) << j for j in range(3)) for p in range(64)] for b in range(2)])


def viterbi_tailbite(d):
    """d [3][K]: the tail-biting decoder that MINIMISES sum -(+-d): one trellis per start state, the end state forced equal, the lowest
    start state among the best end metrics -> (bits [K], end metrics [64] ascending by start state)"""
    K = d.shape[1]
    pm = np.where(np.eye(64, dtype=bool), 0.0, np.inf)            # [start, state]
    dec = np.zeros((K, 64, 64), bool)
    j = np.arange(32)
    with np.errstate(invalid="ignore"):
        for t in range(K):
            sgn = 1 - 2 * ((np.arange(8)[:, None] >> np.arange(3)[None, :]) & 1)      # word -> +-1 per generator
            bm = ((-sgn[:, 2] * d[2, t]) + (-sgn[:, 1] * d[1, t])) + (-sgn[:, 0] * d[0, t])
            new = np.empty_like(pm)
            for b in range(2):
                m0 = pm[:, 2 * j] + bm[_WORD[b, 2 * j]][None, :]
                m1 = pm[:, 2 * j + 1] + bm[_WORD[b, 2 * j + 1]][None, :]
                take = m1 < m0
                new[:, j + 32 * b] = np.where(take, m1, m0)
                dec[t][:, j + 32 * b] = take
            pm = new
    end = pm[np.arange(64), np.arange(64)]
    ss = int(np.argmin(np.where(np.isfinite(end), end, np.inf)))
    bits, s = np.zeros(K, np.int64), ss
    for t in range(K - 1, -1, -1):
        bits[t] = (s >> 5) & 1
        s = ((s << 1) & 63) | int(dec[t, ss, s])
    return bits, end


def decode_candidate(llr, cce, L, A, rnti_mask=7):
    """-> dict(bits int, rnti_x, flags, quality, gap): gap = (second-best - best end metric) / sum |coded bit| (inf when silent)"""
    K = A + 16
    cl = llr[72 * cce:72 * (cce + L)]
    d = np.array([cl[p].sum() if p.size else 0.0 for p in derm_lists(K, 72 * L)]).reshape(3, K)
    if not np.all(np.isfinite(d)):
        return dict(bits=0, rnti_x=0, flags=0, quality=0.0, gap=np.inf)
    bits, end = viterbi_tailbite(d)
    den = np.abs(d).sum()
    srt = np.sort(end)
    par = sum(int(bits[A + t]) << (15 - t) for t in range(16))
    rnti_x = crc16_int(bits[:A]) ^ par
    kind = 1 if rnti_x == 0xFFFF else 2 if rnti_x == 0xFFFE else 4 if 1 <= rnti_x <= 60 else 0
    return dict(bits=sum(int(bits[t]) << t for t in range(A)), rnti_x=rnti_x, flags=1 | (2 if kind & rnti_mask else 0),
                quality=float(-srt[0] / den) if den > 0 else 0.0, gap=float((srt[1] - srt[0]) / den) if den > 0 else np.inf)


def is_read(g, n_ofdm, cp_type, n_rb, dl_mask, dur=1, tdd=False):
    r0 = 2 * g * PR.n_symb_of(cp_type)
    if not (dl_mask >> (g % 10)) & 1 or r0 + (4 if n_rb <= 10 else 3) - 1 >= n_ofdm:
        return False
    return not (tdd and dur == 2 and g % 10 in (1, 6))


def receive(tfg, n_id, cp_type, n_ports, n_rb, cfi, dur, res, sizes, dl_mask=0x3FF, rnti_mask=7, mi=None):
    """the rule on a grid with the CFI of every subframe given (cfi [n_sf], 0: not decoded) -> dict: n_sf, cfi / n_reg / n_cce [n_sf],
    llr {g: [1152]}, dec {(g, slot, size index): decode_candidate's dict}, and the record's counts"""
    tfg = np.asarray(tfg, np.complex128)
    P, n_sf = PR.ports_of(n_ports), PR.n_sf_of(tfg.shape[0], cp_type)
    out = dict(n_sf=n_sf, cfi=np.zeros(n_sf, np.int32), n_reg=np.zeros(n_sf, np.int32), n_cce=np.zeros(n_sf, np.int32), llr={}, dec={})
    for g in range(n_sf):
        c = int(cfi[g])
        if not is_read(g, tfg.shape[0], cp_type, n_rb, dl_mask, dur, mi is not None) or not 1 <= c <= 3:
            continue
        lay = layout(n_id, cp_type, P, n_rb, c, dur, res, 1 if mi is None else mi[g % 10])
        if lay is None or lay["n_cce"] == 0:
            continue
        out["cfi"][g], out["n_reg"][g], out["n_cce"][g] = c, lay["n_reg"], lay["n_cce"]
        with np.errstate(all="ignore"):
            llr = out["llr"][g] = soft_bits(tfg, g, n_id, cp_type, P, n_rb, lay)
            for s, L, cce in candidates(lay["n_cce"]):
                for i, A in enumerate(sizes):
                    out["dec"][(g, s, i)] = decode_candidate(llr, cce, L, A, rnti_mask)
    acc = [d for d in out["dec"].values() if d["flags"] & 2]
    out.update(n_read=int((out["cfi"] > 0).sum()), n_accepted=len(acc), n_si=sum(d["rnti_x"] == 0xFFFF for d in acc),
               n_paging=sum(d["rnti_x"] == 0xFFFE for d in acc), n_ra=sum(1 <= d["rnti_x"] <= 60 for d in acc))
    return out
