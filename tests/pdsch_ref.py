"""numpy statement of the PDSCH rule (include/lcs.h: lcs_pdsch_info), transmit and receive side, written from 36.211 6.3 / 6.4, 36.212
5.1.1 / 5.1.3.2 / 5.1.4.1, 36.213 7.1.7 and the rule's text, not from the product's header: the reference of every test of that stage.
Grid, subframes, reference signals, channel values and combining as tests/pcfich_ref.py; grants as tests/pdcch_ref.py.

What is pinned to the reference project elsewhere: the Gold bits and the reference signals (test_pdsch_ref.py ties this file's to
them).  What rests on this file's reading of the standard alone: the resource map, the turbo code, its rate matching and the decoder.
The transport block sizes and the QPP parameters are the product's numbers (capi._TBS_1A, synth.TURBO_QPP), from memory of the
standard: bijection and "size + 24 is a block size" are what pin them.

The decoder comes in two forms from one function: windows of 32 steps vectorised over the windows (the rule), and one window as
long as the block (plain max-log-MAP), for comparison."""
import functools

import numpy as np

import pcfich_ref as PR
import pdcch_ref as DR
from conftest import load_pkg

WIN = 32
STATUS = dict(ok=1, crc=2, distributed=3, mcs=4, rows=5, special=6, silent=7, bad_alloc=8, no_cfi=9)
# the constituent code: state (r1, r2, r3) as 4 r1 + 2 r2 + r3, a = u ^ r2 ^ r3 fed back (1 + D^2 + D^3), parity a ^ r1 ^ r3 (1 + D + D^3)
NEXT = np.zeros((8, 2), np.int64)
PAR = np.zeros((8, 2), np.int64)
for _s in range(8):
    _r1, _r2, _r3 = _s >> 2, (_s >> 1) & 1, _s & 1
    for _u in range(2):
        _a = _u ^ _r2 ^ _r3
        NEXT[_s, _u], PAR[_s, _u] = 4 * _a + 2 * _r1 + _r2, _a ^ _r1 ^ _r3
# the two branches into every state: from P0 with input 0, from P1 with input 1
P0 = np.array([next(s for s in range(8) if NEXT[s, 0] == n) for n in range(8)])
P1 = np.array([next(s for s in range(8) if NEXT[s, 1] == n) for n in range(8)])
GI0, GI1 = PAR[P0, 0], 2 + PAR[P1, 1]


def block_size(tbs):
    """(K, F) of a transport block of tbs bits: one code block"""
    K = next(k for k in load_pkg().synth.TURBO_K if k >= tbs + 24)
    return K, K - (tbs + 24)


def fields_1a(bits, n_rb, tdd):
    """capi.dci_1a_fields restated for an int payload (bit t = the t-th bit sent)"""
    nb = (n_rb * (n_rb + 1) // 2 - 1).bit_length()
    seq = [(bits >> t) & 1 for t in range(64)]
    pos = [0]

    def take(n):
        v = 0
        for b in seq[pos[0]:pos[0] + n]:
            v = (v << 1) | b
        pos[0] += n
        return v
    f = dict(flag=take(1), distributed=take(1))
    riv = take(nb)
    length, start = riv // n_rb + 1, riv % n_rb
    if length + start > n_rb:
        length, start = n_rb - length + 2, n_rb - 1 - start
    f.update(rb_start=start, n_prb=length, mcs=take(5))
    take(4 if tdd else 3)
    take(1)
    f.update(rv=take(2), tpc=take(2))
    return f


@functools.lru_cache(maxsize=None)
def elements(n_id, cp_type, ports, n_rb, sf, n_ctrl, rb_start, n_prb, tdd):
    """[(l, k)] in mapping order, by brute force over the allocation"""
    n = PR.n_symb_of(cp_type)
    out = []
    for l in range(n_ctrl, 2 * n):
        slot, ls = 2 * sf + l // n, l % n
        crs = set()
        if ls in (0, n - 3):
            crs = {PR.shift_of(p, n_id, slot) if ls == 0 else (PR.shift_of(p, n_id, slot) + 3) % 6 for p in range(min(ports, 2))}
            if ports >= 2:
                crs = {c % 3 for c in crs} | {c % 3 + 3 for c in crs}
        elif ls == 1 and ports == 4:
            crs = {PR.shift_of(2, n_id, slot), PR.shift_of(3, n_id, slot)}
            crs = {c % 3 for c in crs} | {c % 3 + 3 for c in crs}
        central = (sf == 0 and n <= l < n + 4) or (sf in (0, 5) and (l == 2 * n - 1 if tdd else l in (n - 2, n - 1)))
        for k in range(12 * rb_start, 12 * (rb_start + n_prb)):
            if k % 6 in crs or (central and 6 * n_rb - 36 <= k < 6 * n_rb + 36):
                continue
            out.append((l, k))
    return out


def ref_rows(port, cp_type):
    """the symbols of a subframe that carry the port's reference elements, with the shift's change against the slot's first"""
    n = PR.n_symb_of(cp_type)
    return [(0, 0), (n - 3, 3), (n, 0), (2 * n - 3, 3)] if port < 2 else [(1, 0), (n + 1, 0)]


def channel_at(tfg, row0, n_id, cp_type, n_rb, sf, port, ls, ks):
    """h of the port at the elements (ls[i], ks[i]): per reference row PR.channel, linear in time between the rows that bracket l"""
    n = PR.n_symb_of(cp_type)
    rows = ref_rows(port, cp_type)
    H = []
    for l, dv in rows:
        slot, sym = 2 * sf + l // n, l % n
        shift = (PR.shift_of(port, n_id, slot) + dv) % 6
        H.append(PR.channel(tfg[row0 + l], PR.rs_row(n_id, cp_type, n_rb, slot, sym), shift, ks))
    L = np.array([l for l, _ in rows])
    out = np.empty(len(ks), np.complex128)
    for i, l in enumerate(ls):
        ia = np.flatnonzero(L <= l)
        ib = np.flatnonzero(L >= l)
        a = ia[-1] if ia.size else 0
        b = ib[0] if ib.size else len(L) - 1
        if a == b or l <= L[a]:
            out[i] = H[a][i]
        elif l >= L[b]:
            out[i] = H[b][i]
        else:
            t = float(l - L[a]) / float(L[b] - L[a])
            out[i] = complex(H[a][i].real + (H[b][i].real - H[a][i].real) * t, H[a][i].imag + (H[b][i].imag - H[a][i].imag) * t)
    return out


@functools.lru_cache(maxsize=None)
def scrambling(rnti, sf, n_id, n):
    return load_pkg().synth._pn((rnti << 14) + sf * 512 + n_id, n).astype(np.int64)


def soft_bits(tfg, g, n_id, cp_type, ports, n_rb, n_ctrl, rb_start, n_prb, rnti, tdd):
    """the G = 2 N_RE soft bits of a grant in grid subframe g"""
    n, sf = PR.n_symb_of(cp_type), g % 10
    el = elements(n_id, cp_type, ports, n_rb, sf, n_ctrl, rb_start, n_prb, tdd)
    if not el:
        return np.zeros(0)
    ls, ks = np.array([l for l, _ in el]), np.array([k for _, k in el])
    row0 = 2 * g * n
    y = tfg[row0 + ls, ks]
    h = {p: channel_at(tfg, row0, n_id, cp_type, n_rb, sf, p, ls, ks) for p in range(ports)}
    N = len(el)
    s = np.zeros(N, np.complex128)
    if ports == 1:
        s = np.conj(h[0]) * y
    else:
        yy = np.concatenate([y, [0.0]])
        for e in range(N):
            pair = (e >> 1) & 1
            a, b = (pair, pair + 2) if ports == 4 else (0, 1)
            o = e ^ 1
            hb = h[b][o] if o < N else 0.0
            t1, t2 = np.conj(h[a][e]) * y[e], hb * np.conj(yy[min(o, N)])
            s[e] = t1 - t2 if e & 1 else t1 + t2
    llr = np.empty(2 * N)
    llr[0::2], llr[1::2] = s.real, s.imag
    return llr * (1 - 2 * scrambling(rnti, sf, n_id, 2 * N))


@functools.lru_cache(maxsize=None)
def derm_index(K, F, rv):
    """(order, N): order[r] = s (K + 4) + k of the value that the non-null of rank r counted from k0 is (synth.turbo_ratematch run on
    indices over one turn of the circular buffer)"""
    synth = load_pkg().synth
    D = K + 4
    idx = np.arange(3 * D, dtype=np.int64).reshape(3, D)
    N = 3 * D - 2 * F
    return synth.turbo_ratematch(idx, N, rv, F), N


def derm(llr, K, F, rv):
    """d [3][K + 4]: every value the sum of its soft bits in ascending e (0 for a null)"""
    order, N = derm_index(K, F, rv)
    assert len(set(order.tolist())) == N
    d = np.zeros(3 * (K + 4))
    for rep in range(-(-len(llr) // N) if len(llr) else 0):
        part = llr[rep * N:(rep + 1) * N]
        d[order[:len(part)]] = d[order[:len(part)]] + part
    return d.reshape(3, K + 4)


def crc24a_int(bits):
    crc = 0
    for b in bits:
        msb = ((crc >> 23) & 1) ^ int(b)
        crc = (crc << 1) & 0xFFFFFF
        if msb:
            crc ^= 0x864CFB
    return crc


def tail_beta(x, z):
    b = np.where(np.arange(8) == 0, 0.0, -np.inf)
    for t in (2, 1, 0):
        nb = np.empty(8)
        for s in range(8):
            r1, r2, r3 = s >> 2, (s >> 1) & 1, s & 1
            u, zz = r2 ^ r3, r1 ^ r3
            nb[s] = 0.5 * ((-x[t] if u else x[t]) + (-z[t] if zz else z[t])) + b[2 * r1 + r2]
        b = nb
    return b


def half_iteration(sys_, par, ext, jmap, F, A, B, win):
    """one constituent decoder over all windows at once.  sys_, ext indexed by jmap[k]; par by k.  A [n_win + 1][8]: forward metrics at
    the window boundaries (row w: start of window w), B likewise backward; both are read as they stand and rewritten for the next
    iteration.  -> posterior L [K] in the decoder's own order (nan at filler steps)"""
    K = len(jmap)
    n_win = -(-K // win)
    k = np.arange(n_win)[:, None] * win + np.arange(win)[None, :]
    live = k < K
    kk = np.where(live, k, 0)
    j = jmap[kk]
    ls, lp = sys_[j], par[kk]
    filler = (j < F) & live
    a = A[:n_win].copy()
    b = B[1:n_win + 1].copy()
    alphas = np.empty((win, n_win, 8))
    with np.errstate(invalid="ignore"):
        for t in range(win):
            alphas[t] = a
            x = ls[:, t] + ext[j[:, t]]
            g = np.stack([0.5 * (x + lp[:, t]), 0.5 * (x - lp[:, t]), 0.5 * (-x + lp[:, t]), 0.5 * (-x - lp[:, t])], axis=1)
            n0, n1 = a[:, P0] + g[:, GI0], a[:, P1] + g[:, GI1]
            nx = np.where(filler[:, t, None], n0, np.maximum(n0, n1))
            a = np.where(live[:, t, None], nx, a)
        L = np.full(K, np.nan)
        for t in range(win - 1, -1, -1):
            la = ext[j[:, t]]
            x = ls[:, t] + la
            g = np.stack([0.5 * (x + lp[:, t]), 0.5 * (x - lp[:, t]), 0.5 * (-x + lp[:, t]), 0.5 * (-x - lp[:, t])], axis=1)
            t0, t1 = g[:, PAR[:, 0]] + b[:, NEXT[:, 0]], g[:, 2 + PAR[:, 1]] + b[:, NEXT[:, 1]]
            nb = np.where(filler[:, t, None], t0, np.maximum(t0, t1))
            m0, m1 = (alphas[t] + t0).max(axis=1), (alphas[t] + t1).max(axis=1)
            post = m0 - m1
            upd = live[:, t] & ~filler[:, t]
            L[kk[upd, t]] = post[upd]
            ext[j[upd, t]] = 0.75 * ((post[upd] - ls[upd, t]) - la[upd])
            b = np.where(live[:, t, None], nb, b)
    A[1:n_win] = a[:n_win - 1]
    B[1:n_win] = b[1:]
    return L


def turbo_decode(d, K, F=0, max_iter=8, win=WIN):
    """the rule's decoder on d [3][K + 4] -> dict(status, n_iter, bits [K], margin): margin = the smallest non-zero |posterior| of the
    second decoder over all iterations run, relative to the largest of that iteration (inf for a block that is not decoded)"""
    synth = load_pkg().synth
    d = np.asarray(d, np.float64)
    if not np.all(np.isfinite(d)) or not np.any(d != 0.0):
        return dict(status=STATUS["silent"], n_iter=0, bits=np.zeros(K, np.uint8), margin=np.inf)
    perm = synth.turbo_interleaver(K)
    ident = np.arange(K)
    n_win = -(-K // win)
    x1, z1 = [d[0, K], d[2, K], d[1, K + 1]], [d[1, K], d[0, K + 1], d[2, K + 1]]
    x2, z2 = [d[0, K + 2], d[2, K + 2], d[1, K + 3]], [d[1, K + 2], d[0, K + 3], d[2, K + 3]]
    AB = []
    for x, z in ((x1, z1), (x2, z2)):
        A, B = np.zeros((n_win + 1, 8)), np.zeros((n_win + 1, 8))
        A[0, 1:] = -np.inf
        B[n_win] = tail_beta(x, z)
        AB.append((A, B))
    ext = np.zeros(K)
    bits, margin, n_iter, ok = np.zeros(K, np.uint8), np.inf, 0, False
    for it in range(1, max_iter + 1):
        half_iteration(d[0, :K], d[1, :K], ext, ident, F, AB[0][0], AB[0][1], win)
        L = half_iteration(d[0, :K], d[2, :K], ext, perm, F, AB[1][0], AB[1][1], win)
        val = ~np.isnan(L)
        nz = val & (L != 0.0)                        # (an exact zero is a tie of equal sums on both sides of the comparison: it decides 0)
        if nz.any():
            margin = min(margin, float(np.abs(L[nz]).min() / np.abs(L[nz]).max()))
        bits = np.zeros(K, np.uint8)
        bits[perm[val]] = L[val] < 0
        n_iter, ok = it, crc24a_int(bits[F:]) == 0
        if ok:
            break
    return dict(status=STATUS["ok"] if ok else STATUS["crc"], n_iter=n_iter, bits=bits, margin=margin)


def payload_bytes(bits, F, tbs):
    a = np.concatenate([bits[F:F + tbs], np.zeros(-tbs % 8, np.uint8)])
    return np.concatenate([np.packbits(a), np.zeros(280, np.uint8)])[:280]


def kind_of(rnti):
    return 1 if rnti == 0xFFFF else 2 if rnti == 0xFFFE else 4 if 1 <= rnti <= 60 else 0


def whole(g, n_ofdm, cp_type):
    return 2 * (g + 1) * PR.n_symb_of(cp_type) <= n_ofdm


def grants_of(pdc_dec, g, i_1a, n_rb, tdd, rnti_mask=7):
    """the at most two grants of subframe g from the accepted decodes {(g, slot, i): dict(bits, rnti_x, flags)}"""
    capi = load_pkg().capi
    out, seen = [], set()
    for s in range(DR.SLOTS):
        d = pdc_dec.get((g, s, i_1a))
        if d is None or not d["flags"] & 2 or not d["bits"] & 1 or not kind_of(d["rnti_x"]) & rnti_mask:
            continue
        if (d["bits"], d["rnti_x"]) in seen:
            continue
        seen.add((d["bits"], d["rnti_x"]))
        if len(out) == 2:
            break
        f = fields_1a(d["bits"], n_rb, tdd)
        st = STATUS["distributed"] if f["distributed"] else STATUS["mcs"] if f["mcs"] > 26 else 0
        out.append(dict(subframe=g, slot=s, rnti=d["rnti_x"], rb_start=f["rb_start"], n_prb=f["n_prb"], mcs=f["mcs"], rv=f["rv"],
                        tbs=0 if st else capi.tbs_1a(f["mcs"], f["tpc"]), status=st))
    return out


def receive(tfg, n_id, cp_type, n_ports, n_rb, pdc, i_1a=0, tdd=False, dl_mask=0x3FF, dur=1, max_iter=8, forced=None, rnti_mask=7, win=WIN):
    """the rule on a grid, given pdcch_ref.receive's dict (its cfi and dec) -> list of block dicts in (subframe, slot) order with
    llr, d and margin beside the record's fields"""
    tfg = np.asarray(tfg, np.complex128)
    P, n_sf = PR.ports_of(n_ports), PR.n_sf_of(tfg.shape[0], cp_type)
    blocks = []
    for g in range(n_sf):
        sf = g % 10
        cfi = int(pdc["cfi"][g])
        if forced:
            gr = [dict(subframe=g, slot=f, rnti=x[1], rb_start=x[2], n_prb=x[3], mcs=-1, rv=x[5], tbs=x[4], status=0) for f, x in enumerate(forced) if x[0] == g][:2]
        else:
            gr = grants_of(pdc["dec"], g, i_1a, n_rb, tdd, rnti_mask) if cfi else []
        for b in gr:
            b.update(kind=kind_of(b["rnti"]), n_re=0, K=0, F=0, n_iter=0, payload=np.zeros(280, np.uint8), margin=np.inf)
            read = DR.is_read(g, tfg.shape[0], cp_type, n_rb, dl_mask, dur, tdd)
            if not b["status"]:
                if b["rb_start"] < 0 or b["n_prb"] < 1 or b["rb_start"] + b["n_prb"] > n_rb:
                    b["status"] = STATUS["bad_alloc"]
                elif tdd and sf in (1, 6):
                    b["status"] = STATUS["special"]
                elif not (read and whole(g, tfg.shape[0], cp_type)):
                    b["status"] = STATUS["rows"]
                elif not 1 <= cfi <= 3:
                    b["status"] = STATUS["no_cfi"]
            blocks.append(b)
            if b["status"]:
                continue
            K, F = block_size(b["tbs"])
            n_ctrl = DR.n_ctrl_of(cfi, n_rb)
            with np.errstate(all="ignore"):
                llr = soft_bits(tfg, g, n_id, cp_type, P, n_rb, n_ctrl, b["rb_start"], b["n_prb"], b["rnti"], tdd)
                d = derm(llr, K, F, b["rv"])
            res = turbo_decode(d, K, F, max_iter, win)
            b.update(n_re=len(llr) // 2, K=K, F=F, n_iter=res["n_iter"], status=res["status"], margin=res["margin"], llr=llr, d=d)
            if res["status"] in (1, 2):
                b["payload"] = payload_bytes(res["bits"], F, b["tbs"])
    return blocks


# ------------------------------------------------------------------ transmit: onto a grid
def plant(tfg, g, n_id, cp_type, ports, n_rb, cfi, grant, chan, tdd=False, silent=False):
    """puts the PDSCH of one grant (dict(rnti, rb_start, n_prb, rv, bits)) on grid subframe g through synth.pdsch_region; silent:
    its elements are cleared instead"""
    synth = load_pkg().synth
    row0 = 2 * g * PR.n_symb_of(cp_type)
    for l, cols, x in synth.pdsch_region(n_id, n_rb, ports, cp_type == 1, g % 10, cfi, grant, tdd):
        tfg[row0 + l, cols] = 0.0 if silent else sum(x[p] * chan(p, row0 + l, cols) for p in range(ports))
