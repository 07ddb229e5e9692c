"""numpy statement of the rule for distributed allocations and format 1C (include/lcs.h: lcs_pdsch_alloc_cfg), written from that text,
not from the product's header: the VRB to PRB map, the 1C fields and sizes, the assumed redundancy version, the elements over a
per-slot set of resource blocks, and the PDSCH receiver of tests/pdsch_ref.py with the setting.  Everything the setting does not
touch (channel, combining, de-rate-matching, decoder) is tests/pdsch_ref.py's.

The rule is this project's reading of 36.211 6.2.3.2, 36.212 5.3.3.1.3 / .4, 36.213 7.1.6.3 / 7.1.7.2.3 and 36.321 5.3.1, from memory of
the standard.  What pins it (tests/test_pdsch_dvrb_host.py): every slot's map is a permutation into [0, n_rb), the two PRBs of a VRB
lie exactly N_gap apart, N_VRB <= n_rb, the 1C width is the PDCCH table's, every 1C size + 24 is a turbo block size."""
import functools

import numpy as np

import pcfich_ref as PR
import pdcch_ref as DR
import pdsch_ref as SR

TBS_1C = [40, 56, 72, 120, 136, 144, 176, 208, 224, 256, 280, 296, 328, 336, 392, 488, 552, 600, 632, 696, 776, 840, 904, 1000, 1064, 1128, 1224, 1288, 1384, 1480,
          1608, 1736]
GAP_TABLE = [(6, 10, None, None), (11, 11, 4, None), (12, 19, 8, None), (20, 26, 12, None), (27, 44, 18, None), (45, 49, 27, None), (50, 63, 27, 9), (64, 79, 32, 16),
             (80, 110, 48, 16)]


def gaps(n_rb):
    """(N_gap,1, N_gap,2 or None)"""
    lo, hi, g1, g2 = next(r for r in GAP_TABLE if r[0] <= n_rb <= r[1])
    return (-(-n_rb // 2) if g1 is None else g1), g2


@functools.lru_cache(maxsize=None)
def sizes(n_rb, gap):
    """dict(n_gap, n_vrb, unit, n_row, n_null) of gap index 0 / 1"""
    n_gap = gaps(n_rb)[gap]
    n_vrb = 2 * min(n_gap, n_rb - n_gap) if gap == 0 else (n_rb // (2 * n_gap)) * 2 * n_gap
    unit = n_vrb if gap == 0 else 2 * n_gap
    P = 1 if n_rb <= 10 else 2 if n_rb <= 26 else 3 if n_rb <= 63 else 4
    n_row = -(-unit // (4 * P)) * P
    return dict(n_gap=n_gap, n_vrb=n_vrb, unit=unit, n_row=n_row, n_null=4 * n_row - unit)


def prb_of(n_rb, gap, v, slot):
    z = sizes(n_rb, gap)
    N, n_row, n_null = z["unit"], z["n_row"], z["n_null"]
    t, o = v % N, N * (v // N)
    a = 2 * n_row * (t % 2) + t // 2
    b = n_row * (t % 4) + t // 4
    if n_null != 0 and t >= N - n_null and t % 2 == 1:
        r = a - n_row
    elif n_null != 0 and t >= N - n_null and t % 2 == 0:
        r = a - n_row + n_null // 2
    elif n_null != 0 and t < N - n_null and t % 4 >= 2:
        r = b - n_null // 2
    else:
        r = b
    if slot % 2 == 1:
        r = (r + N // 2) % N
    return o + (r if r < N // 2 else r + z["n_gap"] - N // 2)


def n_step_of(n_rb):
    return 2 if n_rb < 50 else 4


def riv_bits_1c(n_rb):
    v1 = sizes(n_rb, 0)["n_vrb"] // n_step_of(n_rb)
    return int(np.ceil(np.log2(v1 * (v1 + 1) / 2)))


def size_1c(n_rb):
    return (1 if n_rb >= 50 else 0) + riv_bits_1c(n_rb) + 5


def fields_1c(bits, n_rb):
    """the fields of an int payload (bit t = the t-th bit sent)"""
    seq = [(bits >> t) & 1 for t in range(64)]
    pos = [0]

    def take(n):
        v = 0
        for b in seq[pos[0]:pos[0] + n]:
            v = (v << 1) | b
        pos[0] += n
        return v
    gap = take(1) if n_rb >= 50 else 0
    step = n_step_of(n_rb)
    riv = take(riv_bits_1c(n_rb))
    n = sizes(n_rb, gap)["n_vrb"] // step
    length, start = riv // n + 1, riv % n
    if length + start > n:
        length, start = n - length + 2, n - 1 - start
    return dict(gap=gap, riv=riv, riv_ok=riv < n * (n + 1) // 2, rb_start=step * start, n_prb=step * length, n_step=step, i_tbs=take(5))


def pack_1c(gap, rb_start, n_prb, i_tbs, n_rb, riv=None):
    """the payload bits of format 1C in the order sent; riv: a raw RIV in place of (rb_start, n_prb)"""
    step = n_step_of(n_rb)
    n = sizes(n_rb, gap)["n_vrb"] // step
    if riv is None:
        L, S = n_prb // step, rb_start // step
        riv = n * (L - 1) + S if L - 1 <= n // 2 else n * (n - L + 1) + (n - 1 - S)
    out = []
    for v, w in ([(gap, 1)] if n_rb >= 50 else []) + [(riv, riv_bits_1c(n_rb)), (i_tbs, 5)]:
        out += [(v >> (w - 1 - i)) & 1 for i in range(w)]
    return out


def rv_1c(kind, g, sfn0, si_window):
    """the redundancy version a 1C grant is assumed to have"""
    if kind != 1 or sfn0 < 0:
        return 0
    sfn, sf = (sfn0 + g // 10) % 1024, g % 10
    if sf == 5 and sfn % 2 == 0:
        k = (sfn // 2) % 4
    elif si_window > 0 and si_window != 15:
        k = ((10 * sfn + sf) % si_window) % 4
    else:
        return 0
    return -(-3 * k // 2) % 4


def prb_lists(n_rb, gap, rb_start, n_prb):
    return [[prb_of(n_rb, gap, v, s) for v in range(rb_start, rb_start + n_prb)] for s in range(2)]


@functools.lru_cache(maxsize=None)
def elements(n_id, cp_type, ports, n_rb, sf, n_ctrl, gap, rb_start, n_prb, tdd):
    """[(l, k)] in mapping order, by brute force: the localized enumeration of every resource block of the slot's set"""
    n = PR.n_symb_of(cp_type)
    sets = [sorted(s) for s in prb_lists(n_rb, gap, rb_start, n_prb)]
    per_rb = {}
    out = []
    for l in range(n_ctrl, 2 * n):
        for p in sets[l // n]:
            if p not in per_rb:
                per_rb[p] = SR.elements(n_id, cp_type, ports, n_rb, sf, n_ctrl, p, 1, tdd)
            out += [e for e in per_rb[p] if e[0] == l]
    return out


def soft_bits(tfg, g, n_id, cp_type, ports, n_rb, el, rnti):
    """tests/pdsch_ref.py's soft bits over a given element list"""
    n, sf = PR.n_symb_of(cp_type), g % 10
    if not el:
        return np.zeros(0)
    ls, ks = np.array([l for l, _ in el]), np.array([k for _, k in el])
    row0 = 2 * g * n
    y = tfg[row0 + ls, ks]
    h = {p: SR.channel_at(tfg, row0, n_id, cp_type, n_rb, sf, p, ls, ks) for p in range(ports)}
    N = len(el)
    if ports == 1:
        s = np.conj(h[0]) * y
    else:
        s = np.zeros(N, np.complex128)
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
    return llr * (1 - 2 * SR.scrambling(rnti, sf, n_id, 2 * N))


def grants_of(pdc_dec, g, i_1a, n_rb, tdd, flags, sfn0, si_window, rnti_mask=7):
    """the at most two grants of subframe g: by ascending slot, then size index"""
    from conftest import load_pkg
    capi = load_pkg().capi
    out, seen = [], set()
    for s in range(DR.SLOTS):
        for i in range(2):
            is_1c = bool(flags & 2) and i == 1 - i_1a
            if i != i_1a and not is_1c:
                continue
            d = pdc_dec.get((g, s, i))
            if d is None or not d["flags"] & 2 or not SR.kind_of(d["rnti_x"]) & rnti_mask or (not is_1c and not d["bits"] & 1):
                continue
            if (d["bits"], d["rnti_x"], i) in seen or len(out) == 2:
                continue
            seen.add((d["bits"], d["rnti_x"], i))
            b = dict(subframe=g, slot=s, rnti=d["rnti_x"], status=0, tbs=0, gap=0, set=False, format="1a", distributed=0)
            if is_1c:
                f = fields_1c(d["bits"], n_rb)
                b.update(rb_start=f["rb_start"], n_prb=f["n_prb"], mcs=f["i_tbs"], rv=rv_1c(SR.kind_of(d["rnti_x"]), g, sfn0, si_window), gap=f["gap"], set=True,
                         format="1c", distributed=1)
                if not f["riv_ok"]:
                    b["status"] = SR.STATUS["bad_alloc"]
                else:
                    b["tbs"] = TBS_1C[f["i_tbs"]]
            else:
                f = SR.fields_1a(d["bits"], n_rb, tdd)
                ndi = (d["bits"] >> (2 + (n_rb * (n_rb + 1) // 2 - 1).bit_length() + 5 + (4 if tdd else 3))) & 1
                b.update(rb_start=f["rb_start"], n_prb=f["n_prb"], mcs=f["mcs"], rv=f["rv"], distributed=f["distributed"])
                if f["distributed"] and flags & 1:
                    b.update(set=True, gap=1 if n_rb >= 50 and ndi else 0)
                if f["distributed"] and not flags & 1:
                    b["status"] = SR.STATUS["distributed"]
                elif f["mcs"] > 26:
                    b["status"] = SR.STATUS["mcs"]
                else:
                    b["tbs"] = capi.tbs_1a(f["mcs"], f["tpc"])
            out.append(b)
    return out


def alloc_of(b, n_rb):
    """what lcs_pdsch_last_alloc says of the block"""
    unread = b["distributed"] and not b["set"]
    z = sizes(n_rb, b["gap"]) if b["distributed"] else dict(n_gap=0, n_vrb=n_rb)
    inside = not unread and b["rb_start"] >= 0 and b["n_prb"] >= 1 and b["rb_start"] + b["n_prb"] <= z["n_vrb"]
    n = b["n_prb"] if inside else 0
    lists = prb_lists(n_rb, b["gap"], b["rb_start"], n) if b["set"] else [list(range(b["rb_start"], b["rb_start"] + n))] * 2
    return dict(format=b["format"], distributed=int(bool(b["distributed"])), gap=b["gap"], n_gap=z["n_gap"], n_vrb=z["n_vrb"],
                n_step=n_step_of(n_rb) if b["format"] == "1c" else 1, n_prb=n, prb=[list(x) for x in lists])


def receive(tfg, n_id, cp_type, n_ports, n_rb, pdc, flags, sfn0=-1, si_window=0, i_1a=0, tdd=False, dl_mask=0x3FF, dur=1, max_iter=8, rnti_mask=7):
    """tests/pdsch_ref.py's receive with the setting -> its block dicts, with alloc beside them"""
    tfg = np.asarray(tfg, np.complex128)
    P, n_sf = PR.ports_of(n_ports), PR.n_sf_of(tfg.shape[0], cp_type)
    blocks = []
    for g in range(n_sf):
        sf, cfi = g % 10, int(pdc["cfi"][g])
        for b in (grants_of(pdc["dec"], g, i_1a, n_rb, tdd, flags, sfn0, si_window, rnti_mask) if cfi else []):
            b.update(kind=SR.kind_of(b["rnti"]), n_re=0, K=0, F=0, n_iter=0, payload=np.zeros(280, np.uint8), margin=np.inf, alloc=alloc_of(b, n_rb))
            read = DR.is_read(g, tfg.shape[0], cp_type, n_rb, dl_mask, dur, tdd)
            if not b["status"]:
                limit = sizes(n_rb, b["gap"])["n_vrb"] if b["set"] else n_rb
                if b["rb_start"] < 0 or b["n_prb"] < 1 or b["rb_start"] + b["n_prb"] > limit:
                    b["status"] = SR.STATUS["bad_alloc"]
                elif tdd and sf in (1, 6):
                    b["status"] = SR.STATUS["special"]
                elif not (read and SR.whole(g, tfg.shape[0], cp_type)):
                    b["status"] = SR.STATUS["rows"]
                elif not 1 <= cfi <= 3:
                    b["status"] = SR.STATUS["no_cfi"]
            blocks.append(b)
            if b["status"]:
                continue
            K, F = SR.block_size(b["tbs"])
            n_ctrl = DR.n_ctrl_of(cfi, n_rb)
            if b["set"]:
                el = elements(n_id, cp_type, P, n_rb, sf, n_ctrl, b["gap"], b["rb_start"], b["n_prb"], tdd)
            else:
                el = SR.elements(n_id, cp_type, P, n_rb, sf, n_ctrl, b["rb_start"], b["n_prb"], tdd)
            with np.errstate(all="ignore"):
                llr = soft_bits(tfg, g, n_id, cp_type, P, n_rb, el, b["rnti"])
                d = SR.derm(llr, K, F, b["rv"])
            res = SR.turbo_decode(d, K, F, max_iter)
            b.update(n_re=len(llr) // 2, K=K, F=F, n_iter=res["n_iter"], status=res["status"], margin=res["margin"], llr=llr, d=d)
            if res["status"] in (1, 2):
                b["payload"] = SR.payload_bytes(res["bits"], F, b["tbs"])
    return blocks
