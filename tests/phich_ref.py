"""numpy statement of the PHICH rule (include/lcs.h: lcs_phich_info), written from the rule's text and 36.211 6.9, not from the
product's header: the reference of every test of that stage.  The REG list is synth.pdcch_layout's `phich` list (the generator's,
pinned to the product's by tests/test_phich_host.py); the reference signals, the channel and the scrambling are tests/pcfich_ref.py's.

decode() works subframe by subframe: the elements of every unit, the channel of the pair's ports at their columns, the combining,
the descrambling, the despreading against the eight (four) sequences per repetition, the weighted mean of the three repetitions,
their spread as the noise, and the decision."""
import numpy as np

import pcfich_ref as PR
from conftest import load_pkg

MAX_HI = 1024
# 36.211 table 6.9.1-2
W4 = np.array([[1, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1]], np.complex128)
SEQ = {1: np.concatenate([W4, 1j * W4]), 2: np.array([[1, 1], [1, -1], [1j, 1j], [1j, -1j]], np.complex128)}
AXIS = (1 + 1j) / np.sqrt(2.0)


def n_seq_of(cp_type):
    return 8 if cp_type == 1 else 4


def n_units(n_rb, phich_resource, mi=1):
    num, den = ((1, 6), (1, 2), (1, 1), (2, 1))[phich_resource - 1]
    return int(mi) * -(-(num * n_rb) // (8 * den))


def units(n_id_cell, n_rb, n_ports, cp_type, phich_duration, phich_resource, mi):
    """-> (l [U][3], cols [U][3][4]) of the mapping units of m_i, None for a refused map"""
    if mi == 0:
        return np.zeros((0, 3), np.int64), np.zeros((0, 3, 4), np.int64)
    try:
        _, _, regs, cols = load_pkg().synth.pdcch_layout(n_id_cell, n_rb, PR.ports_of(n_ports), cp_type == 1, 3, phich_duration == 2, phich_resource - 1, mi)
    except ValueError:
        return None
    U = len(regs) // 3
    assert U == n_units(n_rb, phich_resource, mi)
    l = np.array([r[1] for r in regs], np.int64).reshape(U, 3)
    c = np.array([cols(k, ll) for k, ll in regs], np.int64).reshape(U, 3, 4)
    return l, c


def rows_needed(n_ports, phich_duration):
    return 3 if phich_duration == 2 else 2 if PR.ports_of(n_ports) == 4 else 1


def subframe_read(g, n_ofdm, cp_type, n_ports, phich_duration, tdd, dl_mask):
    n = PR.n_symb_of(cp_type)
    if not (dl_mask >> (g % 10)) & 1 or 2 * g * n + rows_needed(n_ports, phich_duration) - 1 >= n_ofdm:
        return False
    return not (tdd and phich_duration == 2 and g % 10 in (1, 6))


def decode_subframe(tfg, g, n_id_cell, cp_type, n_ports, n_rb, un):
    """-> (value, dsum, S) [n_group][n_seq] of grid subframe g with the units un; value 0 / dsum 0 marks an entry that does not read"""
    P, n = PR.ports_of(n_ports), PR.n_symb_of(cp_type)
    r0, sf = 2 * g * n, g % 10
    l, cols = un
    U, n_sf, n_seq = l.shape[0], (4 if cp_type == 1 else 2), n_seq_of(cp_type)
    if U == 0:
        z = np.zeros((0, n_seq))
        return z, z.copy(), z.copy()
    with np.errstate(all="ignore"):
        y = tfg[r0 + l[:, :, None], cols]                               # [U][3][4]
        flat = cols.reshape(-1)
        h = [PR.channel(tfg[r0 + (0 if p < 2 else 1)], PR.rs_row(n_id_cell, cp_type, n_rb, 2 * sf, 0 if p < 2 else 1), PR.shift_of(p, n_id_cell, 2 * sf), flat).reshape(U, 3, 4)
             for p in range(P)]
        if P == 1:
            s, G = np.conj(h[0]) * y, np.abs(h[0]) ** 2
        else:
            if P == 4:
                q = (np.arange(3)[None, :] + np.arange(U)[:, None]) & 1      # quadruplet i of unit m': ports (q, q + 2)
                ha = np.where(q[:, :, None] == 0, h[0], h[1])
                hb = np.where(q[:, :, None] == 0, h[2], h[3])
            else:
                ha, hb = h[0], h[1]
            s, G = np.empty_like(y), np.empty(y.shape)
            e0, e1 = slice(0, 4, 2), slice(1, 4, 2)
            s[..., e0] = np.conj(ha[..., e0]) * y[..., e0] + hb[..., e1] * np.conj(y[..., e1])
            s[..., e1] = np.conj(ha[..., e1]) * y[..., e1] - hb[..., e0] * np.conj(y[..., e0])
            G[..., e0] = np.abs(ha[..., e0]) ** 2 + np.abs(hb[..., e1]) ** 2
            G[..., e1] = np.abs(ha[..., e1]) ** 2 + np.abs(hb[..., e0]) ** 2
        c = 1 - 2.0 * PR.load_pkg().synth._pn((sf + 1) * (2 * n_id_cell + 1) * 512 + n_id_cell, 3 * n_sf).reshape(3, n_sf)
        if cp_type == 1:
            sg, Gg = s, G                                               # group n = unit n: [U][3][4]
        else:
            sg = np.stack([s[..., 0:2], s[..., 2:4]], axis=1).reshape(2 * U, 3, 2)      # groups 2 m', 2 m' + 1
            Gg = np.stack([G[..., 0:2], G[..., 2:4]], axis=1).reshape(2 * U, 3, 2)
        t = sg * c[None]
        K = 1.0 if P == 1 else np.sqrt(2.0)
        # a[group][seq][r] = K Re(conj(axis) sum_j conj(w_j) t_j), d[group][r] = sum_j G_j
        X = np.einsum("qj,grj->gqr", np.conj(SEQ[cp_type]), t)
        a = K * np.real(np.conj(AXIS) * X)
        d = Gg.sum(axis=2)[:, None, :] * np.ones((1, n_seq, 1))
        ds, asum = d.sum(axis=2), a.sum(axis=2)
        value = asum / ds
        dev = np.where(d > 0, a / np.where(d > 0, d, 1.0) - value[..., None], 0.0)
        S = (d * dev ** 2).sum(axis=2)
        ok = (ds > 0) & np.isfinite(ds) & np.isfinite(asum) & np.isfinite(value) & np.isfinite(S)
    return np.where(ok, value, 0.0), np.where(ok, ds, 0.0), np.where(ok, S, 0.0)


def decide(value, dsum, noise, min_amp, min_sigma):
    """-> (flags, sigma) of the entries of a subframe"""
    with np.errstate(all="ignore"):
        sigma = np.sqrt(noise / (2.0 * np.where(dsum > 0, dsum, 1.0)))
    ok = (dsum > 0) & np.isfinite(sigma)
    sigma = np.where(ok, sigma, 0.0)
    present = ok & (np.abs(value) >= min_amp) & (np.abs(value) >= min_sigma * sigma)
    return np.where(present, np.where(value < 0, 3, 1), 0), sigma


def decode(tfg, n_id_cell, cp_type, n_ports, n_rb, dl_mask=0x3FF, phich_duration=1, phich_resource=3, mi=None, min_amp=0.25, min_sigma=3.5):
    """the rule on a grid -> dict: the head of lcs_phich_info, sf (list of dicts), values / sigma / flags (per subframe [n_group][n_seq], None
    for a subframe that is not read), hi (the present entries in order, cut at MAX_HI).  mi: None = FDD, else ten values 0 .. 2"""
    tfg = np.asarray(tfg, np.complex128)
    assert tfg.shape[1] == 12 * n_rb and n_rb in PR.BANDWIDTHS
    tdd = mi is not None
    mi = [1] * 10 if mi is None else [int(m) for m in mi]
    n_ofdm, n_sf = tfg.shape[0], PR.n_sf_of(tfg.shape[0], cp_type)
    maps = {m: units(n_id_cell, n_rb, n_ports, cp_type, phich_duration, phich_resource, m) for m in set(mi)}
    n_seq = n_seq_of(cp_type)
    sf, values, sigmas, flagss, hi = [], [], [], [], []
    for g in range(n_sf):
        un = maps[mi[g % 10]]
        if not subframe_read(g, n_ofdm, cp_type, n_ports, phich_duration, tdd, dl_mask) or un is None:
            sf.append(dict(n_unit=-1, n_group=0, n_present=0, n_ack=0, n_nack=0, noise=0.0))
            values.append(None); sigmas.append(None); flagss.append(None)
            continue
        value, dsum, S = decode_subframe(tfg, g, n_id_cell, cp_type, n_ports, n_rb, un)
        valid = dsum > 0
        noise = float(S[valid].sum() / valid.sum()) if valid.any() else 0.0
        flags, sigma = decide(value, dsum, noise, min_amp, min_sigma)
        sf.append(dict(n_unit=un[0].shape[0], n_group=value.shape[0], n_present=int((flags & 1).sum()), n_ack=int((flags == 3).sum()),
                       n_nack=int((flags == 1).sum()), noise=noise))
        values.append(value); sigmas.append(sigma); flagss.append(flags)
        for grp, seq in zip(*np.nonzero(flags)):
            hi.append(dict(g=g, group=int(grp), seq=int(seq), flags=int(flags[grp, seq]), value=float(value[grp, seq]), sigma=float(sigma[grp, seq])))
    n_p = sum(s["n_present"] for s in sf)
    n_a = sum(s["n_ack"] for s in sf)
    return dict(n_sf=n_sf, n_read=sum(s["n_unit"] >= 0 for s in sf), n_present=n_p, n_ack=n_a, n_nack=n_p - n_a, n_hi=min(n_p, MAX_HI), n_dropped=max(n_p - MAX_HI, 0),
                dl_mask=dl_mask, n_rb=n_rb, n_ports=PR.ports_of(n_ports), sf=sf, values=values, sigma=sigmas, flags=flagss, hi=hi[:MAX_HI], n_seq=n_seq)
