"""The cancellation rule of csrc/sic.h in numpy, fp64, on top of the oracle's tables (test infrastructure).

cancel(cap, cells, ...) -> (residual, info): for every cell record the known signals (PSS, SSS, CRS, PBCH) are rebuilt through
the cell's own channel estimate and subtracted.  Every step below is the step of the same name in sic.h; the device kernels
(csrc/sic.hip) are compared with this file, never the other way round."""
import numpy as np

import oracle as O
from conftest import load_pkg

PSS, SSS, CRS, PBCH, ALL = 1, 2, 4, 8, 15
FDD, TDD = 0, 1
WIN_IN_CP = 2          # the transform window of extract_tfg starts this many samples before the symbol's useful part
AVG_SLOTS = 4          # the channel estimate of a slot averages the slots within +- this many
FS_LTE = 30720000.0


def geometry(cell, n_cap, fc_req, fc_prog, fs):
    """Symbol t (t = 0: the first symbol of extract_tfg's grid, t < 0 before it) has its transform window at w(t) and owns the
    samples [a(t), a(t + 1)); the last symbol of the capture owns up to the end of its window."""
    normal = cell.cp_type == 1
    n_symb = 7 if normal else 6
    k = (fc_req - cell.freq_fine) / fc_prog
    step = 16 / FS_LTE * fs * k                                   # receiver samples per nominal 1.92 MHz sample
    d0 = cell.frame_start + (10 if normal else 32) * step
    if d0 - .01 * fs * k > -0.5:
        d0 = d0 - .01 * fs * k

    def nominal(t):
        t = np.asarray(t, np.int64)
        return (960 * (t // 7) + 137 * (t % 7)) if normal else 160 * t

    def cp(t):
        t = np.asarray(t, np.int64)
        return np.where(t % 7 == 0, 10, 9) if normal else np.full(t.shape, 32)

    def d(t):
        return d0 + nominal(t).astype(np.float64) * step

    def w(t):
        return np.rint(d(t)).astype(np.int64)

    def a(t):
        return w(t) - cp(t) + WIN_IN_CP

    # every symbol that can touch the capture: a slot is 960 nominal samples and n_symb symbols, so the symbols whose nominal
    # position lies within a slot of sample 0 and of sample n_cap bracket t_lo and t_hi whatever n_cap, d0 and step are
    first = int(np.floor((-d0 / step - 960.0) * n_symb / 960.0)) - 1
    last = int(np.ceil(((n_cap - d0) / step + 960.0) * n_symb / 960.0)) + 1
    t_all = np.arange(first, last + 1)
    ok = (a(t_all) >= 0) & (w(t_all) + 128 <= n_cap)
    t_lo, t_hi = int(t_all[ok][0]), int(t_all[ok][-1])
    assert first < t_lo and t_hi < last                           # the bracket held: both neighbours were looked at and refused
    j_lo, j_hi = t_lo // n_symb, t_hi // n_symb
    return dict(n_symb=n_symb, normal=normal, k=k, step=step, d0=d0, d=d, w=w, a=a, t_lo=t_lo, t_hi=t_hi, n_sym=t_hi - t_lo + 1,
                j_lo=j_lo, n_slots=j_hi - j_lo + 1, f_lo=j_lo // 20, n_frames=j_hi // 20 - j_lo // 20 + 1,      # as sic.h's SicGeom
                rot=cell.freq_superfine / (fs * k))               # cycles per sample of the cell's carrier offset


def owner_nominal(geo, n):
    """the symbol whose nominal stretch holds sample n"""
    r = (n - geo["d0"]) / geo["step"] + ((10 if geo["normal"] else 32) - WIN_IN_CP)
    if geo["normal"]:
        slot = np.floor(r / 960.0)
        rr = r - 960.0 * slot
        sym = np.where(rr < 138.0, 0, np.minimum(6, 1 + np.floor((rr - 138.0) / 137.0)))
        return (7 * slot + sym).astype(np.int64)
    return np.floor(r / 160.0).astype(np.int64)


def owner_corrected(geo, n, t):
    """... corrected by at most one symbol to the rounded boundaries a(t)"""
    return np.where(n < geo["a"](t), t - 1, np.where(n >= geo["a"](t + 1), t + 1, t))


def window_offset(n, w):
    """offset of sample n into the periodic extension of the window at w, backwards into the cyclic prefix too"""
    return (n - w) % 128


def owner(geo, n):
    """sample -> (symbol, offset into the periodic extension of its window), by the closed form of sic.h; symbol < t_lo: none"""
    n = np.asarray(n, np.int64)
    t = owner_corrected(geo, n, owner_nominal(geo, n))
    inside = (t >= geo["t_lo"]) & ((t < geo["t_hi"]) | ((t == geo["t_hi"]) & (n < geo["w"](t) + 128)))
    return np.where(inside, t, geo["t_lo"] - 1), window_offset(n, geo["w"](t))


def cn():
    i = np.arange(72)
    return np.where(i < 36, i - 36, i - 35)


def bins():
    i = np.arange(72)
    return np.where(i < 36, 92 + i, i - 35)


def grid(cap, geo):
    """[n_sym][72]: de-rotated by the cell's frequency at absolute sample time, unscaled 128-point transform, `late` phase"""
    t = np.arange(geo["t_lo"], geo["t_hi"] + 1)
    w, d = geo["w"](t), geo["d"](t)
    idx = w[:, None] + np.arange(128)[None, :]
    ph = geo["rot"] * idx
    x = cap[idx] * np.exp(-2j * np.pi * (ph - np.rint(ph)))
    X = np.fft.fft(x, axis=1)[:, bins()]
    late = w - d
    return X * np.exp(-2j * np.pi * late[:, None] * cn()[None, :] / 128)


def usable(geo, t, dl_mask, special):
    """whether the CRS / PBCH of symbol t are cancelled (and its CRS feed the estimate): the subframe is in the mask, or, with
    `special`, the symbol is symbol 0 of subframe 1 or 6"""
    j, sym = t // geo["n_symb"], t % geo["n_symb"]
    s = j % 20
    sf = s >> 1
    return bool((dl_mask >> sf) & 1) or (special and sf in (1, 6) and (s & 1) == 0 and sym == 0)


def crs_third_symbol(n_symb):
    """the second symbol of a slot with the CRS of ports 0 and 1 (36.211 6.10.1.2: l = N_symb - 3)"""
    return n_symb - 3


def crs_v23(s):
    """v of port 2 in symbol 1 of slot-in-frame s (port 3: 3 more): it alternates with the slot's parity"""
    return 3 * (s & 1)


def crs_of(geo, ident, cell, t):
    """{port: (first subcarrier, 12 values)} of symbol t"""
    n_symb = geo["n_symb"]
    j, sym = t // n_symb, t % n_symb
    s = j % 20
    if sym == 0:
        v = {0: 0, 1: 3}
    elif sym == crs_third_symbol(n_symb):
        v = {0: 3, 1: 0}
    elif sym == 1:
        v = {2: crs_v23(s), 3: 3 + crs_v23(s)}
    else:
        return {}
    rs = ident["rs"][s * n_symb + sym]
    return {p: ((vv + ident["id"]) % 6, rs) for p, vv in v.items() if p < cell.n_ports}


def channel(G, geo, ident, cell, dl_mask, special):
    """[n_slots][n_ports][72] from the CRS alone: least squares on the reference elements, the mean over the usable elements of
    the same subcarrier in slots j - AVG_SLOTS .. j + AVG_SLOTS, linear interpolation over the true subcarrier numbers (flat
    beyond the outermost reference elements' linear continuation), the same for every symbol of slot j"""
    n_symb = geo["n_symb"]
    j_lo, j_hi = geo["t_lo"] // n_symb, geo["t_hi"] // n_symb
    n_slots = j_hi - j_lo + 1
    c3 = ident["id"] % 3
    acc = np.zeros((n_slots, 4, 24), np.complex128)
    cnt = np.zeros((n_slots, 4, 24))
    for t in range(geo["t_lo"], geo["t_hi"] + 1):
        if not usable(geo, t, dl_mask, special):
            continue
        for p, (sh, rs) in crs_of(geo, ident, cell, t).items():
            m = (sh - c3) // 3 + 2 * np.arange(12)
            acc[t // n_symb - j_lo, p, m] += G[t - geo["t_lo"], sh + 6 * np.arange(12)] * np.conj(rs)
            cnt[t // n_symb - j_lo, p, m] += 1
    H = np.zeros((n_slots, cell.n_ports, 72), np.complex128)
    q = c3 + 3 * np.arange(24)
    cnq = cn()[q].astype(np.float64)
    kk = np.arange(72)
    m0 = np.clip((kk - c3) // 3, 0, 22)
    fr = (cn()[kk] - cnq[m0]) / (cnq[m0 + 1] - cnq[m0])
    for j in range(n_slots):
        lo, hi = max(0, j - AVG_SLOTS), min(n_slots, j + AVG_SLOTS + 1)
        for p in range(cell.n_ports):
            a, c = acc[lo:hi, p].sum(0), cnt[lo:hi, p].sum(0)
            h = np.where(c > 0, a / np.maximum(c, 1), 0)
            H[j, p] = h[m0] + fr * (h[m0 + 1] - h[m0])
    return H, j_lo


def sync_symbols(geo, duplex):
    """[(t, 'pss' | 'sss', slot of the sequence)] of every half frame inside the capture"""
    out = []
    n_symb = geo["n_symb"]
    for t in range(geo["t_lo"], geo["t_hi"] + 1):
        j, sym = t // n_symb, t % n_symb
        s = j % 20
        if duplex == FDD:
            if s % 10 == 0 and sym == n_symb - 1:
                out.append((t, "pss", s))
            if s % 10 == 0 and sym == n_symb - 2:
                out.append((t, "sss", s))
        else:
            if s % 10 == 2 and sym == 2:
                out.append((t, "pss", s - 2))
            if s % 10 == 1 and sym == n_symb - 1:
                out.append((t, "sss", s - 1))
    return out


def frame_sfn(cell, geo, frame):
    """the system frame number of frame `frame` of the grid (frame 0 carries the record's sfn: decode_mib's rule; frames before it
    and frames past 1023 wrap)"""
    return (cell.sfn + frame) % 1024


def pbch_quarter(cell, ident, geo, frame):
    """the PBCH symbols of frame `frame` of the grid"""
    synth = load_pkg().synth
    sfn = frame_sfn(cell, geo, frame)
    key = sfn - sfn % 4
    if key not in ident["pbch"]:
        ident["pbch"][key] = synth.pbch_symbols(ident["id"], cell.n_ports, cell.n_rb_dl, 1 if cell.phich_duration == 2 else 0,
                                                cell.phich_resource - 1, key, geo["normal"]).reshape(4, -1)
    return ident["pbch"][key][sfn % 4]


def pbch_mate(s):
    """element i's partner in its SFBC pair: element i ^ 1"""
    return s.reshape(-1, 2)[:, ::-1].reshape(-1)


def pbch_skip(sym, normal):
    """whether symbol `sym` of slot 1 leaves out the subcarriers k mod 3 == id mod 3 (where the CRS of any of four ports may lie)"""
    return sym in (0, 1) or (sym == 3 and not normal)


def pbch_layers(s, n_ports):
    """[n_ports][len(s)]: what each port sends on the elements that carry s (36.211 6.3.4.3: SFBC, SFBC-FSTD)"""
    x = np.zeros((n_ports, s.size), np.complex128)
    if n_ports == 1:
        x[0] = s
        return x
    a = np.empty((2, s.size), np.complex128)
    m = pbch_mate(s)
    a[0] = s
    a[1, 0::2], a[1, 1::2] = -np.conj(m[0::2]), np.conj(m[1::2])
    a /= np.sqrt(2.0)
    if n_ports == 2:
        return a
    pair = (np.arange(s.size) // 2) & 1
    x[0][pair == 0], x[2][pair == 0] = a[0][pair == 0], a[1][pair == 0]
    x[1][pair == 1], x[3][pair == 1] = a[0][pair == 1], a[1][pair == 1]
    return x


def known(G, H, j_lo, geo, ident, cell, duplex, mask, dl_mask, special):
    """-> (T [4 components][n_sym][72]: the components' elements through the channel, sync gain)"""
    n_symb = geo["n_symb"]
    T = np.zeros((4, geo["n_sym"], 72), np.complex128)
    syncs = sync_symbols(geo, duplex)
    num, den = 0j, 0.0
    for t, kind, s in syncs:
        if kind == "sss":
            ref = H[t // n_symb - j_lo, 0, 5:67] * ident["sss"][s]
            num += np.sum(G[t - geo["t_lo"], 5:67] * np.conj(ref))
            den += np.sum(np.abs(ref) ** 2)
    gain = num / den if den > 0 else 0j
    for t, kind, s in syncs:
        seq = ident["pss"] if kind == "pss" else ident["sss"][s]
        T[0 if kind == "pss" else 1, t - geo["t_lo"], 5:67] = gain * H[t // n_symb - j_lo, 0, 5:67] * seq
    for t in range(geo["t_lo"], geo["t_hi"] + 1):
        if not usable(geo, t, dl_mask, special):
            continue
        j, sym = t // n_symb, t % n_symb
        for p, (sh, rs) in crs_of(geo, ident, cell, t).items():
            k = sh + 6 * np.arange(12)
            T[2, t - geo["t_lo"], k] += H[j - j_lo, p, k] * rs
        if j % 20 == 1 and sym <= 3:
            skip = pbch_skip(sym, geo["normal"])
            sc = np.array([k for k in range(72) if not (skip and k % 3 == ident["id"] % 3)])
            per = [48, 48, 72, 72] if geo["normal"] else [48, 48, 72, 48]
            q = pbch_quarter(cell, ident, geo, j // 20)
            seg = np.zeros(sc.size, np.complex128)               # sc.size == per[sym]: the quarter's share of this symbol
            part = q[sum(per[:sym]):sum(per[:sym]) + sc.size]
            seg[:part.size] = part
            x = pbch_layers(seg, cell.n_ports)
            T[3, t - geo["t_lo"], sc] = np.sum(H[j - j_lo, :, sc].T * x, axis=0)
    for i, bit in enumerate((PSS, SSS, CRS, PBCH)):
        if not mask & bit:
            T[i] = 0
    return T, gain


def identity(cell):
    ident = dict(id=cell.n_id_2 + 3 * cell.n_id_1, pbch={})
    ident["rs"], _ = O.rs_dl(ident["id"], cell.cp_type)
    ident["pss"] = O.pss_fd(cell.n_id_2)
    ident["sss"] = {s: O.sss_fd(cell.n_id_1, cell.n_id_2, s).astype(np.float64) for s in (0, 10)}
    return ident


def synthesis_phase(geo, t):
    """[len(t)][72]: the grid's `late` phase put back before the inverse transform"""
    late = geo["w"](t) - geo["d"](t)
    return np.exp(2j * np.pi * late[:, None] * cn()[None, :] / 128)


def pss_energy(G, geo, duplex):
    return sum(np.sum(np.abs(G[t - geo["t_lo"], 5:67]) ** 2) for t, kind, _ in sync_symbols(geo, duplex) if kind == "pss")


def dl_mask_for(duplex, ul_dl_config=None):
    """the subframes whose CRS / PBCH are cancelled -> (mask, special): FDD all; TDD 0 and 5, or the configuration's downlink
    subframes and symbol 0 of the special ones once the configuration is known"""
    if duplex == FDD:
        return 0x3ff, False
    if ul_dl_config is None or not 0 <= int(ul_dl_config) <= 6:
        return 0x021, False
    return load_pkg().capi.load().lcs_tdd_dl_mask(int(ul_dl_config)), True


def cancel(cap, cells, fc_req, fc_prog, fs, duplex=FDD, mask=ALL, ul_dl_config=None, waveforms=False):
    """-> (residual complex128, [dict per cell: power [4], gain, n_sym, n_pss, pss_before, pss_after, suppression_db]); with
    `waveforms` also [per cell: the waveform y_c that was subtracted].  One capture, the cells of its buffer in list order: a batch
    is one call per buffer, each with the buffer's own fc_req / fc_prog.
    ul_dl_config: one uplink-downlink configuration for every cell, or a list with one per cell (None / outside 0..6: not known)"""
    cap = np.asarray(cap, np.complex128)
    res = cap.copy()
    configs = list(ul_dl_config) if isinstance(ul_dl_config, (list, tuple)) else [ul_dl_config] * len(cells)
    n = np.arange(cap.size)
    work, ys = [], []
    for cell, config in zip(cells, configs):
        dl_mask, special = dl_mask_for(duplex, config)
        geo, ident = geometry(cell, cap.size, fc_req, fc_prog, fs), identity(cell)
        G = grid(cap, geo)
        H, j_lo = channel(G, geo, ident, cell, dl_mask, special)
        T, gain = known(G, H, j_lo, geo, ident, cell, duplex, mask, dl_mask, special)
        X = np.zeros((geo["n_sym"], 128), np.complex128)
        t = np.arange(geo["t_lo"], geo["t_hi"] + 1)
        X[:, bins()] = T.sum(0) * synthesis_phase(geo, t)
        td = np.fft.ifft(X, axis=1)
        sym, off = owner(geo, n)
        inside = sym >= geo["t_lo"]
        ph = geo["rot"] * n
        y = np.where(inside, td[np.where(inside, sym - geo["t_lo"], 0), off], 0) * np.exp(2j * np.pi * (ph - np.rint(ph)))
        res -= y
        ys.append(y)
        work.append((geo, G, dict(power=[float(np.sum(np.abs(T[i]) ** 2) / 128) for i in range(4)], gain=complex(gain), n_sym=geo["n_sym"],
                                  n_pss=sum(kind == "pss" for _, kind, _ in sync_symbols(geo, duplex)))))
    for geo, G, info in work:
        info["pss_before"] = float(pss_energy(G, geo, duplex))
        info["pss_after"] = float(pss_energy(grid(res, geo), geo, duplex))
        info["suppression_db"] = 10 * np.log10(info["pss_before"] / info["pss_after"]) if info["pss_after"] > 0 else np.inf
    return (res, [w[2] for w in work], ys) if waveforms else (res, [w[2] for w in work])
