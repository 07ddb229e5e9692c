"""Inputs the PBCH soft-path tests share (tests/test_pbch_ref.py, tests/test_gpu_pbch_soft.py): crafted compensated grids, seeded,
with a known PBCH in them, two grids taken through the oracle's chain from generated captures, and per case the oracle's soft values
of all twelve candidates with the numpy reference's classification of them (computed once, never changed).

A crafted grid [854 | 732][72]: the reference signals of the transmitted ports times a channel (a complex gain per port, a phase
ramp over the subcarriers, a slow common phase over the rows, a mild amplitude ripple), the PBCH built from 24 raw MIB bits (so the
reserved bandwidth codes are possible) through the generator's CRC, coder, rate matcher, scrambler and transmit diversity, QPSK load
elsewhere, complex noise of a chosen variance.  Frame f of the grid carries quarter (f - g_true) mod 4 of the PBCH period."""
import functools

import numpy as np

import oracle as O
import pbch_ref as PB
import pcfich_ref as PR
from conftest import load_pkg

FC = 739e6
FS = 1.92e6


def raw_mib(bw_code, phich_duration_ext, phich_res, sfn8, spare=0):
    """24 bits: dl-Bandwidth code (3, MSB first), phich-Duration, phich-Resource (2), the SFN's eight MSBs, ten spare bits"""
    b = [(bw_code >> 2) & 1, (bw_code >> 1) & 1, bw_code & 1, int(phich_duration_ext), (phich_res >> 1) & 1, phich_res & 1]
    b += [(sfn8 >> (7 - i)) & 1 for i in range(8)]
    b += [(spare >> (9 - i)) & 1 for i in range(10)]
    return np.array(b, np.uint8)


def pbch_symbols(mib24, n_id_cell, n_tx, cp_type):
    """the QPSK symbols of one PBCH period from raw MIB bits (the generator's pieces, as synth.pbch_symbols chains them)"""
    synth = load_pkg().synth
    p = synth.crc16(mib24)
    if n_tx == 2:
        p = p ^ 1
    elif n_tx == 4:
        p = p ^ (np.arange(16) & 1).astype(np.uint8)
    d = synth.conv_encode_tailbite(np.concatenate([mib24, p]))
    n_e = PB.m_bit_of(cp_type)
    e = synth.conv_ratematch(d, n_e) ^ synth._pn(n_id_cell, n_e)
    return ((1 - 2.0 * e[0::2]) + 1j * (1 - 2.0 * e[1::2])) / np.sqrt(2.0)


def crafted_grid(n_id_cell, cp_type, n_tx, g_true, mib24, noise_var, seed=0, pbch_zero=False, smooth=False):
    rng = np.random.default_rng(seed)
    synth = load_pkg().synth
    n, n_ofdm = PB.n_symb_of(cp_type), PB.n_ofdm_of(cp_type)
    k = np.arange(72)
    qpsk = lambda size: ((1 - 2.0 * rng.integers(0, 2, size)) + 1j * (1 - 2.0 * rng.integers(0, 2, size))) / np.sqrt(2.0)
    tau, f_row = 0.37 + 0.2 * rng.random(), 0.004 * (rng.random() - 0.5)
    gain = np.exp(2j * np.pi * rng.random(4)) * (0.8 + 0.4 * rng.random(4))
    ripple = 0.15
    if smooth:            # a channel the estimator's interpolation follows almost exactly: the estimated noise power is tiny
        tau, f_row, ripple = 0.02, 0.0, 0.0

    def chan(r):          # the common part of the ports' channels on row r
        return (np.exp(-2j * np.pi * tau * (k - 35.5) / 128.0) * np.exp(2j * np.pi * f_row * r)) * (1.0 + ripple * np.cos(2 * np.pi * k / 72 + r / 57.0))

    tfg = np.zeros((n_ofdm, 72), np.complex128)
    for r in range(n_ofdm):
        sym, slot = r % n, (r // n) % 20
        row = 0.7 * qpsk(72) * chan(r) * gain[0]
        ports = (0, 1) if sym in (0, n - 3) else ((2, 3) if sym == 1 else ())
        for port in ports:
            if port < n_tx:
                v = (0, 3)[port] if sym == 0 else ((3, 0)[port] if sym == n - 3 else (3 * (slot & 1), 3 + 3 * (slot & 1))[port - 2])
                idx = (v + n_id_cell) % 6 + 6 * np.arange(12)
                row[idx] = PR.rs_row(n_id_cell, cp_type, 6, slot, sym) * chan(r)[idx] * gain[port]
        tfg[r] = row
    x = synth._tx_diversity(pbch_symbols(mib24, n_id_cell, n_tx, cp_type), n_tx)           # [n_tx][960 | 864]
    fe = PB.frame_elements(n_id_cell, cp_type)
    per_frame = fe.shape[0]
    for f in range(n_ofdm // (20 * n) + 1):
        q = (f - g_true) % 4
        rows, cols = f * 20 * n + n + fe[:, 0], fe[:, 1]
        if rows.max() >= n_ofdm:
            break
        for i in range(per_frame):
            tfg[rows[i], cols[i]] = 0.0 if pbch_zero else (gain[:n_tx] * x[:, q * per_frame + i]).sum() * chan(rows[i])[cols[i]]
    sigma = np.sqrt(noise_var / 2.0)
    noise = sigma * (rng.standard_normal(tfg.shape) + 1j * rng.standard_normal(tfg.shape))
    if pbch_zero:         # the PBCH ROWS are all zero: the channel estimates there are interpolated, the received values are 0
        for f in range(n_ofdm // (20 * n) + 1):
            for l in range(4):
                r = f * 20 * n + n + l
                if r < n_ofdm:
                    tfg[r] = 0.0
                    noise[r] = 0.0
    tfg += noise
    tfg.setflags(write=False)
    return tfg


def cell_of(n_id_cell, cp_type, n_rb_dl=-1):
    return dict(n_id_1=n_id_cell // 3, n_id_2=n_id_cell % 3, cp_type=cp_type, n_rb_dl=n_rb_dl)


def snr_var(db):
    return 10.0 ** (-db / 10.0)


# ---- the case set: name -> how its grid is made
def _cases():
    out = {}
    ids = {0: 300, 1: 7, 2: 503}
    i = 0
    for v3 in (0, 1, 2):
        for cp in (1, 2):
            for n_tx in (1, 2, 4):
                g = i % 4
                out[f"id{ids[v3]}-cp{cp}-tx{n_tx}-g{g}"] = dict(kind="crafted", n_id=ids[v3], cp=cp, n_tx=n_tx, g=g, mib=raw_mib(2 + i % 4, i & 1, i % 4, 37 + 11 * i),
                                                          var=snr_var(15.0), seed=100 + i)
                i += 1
    # the noise series: from the linear branch through the exact one, the subnormal band and the cut to zero, to all-zero LLRs
    for db in NOISE_SERIES:
        out[f"series-cp1-tx2-{db}dB"] = dict(kind="crafted", n_id=77 * 3 + 2, cp=1, n_tx=2, g=1, mib=raw_mib(2, 0, 2, 125), var=snr_var(db), seed=7)
        out[f"series-cp2-tx1-{db}dB"] = dict(kind="crafted", n_id=3 * 3 + 0, cp=2, n_tx=1, g=2, mib=raw_mib(2, 0, 2, 125), var=snr_var(db), seed=8)
    out["noise-free"] = dict(kind="crafted", n_id=77 * 3 + 2, cp=1, n_tx=2, g=1, mib=raw_mib(2, 0, 2, 125), var=0.0, seed=7, n_rb_dl=25, smooth=True)
    out["reserved-bw6"] = dict(kind="crafted", n_id=41 * 3 + 1, cp=1, n_tx=2, g=3, mib=raw_mib(6, 1, 3, 200), var=snr_var(15.0), seed=21, n_rb_dl=50)
    out["reserved-bw7"] = dict(kind="crafted", n_id=12 * 3 + 2, cp=2, n_tx=4, g=0, mib=raw_mib(7, 0, 1, 3, spare=0x155), var=snr_var(15.0), seed=22, n_rb_dl=15)
    out["pbch-rows-zero"] = dict(kind="crafted", n_id=5 * 3 + 1, cp=1, n_tx=1, g=0, mib=raw_mib(3, 0, 0, 9), var=snr_var(20.0), seed=23, pbch_zero=True)
    out["chain-10dB"] = dict(kind="chain", snr=10.0, cell=dict(n_id_1=77, n_id_2=2, cp_normal=True, n_ports=2, n_rb_dl=25, sfn0=500, f_off=300.0, t0=3000.0))
    out["chain-25dB"] = dict(kind="chain", snr=25.0, cell=dict(n_id_1=3, n_id_2=0, cp_normal=False, n_ports=1, n_rb_dl=50, sfn0=321, f_off=-450.0, t0=5100.0))
    return out


NOISE_SERIES = (21.0, 22.5, 24.0, 25.5, 27.0, 32.0)
CASES = _cases()
NAMES = list(CASES)
INTEGERS_ONLY = ("pbch-rows-zero",)      # only crc_ok, the decoded bits and decode_mib's record are compared


@functools.lru_cache(maxsize=None)
def grid(name):
    """-> (oracle cell record that goes into decode_mib / pbch_soft, tfg_comp)"""
    c = CASES[name]
    if c["kind"] == "crafted":
        tfg = crafted_grid(c["n_id"], c["cp"], c["n_tx"], c["g"], c["mib"], c["var"], c["seed"], c.get("pbch_zero", False), c.get("smooth", False))
        return O.new_cell(**cell_of(c["n_id"], c["cp"], c.get("n_rb_dl", -1))), tfg
    synth = load_pkg().synth
    cap = synth.iq_u8_to_complex(synth.make_capbuf(7, FC, [dict(c["cell"])], snr_db=c["snr"])[0])
    O.set_threads(8)
    cells, _ = O.search_capbuf(cap, np.arange(-5e3, 5e3 + 1, 5e3), FC, FC, FS)
    cell = next(x for x in cells if (x.n_id_1, x.n_id_2) == (c["cell"]["n_id_1"], c["cell"]["n_id_2"]))
    tfg, ts = O.extract_tfg(cell, cap, FC, FC, FS)         # the cell's own grid once more, as the chain formed it
    cell, tfgc, _ = O.tfoec(cell, tfg, ts, FC, FC)
    cell.n_ports, cell.n_rb_dl, cell.phich_duration, cell.phich_resource, cell.sfn = -1, -1, 0, 0, -1      # as before decode_mib
    tfgc.setflags(write=False)
    return cell, tfgc


def cell_fields(cell):
    return (cell.n_ports, cell.n_rb_dl, cell.phich_duration, cell.phich_resource, cell.sfn, cell.cp_type, cell.n_id_1, cell.n_id_2)


@functools.lru_cache(maxsize=None)
def oracle_soft(name):
    """the oracle's (e_est [12][m_bit], d_est [12][3][40], c_est [12][40], crc_ok [12]) of the twelve candidates, and its decode_mib record"""
    cell, tfg = grid(name)
    e, d, c, ok = O.pbch_soft_many(cell, tfg)
    for a in (e, d, c, ok):
        a.setflags(write=False)
    return e, d, c, ok, O.decode_mib(cell, tfg)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the numpy reference's twelve records (pbch_ref.soft) on the oracle's channel estimate"""
    cell, tfg = grid(name)
    ce, npv = zip(*[O.chan_est(cell, tfg, p) for p in range(4)])
    return PB.soft_all(tfg, ce, npv, cell.n_id_cell(), cell.cp_type)


def compare(got_e, got_d, name, k):
    """|got - oracle| / allowance of candidate k over the elements that are compared -> dict(worst per regime, d_worst, n_edge, n);
    raises where an element exceeds its allowance or a ZERO element is not exactly 0"""
    e, d, _, _, _ = oracle_soft(name)
    r = reference(name)[k]
    keep = ~r["edge"]
    with np.errstate(all="ignore"):
        ratio = np.where(got_e == e[k], 0.0, np.abs(got_e - e[k]) / r["tol"])          # (equal values: within any allowance, 0 included)
    worst = {}
    for reg, nm in enumerate(PB.REGIMES):
        m = keep & (r["regime"] == reg)
        worst[nm] = float(ratio[m].max()) if m.any() else 0.0
    bad = keep & ~(ratio <= 1.0)
    assert not bad.any(), (name, PB.CANDIDATES[k], "e_est", [(int(t), PB.REGIMES[r["regime"][t]], got_e[t], e[k][t], r["tol"][t]) for t in np.flatnonzero(bad)[:8]], int(bad.sum()))
    z = keep & (r["regime"] == PB.ZERO)
    assert (got_e[z] == 0.0).all(), (name, PB.CANDIDATES[k], "a ZERO element is not exactly 0")
    dkeep = ~r["d_edge"]
    with np.errstate(all="ignore"):
        dratio = np.where(got_d == d[k], 0.0, np.abs(got_d - d[k]) / r["d_tol"])
    dbad = dkeep & ~(dratio <= 1.0)
    assert not dbad.any(), (name, PB.CANDIDATES[k], "d_est", [(int(t), got_d.reshape(-1)[t], d[k].reshape(-1)[t], r["d_tol"].reshape(-1)[t]) for t in np.flatnonzero(dbad.reshape(-1))[:8]])
    worst["d_est"] = float(dratio[dkeep].max()) if dkeep.any() else 0.0
    return dict(worst=worst, n_edge=int(r["edge"].sum()), n_d_edge=int(r["d_edge"].sum()), n=int(keep.size))
