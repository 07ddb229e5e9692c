"""numpy statement of the PBCH soft path between the channel estimate and the Viterbi decoder, written from 36.211 6.6 / 6.3.4 and
36.212 5.1.4.2 and the reference's formulas, not from the oracle's C or the product's device code: which resource elements carry the
PBCH, the equalisation for one, two and four antenna ports, the exact log-MAP QPSK demodulator with its truncated logarithm,
descrambling, and de-rate-matching.  tests/test_pbch_ref.py holds it to the oracle; tests/test_gpu_pbch_soft.py uses its per-LLR
classification and allowance to compare the device with the oracle.

Inputs: the compensated grid tfg [854 | 732][72], the four ports' channel estimates ce [4][n_ofdm][72] and noise powers np_v [4]
(chan_est: compared with the oracle element by element elsewhere in the suite), the cell identity, the CP type, and the candidate
(frame_timing_guess 0..3, n_ports 1 / 2 / 4).

Every LLR is l = tlog(A) - tlog(B) with A, B sums of two of the symbol's four likelihoods e^{-|rx - g s|^2}.  Its REGIME, exactly one:
  LINEAR     (|rx.re| + g a)^2 + (|rx.im| + g a)^2 < 600: no likelihood is anywhere near underflow, l = 4 rx g a up to rounding;
  ZERO       all four likelihoods are exactly 0: l = tlog(0) - tlog(0) = 0 exactly;
  CLIPPED    A or B is exactly 0 (its tlog is log(DBL_MIN)), not both;
  SUBNORMAL  A or B is positive and below DBL_MIN;
  EXACT      the rest: both sums are normal numbers.
Its ALLOWANCE: 1e-9 (|l| + median |e_est|) + sum over the subnormal sums X among A, B of 4 * 2^-1074 / X.  1e-9 is the suite's array
tolerance for the grid and the channel estimate that feed this stage; the second term is two units in the last place of a
subnormal sum -- one for the host's exp, one for the device's -- seen through the logarithm.
Its EDGE flag: one of the symbol's four exponent arguments lies within 1e-6 of 1075 ln 2 = 745.1332..., where e^{-x} rounds to
2^-1074 on one side and to 0 on the other, so tlog jumps by 36: there the reference itself is discontinuous in its input."""
import functools

import numpy as np

from conftest import load_pkg

LINEAR, EXACT, SUBNORMAL, CLIPPED, ZERO = 0, 1, 2, 3, 4
REGIMES = ("LINEAR", "EXACT", "SUBNORMAL", "CLIPPED", "ZERO")
DBL_MIN = np.finfo(np.float64).tiny
DBL_MAX = np.finfo(np.float64).max
DENORM_MIN = 2.0 ** -1074
EDGE_X = 1075 * np.log(2.0)          # e^{-x} < 2^-1075 rounds to zero
EDGE_W = 1e-6
REL = 1e-9
CANDIDATES = [(g, p) for g in range(4) for p in (1, 2, 4)]      # decode_mib's loop order


def n_symb_of(cp_type):
    return 7 if cp_type == 1 else 6


def m_bit_of(cp_type):
    return 1920 if cp_type == 1 else 1728


def n_ofdm_of(cp_type):
    return 854 if cp_type == 1 else 732


def frame_elements(n_id_cell, cp_type):
    """(symbol of slot 1, subcarrier) of one frame's PBCH elements in mapping order (36.211 6.6.4: subcarrier first, then symbol;
    the elements reserved for the reference signals of ports 0..3 are left out whatever the number of ports: every third
    subcarrier, k = N_ID mod 3, of symbols 0 and 1 and -- extended CP -- of symbol 3)"""
    n = n_symb_of(cp_type)
    with_rs = {0, 1} | ({3} if n == 6 else set())
    out = [(l, k) for l in range(4) for k in range(72) if not (l in with_rs and k % 3 == n_id_cell % 3)]
    return np.array(out)


def elements(n_id_cell, cp_type, guess):
    """grid (row, column) of the candidate's m_bit / 2 symbols: four frames from frame `guess` of the grid"""
    n = n_symb_of(cp_type)
    fe = frame_elements(n_id_cell, cp_type)
    rows = np.concatenate([(guess + f) * 20 * n + n + fe[:, 0] for f in range(4)])
    cols = np.concatenate([fe[:, 1]] * 4)
    return rows, cols


def equalise(x, h, np_v, n_ports):
    """x [n] received, h [4][n] the ports' channels there -> (symbols [n], their noise powers [n]).  One port: zero forcing.  Two:
    the Alamouti pair (t, t + 1) through the pair's mean channels.  Four: the same with ports (0, 2) on even pairs and (1, 3) on odd."""
    n = x.size
    if n_ports == 1:
        gain = np.conj(h[0] / (h[0].real ** 2 + h[0].imag ** 2))
        return x * gain, np_v[0] * (gain.real ** 2 + gain.imag ** 2)
    pair = np.arange(n // 2)
    if n_ports == 2:
        pa, pb = np.zeros(n // 2, int), np.ones(n // 2, int)
    else:
        pa = pair & 1
        pb = pa + 2
    e, o = 2 * pair, 2 * pair + 1
    h1 = (h[pa, e] + h[pa, o]) / 2
    h2 = (h[pb, e] + h[pb, o]) / 2
    npw = (np.asarray(np_v)[pa] + np.asarray(np_v)[pb]) / 2
    scale = h1.real ** 2 + h1.imag ** 2 + h2.real ** 2 + h2.imag ** 2
    s = np.empty(n, np.complex128)
    s[e] = (np.conj(h1) * x[e] + h2 * np.conj(x[o])) / scale
    s[o] = np.conj((-np.conj(h2) * x[e] + h1 * np.conj(x[o])) / scale)
    npo = np.empty(n)
    npo[e] = npo[o] = ((np.abs(h1) / scale) ** 2 + (np.abs(h2) / scale) ** 2) * npw
    return s * np.sqrt(2.0), npo


def tlog(x):
    """itpp::trunc_log"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x == np.inf, np.log(DBL_MAX), np.where(x <= 0, np.log(DBL_MIN), np.log(np.where(x > 0, x, 1.0))))


def demodulate(syms, npv):
    """-> dict(llr [2n], regime [2n], sub [2n] (the allowance's subnormal term), edge [2n]).  QPSK map 00 -> (1, 1), 01 -> (1, -1),
    10 -> (-1, 1), 11 -> (-1, -1), all / sqrt 2; rx = sym / sqrt(np), the constellation scaled by g = 1 / sqrt(np), N0 = 1."""
    a = 1 / np.sqrt(2.0)
    with np.errstate(all="ignore"):
        g = 1.0 / np.sqrt(npv)
        rx = syms * g
        ga = g * a
        arg = (np.abs(rx.real) + ga) ** 2 + (np.abs(rx.imag) + ga) ** 2
        S = np.array([a + 1j * a, a - 1j * a, -a + 1j * a, -a - 1j * a])
        dist = rx[:, None] - g[:, None] * S[None, :]
        ex = dist.real ** 2 + dist.imag ** 2                    # the four exponent arguments [n][4]
        m = np.exp(-ex)
        A = np.stack([m[:, 0] + m[:, 1], m[:, 0] + m[:, 2]], axis=1)      # bit = 0: [n][2]
        B = np.stack([m[:, 2] + m[:, 3], m[:, 1] + m[:, 3]], axis=1)      # bit = 1
        llr = tlog(A) - tlog(B)
        linear = (arg < 600.0)[:, None] & np.ones((1, 2), bool)
        all_zero = (m == 0).all(axis=1)[:, None] & np.ones((1, 2), bool)
        clipped = (A == 0) | (B == 0)
        subA, subB = (A > 0) & (A < DBL_MIN), (B > 0) & (B < DBL_MIN)
        regime = np.full(A.shape, EXACT)
        regime[subA | subB] = SUBNORMAL
        regime[clipped] = CLIPPED
        regime[all_zero] = ZERO
        regime[linear] = LINEAR
        sub = np.where(subA, 4 * DENORM_MIN / np.where(subA, A, 1.0), 0.0) + np.where(subB, 4 * DENORM_MIN / np.where(subB, B, 1.0), 0.0)
        sub = np.where(linear, 0.0, sub)
        edge = (np.abs(ex - EDGE_X) <= EDGE_W).any(axis=1)[:, None] & ~linear
    return dict(llr=llr.reshape(-1), regime=regime.reshape(-1), sub=sub.reshape(-1), edge=edge.reshape(-1), arg=arg)


@functools.lru_cache(maxsize=None)
def scrambling(n_id_cell, n):
    return load_pkg().synth._pn(n_id_cell, n).astype(bool)


@functools.lru_cache(maxsize=None)
def coded_bit_of(n_e):
    """which of the 120 coded bits (stream * 40 + column) each of the n_e rate-matched positions carries: the generator's rate
    matcher (36.212 5.1.4.2) run on the bits' own numbers"""
    synth = load_pkg().synth
    out = synth.conv_ratematch(np.arange(120, dtype=np.uint8).reshape(3, 40), n_e).astype(np.int64)
    out.setflags(write=False)
    return out


def deratematch(e_est):
    """the mean of every coded bit's observations, added in ascending position -> [3][40]"""
    which = coded_bit_of(e_est.size)
    d, cnt = np.zeros(120), np.zeros(120, int)
    for t in range(e_est.size):
        d[which[t]] += e_est[t]
        cnt[which[t]] += 1
    return (np.where(cnt > 1, d / np.maximum(cnt, 1), d)).reshape(3, 40)


def soft(tfg, ce, np_v, n_id_cell, cp_type, guess, n_ports):
    """One candidate -> dict(e_est [m_bit], d_est [3][40], regime, edge, tol [m_bit], d_tol [3][40], d_edge [3][40])"""
    rows, cols = elements(n_id_cell, cp_type, guess)
    x = tfg[rows, cols]
    h = np.stack([ce[p][rows, cols] for p in range(4)])
    with np.errstate(all="ignore"):
        syms, npv = equalise(x, h, np_v, n_ports)
    dm = demodulate(syms, npv)
    m_bit = m_bit_of(cp_type)
    e_est = np.where(scrambling(n_id_cell, m_bit), -dm["llr"], dm["llr"])
    d_est = deratematch(e_est)
    fin = np.isfinite(e_est)
    med = float(np.median(np.abs(e_est[fin]))) if fin.any() else np.nan
    with np.errstate(all="ignore"):
        tol = REL * (np.abs(e_est) + med) + dm["sub"]
    which = coded_bit_of(m_bit)
    cnt = np.bincount(which, minlength=120)
    d_tol = (np.bincount(which, weights=np.where(np.isfinite(tol), tol, np.inf), minlength=120) / cnt).reshape(3, 40)
    d_edge = (np.bincount(which, weights=dm["edge"].astype(float), minlength=120) > 0).reshape(3, 40)
    return dict(e_est=e_est, d_est=d_est, regime=dm["regime"], edge=dm["edge"], tol=tol, d_tol=d_tol, d_edge=d_edge, arg=dm["arg"], median=med)


def soft_all(tfg, ce, np_v, n_id_cell, cp_type, candidates=None):
    return [soft(tfg, ce, np_v, n_id_cell, cp_type, g, p) for g, p in (CANDIDATES if candidates is None else candidates)]
