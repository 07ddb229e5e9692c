"""Float64 restatement of the rational channelizer's contract (include/lcs.h, lcs_channelize_rational): the yardstick of its tests.

    y_k[m] = up * sum_n g[m down + Tg-1 - n up] x[n] exp(-2 pi i df_k / fs_in n),   Tg = 16 down,
             n = ceil(m down / up) .. floor((m down + Tg-1) / up),   m = m_first .. m_first + n_out - 1

One exp per input sample in double, then the direct sum per output over its own n range.  Only numpy."""
import numpy as np

import chan_ref as R

# The capture of the host fixture test and of the GPU end-to-end test (synth.make_wideband_rate with these arguments): 80 ms at
# 20 Msps (a HackRF; up / down = 12 / 125) around FC_CENTRE, two cells on two carriers (normal / extended CP, 1 / 2 ports, LO
# error inside the grid), one empty carrier, and the carrier one output rate (1.92 MHz) above the strong cell: everything of
# that cell aliases onto it.  snr_db = 10 puts the noise of a 1.92 MHz channel 10 dB below a gain_db = 0 cell, so the
# gain_db = 30 cell is 40 dB above it; the float64 reference alone is clean on the alias carrier at that gain (stopband
# -78 dB at the fine rate: the cell lands 38 dB under the noise), so it was not lowered.
WBR = dict(seed=2020, fc_centre=740.0e6, up=12, down=125, snr_db=10.0, n_out=153584)
WBR_FS_IN = 20.0e6
WBR_STRONG = 735.0e6
WBR_PLACED = [
    (WBR_STRONG, [dict(n_id_1=25, n_id_2=1, cp_normal=True, n_ports=1, n_rb_dl=25, f_off=7.3e3, gain_db=30.0)]),
    (740.5e6, [dict(n_id_1=101, n_id_2=2, cp_normal=False, n_ports=2, n_rb_dl=50, f_off=-8.2e3, gain_db=0.0)]),
]
WBR_EMPTY = [738.5e6]
WBR_ALIAS = WBR_STRONG + 1.92e6
WBR_GRID = np.arange(-10e3, 10.1e3, 5e3)      # one five-point grid that holds both planted offsets (the GPU end-to-end test)


def wbr_carriers():
    return np.array([c for c, _ in WBR_PLACED] + WBR_EMPTY + [WBR_ALIAS])


def wbr_capture(pkg):
    """-> (interleaved int16 capture, the complex128 values it stands for, truth)"""
    iq, truth = pkg.synth.make_wideband_rate(WBR["seed"], WBR["fc_centre"], WBR["up"], WBR["down"], WBR_PLACED, WBR["snr_db"], pkg.FMT_IQ_S16)
    return iq, pkg.synth.wideband_to_complex(iq, pkg.FMT_IQ_S16), truth


def n_in_min(n_out, up, down):
    """the least capture length n_out outputs need"""
    return ((n_out - 1) * down + 16 * down - 1) // up + 1


def channelize_rate_ref(x, fs_in, up, down, f_shift, n_out, m_first=0, taps=None):
    """x: complex128 capture (ALL of it: the phase counts from its sample 0); -> [len(f_shift)][n_out] complex128"""
    x = np.asarray(x, np.complex128)
    U, D = int(up), int(down)
    Tg = 16 * D
    g = R.taps_ref(D) if taps is None else np.asarray(taps, np.float64)
    m_last = m_first + n_out - 1
    lo, hi = -(-m_first * D // U), (m_last * D + Tg - 1) // U + 1          # the samples any output of the range reads
    assert x.size >= hi
    n = np.arange(lo, hi, dtype=np.float64)
    out = np.empty((len(f_shift), n_out), np.complex128)
    for k, df in enumerate(f_shift):
        xm = x[lo:hi] * np.exp(-2j * np.pi * (float(df) / fs_in) * n)
        for q in range(U):
            # outputs m = q + U i: n runs from ceil(m D / U) = s_q + i D over the L taps g[m D + Tg-1 - n U] = g[q D + Tg-1 - (s_q + j) U]
            m0 = m_first + (q - m_first) % U
            if m0 > m_last:
                continue
            cnt = (m_last - m0) // U + 1
            s_q = -(-q * D // U)
            L = (q * D + Tg - 1) // U - s_q + 1
            c = U * g[q * D + Tg - 1 - (s_q + np.arange(L)) * U]
            first = -(-m0 * D // U) - lo
            for a in range(0, cnt, 8192):
                b = min(cnt, a + 8192)
                w = np.lib.stride_tricks.as_strided(xm[first + a * D:], shape=(b - a, L), strides=(D * xm.itemsize, xm.itemsize), writeable=False)
                out[k, m0 - m_first + a * U:m0 - m_first + (b - 1) * U + 1:U] = w @ c
    return out
