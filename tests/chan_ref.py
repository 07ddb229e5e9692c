"""Float64 restatement of the channelizer's contract (include/lcs.h, lcs_channelize): the yardstick of the channelizer tests.

    y_k[m] = sum_t h[t] x[m D + T-1-t] exp(-2 pi i df_k / fs_in (m D + T-1-t)),   T = 16 D,  m = m_first .. m_first + n_out - 1

One exp per input sample in double, then the direct sum.  Only numpy."""
import numpy as np

# The capture of the host fixture test and of the GPU end-to-end test (synth.make_wideband with these arguments): 15.36 Msps
# around FC_CENTRE, three cells on three carriers (normal and extended CP, 1 / 2 / 4 ports, LO error inside the grid), two
# empty carriers, and the carrier one output rate (1.92 MHz) above the strong cell: everything of that cell aliases onto it.
# snr_db = 10 puts the noise of a 1.92 MHz channel 10 dB below a gain_db = 0 cell, so the gain_db = 30 cell is 40 dB above it
# -- the gain the issue asks for; the float64 reference alone is clean on the alias carrier at it (stopband -78 dB: the cell
# lands 38 dB under the noise), so it was not lowered.
WB = dict(seed=4242, fc_centre=740.0e6, decim=8, snr_db=10.0, n_out=153584)
WB_STRONG = 735.0e6
WB_PLACED = [
    (WB_STRONG, [dict(n_id_1=25, n_id_2=1, cp_normal=True, n_ports=1, n_rb_dl=25, f_off=7.3e3, gain_db=30.0)]),
    (740.5e6, [dict(n_id_1=101, n_id_2=2, cp_normal=False, n_ports=2, n_rb_dl=50, f_off=-11.2e3, gain_db=0.0)]),
    (742.6e6, [dict(n_id_1=60, n_id_2=0, cp_normal=True, n_ports=4, n_rb_dl=100, f_off=3.9e3, gain_db=3.0)]),
]
WB_EMPTY = [738.5e6, 744.5e6]
WB_ALIAS = WB_STRONG + 1.92e6
WB_GRID = np.arange(-15e3, 10.1e3, 5e3)      # one grid that holds every planted offset (the GPU end-to-end test)


def wb_carriers():
    return np.array([c for c, _ in WB_PLACED] + WB_EMPTY + [WB_ALIAS])


def wb_capture(pkg):
    """-> (interleaved int16 capture, the complex128 values it stands for, truth)"""
    iq, truth = pkg.synth.make_wideband(WB["seed"], WB["fc_centre"], WB["decim"], WB_PLACED, WB["snr_db"], pkg.FMT_IQ_S16)
    return iq, pkg.synth.wideband_to_complex(iq, pkg.FMT_IQ_S16), truth


def cell_key(c):
    return (c.n_id_cell(), c.cp_type, c.n_ports, c.n_rb_dl, c.phich_duration, c.phich_resource, c.sfn)


def taps_ref(D):
    T = 16 * D
    t = np.arange(T)
    h = np.sinc((t - (T - 1) / 2) / D) * np.kaiser(T, 7.75)
    return h / h.sum()


def channelize_ref(x, fs_in, D, f_shift, n_out, m_first=0, taps=None):
    """x: complex128 capture (ALL of it: the phase counts from its sample 0); -> [len(f_shift)][n_out] complex128"""
    x = np.asarray(x, np.complex128)
    T = 16 * D
    h = taps_ref(D) if taps is None else np.asarray(taps, np.float64)
    assert x.size >= (m_first + n_out - 1) * D + T
    lo, hi = m_first * D, (m_first + n_out - 1) * D + T
    n = np.arange(lo, hi, dtype=np.float64)
    hr = np.ascontiguousarray(h[::-1])          # window position j = T-1-t carries h[t]
    out = np.empty((len(f_shift), n_out), np.complex128)
    for k, df in enumerate(f_shift):
        xm = x[lo:hi] * np.exp(-2j * np.pi * (float(df) / fs_in) * n)
        for a in range(0, n_out, 8192):
            b = min(n_out, a + 8192)
            w = np.lib.stride_tricks.as_strided(xm[a * D:], shape=(b - a, T), strides=(D * xm.itemsize, xm.itemsize), writeable=False)
            out[k, a:b] = w @ hr
    return out


def quantise(x, fmt):
    """complex capture -> (interleaved integer array as the device takes it | complex64, the complex128 values it stands for)"""
    if fmt == "c64":
        q = np.asarray(x, np.complex64)
        return q, q.astype(np.complex128)
    bits, dt = (8, np.int8) if fmt == "s8" else (16, np.int16)
    sc = float(1 << (bits - 1))
    iq = np.empty(2 * x.size, dt)
    iq[0::2] = np.clip(np.rint(x.real * sc), -sc, sc - 1).astype(dt)
    iq[1::2] = np.clip(np.rint(x.imag * sc), -sc, sc - 1).astype(dt)
    return iq, (iq[0::2].astype(np.float64) + 1j * iq[1::2].astype(np.float64)) / sc
