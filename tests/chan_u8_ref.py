"""Numpy restatement of the 8-bit channelizer output's rule (include/lcs.h, lcs_channelize_u8), on top of the float64 channelizers
of chan_ref.py and chan_rate_ref.py: the yardstick of the u8 tests.

    P_k = mean_m |y_k[m]|^2,   e_k: the integer with 16^2 < 4^e_k P_k / 2 <= 32^2   (0 when P_k is zero or not finite)
    code = clip(127 + rint(2^e_k * component), 0, 255), ties to even; 127 for a component that is not finite;  I then Q

Only numpy."""
import numpy as np

import chan_rate_ref as RR
import chan_ref as R

LO, HI = 16.0 ** 2, 32.0 ** 2      # the component power 4^e P / 2 lies in (LO, HI]


def exponent(P):
    """A search by exact steps: scaling a double by 4 is exact, so the comparisons are the rule itself."""
    P = float(P)
    if not np.isfinite(P) or P <= 0.0:
        return 0
    e, v = 0, P / 2.0
    while v > HI:
        v, e = v / 4.0, e - 1
    while v <= LO:
        v, e = v * 4.0, e + 1
    return e


def code(z):
    """z: scaled components (any float array) -> uint8 codes.  np.rint rounds ties to even."""
    z = np.asarray(z, np.float64)
    with np.errstate(invalid="ignore"):
        c = np.clip(127.0 + np.rint(z), 0.0, 255.0)
    return np.where(np.isfinite(z), c, 127.0).astype(np.uint8)


def quantise_ref(y):
    """y: [n_ch][n_out] complex (the float64 channelizer's output) -> (codes uint8 [n_ch][n_out][2], gains float64 [n_ch] = 2^e,
    scaled components float64 [n_ch][n_out][2] = 2^e * (re, im): what the codes were rounded from)"""
    y = np.asarray(y, np.complex128)
    with np.errstate(over="ignore", invalid="ignore"):
        P = np.mean(y.real ** 2 + y.imag ** 2, axis=1)
    g = np.array([np.ldexp(1.0, exponent(p)) for p in P])
    z = np.stack([y.real, y.imag], axis=-1) * g[:, None, None]
    return code(z), g, z


def channelize_u8_ref(x, fs_in, up, down, f_shift, n_out, taps=None):
    """The contract end to end: the integer form for up == 1 and down in 2..16, the rational form otherwise."""
    if up == 1 and 2 <= down <= 16:
        y = R.channelize_ref(x, fs_in, down, f_shift, n_out, taps=taps)
    else:
        y = RR.channelize_rate_ref(x, fs_in, up, down, f_shift, n_out, taps=taps)
    return quantise_ref(y) + (y,)


def rounding_band(z, rel=1e-5):
    """The components whose scaled reference value lies within rel * max|2^e y_ref| of a half-integer, per carrier: there the
    channelizer's standing 1e-5 error may carry a value across a rounding boundary.  z: [n_ch][n_out][2] -> bool, same shape."""
    mag = np.sqrt(z[..., 0] ** 2 + z[..., 1] ** 2).max(axis=1)
    d = np.abs(z - np.floor(z) - 0.5)
    return d <= (rel * mag)[:, None, None]
