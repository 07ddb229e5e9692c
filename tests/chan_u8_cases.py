"""The captures and the float64 references of the 8-bit channelizer's GPU tests (tests/test_gpu_channelizer_u8.py), built and
checked on the CPU: tests/test_channelizer_u8_host.py asserts, on the reference alone, the two conditions those tests rest on.

A capture is one tone per carrier, 37 kHz (and a little more per carrier) off its centre, the amplitudes 60 dB apart over the 17
carriers, over a noise floor 100 dB below the loudest tone; a c64 capture is scaled by 2^10, so that its loud carriers need
negative exponents.  Only numpy."""
import functools

import numpy as np

import chan_rate_ref as RR
import chan_ref as R
import chan_u8_ref as U

FS_OUT = 1.92e6
N_CH = 17                                                  # two carrier blocks of 16
INTEGER = [(D, fmt) for D in (2, 16) for fmt in ("s8", "s16", "c64")]
RATIONAL = [(12, 125), (3, 4), (127, 128)]                 # s16
# per case: the loudest tone's amplitude.  Chosen on the CPU so that no carrier's 4^e P / 2 lies within 1 % of 16^2 or 32^2
# (test_channelizer_u8_host.py::test_gpu_cases_hold_their_premises); the sum of the 17 amplitudes stays below 1.
A0 = {(1, 2, "s8"): 0.30, (1, 2, "s16"): 0.30, (1, 2, "c64"): 0.30, (1, 16, "s8"): 0.30, (1, 16, "s16"): 0.30, (1, 16, "c64"): 0.30,
      (12, 125, "s16"): 0.30, (3, 4, "s16"): 0.30, (127, 128, "s16"): 0.30}


def shifts(fs_in, n_ch=N_CH):
    return np.linspace(-0.44, 0.44, N_CH)[:n_ch] * fs_in


def amplitudes(a0, n_ch=N_CH):
    return a0 * 10.0 ** (-3.0 * np.arange(n_ch) / (N_CH - 1))          # 0 .. -60 dB


def capture(seed, n_in, fs_in, f_shift, amp, fmt):
    """-> (the capture as the device takes it, the complex128 values it stands for)"""
    rng = np.random.default_rng(seed)
    n = np.arange(n_in, dtype=np.float64)
    x = 3e-6 * (rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in))
    for k, (f, a) in enumerate(zip(f_shift, amp)):
        x += a * np.exp(2j * np.pi * ((f + 37e3 + 1.7e3 * k) / fs_in) * n + 1j * rng.uniform(0, 2 * np.pi))
    if fmt == "c64":
        x = x * 1024.0
    return R.quantise(x, fmt)


def n_in_for(n_out, up, down):
    return (n_out - 1) * down + 16 * down if up == 1 else RR.n_in_min(n_out, up, down)


@functools.lru_cache(maxsize=None)
def arrays_case(up, down, fmt, n_out):
    """-> dict(q, n_in, fs_in, shifts, n_out, codes, gain, z, y): computed once, shared, never written to"""
    fs_in = FS_OUT * down / up
    n_in = n_in_for(n_out, up, down)
    f = shifts(fs_in)
    q, xq = capture(1000 * down + 10 * up + len(fmt), n_in, fs_in, f, amplitudes(A0[(up, down, fmt)]), fmt)
    codes, gain, z, y = U.channelize_u8_ref(xq, fs_in, up, down, f, n_out)
    for a in (q, codes, gain, z, y, f):
        a.setflags(write=False)
    return dict(q=q, n_in=n_in, fs_in=fs_in, shifts=f, n_out=n_out, codes=codes, gain=gain, z=z, y=y, up=up, down=down, fmt=fmt)


def premises(case):
    """-> (largest share of a carrier's components inside the rounding band, smallest relative distance of a carrier's 4^e P / 2
    from an end of (16^2, 32^2]), both from the reference alone"""
    band = U.rounding_band(case["z"])
    share = band.reshape(band.shape[0], -1).mean(axis=1).max()
    v = case["gain"] ** 2 * np.mean(np.abs(case["y"]) ** 2, axis=1) / 2.0
    return float(share), float(np.minimum(v / U.LO - 1.0, 1.0 - v / U.HI).min())


@functools.lru_cache(maxsize=None)
def burst_case():
    """c64, decim 2, one carrier at the capture's centre: quiet but for two bursts of opposite sign, eight samples each.  The rms
    sets e; the bursts land far beyond +-128 after scaling."""
    D, n_out = 2, 4099
    fs_in, n_in = D * FS_OUT, n_in_for(4099, 1, 2)
    rng = np.random.default_rng(77)
    x = 0.01 * (rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in))
    x[3000:3008] += 1.0 + 1.0j
    x[5000:5008] -= 1.0 + 1.0j
    q, xq = R.quantise(x, "c64")
    f = np.array([0.0])
    codes, gain, z, y = U.channelize_u8_ref(xq, fs_in, 1, D, f, n_out)
    return dict(q=q, n_in=n_in, fs_in=fs_in, shifts=f, n_out=n_out, codes=codes, gain=gain, z=z, y=y, up=1, down=D, fmt="c64")
