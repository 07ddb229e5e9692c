"""The streams of the 8-bit capture tests (tests/test_gpu_channelizer_stream_u8.py), built on the CPU: 17 carriers (T.shifts17), n_cap =
corner(U, D)[0] and three captures plus half of a fourth.  The input is
T.noise_and_tones far down plus one tone per carrier, 37 kHz (and a little more per carrier) off its centre, the amplitudes 60 dB apart
over the 17 carriers as in tests/chan_u8_cases.py; carrier BURST_CH also carries, in the middle of capture 1, a burst 30 dB above its
mean: two pieces of two outputs' length, of opposite sign.  n_cap is odd where up is even: 12/125 has rows of bytes at odd multiples of
two.  tests/test_channelizer_stream_u8_host.py asserts on the float64 reference (tests/chan_rate_ref.py) the condition the GPU tests
rest on: every capture's 4^e P / 2 of every carrier lies clear of 16^2 and 32^2, and the burst reaches both clamps.
The rule itself is restated in rule(): what the GPU tests compare bytes and gains with, EQUAL.  Only numpy."""
import functools

import numpy as np

import chan_rate_ref as RR
import chan_rate_twin as T
import chan_ref as R
import chan_u8_cases as K
import chan_u8_ref as U8

FS_OUT = 1.92e6
CASES = [(1, 16, "s16"), (1, 2, "s8"), (3, 4, "s8"), (12, 125, "s16"), (127, 128, "s16"), (31, 94, "c64"), (3, 47, "s16")]
BYTES = {"c64": 8, "s16": 4, "s8": 2}
BURST_CH = 9
MARGIN = 0.01      # the issue's condition on 4^e P / 2, on the GPU's own floats
# per case: the loudest tone's amplitude, chosen on the CPU so that the reference holds the condition with twice the margin and the
# burst passes +-135 codes (test_channelizer_stream_u8_host.py::test_gpu_cases_hold_their_premise).  Small, so that the burst -- 30 dB
# above all its carrier's filter passes, most of the band at 127/128 -- stays below full scale with the tones.
A0 = {(1, 16, "s16"): 0.017, (1, 2, "s8"): 0.020, (3, 4, "s8"): 0.020, (12, 125, "s16"): 0.019, (127, 128, "s16"): 0.012, (31, 94, "c64"): 0.020,
      (3, 47, "s16"): 0.017}


def count(N, U, D):
    """M(N) of include/lcs.h"""
    return 0 if N * U < 16 * D else (N * U - 16 * D) // D + 1


def need(t, U, D):
    """the least N with M(N) >= t >= 1"""
    return -(-((t - 1) * D + 16 * D) // U)


def corner(U, D):
    """two full workgroups and a partial column of outputs (256 columns per workgroup at up == 1), the stream no longer than they need"""
    NI = 8 if U == 1 else T.geometry(U, D)[1]
    n_out = 2 * (32 * NI * U) + U + 1
    n_in = RR.n_in_min(n_out, U, D)
    assert count(n_in, U, D) == n_out
    return n_out, n_in


def signal(seed, n_in, fs_in, shifts, a0, burst_at=0, burst_len=0, burst_amp=0.0):
    """burst_amp: the amplitude of the burst on carrier BURST_CH's tone, burst_len samples from burst_at on"""
    rng = np.random.default_rng(seed)
    n = np.arange(n_in, dtype=np.float64)
    amp = K.amplitudes(a0, len(shifts))
    x = 1e-4 * a0 * T.noise_and_tones(seed, n_in, fs_in)
    for k, (f, a) in enumerate(zip(shifts, amp)):
        tone = np.exp(2j * np.pi * ((f + 37e3 + 1.7e3 * k) / fs_in) * n + 1j * rng.uniform(0, 2 * np.pi))
        x += a * tone
        if k == BURST_CH:      # two pieces of opposite sign, twenty pieces' length apart: both clamps
            for at, sign in ((burst_at, 1.0), (burst_at + 20 * burst_len, -1.0)):
                x[at:at + burst_len] += sign * burst_amp * tone[at:at + burst_len]
    assert np.abs(x.real).max() < 1 and np.abs(x.imag).max() < 1
    return x


def rule(y, n_cap):
    """y: [n_ch][>= n_caps n_cap] complex64, the float stream's outputs -> (codes uint8 [n_caps][n_ch][n_cap][2], gains float32
    [n_caps][n_ch], v = 4^e P / 2 float64 [n_caps][n_ch]): P in float64 from the floats, e by chan_u8_ref.exponent, codes =
    clip(127 + rint(float32(2^e) * y), 0, 255) and 127 where y is not finite.  2^e * y is exact in fp32."""
    y = np.asarray(y, np.complex64)
    n_caps = y.shape[1] // n_cap
    yc = y[:, :n_caps * n_cap].reshape(y.shape[0], n_caps, n_cap).transpose(1, 0, 2)
    comp = np.stack([yc.real, yc.imag], axis=-1).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        P = np.mean(comp.astype(np.float64) ** 2, axis=(2, 3)) * 2.0
        e = np.array([[U8.exponent(p) for p in row] for row in P]).reshape(P.shape)
        gain = np.ldexp(np.float32(1.0), e).astype(np.float32)
        z = gain[:, :, None, None] * comp
        v = np.where(np.isfinite(P), 4.0 ** e * P / 2.0, np.nan)
    return U8.code(z), gain, v


def margin(v):
    """the least relative distance of a 4^e P / 2 from an end of (16^2, 32^2]; captures without a finite, positive power do not count"""
    v = v[np.isfinite(v) & (v > 0)]
    return float(np.minimum(v / U8.LO - 1.0, 1.0 - v / U8.HI).min())


@functools.lru_cache(maxsize=None)
def stream_case(U, D, fmt, a0=None):
    """-> dict(q, n_in, fs_in, shifts, n_cap, n_caps, n_out): computed once, shared, never written to.  q: the stream as the device takes
    it, n_out = M(n_in) = 3 n_cap + n_cap // 2."""
    n_cap = corner(U, D)[0]
    n_out = 3 * n_cap + n_cap // 2
    n_in = RR.n_in_min(n_out, U, D)
    fs_in = FS_OUT * D / U
    f = T.shifts17(fs_in)
    seed, a0 = 1000 * D + 10 * U + len(fmt), A0[(U, D, fmt)] if a0 is None else a0
    # the burst: 30 dB above the rms carrier BURST_CH has without it (its own tone and whatever else of the band its filter passes)
    quiet = RR.channelize_rate_ref(R.quantise(signal(seed, n_in, fs_in, f, a0), fmt)[1], fs_in, U, D, f[BURST_CH:BURST_CH + 1], n_out)
    burst_amp = 10.0 ** 1.5 * float(np.sqrt(np.mean(np.abs(quiet) ** 2)))
    x = signal(seed, n_in, fs_in, f, a0, need(n_cap + n_cap // 2, U, D), -(-2 * D // U), burst_amp)
    q, xq = R.quantise(x, fmt)
    for a in (q, xq, f):
        a.setflags(write=False)
    return dict(q=q, xq=xq, n_in=n_in, fs_in=fs_in, shifts=f, n_cap=n_cap, n_caps=3, n_out=n_out, up=U, down=D, fmt=fmt)


def reference(case):
    """the float64 channelizer's outputs of the whole stream, as complex64: what the premise is checked on beforehand"""
    return RR.channelize_rate_ref(case["xq"], case["fs_in"], case["up"], case["down"], case["shifts"], case["n_out"]).astype(np.complex64)


def chunkings(U, D, n_in, seed):
    """the five cuts of tests/test_gpu_channelizer_stream.py"""
    rng = np.random.default_rng(seed)
    L = -(-16 * D // U)                       # the first output needs L samples
    rand = []
    while sum(rand) < n_in:
        rand.append(min(int(rng.integers(1, 3 * D + 1)), n_in - sum(rand)))
    short = [max(1, (L - 1) // 5)] * 5        # together shorter than the filter
    return {"one": [n_in],
            "ones_across_a_window": [L - 3] + [1] * (2 * D + 8) + [n_in - (L - 3) - (2 * D + 8)],
            "all_of_down": [D] * (n_in // D) + ([n_in % D] if n_in % D else []),
            "random": rand,
            "short_start": short + [n_in - sum(short)]}


# ---- the smaller streams: T.noise_and_tones as it is, n_caps whole captures and nothing behind them.  The seed is chosen on the CPU so
# that the reference holds the condition with MARGIN_REF (test_channelizer_stream_u8_host.py::test_gpu_cases_hold_their_premise).
MARGIN_REF = 0.012     # on the float64 reference: the GPU's floats differ from it by 1e-5, so its own 4^e P / 2 keeps MARGIN
# name -> (U, D, fmt, n_cap (None: corner(U, D)[0]), n_caps, n_ch, seed)
NONFINITE_SEED = 36    # T.nonfinite_case(NONFINITE_SEED) cut into captures of n_out // 3: the Inf spoils outputs of capture 1 only
SIMPLE = {
    "nine_12_125_n5": (12, 125, "s16", 5, 9, 17, 1), "nine_12_125_n1": (12, 125, "s16", 1, 9, 17, 2), "nine_12_125_n8": (12, 125, "s16", 8, 9, 17, 1),
    "nine_1_16_n5": (1, 16, "s16", 5, 9, 17, 2), "nine_1_16_n1": (1, 16, "s16", 1, 9, 17, 13), "nine_1_16_n8": (1, 16, "s16", 8, 9, 17, 3),
    "guard_2_3": (2, 3, "s8", None, 1, 33, 1),
}


@functools.lru_cache(maxsize=None)
def simple_case(name, seed=None):
    U, D, fmt, n_cap, n_caps, n_ch, seed0 = SIMPLE[name]
    seed = seed0 if seed is None else seed
    n_cap = corner(U, D)[0] if n_cap is None else n_cap
    n_out = n_caps * n_cap
    n_in = need(n_out, U, D)
    fs_in = FS_OUT * D / U
    f = np.resize(T.shifts17(fs_in), n_ch)
    q, xq = R.quantise(T.noise_and_tones(seed, n_in, fs_in), fmt)
    for a in (q, xq, f):
        a.setflags(write=False)
    return dict(q=q, xq=xq, n_in=n_in, fs_in=fs_in, shifts=f, n_cap=n_cap, n_caps=n_caps, n_out=n_out, up=U, down=D, fmt=fmt)


# ---- the long stream: 2^21 s16 samples at 12/125, n_cap = 4099: 49 captures.  The tones of signal() without the burst: a carrier's power
# is its tones', the same in every capture, so one amplitude puts all 17 x 49 values clear of the ends.
LONG = dict(U=12, D=125, fmt="s16", n_in=1 << 21, n_cap=4099, a0=0.25)


@functools.lru_cache(maxsize=None)
def long_case(a0=None):
    U, D, n_in = LONG["U"], LONG["D"], LONG["n_in"]
    fs_in = FS_OUT * D / U
    f = T.shifts17(fs_in)
    q, xq = R.quantise(signal(2021, n_in, fs_in, f, LONG["a0"] if a0 is None else a0), "s16")
    n_out = count(n_in, U, D)
    for a in (q, xq, f):
        a.setflags(write=False)
    return dict(q=q, xq=xq, n_in=n_in, fs_in=fs_in, shifts=f, n_cap=LONG["n_cap"], n_caps=n_out // LONG["n_cap"], n_out=n_out, up=U, down=D, fmt="s16")
