"""What the channelizer's entry points refuse (channelizer.h: chan_refusal, compiled for the host in tests/host/chan_args_host.cpp):
the exact text of the first rule a call breaks, per case.  The cases are those of test_bad_arguments_are_refused_and_leave_the_
context_usable in the three GPU files, one pair of broken rules per step of the order, and the n_in bound of either form."""
import ctypes as C

import numpy as np
import pytest

import chan_rate_twin as T

C64, U8, S8, S16 = 0, 1, 3, 4
FS_OUT = 1.92e6
NULL, DOWN, UP, INTERP, RATIO, COMMON = ("null pointer", "down outside 2..128", "up outside 1..127", "up >= down: interpolation is not supported",
                                         "down / up > 16", "up and down have a common factor")
DECIM, N_CH, N_OUT, FS = "decim outside 2..16", "n_ch < 1", "n_out < 1", "fs_in is not a positive rate"
SHORT_INT = "n_in < (n_out-1)*decim + 16*decim: the capture is too short for n_out outputs"
SHORT_RAT = "n_in < floor(((n_out-1)*down + 16*down - 1) / up) + 1: the capture is too short for n_out outputs"
FMT, SHIFT, OUT, WIDE = "unknown sample format", "|f_shift| > fs_in/2", "d_out is not 16-byte aligned", "d_wide is not aligned to its sample size"

SHIFTS = (0.0, 250e3, -1.0e6)
# a valid call of each form (the GPU files' own): decim = lcs_channelize, rational = lcs_channelize_rational, u8 = lcs_channelize_u8
# at up == 1.  n_in is the least the call takes: 511 * 4 + 64; floor((511 * 4 + 63) / 3) + 1; 256 * 16 + 256.
GOOD = dict(decim=dict(form=1, wide=0x10000, fmt=S16, n_in=2108, fs=4 * FS_OUT, up=1, down=4, f=SHIFTS, n_ch=3, out=0x20000, n_out=512),
            rational=dict(form=0, wide=0x10000, fmt=S16, n_in=703, fs=FS_OUT * 4 / 3, up=3, down=4, f=SHIFTS, n_ch=3, out=0x20000, n_out=512),
            u8=dict(form=0, wide=0x10000, fmt=S16, n_in=4352, fs=16 * FS_OUT, up=1, down=16, f=SHIFTS, n_ch=3, out=0x20000, n_out=257))

CASES = [
    # ---- tests/test_gpu_channelizer.py
    ("decim", "null_wide", dict(wide=0), NULL), ("decim", "null_shift", dict(f=None), NULL), ("decim", "null_out", dict(out=0), NULL),
    ("decim", "decim_1", dict(down=1), DECIM), ("decim", "decim_17", dict(down=17), DECIM), ("decim", "no_channel", dict(n_ch=0), N_CH),
    ("decim", "short_capture", dict(n_in=2107), SHORT_INT),
    ("decim", "shift_beyond_nyquist", dict(f=(0.0, 0.5 * 4 * FS_OUT + 1.0, 0.0)), SHIFT),
    ("decim", "negative_shift_beyond", dict(f=(-0.51 * 4 * FS_OUT, 0.0, 0.0)), SHIFT),
    ("decim", "unknown_fmt", dict(fmt=U8), FMT), ("decim", "unknown_fmt_9", dict(fmt=9), FMT), ("decim", "misaligned_out", dict(out=0x20008), OUT),
    # ---- tests/test_gpu_channelizer_rate.py
    ("rational", "rate_25_16", dict(up=25, down=16), INTERP), ("rational", "rate_1_17", dict(up=1, down=17), RATIO),
    ("rational", "rate_1_129", dict(up=1, down=129), DOWN), ("rational", "rate_6_8", dict(up=6, down=8), COMMON),
    ("rational", "rate_4_4", dict(up=4, down=4), INTERP), ("rational", "rate_7_113", dict(up=7, down=113), RATIO),
    ("rational", "up_0", dict(up=0), UP), ("rational", "short_capture", dict(n_in=702), SHORT_RAT),
    ("rational", "shift_beyond_nyquist", dict(f=(0.0, 0.5 * FS_OUT * 4 / 3 + 1.0, 0.0)), SHIFT), ("rational", "unknown_fmt", dict(fmt=U8), FMT),
    ("rational", "misaligned_out", dict(out=0x20008), OUT), ("rational", "null_wide", dict(wide=0), NULL),
    ("rational", "null_shift", dict(f=None), NULL), ("rational", "null_out", dict(out=0), NULL), ("rational", "no_channel", dict(n_ch=0), N_CH),
    # ---- tests/test_gpu_channelizer_u8.py (363 = floor((256 * 4 + 63) / 3) + 1 is what 257 outputs at 3/4 take)
    ("u8", "null_out", dict(out=0), NULL), ("u8", "misaligned_out", dict(out=0x20008), OUT), ("u8", "up_equals_down", dict(up=4, down=4), INTERP),
    ("u8", "up_above_down", dict(up=5, down=4), INTERP), ("u8", "ratio_above_16", dict(up=1, down=17), RATIO),
    ("u8", "ratio_above_16_rational", dict(up=3, down=49), RATIO), ("u8", "short_capture", dict(n_in=4351), SHORT_INT),
    ("u8", "short_capture_rational", dict(up=3, down=4, n_in=362), SHORT_RAT), ("u8", "no_channel", dict(n_ch=0), N_CH),
    ("u8", "u8_as_input", dict(fmt=U8), FMT),
    # ---- the order: a call that breaks two rules is refused by the earlier one
    ("decim", "null_before_decim", dict(wide=0, down=17), NULL), ("rational", "null_before_rate", dict(out=0, down=200), NULL),
    ("decim", "decim_before_n_ch", dict(down=17, n_ch=0), DECIM), ("rational", "down_before_up", dict(up=0, down=200), DOWN),
    ("rational", "up_before_interpolation", dict(up=200, down=100), UP), ("rational", "interpolation_before_common_factor", dict(up=8, down=4), INTERP),
    ("rational", "ratio_before_common_factor", dict(up=2, down=34), RATIO), ("rational", "common_factor_before_n_ch", dict(up=6, down=8, n_ch=0), COMMON),
    ("decim", "n_ch_before_n_out", dict(n_ch=0, n_out=0), N_CH), ("rational", "n_ch_before_n_out", dict(n_ch=-1, n_out=0), N_CH),
    ("decim", "n_out_before_fs", dict(n_out=0, fs=0.0), N_OUT), ("rational", "n_out_before_fs", dict(n_out=0, fs=-1.0), N_OUT),
    ("decim", "fs_before_n_in", dict(fs=float("nan"), n_in=0), FS), ("rational", "fs_before_n_in", dict(fs=float("inf"), n_in=0), FS),
    ("decim", "n_in_before_fmt", dict(n_in=2107, fmt=9), SHORT_INT), ("rational", "n_in_before_fmt", dict(n_in=702, fmt=9), SHORT_RAT),
    ("decim", "fmt_before_shift", dict(fmt=2, f=(0.0, 1e9, 0.0)), FMT), ("rational", "fmt_before_shift", dict(fmt=-1, f=(0.0, 1e9, 0.0)), FMT),
    ("decim", "shift_before_out", dict(f=(0.0, 0.0, float("nan")), out=0x20008), SHIFT), ("rational", "shift_before_out", dict(f=(1e9, 0.0, 0.0), out=0x20004), SHIFT),
    ("decim", "out_before_wide", dict(out=0x20008, wide=0x10001), OUT), ("rational", "out_before_wide", dict(out=0x20001, wide=0x10002), OUT),
    ("decim", "wide_s16_at_2", dict(wide=0x10002), WIDE), ("rational", "wide_c64_at_4", dict(fmt=C64, wide=0x10004), WIDE),
    ("u8", "wide_s8_at_1", dict(fmt=S8, wide=0x10001), WIDE),
    # ---- the n_in rule at the bound and one below it: the integer form's text at up == 1 from either set of rate rules
    ("decim", "n_in_at_bound", dict(), None), ("decim", "n_in_below_bound", dict(n_in=2107), SHORT_INT),
    ("u8", "n_in_at_bound_up_1", dict(), None), ("u8", "n_in_below_bound_up_1", dict(n_in=4351), SHORT_INT),
    ("rational", "n_in_at_bound", dict(), None), ("rational", "n_in_below_bound", dict(n_in=702), SHORT_RAT),
    ("rational", "n_in_at_bound_12_125", dict(up=12, down=125, n_out=126, n_in=1469), None),       # floor((125 * 125 + 1999) / 12) + 1
    ("rational", "n_in_below_bound_12_125", dict(up=12, down=125, n_out=126, n_in=1468), SHORT_RAT),
    # ---- valid calls: the edges of what is taken
    ("decim", "valid_decim_2_s8_wide_at_2", dict(down=2, fmt=S8, wide=0x10002), None), ("decim", "valid_decim_16_c64", dict(down=16, fmt=C64, n_in=8432), None),
    ("rational", "valid_127_128", dict(up=127, down=128, n_in=4096), None), ("rational", "valid_shift_at_nyquist", dict(f=(0.5 * FS_OUT * 4 / 3, 0.0, 0.0)), None),
    ("u8", "valid_3_4", dict(up=3, down=4, n_in=363), None), ("u8", "valid_out_at_any_16", dict(out=0x20010), None),
]


@pytest.fixture(scope="module")
def host():
    L = T.host_lib("chan_args_host")
    L.chan_args_refusal.argtypes = [C.c_int, C.c_ulonglong, C.c_int, C.c_ulonglong, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int,
                                    C.c_ulonglong, C.c_uint]
    L.chan_args_refusal.restype = C.c_char_p
    return L


def test_every_refusal_has_the_text_of_the_first_rule_the_call_breaks(host):
    assert len({(form, name) for form, name, _, _ in CASES}) == len(CASES)
    wrong = []
    for form, name, kw, text in CASES:
        a = dict(GOOD[form], **kw)
        f = None if a["f"] is None else np.array(a["f"], np.float64)
        got = host.chan_args_refusal(a["form"], a["wide"], a["fmt"], a["n_in"], a["fs"], a["up"], a["down"],
                                     None if f is None else f.ctypes.data_as(C.POINTER(C.c_double)), a["n_ch"], a["out"], a["n_out"])
        got = None if got is None else got.decode()
        if got != text:
            wrong.append((form, name, got, text))
    assert not wrong, wrong
