"""The channelizer's continuous form on the host (channelizer.h: cs_count, cs_base, cs_keep_max, cs_plan_push, cs_source,
chan_stream_refusal -- compiled for the host in tests/host/chan_stream_host.cpp): counting against chan_refusal and the premises
of a push's kernels over the whole rate domain, the refusal texts and their order, a CPU walk of chunked streams against the
one-shot launch, and the same counting and source-map cases as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import chan_rate_twin as T

C64, U8, S8, S16 = 0, 1, 3, 4
DOMAIN = [(1, d) for d in range(2, 17)] + T.PAIRS
OPEN, COUNT, PUSH, CLOSE = 0, 1, 2, 3
PREMISES = {1: "kept samples exceed a history slot", 2: "the aligned base moved back", 3: "the aligned base lies behind the next output's window",
            4: "the history does not start at the first launched column", 5: "a workgroup reads in front of the base", 6: "history index outside",
            7: "chunk index outside", 8: "a zero where a sample has arrived", 9: "a stored output's window has not arrived",
            10: "the history append reads no real sample", 11: "a stored output lies in no launched column", 12: "base + kept != N"}


@pytest.fixture(scope="module")
def host():
    L = T.host_lib("chan_stream_host")
    ull, up = C.c_ulonglong, C.POINTER(C.c_ulonglong)
    L.cs_host_count.argtypes, L.cs_host_count.restype = [ull, C.c_int, C.c_int], ull
    L.cs_host_keep_max.argtypes, L.cs_host_keep_max.restype = [C.c_int, C.c_int], C.c_uint
    L.cs_host_check_counts.argtypes, L.cs_host_check_counts.restype = [C.c_int, C.c_int], C.c_longlong
    L.cs_host_check_stream.argtypes, L.cs_host_check_stream.restype = [C.c_int, C.c_int, ull, C.c_int], C.c_longlong
    L.cs_host_check_chunks.argtypes, L.cs_host_check_chunks.restype = [C.c_int, C.c_int, up, C.c_int], C.c_longlong
    L.cs_host_refusal.argtypes, L.cs_host_refusal.restype = [C.c_int, C.c_int, C.c_int, ull, ull, ull, C.c_uint, C.c_uint, ull], C.c_char_p
    L.cs_host_open_refusal.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int]
    L.cs_host_open_refusal.restype = C.c_char_p
    L.cs_host_run.argtypes = [C.c_int, C.c_void_p, ull, C.c_int, C.c_int, up, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_float), up, C.c_int]
    L.cs_host_run.restype = C.c_longlong
    return L


def count_py(N, U, D):
    """M(N) of include/lcs.h"""
    return 0 if N * U < 16 * D else (N * U - 16 * D) // D + 1


def test_the_domain_is_the_one_the_entry_points_take():
    assert len(T.PAIRS) == 4696 and len(DOMAIN) == 4711


def test_count_is_the_largest_n_out_the_one_shot_call_takes(host):
    """over the whole domain, a few hundred N per rate around Tg / up and around multiples of down: n_out = M(N) passes chan_refusal,
    n_out = M(N) + 1 is refused as too short; M never falls and grows by at most one per sample"""
    bad, total = [], 0
    for U, D in DOMAIN:
        n = host.cs_host_check_counts(U, D)
        if n < 0:
            bad.append((U, D, -n - 1))
        total += max(n, 0)
    assert not bad, bad[:8]
    assert total >= 200 * len(DOMAIN)
    for U, D, N in ((12, 125, 1600000), (1, 16, 2457600), (127, 128, 2 ** 62), (2, 3, 2 ** 64 - 1)):      # no limit below 2^64 samples
        assert host.cs_host_count(N, U, D) == count_py(N, U, D)


def test_history_slot_holds_what_the_bound_says(host):
    """cs_keep_max is ceil(16 D / U + D - D / U) - 1: below 16 * down / up + down, 365 at the most (8/127)"""
    worst = 0
    for U, D in DOMAIN:
        k = host.cs_host_keep_max(U, D)
        assert k == -(-(16 * D + (U - 1) * D) // U) - 1 and k < 16 * D / U + D
        worst = max(worst, k)
    assert worst == 365 and host.cs_host_keep_max(8, 127) == 365


def test_every_push_of_seeded_streams_keeps_the_kernels_premises(host):
    """three seeded chunk sequences per rate (runs of 0, 1 and 2 samples among them): the kept count fits the slot, the aligned base
    neither moves back nor passes the next output's window, and every staged index of every launched workgroup is a real sample of
    the history or the chunk, or a zero behind the chunk's end -- never a sample in front of the base"""
    bad = []
    for U, D in DOMAIN:
        for seed in range(3):
            rc = host.cs_host_check_stream(U, D, seed + 7 * U + 1000 * D, 60)
            if rc:
                bad.append((U, D, seed, "push %d" % (rc // 100 - 1), PREMISES[rc % 100]))
    assert not bad, bad[:8]


@pytest.mark.parametrize("U,D", [(1, 2), (1, 16), (2, 3), (12, 125), (127, 128), (31, 94), (3, 47), (8, 127)])
def test_tiny_chunks_hold_the_premises_too(host, U, D):
    for chunks in ([1] * (40 * D), [0, 1, 2] * (12 * D), [D] * 80, [16 * D // U - 1, 0, 1, 1, 1, 2, 5 * D, 1, 0, 3 * 256 * D + 1, 1]):
        a = np.array(chunks, np.uint64)
        rc = host.cs_host_check_chunks(U, D, a.ctypes.data_as(C.POINTER(C.c_ulonglong)), a.size)
        assert rc == 0, (chunks[:6], "push %d" % (rc // 100 - 1), PREMISES[rc % 100])


# ---- refusals
ALREADY, NONE = "a channelizer stream is already open on this context", "no channelizer stream is open on this context"
BIG, NULL_CHUNK, CHUNK_ALIGN = "n_chunk > 2^31", "null chunk with n_chunk > 0", "d_chunk is not aligned to its sample size"
NULL_OUT, OUT_ALIGN, STRIDE = "null d_out with outputs to hand out", "d_out is not 8-byte aligned", "row_stride < out_cap"
CAP = "out_cap < n_emit: size or split the chunk by lcs_chan_stream_count"
GOOD = dict(entry=PUSH, open=1, fmt=S16, chunk=0x10000, n_chunk=4096, out=0x20008, stride=300, cap=256, n_emit=256)
PUSH_CASES = [
    ("valid", dict(), None), ("valid_out_at_8_not_16", dict(out=0x20008), None), ("valid_nothing_to_do", dict(chunk=0, n_chunk=0, out=0, n_emit=0), None),
    ("valid_no_output_null_out", dict(out=0, n_emit=0, cap=0, stride=0), None), ("valid_s8_at_2", dict(fmt=S8, chunk=0x10002), None),
    ("valid_n_chunk_at_2_31", dict(n_chunk=2 ** 31, n_emit=200), None), ("valid_stride_equals_cap", dict(stride=256), None),
    ("not_open", dict(open=0), NONE), ("count_not_open", dict(entry=COUNT, open=0), NONE), ("close_not_open", dict(entry=CLOSE, open=0), NONE),
    ("open_twice", dict(entry=OPEN), ALREADY), ("open_first", dict(entry=OPEN, open=0), None), ("close_open", dict(entry=CLOSE), None),
    ("too_long", dict(n_chunk=2 ** 31 + 1), BIG), ("count_too_long", dict(entry=COUNT, n_chunk=2 ** 31 + 1), BIG),
    ("count_looks_at_nothing_else", dict(entry=COUNT, chunk=0, out=3, stride=0), None),
    ("null_chunk", dict(chunk=0), NULL_CHUNK), ("chunk_s16_at_2", dict(chunk=0x10002), CHUNK_ALIGN), ("chunk_c64_at_4", dict(fmt=C64, chunk=0x10004), CHUNK_ALIGN),
    ("chunk_s8_at_1", dict(fmt=S8, chunk=0x10001), CHUNK_ALIGN), ("null_out", dict(out=0), NULL_OUT), ("out_at_4", dict(out=0x20004), OUT_ALIGN),
    ("stride_below_cap", dict(stride=255), STRIDE), ("cap_one_short", dict(cap=255, stride=255), CAP), ("cap_zero", dict(cap=0), CAP),
    # the order: a push that breaks two rules is refused by the earlier one
    ("open_before_length", dict(open=0, n_chunk=2 ** 32), NONE), ("length_before_null_chunk", dict(n_chunk=2 ** 31 + 1, chunk=0), BIG),
    ("null_chunk_before_out", dict(chunk=0, out=0x20004), NULL_CHUNK), ("chunk_align_before_null_out", dict(chunk=0x10002, out=0), CHUNK_ALIGN),
    ("null_out_before_stride", dict(out=0, stride=1), NULL_OUT), ("out_align_before_stride", dict(out=0x20004, stride=1), OUT_ALIGN),
    ("stride_before_cap", dict(stride=100, cap=200), STRIDE),
]
FS_OUT = 1.92e6
OPEN_GOOD = dict(open=0, fmt=S16, fs=FS_OUT * 125 / 12, up=12, down=125, f=(0.0, 250e3, -1.0e6), n_ch=3)
OPEN_CASES = [
    ("valid", dict(), None), ("valid_decim_16", dict(up=1, down=16, fs=16 * FS_OUT), None), ("valid_127_128", dict(up=127, down=128), None),
    ("null_shift", dict(f=None), "null pointer"), ("rate_25_16", dict(up=25, down=16), "up >= down: interpolation is not supported"),
    ("rate_1_17", dict(up=1, down=17), "down / up > 16"), ("rate_1_129", dict(up=1, down=129), "down outside 2..128"),
    ("rate_6_8", dict(up=6, down=8), "up and down have a common factor"), ("up_0", dict(up=0), "up outside 1..127"), ("no_channel", dict(n_ch=0), "n_ch < 1"),
    ("bad_fs", dict(fs=0.0), "fs_in is not a positive rate"), ("u8_as_input", dict(fmt=U8), "unknown sample format"),
    ("shift_beyond_nyquist", dict(f=(0.0, 0.5 * FS_OUT * 125 / 12 + 1.0, 0.0)), "|f_shift| > fs_in/2"),
    # the one-shot rules come first, in their order; "already open" is the last
    ("rate_before_n_ch", dict(up=6, down=8, n_ch=0), "up and down have a common factor"), ("n_ch_before_fs", dict(n_ch=0, fs=-1.0), "n_ch < 1"),
    ("fs_before_fmt", dict(fs=float("nan"), fmt=9), "fs_in is not a positive rate"), ("fmt_before_shift", dict(fmt=2, f=(1e9, 0.0, 0.0)), "unknown sample format"),
    ("shift_before_already_open", dict(open=1, f=(1e9, 0.0, 0.0)), "|f_shift| > fs_in/2"), ("already_open", dict(open=1), ALREADY),
]


def test_every_refusal_has_the_text_of_the_first_rule_the_call_breaks(host):
    wrong = []
    assert len({n for n, _, _ in PUSH_CASES}) == len(PUSH_CASES) and len({n for n, _, _ in OPEN_CASES}) == len(OPEN_CASES)
    for name, kw, text in PUSH_CASES:
        a = dict(GOOD, **kw)
        got = host.cs_host_refusal(a["entry"], a["open"], a["fmt"], a["chunk"], a["n_chunk"], a["out"], a["stride"], a["cap"], a["n_emit"])
        if (None if got is None else got.decode()) != text:
            wrong.append((name, got, text))
    for name, kw, text in OPEN_CASES:
        a = dict(OPEN_GOOD, **kw)
        f = None if a["f"] is None else np.array(a["f"], np.float64)
        got = host.cs_host_open_refusal(a["open"], a["fmt"], a["fs"], a["up"], a["down"], None if f is None else f.ctypes.data_as(C.POINTER(C.c_double)), a["n_ch"])
        if (None if got is None else got.decode()) != text:
            wrong.append(("open", name, got, text))
    assert not wrong, wrong


# ---- the walk
def _run(host, q, n_in, U, D, st, taps, chunks):
    n_out = count_py(n_in, U, D)
    out = np.full((st.size, n_out), np.nan, np.complex64)
    ch = np.array(chunks, np.uint64)
    rc = host.cs_host_run(S8, q.ctypes.data_as(C.c_void_p), n_in, U, D, st.ctypes.data_as(C.POINTER(C.c_ulonglong)), taps.ctypes.data_as(C.POINTER(C.c_float)),
                          st.size, out.ctypes.data_as(C.POINTER(C.c_float)), ch.ctypes.data_as(C.POINTER(C.c_ulonglong)), len(chunks))
    assert rc == 0, rc
    return out


def _chunkings(seed, n_in, D):
    """three seeded cuts of n_in samples: lengths in 0..3 D; 1..3 D with a run of forty ones and twos; a few long pieces"""
    rng = np.random.default_rng(seed)

    def cut(draw):
        out = []
        while sum(out) < n_in:
            out.append(min(int(draw(len(out))), n_in - sum(out)))
        return out
    return [cut(lambda k: rng.integers(0, 3 * D + 1)), cut(lambda k: rng.integers(1, 3) if 3 <= k < 43 else rng.integers(1, 3 * D + 1)),
            cut(lambda k: rng.integers(1, n_in // 3 + 2))]


@pytest.mark.parametrize("U,D", [(2, 3), (12, 125), (127, 128), (1, 2), (1, 16)])
def test_chunked_walk_equals_the_one_shot_walk_bit_for_bit(host, U, D):
    """Integer taps, raw s8 samples and carriers a whole number of quarter turns per sample: every product and every sum is exact in
    fp32.  17 carriers (two row blocks); two full workgroups and a partial column of outputs."""
    NI = 8 if U == 1 else T.geometry(U, D)[1]
    n_out = 2 * (32 * NI * U) + U + 1
    n_in = ((n_out - 1) * D + 16 * D - 1) // U + 1
    assert count_py(n_in, U, D) == n_out
    rng = np.random.default_rng(1000 * D + U)
    q = rng.integers(-128, 128, 2 * n_in).astype(np.int8)
    taps = rng.integers(-8, 9, 16 * D).astype(np.float32)
    st = (np.arange(17, dtype=np.uint64) % np.uint64(4)) << np.uint64(62)
    whole = _run(host, q, n_in, U, D, st, taps, [])
    assert np.isfinite(whole).all() and np.abs(whole).max() > 0
    # carrier 0 (no shift) against the sum of include/lcs.h in integers
    x = (q[0::2].astype(np.int64) + 1j * q[1::2].astype(np.int64))
    for m in (0, 1, U, n_out // 2, n_out - 1):
        n = np.arange(-(-m * D // U), (m * D + 16 * D - 1) // U + 1)
        want = U * np.sum(taps[m * D + 16 * D - 1 - n * U].astype(np.float64) * x[n]) / 128.0
        assert whole[0, m] == np.complex64(want), (m, whole[0, m], want)
    for chunks in _chunkings(10 * D + U, n_in, D):
        got = _run(host, q, n_in, U, D, st, taps, chunks)
        assert got.tobytes() == whole.tobytes(), (chunks[:8], np.argwhere(got != whole)[:4])


def test_stand_alone_program_is_clean_under_address_and_ub_sanitizers(tmp_path):
    """the same source as a program with its own main (-DCS_HOST_MAIN: counting and source map over every rate), built with
    -fsanitize=address,undefined and run as a process of its own"""
    exe = str(tmp_path / "chan_stream_host_san")
    src = os.path.join(T.ROOT, "tests", "host", "chan_stream_host.cpp")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-DCS_HOST_MAIN",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(T.ROOT, "include"), "-o", exe, src])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith(": ok"), (p.returncode, p.stdout[-500:], p.stderr[-2000:])
    assert p.stdout.startswith("4711 rates")


def test_new_symbols_are_declared_exported_and_prototyped():
    import re
    names = ["lcs_chan_stream_open", "lcs_chan_stream_count", "lcs_chan_stream_push", "lcs_chan_stream_close"]
    hdr = open(os.path.join(T.ROOT, "include", "lcs.h")).read()
    capi = open(os.path.join(T.ROOT, "lte-cell-scanner_amd", "capi.py")).read()
    for n in names:
        assert re.search(r"\bint %s\(lcs_ctx \*ctx" % n, hdr) and '"%s"' % n in capi and "L.%s.argtypes" % n in capi
