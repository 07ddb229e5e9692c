"""The channelizer stream's 8-bit captures on the host (channelizer.h: cs_need, cs_cap_segment, cs_cap_plan, chan_stream_u8_refusal --
compiled for the host in tests/host/chan_stream_u8_host.cpp): the inverse of the output count and the launcher's cut of a push where
captures fill over the whole rate domain, the refusal texts and their order, the same cases as a stand-alone program under
AddressSanitizer and UBSan, the premise of the GPU tests' exact comparison on the float64 reference, and sweep.records_with_gain."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import chan_rate_twin as T
import chan_stream_u8_cases as S
from conftest import load_pkg

C64, U8, S8, S16 = 0, 1, 3, 4
DOMAIN = [(1, d) for d in range(2, 17)] + T.PAIRS
OPEN, COUNT, PUSH, CLOSE = 0, 1, 2, 3
N_CAPS = (1, 5, 257, 153600)
PREMISES = {1: "the pieces do not add up to the chunk", 2: "an empty piece", 3: "a piece's outputs cross a capture's end", 4: "a piece's n_emit is not M's",
            5: "fills is not 'the capture is full'", 6: "a capture is complete inside a piece, or not at its end", 7: "n_done is not the closed form",
            8: "the fill count is not M(N) mod n_cap", 9: "a piece behind one that left its capture open", 90: "the chunk of nine captures",
            91: "a chunk cut in two completes other captures"}


@pytest.fixture(scope="module")
def host():
    L = T.host_lib("chan_stream_u8_host")
    ull, up = C.c_ulonglong, C.POINTER(C.c_ulonglong)
    L.csu_host_need.argtypes, L.csu_host_need.restype = [ull, C.c_int, C.c_int], ull
    L.csu_host_count.argtypes, L.csu_host_count.restype = [ull, C.c_int, C.c_int], ull
    L.csu_host_cap_done.argtypes, L.csu_host_cap_done.restype = [ull, ull, C.c_uint, C.c_int, C.c_int], ull
    L.csu_host_check_need.argtypes, L.csu_host_check_need.restype = [C.c_int, C.c_int], C.c_longlong
    L.csu_host_check_stream.argtypes, L.csu_host_check_stream.restype = [C.c_int, C.c_int, C.c_uint, ull, C.c_int], C.c_longlong
    L.csu_host_check_chunks.argtypes, L.csu_host_check_chunks.restype = [C.c_int, C.c_int, C.c_uint, up, C.c_int, up], C.c_longlong
    L.csu_host_plan.argtypes, L.csu_host_plan.restype = [ull, ull, C.c_uint, C.c_uint, C.c_int, C.c_int, up, C.c_longlong], C.c_longlong
    L.csu_host_refusal.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, ull, ull, ull, ull, C.c_uint, C.c_uint, ull]
    L.csu_host_refusal.restype = C.c_char_p
    L.csu_host_open_refusal.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_uint]
    L.csu_host_open_refusal.restype = C.c_char_p
    L.csu_host_float_refusal.argtypes, L.csu_host_float_refusal.restype = [C.c_int, C.c_int, C.c_int, ull], C.c_char_p
    return L


def test_need_is_the_inverse_of_count_over_the_whole_domain(host):
    """t around 1, around multiples of up and out to 2^40: M(need(t)) == t (up < down everywhere) and M(need(t) - 1) == t - 1"""
    assert len(DOMAIN) == 4711
    bad, total = [], 0
    for U, D in DOMAIN:
        n = host.csu_host_check_need(U, D)
        if n < 0:
            bad.append((U, D, -n))
        total += max(n, 0)
    assert not bad, bad[:8]
    assert total >= 80 * len(DOMAIN)
    for t, U, D in ((1, 12, 125), (153600, 12, 125), (2 ** 40, 127, 128), (2 ** 40, 1, 16), (781, 2, 3)):
        N = host.csu_host_need(t, U, D)
        assert N == S.need(t, U, D) and S.count(N, U, D) == t and S.count(N - 1, U, D) == t - 1


def test_every_push_of_seeded_streams_is_cut_where_captures_fill(host):
    """per rate and n_cap in 1, 5, 257, 153600 a seeded chunk sequence (runs of 0, 1 and 2 samples, one chunk that completes nine
    captures): the pieces add up to the chunk, no piece's outputs cross a capture's end, a capture is complete exactly at a piece's end,
    n_done is floor(M(N) / n_cap) - floor(M(N_prev) / n_cap), and every chunk cut in two at a seeded place completes the same captures"""
    bad = []
    for U, D in DOMAIN:
        for n_cap in N_CAPS:
            rc = host.csu_host_check_stream(U, D, n_cap, 5 * U + 1000 * D + n_cap, 30)
            if rc:
                bad.append((U, D, n_cap, "push %d" % (rc // 100 - 1), PREMISES[rc % 100]))
    assert not bad, bad[:8]


@pytest.mark.parametrize("U,D", [(1, 2), (1, 16), (2, 3), (12, 125), (127, 128), (8, 127)])
def test_tiny_chunks_and_a_chunk_of_nine_captures(host, U, D):
    for n_cap in N_CAPS:
        nine = S.need(9 * n_cap, U, D)
        for chunks in ([1] * (20 * D), [0, 1, 2] * (8 * D), [nine], [nine - 1, 1, 0, 1], [16 * D // U - 1, 0, 1, 1, 1, 2, 5 * D, 1, 0, nine]):
            a, done = np.array(chunks, np.uint64), np.zeros(len(chunks), np.uint64)
            rc = host.csu_host_check_chunks(U, D, n_cap, a.ctypes.data_as(C.POINTER(C.c_ulonglong)), a.size, done.ctypes.data_as(C.POINTER(C.c_ulonglong)))
            assert rc == 0, (n_cap, chunks[:6], "push %d" % (rc // 100 - 1), PREMISES[rc % 100])
            N = np.concatenate([[0], np.cumsum(a.astype(object))])
            assert [int(d) for d in done] == [S.count(int(N[k + 1]), U, D) // n_cap - S.count(int(N[k]), U, D) // n_cap for k in range(len(chunks))]
            if chunks == [nine]:
                assert int(done[0]) == 9
            if chunks == [nine - 1, 1, 0, 1]:
                assert [int(d) for d in done[:3]] == [8, 1, 0]      # the sample behind may complete one more (n_cap = 1)


def test_the_pieces_of_one_push(host):
    """12/125, n_cap = 5, a chunk from mid-capture on that completes three captures and starts a fourth"""
    U, D, n_cap = 12, 125, 5
    N_prev = S.need(7, U, D)                      # 7 outputs: capture 1 holds two of them
    n_chunk = S.need(22, U, D) - N_prev           # ... up to output 22: captures 1, 2, 3 complete, two outputs of capture 4
    out = np.zeros(3 * 8, np.uint64)
    n = host.csu_host_plan(N_prev, n_chunk, 2, n_cap, U, D, out.ctypes.data_as(C.POINTER(C.c_ulonglong)), 8)
    pieces = out[:3 * n].reshape(n, 3).tolist()
    ends = [S.need(t, U, D) for t in (10, 15, 20, 22)]
    assert pieces == [[ends[0] - N_prev, 3, 1], [ends[1] - ends[0], 5, 1], [ends[2] - ends[1], 5, 1], [ends[3] - ends[2], 2, 0]]
    assert host.csu_host_cap_done(N_prev, n_chunk, n_cap, U, D) == 3


# ---- refusals
ALREADY, NONE = "a channelizer stream is already open on this context", "no channelizer stream is open on this context"
FLOATS, BYTES_STREAM = "the stream hands out floats: 8-bit captures need lcs_chan_stream_open_u8", "the stream hands out 8-bit captures: push with lcs_chan_stream_push_u8"
BIG, NULL_CHUNK, CHUNK_ALIGN = "n_chunk > 2^31", "null chunk with n_chunk > 0", "d_chunk is not aligned to its sample size"
NULL_OUT, OUT_ALIGN, GAIN_ALIGN = "null d_out with captures to hand out", "d_out is not 16-byte aligned", "d_gain is not aligned to a float"
ROOM, N_CAP = "cap_room < n_done: size d_out or split the chunk by lcs_chan_stream_count_u8", "n_cap < 1"
GOOD = dict(entry=PUSH, open=1, u8=1, fmt=S16, chunk=0x10000, n_chunk=4096, out=0x20010, gain=0x30004, room=2, n_cap=100, n_done=2)
PUSH_CASES = [
    ("valid", dict(), None), ("valid_no_gain", dict(gain=0), None), ("valid_nothing_to_do", dict(chunk=0, n_chunk=0, out=0, n_done=0, room=0), None),
    ("valid_no_capture_null_out", dict(out=0, n_done=0, room=0), None), ("valid_s8_at_2", dict(fmt=S8, chunk=0x10002), None),
    ("valid_n_chunk_at_2_31", dict(n_chunk=2 ** 31), None), ("valid_room_to_spare", dict(room=16), None),
    ("not_open", dict(open=0), NONE), ("count_not_open", dict(entry=COUNT, open=0), NONE), ("float_stream", dict(u8=0), FLOATS),
    ("count_float_stream", dict(entry=COUNT, u8=0), FLOATS), ("too_long", dict(n_chunk=2 ** 31 + 1), BIG), ("count_too_long", dict(entry=COUNT, n_chunk=2 ** 31 + 1), BIG),
    ("count_looks_at_nothing_else", dict(entry=COUNT, chunk=0, out=3, gain=1, room=0), None),
    ("null_chunk", dict(chunk=0), NULL_CHUNK), ("chunk_s16_at_2", dict(chunk=0x10002), CHUNK_ALIGN), ("chunk_c64_at_4", dict(fmt=C64, chunk=0x10004), CHUNK_ALIGN),
    ("chunk_s8_at_1", dict(fmt=S8, chunk=0x10001), CHUNK_ALIGN), ("null_out", dict(out=0), NULL_OUT), ("out_at_8", dict(out=0x20008), OUT_ALIGN),
    ("out_at_8_nothing_done", dict(out=0x20008, n_done=0), OUT_ALIGN), ("gain_at_2", dict(gain=0x30002), GAIN_ALIGN),
    ("room_one_short", dict(room=1), ROOM), ("room_zero", dict(room=0), ROOM),
    # the order: a call that breaks two rules is refused by the earlier one
    ("open_before_kind", dict(open=0, u8=0), NONE), ("kind_before_length", dict(u8=0, n_chunk=2 ** 32), FLOATS), ("length_before_null_chunk", dict(n_chunk=2 ** 31 + 1, chunk=0), BIG),
    ("null_chunk_before_out", dict(chunk=0, out=0x20008), NULL_CHUNK), ("chunk_align_before_null_out", dict(chunk=0x10002, out=0), CHUNK_ALIGN),
    ("null_out_before_room", dict(out=0, room=0), NULL_OUT), ("out_align_before_gain", dict(out=0x20008, gain=0x30002), OUT_ALIGN),
    ("gain_before_room", dict(gain=0x30002, room=1), GAIN_ALIGN),
]
FS_OUT = 1.92e6
OPEN_GOOD = dict(open=0, fmt=S16, fs=FS_OUT * 125 / 12, up=12, down=125, f=(0.0, 250e3, -1.0e6), n_ch=3, n_cap=153600)
OPEN_CASES = [
    ("valid", dict(), None), ("valid_decim_16", dict(up=1, down=16, fs=16 * FS_OUT), None), ("valid_n_cap_1", dict(n_cap=1), None),
    ("null_shift", dict(f=None), "null pointer"), ("rate_25_16", dict(up=25, down=16), "up >= down: interpolation is not supported"),
    ("rate_1_17", dict(up=1, down=17), "down / up > 16"), ("rate_6_8", dict(up=6, down=8), "up and down have a common factor"), ("no_channel", dict(n_ch=0), "n_ch < 1"),
    ("bad_fs", dict(fs=0.0), "fs_in is not a positive rate"), ("u8_as_input", dict(fmt=U8), "unknown sample format"),
    ("shift_beyond_nyquist", dict(f=(0.0, 0.5 * FS_OUT * 125 / 12 + 1.0, 0.0)), "|f_shift| > fs_in/2"), ("n_cap_0", dict(n_cap=0), N_CAP), ("already_open", dict(open=1), ALREADY),
    # open's rules come first, in their order; then n_cap; "already open" is the last
    ("rate_before_n_cap", dict(up=6, down=8, n_cap=0), "up and down have a common factor"), ("shift_before_n_cap", dict(n_cap=0, f=(1e9, 0.0, 0.0)), "|f_shift| > fs_in/2"),
    ("n_cap_before_already_open", dict(open=1, n_cap=0), N_CAP),
]


def test_every_refusal_has_the_text_of_the_first_rule_the_call_breaks(host):
    wrong = []
    assert len({n for n, _, _ in PUSH_CASES}) == len(PUSH_CASES) and len({n for n, _, _ in OPEN_CASES}) == len(OPEN_CASES)
    for name, kw, text in PUSH_CASES:
        a = dict(GOOD, **kw)
        got = host.csu_host_refusal(a["entry"], a["open"], a["u8"], a["fmt"], a["chunk"], a["n_chunk"], a["out"], a["gain"], a["room"], a["n_cap"], a["n_done"])
        if (None if got is None else got.decode()) != text:
            wrong.append((name, got, text))
    for name, kw, text in OPEN_CASES:
        a = dict(OPEN_GOOD, **kw)
        f = None if a["f"] is None else np.array(a["f"], np.float64)
        got = host.csu_host_open_refusal(a["open"], a["fmt"], a["fs"], a["up"], a["down"], None if f is None else f.ctypes.data_as(C.POINTER(C.c_double)), a["n_ch"],
                                         a["n_cap"])
        if (None if got is None else got.decode()) != text:
            wrong.append(("open", name, got, text))
    assert not wrong, wrong


def test_the_float_push_refuses_a_stream_of_8_bit_captures_and_count_and_close_take_it(host):
    dec = lambda b: None if b is None else b.decode()
    assert dec(host.csu_host_float_refusal(PUSH, 1, 1, 100)) == BYTES_STREAM
    assert dec(host.csu_host_float_refusal(PUSH, 1, 1, 2 ** 32)) == BYTES_STREAM      # in front of the chunk's length
    assert dec(host.csu_host_float_refusal(PUSH, 0, 1, 100)) == NONE                  # behind "no stream"
    assert dec(host.csu_host_float_refusal(PUSH, 1, 0, 100)) is None
    assert dec(host.csu_host_float_refusal(COUNT, 1, 1, 100)) is None and dec(host.csu_host_float_refusal(CLOSE, 1, 1, 0)) is None
    assert dec(host.csu_host_float_refusal(OPEN, 1, 1, 0)) == ALREADY


def test_stand_alone_program_is_clean_under_address_and_ub_sanitizers(tmp_path):
    """the same source as a program with its own main (-DCSU_HOST_MAIN: cs_need and seeded plans over every rate and the four capture
    lengths), built with -fsanitize=address,undefined and run as a process of its own"""
    exe = str(tmp_path / "chan_stream_u8_host_san")
    src = os.path.join(T.ROOT, "tests", "host", "chan_stream_u8_host.cpp")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-DCSU_HOST_MAIN",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(T.ROOT, "include"), "-o", exe, src])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith(": ok"), (p.returncode, p.stdout[-500:], p.stderr[-2000:])
    assert p.stdout.startswith("4711 rates")


def test_new_symbols_are_declared_exported_and_prototyped():
    names = ["lcs_chan_stream_open_u8", "lcs_chan_stream_count_u8", "lcs_chan_stream_push_u8"]
    hdr = open(os.path.join(T.ROOT, "include", "lcs.h")).read()
    capi = open(os.path.join(T.ROOT, "lte-cell-scanner_amd", "capi.py")).read()
    for n in names:
        assert re.search(r"\bint %s\(lcs_ctx \*ctx" % n, hdr) and '"%s"' % n in capi and "L.%s.argtypes" % n in capi
    lib = load_pkg().capi.load()      # the library build() made; loading it touches no GPU
    for n in names:
        assert hasattr(lib, n), n


@pytest.mark.parametrize("U,D,fmt", S.CASES)
def test_gpu_cases_hold_their_premise(U, D, fmt):
    """on the float64 reference of every stream of tests/test_gpu_channelizer_stream_u8.py: 4^e P / 2 of every capture of every carrier
    lies 2 % or more clear of 16^2 and 32^2 (the GPU test asserts 1 % on its own floats, which differ from these by 1e-5), and the burst
    carrier's capture passes +-135 codes, so that codes 0 and 255 both occur"""
    case = S.stream_case(U, D, fmt)
    assert case["n_out"] == 3 * case["n_cap"] + case["n_cap"] // 2 == S.count(case["n_in"], U, D) and S.count(case["n_in"] - 1, U, D) == case["n_out"] - 1
    y = S.reference(case)
    codes, gain, v = S.rule(y, case["n_cap"])
    assert codes.shape == (3, 17, case["n_cap"], 2) and np.isfinite(v).all()
    assert S.margin(v) >= 2 * S.MARGIN, S.margin(v)
    b = codes[1, S.BURST_CH]
    z = y[S.BURST_CH, case["n_cap"]:2 * case["n_cap"]] * gain[1, S.BURST_CH]
    assert min(z.real.min(), z.imag.min()) <= -135 and max(z.real.max(), z.imag.max()) >= 135
    assert (b == 0).any() and (b == 255).any()
    assert len(set(gain.ravel().tolist())) >= (1 if (U, D) == (127, 128) else 2)      # at 127/128 every carrier's filter passes most of the band


# ---- sweep.records_with_gain
def _cell(pkg, fc, pss_pow, n_id_1=25, n_id_2=1, freq_superfine=7.3e3):
    c = pkg.capi.LcsCell()
    c.fc_requested = c.fc_programmed = fc
    c.pss_pow, c.n_id_1, c.n_id_2, c.freq_superfine = pss_pow, n_id_1, n_id_2, freq_superfine
    return c


def test_records_with_gain_puts_carriers_on_one_scale():
    """one cell seen by two carriers 100 kHz apart whose bytes carry the gains 4 and 16: in the byte domain the carrier that sees it
    weaker reports the larger pss_pow.  dedup on the raw records keeps that carrier; on records_with_gain it keeps the right one."""
    pkg = load_pkg()
    sw = pkg.sweep
    true_pow = (3.0e-3, 1.0e-3)                                   # carrier 0 sees the cell 4.8 dB stronger
    gain = np.array([4.0, 16.0], np.float32)
    cells = [[_cell(pkg, 735.0e6, true_pow[0] * 4.0 ** 2)], [_cell(pkg, 735.1e6, true_pow[1] * 16.0 ** 2, freq_superfine=-92.7e3)]]
    assert cells[1][0].pss_pow > cells[0][0].pss_pow              # the byte-domain order is the reverse of the true one
    raw = [[sw.record_to_dict(r) for r in sw.cells_to_records(c)] for c in cells]
    kept_raw = sw.dedup(raw)
    assert len(kept_raw) == 1 and kept_raw[0]["fc_requested"] == 735.1e6
    fixed = sw.records_with_gain(cells, gain)
    assert [len(c) for c in fixed] == [1, 1]
    assert fixed[0][0]["pss_pow"] == raw[0][0]["pss_pow"] / 16.0 and fixed[1][0]["pss_pow"] == raw[1][0]["pss_pow"] / 256.0      # exact: powers of four
    for a, b in zip(fixed, raw):
        assert {k: v for k, v in a[0].items() if k != "pss_pow"} == {k: v for k, v in b[0].items() if k != "pss_pow"}
    kept = sw.dedup(fixed)
    assert len(kept) == 1 and kept[0]["fc_requested"] == 735.0e6 and kept[0]["pss_pow"] == pytest.approx(true_pow[0], rel=1e-6)
    with pytest.raises(ValueError):
        sw.records_with_gain(cells, gain[:1])
    assert sw.records_with_gain([[], []], gain) == [[], []]
