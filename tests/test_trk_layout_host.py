"""lte-cell-scanner_amd/csrc/trk_layout.h on the CPU: the one description of how the tracker's host side cuts its buffers into
arrays (block workspace, staging block, statistics, cutter) and the integer rules of the continuous form, through the host twin
tests/host/trk_layout_host.cpp, which includes nothing else.

Domain: every capacity the growth rule gives for n_cells in 1..64 and n_sym in SYMS (the cells, the symbols with their head
room), and under each of them every block shape of the same set that fits.  The references are the expressions the host code held
before the layout had a module, quoted below as literals.  The same source is built once more as a stand-alone program with
-fsanitize=address,undefined and walks the domain by itself: nothing is loaded into Python under a sanitizer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "trk_layout_host.cpp")
LIB = os.path.join(ROOT, "tests", "host", "libtrk_layout_host.so")
SAN = os.path.join(ROOT, "tests", "host", "trk_layout_host_san")
DEPS = [SRC, os.path.join(ROOT, "lte-cell-scanner_amd", "csrc", "trk_layout.h"), os.path.join(ROOT, "include", "lcs.h")]
HIPCC = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include")]
SYMS = [1, 6, 7, 119, 120, 121, 139, 140, 141, 479, 480, 500, 839, 840, 980, 1260, 2000]
CELLS = range(1, 65)
CELL_BYTES, MEAS = 40, 9                 # sizeof(lcs_track_cell), LCS_TRK_MEAS
N_PAIRS = sum(CELLS) * sum(sum(n <= m + m // 8 for n in SYMS) for m in SYMS)      # (capacity, block shape that fits) pairs of the domain
_u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
_i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))


def _stale(target):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in DEPS)


class Twin:
    def __init__(self):
        if _stale(LIB):
            subprocess.check_call(HIPCC + ["-O2", "-fPIC", "-shared", "-o", LIB, SRC])
        self.h = h = C.CDLL(LIB)
        h.trk_host_stream_step.argtypes = [C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.POINTER(C.c_longlong)]
        h.trk_host_mib_first.argtypes = [C.c_longlong, C.c_longlong, C.c_int]
        na, nb = C.c_int(0), C.c_int(0)
        buf, elem, align = (np.zeros(256, np.int32) for _ in range(3))
        h.trk_host_table(C.byref(na), C.byref(nb), _i32(buf), _i32(elem), _i32(align))
        self.n_arr, self.n_buf = na.value, nb.value
        self.buf, self.elem, self.align = buf[:self.n_arr], elem[:self.n_arr].astype(np.uint64), align[:self.n_arr].astype(np.uint64)

    def _out(self, n):
        return np.zeros((n, self.n_arr), np.uint64), np.zeros((n, self.n_arr), np.uint64), np.zeros((n, self.n_buf), np.uint64)

    def layouts(self, shapes):
        """(off [n][arrays] bytes, end [n][arrays] bytes, total [n][buffers] bytes) of n (cells, symbols) shapes"""
        c, s = np.ascontiguousarray([x[0] for x in shapes], np.int32), np.ascontiguousarray([x[1] for x in shapes], np.int32)
        off, ln, tot = self._out(len(shapes))
        self.h.trk_host_layouts(len(shapes), _i32(c), _i32(s), _u64(off), _u64(ln), _u64(tot))
        return off, off + ln * self.elem, tot

    def cut_layouts(self, caps):
        c, n = np.ascontiguousarray([x[0] for x in caps], np.uint64), np.ascontiguousarray([x[1] for x in caps], np.uint64)
        off, ln, tot = self._out(len(caps))
        self.h.trk_host_cut_layouts(len(caps), _u64(c), _u64(n), _u64(off), _u64(ln), _u64(tot))
        return off, off + ln * self.elem, tot, ln


@pytest.fixture(scope="module")
def H():
    return Twin()


# ---- the buffers and arrays by the names trk_layout.h gives them, in its order
BUFS = ["td", "meta", "cells", "syms", "rs", "idx", "raw", "fmeta", "ce", "pw", "small", "stage", "acfd", "actd", "sync", "syncce", "cut_hit", "cut_meta"]
ARRS = ["td", "fo", "ft", "late", "bpo", "cells", "syms", "rs", "shift", "idx", "nrs", "raw", "filt", "fm", "meas", "ce", "pw", "nmeas", "upto", "mibok",
        "mibbits", "mibfirst", "h_fo", "h_ft", "h_late", "h_cells_up", "h_meas", "h_bits", "h_nmeas", "h_upto", "h_mibok", "h_cells_down", "acfd", "actd",
        "sync", "syncce", "cut_hit", "cut_n", "cut_flags", "cut_pos", "cut_late", "cut_cells"]
A = {n: i for i, n in enumerate(ARRS)}
B = {n: i for i, n in enumerate(BUFS)}
BLOCK, STAGE, STATS, CUT = range(0, 11), [11], range(12, 16), range(16, 18)
WORDS64 = ["mibbits", "h_bits", "cut_pos"]            # the 64-bit integer arrays


def parent_block_bytes(cc, cs):
    """trk_ensure_ws before the layout had a module, for the capacity (cc cells, cs symbols): elements x element size"""
    rs_cap, n_off = cs // 3 + 4, max(0, cs // 120 - 3)
    N, C4 = cc * cs, cc * 4
    return dict(td=N * 128 * 16, meta=N * 4 * 8, cells=cc * CELL_BYTES, syms=N * 72 * 16, rs=cc * 140 * 28 * 8, idx=C4 * (rs_cap + 1) * 4,
                raw=C4 * rs_cap * 24 * 16, fmeta=C4 * rs_cap * (4 + MEAS) * 8, ce=C4 * cs * 72 * 16, pw=C4 * cs * 4 * 8,
                small=(C4 * 2 + cc * (n_off + 1) * 3 + cc) * 4)


def parent_stats_bytes(cc, cs):
    """lcs_track_stats, likewise"""
    C4c, rsc, hfc = cc * 4, cs // 3 + 4, cs // 60 + 2
    return dict(acfd=C4c * rsc * 12 * 16, actd=C4c * rsc * 72 * 16, sync=cc * hfc * 4 * 8, syncce=cc * hfc * 72 * 16)


def parent_cut_bytes(capC, capN):
    """lcs_track_cut, likewise"""
    return dict(cut_hit=(capN + 4 * capC + 2) * 4, cut_meta=(capN + 5 * capC) * 8)


def parent_stage_bytes(n_cells, n_sym):
    """trk_block's reservation for its staging block: up_bytes + down_bytes + 64, for the block's own shape"""
    rs_cap, n_off = n_sym // 3 + 4, max(0, n_sym // 120 - 3)
    N, C4 = n_cells * n_sym, n_cells * 4
    n_meas_d, n_small, n_bits = C4 * rs_cap * MEAS, C4 * 2 + n_cells * n_off, n_cells * n_off + 1
    up_bytes = 8 * 3 * N + CELL_BYTES * n_cells
    down_bytes = 8 * n_meas_d + 8 * n_bits + 4 * n_small + CELL_BYTES * n_cells
    return up_bytes + down_bytes + 64


def test_table_names_and_element_alignment(H):
    assert (H.n_arr, H.n_buf) == (len(ARRS), len(BUFS))
    # arrays of a buffer follow each other in the table.  That every buffer STARTS at least 16-byte aligned rests on the allocators
    # (hipMalloc: 256 bytes, malloc: 16) and cannot be checked without them; what is checked here is that no array asks for more
    assert list(H.buf) == sorted(H.buf) and set(H.align) <= {4, 8, 16}
    for name, a in A.items():
        assert H.align[a] >= {16: 16, 8: 8, CELL_BYTES: 8, 4: 4}[int(H.elem[a])], name
    assert all(H.elem[A[n]] == 8 and H.align[A[n]] >= 8 for n in WORDS64)
    assert all(H.elem[A[n]] == 16 and H.align[A[n]] == 16 for n in ("td", "syms", "raw", "filt", "ce", "acfd", "actd", "syncce"))
    assert H.align[A["h_meas"]] == 16                                  # the staging block's down part
    assert H.elem[A["cells"]] == H.elem[A["h_cells_up"]] == H.elem[A["h_cells_down"]] == CELL_BYTES


def test_derived_capacities_and_growth_rule(H):
    out = np.zeros(3, np.int32)
    for n in list(range(0, 2600)):
        H.h.trk_host_caps(n, _i32(out))
        assert list(out) == [n // 3 + 4, max(0, n // 120 - 3), n // 60 + 2], n
    rng = np.random.default_rng(3)
    for _ in range(4000):
        cc, cs = int(rng.integers(0, 65)), int(rng.choice([0] + [n + n // 8 for n in SYMS]))
        c, n = int(rng.integers(1, 65)), int(rng.choice(SYMS))
        H.h.trk_host_grow(cc, cs, c, n, _i32(out))
        assert list(out) == [int(c <= cc and n <= cs), max(c, cc), max(n + n // 8, cs)]      # the parent's: cells max, symbols max(n_sym + n_sym / 8, cap)


def _disjoint_aligned(H, off, end, tot, bufs, what):
    """per layout: the arrays of `bufs` lie behind each other on their alignment and end within the buffer's total"""
    for b in bufs:
        arrs = [a for a in range(H.n_arr) if H.buf[a] == b]
        assert arrs, b
        last = np.zeros(off.shape[0], np.uint64)
        for a in arrs:                       # table order = address order: no array starts before the one in front of it ends
            assert not (off[:, a] % H.align[a]).any(), (what, ARRS[a])
            assert (off[:, a] >= last).all(), (what, ARRS[a])
            last = end[:, a]
        assert (last <= tot[:, b]).all(), (what, BUFS[b])


def test_every_block_shape_lies_inside_every_capacity_that_holds_it(H):
    shapes = [(c, n) for c in CELLS for n in SYMS]
    caps = [(c, n + n // 8) for c in CELLS for n in SYMS]            # what the growth rule makes of a first call; later calls only take maxima of these
    off, end, tot = H.layouts(shapes)
    c_off, c_end, c_tot = H.layouts(caps)
    _disjoint_aligned(H, off, end, tot, list(BLOCK) + list(STAGE) + list(STATS), "block shapes")
    _disjoint_aligned(H, c_off, c_end, c_tot, list(BLOCK) + list(STATS), "capacities")
    # no buffer is larger than the parent's expression for it
    for i, (cc, cs) in enumerate(caps):
        want = dict(parent_block_bytes(cc, cs), **parent_stats_bytes(cc, cs))
        for name, v in want.items():
            assert c_tot[i, B[name]] <= v, (cc, cs, name, int(c_tot[i, B[name]]), v)
    # the staging block is reserved for the block's own shape
    for i, (c, n) in enumerate(shapes):
        assert tot[i, B["stage"]] <= parent_stage_bytes(c, n), (c, n)
    # every array of every block shape ends within the buffer as the capacity sizes it -- all (capacity, shape that fits) pairs
    sh = np.array(shapes)
    dev = np.array([a for a in range(H.n_arr) if H.buf[a] in BLOCK or H.buf[a] in STATS])
    n_pairs = 0
    for i, (cc, cs) in enumerate(caps):
        fit = (sh[:, 0] <= cc) & (sh[:, 1] <= cs)
        assert fit[shapes.index((cc, SYMS[i % len(SYMS)]))]
        assert (end[fit][:, dev] <= c_tot[i, H.buf[dev]][None, :]).all(), (cc, cs)
        n_pairs += int(fit.sum())
    assert n_pairs == N_PAIRS
    # what the one-copy transfers of a block rely on: fo, ft, late adjacent (device and staging), nmeas, upto, mibok likewise
    for a, b, c3 in (("fo", "ft", "late"), ("h_fo", "h_ft", "h_late"), ("nmeas", "upto", "mibok"), ("h_nmeas", "h_upto", "h_mibok")):
        assert np.array_equal(end[:, A[a]], off[:, A[b]]) and np.array_equal(end[:, A[b]], off[:, A[c3]]), a


def test_cutter_is_laid_out_by_its_capacity(H):
    caps = sorted({(cc, c * n) for cc in CELLS for c in range(1, cc + 1) for n in SYMS if c * n >= cc})
    off, end, tot, ln = H.cut_layouts(caps)
    _disjoint_aligned(H, off, end, tot, CUT, "cutter")
    cc, cn = np.array([x[0] for x in caps], np.uint64), np.array([x[1] for x in caps], np.uint64)
    assert np.array_equal(ln[:, A["cut_hit"]], cn) and np.array_equal(ln[:, A["cut_late"]], cn) and np.array_equal(ln[:, A["cut_cells"]], 5 * cc)
    assert all(np.array_equal(ln[:, A[k]], cc) for k in ("cut_n", "cut_flags", "cut_pos"))
    for i, (capC, capN) in enumerate(caps):
        for name, v in parent_cut_bytes(capC, capN).items():
            assert tot[i, B[name]] <= v, (capC, capN, name)


@pytest.mark.parametrize("F", [140, 120])
def test_stream_rules_on_random_cut_sequences(H, F):
    rng = np.random.default_rng(F)
    out = (C.c_longlong * 6)()
    for seq in range(200):
        n_seen = tail = 0
        for _ in range(int(rng.integers(1, 41))):
            n_sym = int(rng.integers(1, 1501))
            H.h.trk_host_stream_step(n_seen, tail, n_sym, F, out)
            n_tail, L, n_after, T_next, keep_from, n_keep = list(out)
            assert T_next % F == 0 and T_next >= tail, (seq, n_seen, n_sym)
            if n_after < 3 * F:
                assert n_keep == n_after
            else:
                assert 3 * F <= n_keep < 4 * F
            assert keep_from + n_keep == L
            # the parent's formulas (lcs_track_stream_block).  Its division truncates where this one floors: below 3 F both give 0 under the max
            p_T_next = max(0, (n_after - 3 * F) // F * F)
            assert (n_tail, L, n_after, T_next, keep_from, n_keep) == (n_seen - tail, n_seen - tail + n_sym, n_seen + n_sym, p_T_next, p_T_next - tail, n_seen + n_sym - p_T_next)
            mib_next = tail // F + int(rng.integers(-2, 6))
            assert H.h.trk_host_mib_first(max(0, mib_next), tail, F) == max(0, max(0, mib_next) - tail // F)
            n_seen, tail = n_after, T_next


def test_stand_alone_program_under_address_and_undefined_sanitizers():
    """the same source with its own main walks the same domain: a clean exit"""
    if _stale(SAN):
        subprocess.check_call(HIPCC + ["-O1", "-g", "-DTRK_LAYOUT_HOST_MAIN", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                                       "-fno-sanitize-recover=undefined", "-o", SAN, SRC])
    r = subprocess.run([SAN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout, r.stderr[-2000:])
    assert r.stdout.split() == [str(N_PAIRS), "pairs,", "0", "failures"]
