"""Inputs the PDSCH tests share (tests/test_pdsch_host.py, tests/test_pdsch_ref.py, tests/test_gpu_pdsch.py): crafted grids of 13
subframes (twelve whole ones and the control symbols of a thirteenth) with planted PCFICH, PDCCH and PDSCH at the smallest bandwidths
at which the rule can still go wrong (6, 15, 25 resource blocks), and the host twin's loader.

A crafted grid: per-port complex gains, a linear phase and an amplitude slope across the band and a slow drift over the rows; CRS of
every port on all its reference rows; load on every other element; the PCFICH of a CFI that changes from subframe to subframe; per
subframe one format 1A DCI (two in subframe 6) and the transport block behind it; noise 20 dB below a resource element.  The plan of
subframe g (PLAN): 0 every resource block (across PBCH, PSS and SSS); 1 one resource block at the band's edge; 2 a distributed
grant; 3 a grant whose PDSCH is silent; 4 mcs 27; 5 the centre blocks (across PSS and SSS); 6 two grants side by side; 7 .. 11 other
allocations; 12 a grant whose rows leave the grid.  rv = g mod 4, the TBS column g mod 2, the RNTIs cycle through SI, paging and RA.

For tests/test_pdsch_sizes_host.py and tests/test_gpu_pdsch_sizes.py: the same grids at 100, 75 and 50 resource blocks (WIDE_CASES), the
decoder's inputs at all 127 block sizes (size_blocks) and forced grants at the largest sizes on the 25 RB grid (large_forced)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import pcfich_cases as PC
import pcfich_ref as PR
import pdcch_cases as DC
import pdcch_ref as DR
import pdsch_ref as SR
from conftest import load_pkg

# (n_id_cell, CP type, ports, n_rb, PHICH resource, TDD m_i or None): every N_ID mod 6, 1 / 2 / 4 ports, both CP types, one TDD table
CASES = [
    (0, 1, 1, 6, 1, None), (503, 2, 2, 6, 3, None), (68, 1, 4, 6, 2, None),
    (141, 1, 2, 15, 1, None), (256, 2, 4, 15, 4, None), (329, 1, 1, 15, 3, None),
    (7, 1, 2, 25, 3, None), (329, 2, 4, 25, 1, None), (142, 1, 2, 25, 3, (0, 1, None, None, 1, 0, 1, None, None, 1)),
]
# the bandwidths at which a block's scrambling sequence needs every jump of the chunk number (bit 7 from 20 480 soft bits on) and an
# allocation crosses the 64th resource block: one grid each at 100, 75 and 50 resource blocks, numbered after CASES
WIDE_CASES = [(4, 1, 1, 100, 1, None), (2, 2, 4, 75, 3, None), (141, 1, 2, 50, 2, None)]
RNTIS = [0xFFFF, 0xFFFE, 17, 0xFFFF, 60, 0xFFFE, 1]
SNR_DB = 20.0
N_SF = 13
SILENT_SF, DISTRIBUTED_SF, MCS_SF, TWO_SF, ROWS_SF = 3, 2, 4, 6, 12


def case_id(case):
    return "id%d-cp%d-p%d-rb%d-r%d%s" % (case[:5] + ("-tdd" if case[5] else "",))


def case_no(case):
    """the case's number in the plan and the seeds: CASES first, WIDE_CASES after them"""
    return CASES.index(case) if case in CASES else len(CASES) + WIDE_CASES.index(case)


def pdcch_case(case):
    """the PDCCH tests' form of the case: normal PHICH duration"""
    return case[:4] + (1, case[4], case[5])


def tdd_of(case):
    return case[5] is not None


def pack_1a(f, n_rb, tdd):
    """the payload bits of format 1A from its fields, in the order sent (36.212 5.3.3.1.3), padded to the table's size"""
    L, S = f["n_prb"], f["rb_start"]
    riv = n_rb * (L - 1) + S if L - 1 <= n_rb // 2 else n_rb * (n_rb - L + 1) + (n_rb - 1 - S)
    out = []
    fields = [(1, 1), (f.get("distributed", 0), 1), (riv, (n_rb * (n_rb + 1) // 2 - 1).bit_length()), (f["mcs"], 5), (f.get("harq", 0), 4 if tdd else 3),
              (f.get("ndi", 0), 1), (f["rv"], 2), (f["tpc"], 2)] + ([(0, 2)] if tdd else [])
    for v, n in fields:
        out += [(v >> (n - 1 - i)) & 1 for i in range(n)]
    size = load_pkg().capi.dci_common_sizes(n_rb, tdd)[0]
    return out + [0] * (size - len(out))


def plan_of(case, g):
    """the grants of grid subframe g: [dict(rb_start, n_prb, mcs, rv, tpc, distributed, rnti, silent)]"""
    n_rb, c_no = case[3], case_no(case)
    rv, tpc = g % 4, g % 2
    rnti = RNTIS[(g + c_no) % len(RNTIS)]
    mk = lambda s, n, mcs, **kw: dict(dict(rb_start=s, n_prb=n, mcs=mcs, rv=rv, tpc=tpc, distributed=0, rnti=rnti, silent=False), **kw)
    mid = n_rb // 2 - 1
    if g == 0:
        return [mk(0, n_rb, {6: 9, 15: 20, 25: 26, 50: 26, 75: 24, 100: 26}[n_rb])]
    if g == 1:
        return [mk(n_rb - 1, 1, 0)]
    if g == DISTRIBUTED_SF:
        return [mk(1, 2, 3, distributed=1)]
    if g == SILENT_SF:
        return [mk(0, 3, 2, silent=True)]
    if g == MCS_SF:
        return [mk(1, 2, 27)]
    if g == 5:
        return [mk(mid, 3, 2)]
    if g == TWO_SF:
        return [mk(0, 2, 1), mk(2, n_rb - 2, {6: 6, 15: 12, 25: 17, 50: 20, 75: 22, 100: 25}[n_rb], rnti=RNTIS[(g + c_no + 1) % len(RNTIS)], rv=(rv + 1) % 4)]
    start = (3 * g + c_no) % (n_rb - 2)
    return [mk(start, 1 + (g + c_no) % min(4, n_rb - start), (2 * g + c_no) % 8)]


def grid_seed(case, seed=0):
    return 9000 + case_no(case) + 100 * seed


def channel_of(case, rng):
    """the grid's channel chan(port, row, columns), from the first twelve draws of the grid's generator"""
    n_rb, nc = case[3], 12 * case[3]
    gain = np.exp(2j * np.pi * rng.random(4)) * (0.7 + 0.6 * rng.random(4))
    tau = 0.2 + 0.5 * rng.random(4)

    def chan(p, row, cols):
        cols = np.asarray(cols)
        return gain[p] * np.exp(-2j * np.pi * tau[p] * (cols - nc / 2) / (128.0 * n_rb / 6)) * (1.0 + 0.3 * (cols / nc - 0.5)) * np.exp(2j * np.pi * 0.002 * row)
    return chan


@functools.lru_cache(maxsize=None)
def crafted(case, snr_db=SNR_DB, seed=0):
    """-> (tfg [12 subframes + 3 rows (4 at 6 RB)], cfi [13], planted: list of dict(g, slot, rnti, rb_start, n_prb, mcs, rv, tpc, tbs,
    bits (the transport block, or None where none is sent), distributed, silent))"""
    n_id, cp, ports, n_rb, res, mi = case
    pkg = load_pkg()
    synth, capi = pkg.synth, pkg.capi
    c_no = case_no(case)
    n, nc = PR.n_symb_of(cp), 12 * n_rb
    n_ofdm = 24 * n + (4 if n_rb <= 10 else 3)
    rng = np.random.default_rng(grid_seed(case, seed))
    chan = channel_of(case, rng)
    tdd = mi is not None
    size = capi.dci_common_sizes(n_rb, tdd)[0]
    mask = DC.dl_mask_of(pdcch_case(case))
    mis = DC.mi_of(pdcch_case(case))

    k = np.arange(nc)
    qpsk = lambda m: ((1 - 2.0 * rng.integers(0, 2, m)) + 1j * (1 - 2.0 * rng.integers(0, 2, m))) / np.sqrt(2.0)
    tfg = np.stack([qpsk(nc) * chan(0, r, k) for r in range(n_ofdm)])
    cfi = np.zeros(N_SF, np.int32)
    planted = []
    for g in range(N_SF):
        sf, row = g % 10, 2 * g * n
        cfi[g] = 2 + (g + n_id) % 2 if n_rb <= 10 else 1 + (g + n_id) % 3      # (6 resource blocks: fewer than three symbols hold no candidate)
        tfg[row:min(row + 4, n_ofdm)] = 0
        for l in range(2 * n):
            r, ls, slot = row + l, l % n, 2 * sf + l // n
            if r >= n_ofdm or not (ls in (0, n - 3) or (ls == 1 and ports == 4)):
                continue
            if ports >= 2:
                tfg[r, k % 3 == n_id % 3] = 0
            for p in ((0, 1) if ls != 1 else (2, 3)):
                if p < ports:
                    idx = (PR.shift_of(p, n_id, slot) + (3 if ls == n - 3 else 0)) % 6 + 6 * np.arange(2 * n_rb)
                    tfg[r, idx] = PR.rs_row(n_id, cp, n_rb, slot, ls) * chan(p, r, idx)
        cols = PR.columns(n_id, n_rb)
        x = synth._tx_diversity(synth.pcfich_symbols(n_id, sf, cfi[g]), ports)
        tfg[row, cols] = sum(x[p] * chan(p, row, cols) for p in range(ports))
        if not DR.is_read(g, n_ofdm, cp, n_rb, mask, 1, tdd):
            continue
        lay = DR.layout(n_id, cp, ports, n_rb, int(cfi[g]), 1, res, 1 if mis is None else mis[sf])
        cand = DR.candidates(lay["n_cce"])
        dcis = []
        for j, f in enumerate(plan_of(case, g)):
            free = [c for c in cand if all(c[2] + c[1] <= d["cce"] or c[2] >= d["cce"] + d["L"] for d in dcis)]
            if not free:
                break
            slot, L, cce = free[(g + c_no) % len(free)] if j == 0 else free[0]
            dcis.append(dict(rnti=f["rnti"], bits=np.array(pack_1a(f, n_rb, tdd)), L=L, cce=cce))
            tbs = capi.tbs_1a(f["mcs"], f["tpc"]) if f["mcs"] <= 26 else 0
            sent = not f["distributed"] and f["mcs"] <= 26 and SR.whole(g, n_ofdm, cp) and not (tdd and sf in (1, 6))
            bits = rng.integers(0, 2, tbs).astype(np.uint8) if sent else None
            planted.append(dict(f, g=g, slot=slot, tbs=tbs, bits=bits))
            if sent:
                SR.plant(tfg, g, n_id, cp, ports, n_rb, int(cfi[g]), dict(rnti=f["rnti"], rb_start=f["rb_start"], n_prb=f["n_prb"], rv=f["rv"], bits=bits), chan, tdd,
                         silent=f["silent"])
        DR.plant(tfg, g, n_id, cp, ports, n_rb, int(cfi[g]), 1, res, dcis, chan, rng=rng, mi=1 if mis is None else mis[sf])
    sigma = 10 ** (-snr_db / 20) / np.sqrt(2.0)
    noise = sigma * (rng.standard_normal(tfg.shape) + 1j * rng.standard_normal(tfg.shape))
    for p in planted:                        # a silent grant's elements stay exactly zero
        if p["silent"] and p["bits"] is not None:
            for l, cols, _ in synth.pdsch_region(n_id, n_rb, ports, cp == 1, p["g"] % 10, int(cfi[p["g"]]), dict(p, bits=p["bits"]), tdd):
                noise[2 * p["g"] * n + l, cols] = 0
    tfg += noise
    tfg.setflags(write=False)
    return tfg, cfi, planted


@functools.lru_cache(maxsize=None)
def reference(case):
    """(pdcch_ref.receive's dict, pdsch_ref.receive's blocks) on the case's grid with the planted CFI: computed once, shared"""
    tfg, cfi, _ = crafted(case)
    n_id, cp, ports, n_rb, res, mi = case
    pc = pdcch_case(case)
    pdc = DR.receive(tfg, n_id, cp, ports, n_rb, cfi, 1, res, DC.sizes_of(pc), DC.dl_mask_of(pc), 7, DC.mi_of(pc))
    return pdc, SR.receive(tfg, n_id, cp, ports, n_rb, pdc, 0, tdd_of(case), DC.dl_mask_of(pc), 1)


# ---------------------------------------------------------------- the host twin (tests/host/pdsch_host.cpp)
ROOT = PC.ROOT
TWIN_SRC = os.path.join(ROOT, "tests", "host", "pdsch_host.cpp")
TWIN_LIB = os.path.join(ROOT, "tests", "host", "libpdsch_host.so")
SAN = os.path.join(ROOT, "tests", "host", "pdsch_host_san")
_dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
_ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
_up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
_bp = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))


def stale(target):
    dep = [TWIN_SRC] + [os.path.join(PC.CSRC, h) for h in ("pdsch.h", "pdcch.h", "pcfich.h", "cell_meas.h", "tdd_config.h", "lte_device.h")] + [os.path.join(ROOT, "include", "lcs.h")]
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in dep)


def load_twin(capi):
    """pdsch.h compiled for the host (built where missing or older than its sources)"""
    if stale(TWIN_LIB):
        subprocess.check_call(PC.HIPCC + ["-O2", "-fPIC", "-shared", "-o", TWIN_LIB, TWIN_SRC])
    h = C.CDLL(TWIN_LIB)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    h.pdsch_host.argtypes = [dp] + [C.c_int] * 7 + [C.POINTER(C.c_uint32), C.c_int, C.c_int, C.POINTER(capi.PdcchInfo), C.POINTER(capi.PdschCfg), dp, C.c_int, dp,
                                                    C.POINTER(capi.PdschInfo)]
    h.pdsch_host.restype = None
    h.pdsch_host_turbo.argtypes = [dp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8), ip]
    h.pdsch_host_qpp.argtypes = [C.c_int, ip]
    h.pdsch_host_qpp.restype = None
    h.pdsch_host_perm.argtypes = [C.c_int, ip]
    h.pdsch_host_perm.restype = None
    h.pdsch_host_crc24a.argtypes = [C.POINTER(C.c_uint8), C.c_int]
    h.pdsch_host_elements.argtypes = [C.c_int] * 9 + [ip, C.c_int]
    h.pdsch_host_1a.argtypes = [C.c_uint64, C.c_int, C.c_int, ip]
    h.pdsch_host_1a.restype = None
    h.pdsch_host_derm.argtypes = [dp, C.c_int, C.c_int, C.c_int, C.c_int, dp]
    h.pdsch_host_derm.restype = None
    h.pdsch_host_scramble.argtypes = [C.c_uint32, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    h.pdsch_host_scramble.restype = None
    h.pdsch_host_c_init.argtypes = [C.c_int] * 3
    h.pdsch_host_c_init.restype = C.c_uint32
    return h


@functools.lru_cache(maxsize=None)
def jump_tables(n_rb):
    """[320]: the PDCCH's two tables, and the jumps by 160 2^b clocks, b < 8, behind them"""
    return np.ascontiguousarray(np.concatenate([PC.jump_tables(n_rb)] + [PC._jump(160 << b) for b in range(8)]).astype(np.uint32))


def make_cfg(capi, **kw):
    kw.setdefault("max_iter", 8)
    kw.setdefault("rnti_mask", 7)
    return capi.PdschCfg.make(**kw)


def twin_record(H, capi, case, tfg, pdc_rec, cfg=None, mask=None, want_soft=False):
    """the twin's record from the grid and a PDCCH record (the PDCCH twin's, or the device's)"""
    n_id, cp, ports, n_rb = case[:4]
    pc = pdcch_case(case)
    tfg = np.ascontiguousarray(tfg, np.complex128)
    cfg = make_cfg(capi) if cfg is None else cfg
    n_sf = PR.n_sf_of(tfg.shape[0], cp)
    stride = 2 * 12 * n_rb * 14
    llr = np.zeros((2 * n_sf, stride)) if want_soft else None
    d = np.zeros((2 * n_sf, 3, 2244)) if want_soft else None
    o = capi.PdschInfo()
    H.pdsch_host(_dp(tfg.view(np.float64)), tfg.shape[0], PR.n_symb_of(cp), n_rb, n_id, cp, ports, DC.dl_mask_of(pc) if mask is None else mask, _up(jump_tables(n_rb)),
                 1, 1 if tdd_of(case) else 0, C.byref(pdc_rec), C.byref(cfg), _dp(llr) if want_soft else None, stride, _dp(d) if want_soft else None, C.byref(o))
    return (o, llr, d) if want_soft else o


def pdcch_twin_record(capi, case, tfg, cfi):
    """the PDCCH twin's record of the grid: what the PDSCH twin reads its grants from"""
    return DC.twin_record(DC.load_twin(capi), capi, pdcch_case(case), tfg, cfi)


def twin_turbo(H, d, K, F=0, max_iter=8):
    d = np.ascontiguousarray(d, np.float64)
    bits, n_iter = np.zeros(K, np.uint8), C.c_int32(0)
    st = H.pdsch_host_turbo(_dp(d), K, F, max_iter, _bp(bits), C.byref(n_iter))
    return bits, n_iter.value, st


def assert_blocks_against_numpy(rec, blocks, what=""):
    """rec: capi.PdschInfo; blocks: pdsch_ref.receive's.  Every field of every block equal; a decoded block whose numpy posterior
    came within 1e-9 of zero (relative) is excused from n_iter, status and payload.  -> (blocks compared, blocks excused)"""
    assert rec.n_blocks == len(blocks), (what, rec.n_blocks, len(blocks))
    excused = 0
    for i, r in enumerate(blocks):
        b = rec.block[i]
        head = ("subframe", "slot", "rnti", "kind", "rb_start", "n_prb", "mcs", "rv", "tbs", "n_re", "K", "F")
        assert tuple(getattr(b, k) for k in head) == tuple(int(r[k]) for k in head), (what, i, [(k, getattr(b, k), r[k]) for k in head])
        if r["margin"] <= 1e-9:
            excused += 1
            continue
        assert (b.n_iter, b.status) == (r["n_iter"], r["status"]), (what, i, b.n_iter, b.status, r["n_iter"], r["status"])
        assert np.array_equal(np.ctypeslib.as_array(b.payload), r["payload"]), (what, i)
    return len(blocks), excused


# ---------------------------------------------------------------- every block size (tests/test_pdsch_sizes_host.py, tests/test_gpu_pdsch_sizes.py)
NOISY_K = (40, 48, 56, 2048, 2112, 2176, 2240)      # the ends of the table, every length of the last window, both sides of the second wave
SLOW_SIGMA = 1.05       # blocks of the three sizes that need the second wave, with noise enough for three iterations and more


def filler_step(K):
    """the largest F + 1 that segmentation into one block can leave at size K: the distance to the size below"""
    return 8 if K <= 512 else 16 if K <= 1024 else 32 if K <= 2048 else 64


def _noisy_block(rng, K, F, sigma):
    synth = load_pkg().synth
    a = rng.integers(0, 2, K - F - 24).astype(np.uint8)
    c = np.concatenate([np.zeros(F, np.uint8), a, synth.crc24a(a)])
    d = (1 - 2.0 * synth.turbo_encode(c)) + sigma * rng.standard_normal((3, K + 4))
    d[:2, :F] = 0
    d.setflags(write=False)
    return c, d


@functools.lru_cache(maxsize=None)
def size_blocks():
    """The decoder's inputs at all 127 block sizes, built as tests/test_pdsch_host.py's test_decoder_against_numpy builds its own: per
    K the first block of default_rng(10 K + F) for (F = 0, sigma = 0.85) and (F = filler_step - 1, sigma = 0.95); for K in NOISY_K the
    second block of the F = 0 generator at sigma = 3.0, which runs out of iterations, at max_iter 1 and 16; for the three sizes of
    the second wave the third block of that generator at SLOW_SIGMA.
    -> list of dict(K, F, sigma, max_iter, c (the encoded block), d [3][K + 4])"""
    out = []
    for K in load_pkg().synth.TURBO_K:
        for F, sigma in ((0, 0.85), (filler_step(K) - 1, 0.95)):
            rng = np.random.default_rng(10 * K + F)
            c, d = _noisy_block(rng, K, F, sigma)
            out.append(dict(K=K, F=F, sigma=sigma, max_iter=8, c=c, d=d))
            if F == 0 and K in NOISY_K:
                c, d = _noisy_block(rng, K, 0, 3.0)
                out += [dict(K=K, F=0, sigma=3.0, max_iter=it, c=c, d=d) for it in (1, 16)]
                if K > 2048:
                    c, d = _noisy_block(rng, K, 0, SLOW_SIGMA)
                    out.append(dict(K=K, F=0, sigma=SLOW_SIGMA, max_iter=8, c=c, d=d))
    return out


@functools.lru_cache(maxsize=None)
def size_blocks_twin():
    """the host twin's (bits, n_iter, status) of every block of size_blocks(): computed once, shared"""
    H = load_twin(load_pkg().capi)
    return [twin_turbo(H, b["d"], b["K"], b["F"], b["max_iter"]) for b in size_blocks()]


# Forced grants at the sizes the crafted grids do not reach, on a copy of the 25 RB grid CASES[6] (CFI 3, 1, 2, 3 in subframes 1 .. 4 and
# 2, 3, 1 in 6 .. 8: 240, 288 or 264 soft bits per resource block): (call, subframe, rb_start, n_prb, K, F, rv, rnti, noise in dB below a
# resource element).  Both blocks of the second wave with and without fillers, the wave's boundary from both sides, the first sizes
# of the 32 and 16 steps with their largest F, and a last window of 24 steps with F = 7; every rv; G < N (punctured) in the three
# blocks that share or nearly fill a subframe and in the smallest, G > N (wrapped) in the others.  The noise is what makes the
# blocks above K = 1056 take two iterations and the first block of subframe 3 three.
LARGE_PLAN = [
    (0, 1, 0, 25, 2240, 63, 2, 0xFFFF, 5.0), (0, 3, 0, 13, 2240, 0, 0, 0xFFFE, 7.0), (0, 3, 13, 12, 2176, 20, 0, 17, 7.0), (0, 2, 0, 25, 2112, 55, 3, 61, 5.0),
    (1, 8, 0, 25, 2048, 0, 1, 0xFFFF, 5.0), (1, 6, 0, 13, 1056, 31, 1, 0xFFFE, 5.0), (1, 6, 13, 7, 528, 15, 3, 60, 5.0), (1, 7, 20, 5, 472, 7, 2, 61, 5.0),
]


@functools.lru_cache(maxsize=None)
def large_forced():
    """-> (case, tfg: the case's grid with LARGE_PLAN's blocks planted by pdsch_ref.plant and noise on their elements, calls: per call
    the list of forced grants (subframe, rnti, rb_start, n_prb, tbs, rv), planted: per call the transport blocks in the same order)"""
    case = CASES[6]
    n_id, cp, ports, n_rb, _, mi = case
    base, cfi, _ = crafted(case)
    tfg = np.array(base)
    chan = channel_of(case, np.random.default_rng(grid_seed(case)))
    rng = np.random.default_rng(9500)
    n = PR.n_symb_of(cp)
    calls, planted = [[], []], [[], []]
    for call, g, start, n_prb, K, F, rv, rnti, snr_db in LARGE_PLAN:
        tbs = K - F - 24
        assert SR.block_size(tbs) == (K, F)
        bits = rng.integers(0, 2, tbs).astype(np.uint8)
        SR.plant(tfg, g, n_id, cp, ports, n_rb, int(cfi[g]), dict(rnti=rnti, rb_start=start, n_prb=n_prb, rv=rv, bits=bits), chan, mi is not None)
        el = SR.elements(n_id, cp, ports, n_rb, g % 10, DR.n_ctrl_of(int(cfi[g]), n_rb), start, n_prb, mi is not None)
        ls, ks = 2 * g * n + np.array([l for l, _ in el]), np.array([k for _, k in el])
        sigma = 10 ** (-snr_db / 20) / np.sqrt(2.0)
        tfg[ls, ks] += sigma * (rng.standard_normal(len(el)) + 1j * rng.standard_normal(len(el)))
        calls[call].append((g, rnti, start, n_prb, tbs, rv))
        planted[call].append(bits)
    tfg.setflags(write=False)
    return case, tfg, calls, planted


@functools.lru_cache(maxsize=None)
def large_forced_reference(call):
    """pdsch_ref.receive's blocks of one call of large_forced(): computed once, shared"""
    case, tfg, calls, _ = large_forced()
    n_id, cp, ports, n_rb = case[:4]
    return SR.receive(tfg, n_id, cp, ports, n_rb, reference(case)[0], forced=calls[call])


# ---------------------------------------------------------------- captures with the generator's PCFICH, PDCCH and PDSCH in them
CAP_SHAPES = [(1, 6, 1, 2), (2, 15, 1, 2)]      # (R, n_rb, CP type, ports)
SIB1 = dict(plmns=[("262", "01", False), ("262", "02", True)], tac=0x1234, cell_id=0xABCDE12, barred=False, intra_freq=True, csg=False, csg_id=None,
            q_rx_lev_min=-60, q_rx_lev_min_offset=None, p_max=23, band=3, sched=[(16, [3]), (32, [5, 6])], tdd=None, si_window=10, value_tag=7)


def capture_grants(n_rb):
    """(frame, subframe) -> the grant of that subframe: SIB1 (rv by the frame) in subframe 5, paging or a random-access response in
    the others; allocations that stay inside the band and move with the subframe"""
    synth = load_pkg().synth
    capi = load_pkg().capi
    sib = synth.sib1_message(SIB1)

    def grants(frame, sf):
        if sf == 5:
            mcs = next(m for m in range(27) if capi.tbs_1a(m, 0) >= len(sib))
            tbs = capi.tbs_1a(mcs, 0)
            bits = np.concatenate([sib, np.zeros(tbs - len(sib), np.uint8)])
            return [dict(rnti=0xFFFF, rb_start=0, n_prb=min(n_rb, 6), mcs=mcs, tpc=0, rv=(frame * 2) % 4, bits=bits)]
        mcs, tpc = (sf + frame) % 6, sf & 1
        bits = np.random.default_rng(1000 * frame + sf).integers(0, 2, capi.tbs_1a(mcs, tpc)).astype(np.uint8)
        start = (2 * sf + frame) % (n_rb - 3)
        return [dict(rnti=0xFFFE if sf % 2 == 0 else 1 + (3 * sf) % 60, rb_start=start, n_prb=3, mcs=mcs, tpc=tpc, rv=sf % 4, bits=bits)]
    return grants


@functools.lru_cache(maxsize=None)
def pdsch_capture(R, n_rb, cp, ports, snr_db=10.0):
    """synth.make_wideband_cell: one cell of n_rb resource blocks at 1.92e6 R on the capture's centre, three frames in noise 10 dB
    below a resource element, with a format 1A DCI from CCE 0 and its transport block in every subframe
    -> (complex64 samples, frame_start of the cell's frame 1 in them)"""
    pkg = load_pkg()
    grants = capture_grants(n_rb)
    n_id = DC.CAP_ID[1] + 3 * DC.CAP_ID[0]

    def dcis(frame, sf):
        n_cce = pkg.synth.pdcch_layout(n_id, n_rb, ports, cp == 1, DC.capture_cfi(frame, sf))[1]
        return [dict(rnti=g["rnti"], bits=pack_1a(g, n_rb, False), L=4, cce=0) for g in grants(frame, sf)] if n_cce >= 4 else []

    def blocks(frame, sf):
        n_cce = pkg.synth.pdcch_layout(n_id, n_rb, ports, cp == 1, DC.capture_cfi(frame, sf))[1]
        return grants(frame, sf) if n_cce >= 4 else []
    cell = dict(n_id_1=DC.CAP_ID[0], n_id_2=DC.CAP_ID[1], cp_normal=cp == 1, n_ports=ports, f_off=0.0, t0=DC.CAP_T0, sfn0=8, n_rb_dl=n_rb,
                cfi=DC.capture_cfi, pdcch=dcis, pdsch=blocks)
    x, _, _ = pkg.synth.make_wideband_cell(60 + R + cp + ports, DC.CAP_FC, R, [(DC.CAP_FC, R, n_rb, cell)], snr_db=snr_db, n_in=3 * 19200 * R)
    x.setflags(write=False)
    return x, (19200.0 - DC.CAP_T0) * R
