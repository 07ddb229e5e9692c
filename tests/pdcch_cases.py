"""Inputs the PDCCH tests share (tests/test_pdcch_host.py, tests/test_pdcch_ref.py, tests/test_gpu_pdcch.py): crafted grids of 13
subframes with planted PCFICH and PDCCH at the smallest bandwidths at which the rule can still go wrong (6, 15, 25 resource blocks),
and the host twin's loader.

A crafted grid: per-port complex gains, a linear phase and an amplitude slope across the band and a slow drift over the rows; CRS
of every port on symbols 0 (and 1 with four ports) of every subframe; the PCFICH of a CFI that changes from subframe to subframe;
the PDCCH of pdcch_ref.plant; noise 20 dB below a resource element.  Plan per subframe g of case number c: one DCI in candidate slot
(g + c) mod 6 with size index ((g + c) // 6) mod 2 (the first slot that exists where that one does not), a second one in a slot that
does not overlap the first where there is one; RNTIs cycle through SI, paging, three RA-RNTIs and 0x1234 (outside the set: decoded,
not accepted).  Subframe 7 carries no PDCCH (noise alone); subframe 9 has every unused CCE filled with random bits (fill = 1)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import pcfich_cases as PC
import pcfich_ref as PR
import pdcch_ref as DR
from conftest import load_pkg

# (n_id_cell, CP type, ports, n_rb, PHICH duration, PHICH resource, TDD m_i or None): every N_ID mod 6, 1 / 2 / 4 ports, both CP
# types, every Ng, both durations, an id beyond N_REG (503 at 6 RB: N_REG <= 58), and two TDD tables (configurations 1 and 0; the second with the extended duration)
CASES = [
    (0, 1, 1, 6, 1, 1, None), (503, 2, 2, 6, 1, 3, None), (68, 1, 4, 6, 2, 2, None), (7, 2, 1, 6, 2, 4, None),
    (141, 1, 2, 15, 1, 1, None), (256, 2, 4, 15, 1, 4, None), (329, 1, 1, 15, 2, 3, None), (14, 2, 2, 15, 2, 2, None),
    (7, 1, 2, 25, 1, 3, None), (329, 2, 4, 25, 2, 1, None), (256, 1, 4, 25, 1, 2, None), (503, 1, 1, 25, 1, 4, None),
    (141, 1, 2, 25, 1, 3, (0, 1, None, None, 1, 0, 1, None, None, 1)), (68, 1, 2, 15, 2, 3, (2, 1, None, None, None, 2, 1, None, None, None)),
]
RNTIS = [0xFFFF, 0xFFFE, 17, 0xFFFF, 60, 0x1234, 1]
SILENT_SF, FILL_SF = 7, 9
SNR_DB = 20.0
N_SF = 13


def case_id(case):
    return "id%d-cp%d-p%d-rb%d-d%d-r%d%s" % (case[:6] + ("-tdd" if case[6] else "",))


def sizes_of(case):
    return load_pkg().capi.dci_common_sizes(case[3], case[6] is not None)


def mi_of(case):
    return None if case[6] is None else [0 if m is None else m for m in case[6]]


def dl_mask_of(case):
    return 0x3FF if case[6] is None else sum(1 << i for i, m in enumerate(case[6]) if m is not None)


def planted_cfi(case, g):
    """a CFI that changes with the subframe, among those the PHICH duration allows"""
    n_rb, dur = case[3], case[4]
    allowed = [c for c in (1, 2, 3) if not (dur == 2 and DR.n_ctrl_of(c, n_rb) < 3)]
    return allowed[(g + case[0]) % len(allowed)]


@functools.lru_cache(maxsize=None)
def crafted(case, snr_db=SNR_DB, fill=None, seed=0):
    """-> (tfg [12 subframes + 3 rows (4 at 6 RB)], cfi [13], planted: list of dict(g, slot, i, L, cce, bits (int), rnti)).
    The tests take the defaults; tools/pdcch_accuracy.py asks for other noise, a fill in every subframe and further seeds."""
    n_id, cp, ports, n_rb, dur, res, _ = case
    c_no = CASES.index(case)
    synth = load_pkg().synth
    n, nc = PR.n_symb_of(cp), 12 * n_rb
    n_ofdm = 24 * n + (4 if n_rb <= 10 else 3)
    rng = np.random.default_rng(7000 + c_no + 100 * seed)
    gain = np.exp(2j * np.pi * rng.random(4)) * (0.7 + 0.6 * rng.random(4))
    tau = 0.2 + 0.5 * rng.random(4)
    sizes, mi, mask = sizes_of(case), mi_of(case), dl_mask_of(case)

    def chan(p, row, cols):
        cols = np.asarray(cols)
        return gain[p] * np.exp(-2j * np.pi * tau[p] * (cols - nc / 2) / (128.0 * n_rb / 6)) * (1.0 + 0.3 * (cols / nc - 0.5)) * np.exp(2j * np.pi * 0.002 * row)

    k = np.arange(nc)
    qpsk = lambda m: ((1 - 2.0 * rng.integers(0, 2, m)) + 1j * (1 - 2.0 * rng.integers(0, 2, m))) / np.sqrt(2.0)
    tfg = np.stack([qpsk(nc) * chan(0, r, k) for r in range(n_ofdm)])
    cfi = np.zeros(N_SF, np.int32)
    planted = []
    for g in range(N_SF):
        sf, row = g % 10, 2 * g * n
        cfi[g] = planted_cfi(case, g)
        tfg[row:min(row + 4, n_ofdm)] = 0
        for p in range(ports):
            r = row + (0 if p < 2 else 1)
            if r < n_ofdm:
                idx = PR.shift_of(p, n_id, 2 * sf) + 6 * np.arange(2 * n_rb)
                tfg[r, idx] = PR.rs_row(n_id, cp, n_rb, 2 * sf, 0 if p < 2 else 1) * chan(p, r, idx)
        cols = PR.columns(n_id, n_rb)
        x = synth._tx_diversity(synth.pcfich_symbols(n_id, sf, cfi[g]), ports)
        tfg[row, cols] = sum(x[p] * chan(p, row, cols) for p in range(ports))
        if not DR.is_read(g, n_ofdm, cp, n_rb, mask, dur, mi is not None):
            continue
        lay = DR.layout(n_id, cp, ports, n_rb, int(cfi[g]), dur, res, 1 if mi is None else mi[sf])
        cand = DR.candidates(lay["n_cce"])
        dcis = []
        if g != SILENT_SF and cand:
            want = (g + c_no) % 6
            first = next((c for c in cand if c[0] == want), cand[0])
            picks = [(first, ((g + c_no) // 6) % 2)]
            other = next((c for c in cand if c[2] + c[1] <= first[2] or c[2] >= first[2] + first[1]), None)
            if other is not None:
                picks.append((other, 1 - picks[0][1]))
            for j, ((slot, L, cce), i) in enumerate(picks):
                bits = rng.integers(0, 2, sizes[i])
                d = dict(g=g, slot=slot, i=i, L=L, cce=cce, bits=bits, rnti=RNTIS[(3 * g + j + c_no) % len(RNTIS)])
                dcis.append(d)
                planted.append(dict(d, bits=sum(int(b) << t for t, b in enumerate(bits))))
        DR.plant(tfg, g, n_id, cp, ports, n_rb, int(cfi[g]), dur, res, dcis, chan, fill=(1.0 if g == FILL_SF else 0.0) if fill is None else fill, rng=rng, mi=1 if mi is None else mi[sf])
    sigma = 10 ** (-snr_db / 20) / np.sqrt(2.0)
    tfg += sigma * (rng.standard_normal(tfg.shape) + 1j * rng.standard_normal(tfg.shape))
    tfg.setflags(write=False)
    return tfg, cfi, planted


@functools.lru_cache(maxsize=None)
def reference(case):
    """pdcch_ref.receive on the case's grid with the planted CFI: computed once, shared by the tests"""
    tfg, cfi, _ = crafted(case)
    n_id, cp, ports, n_rb, dur, res, _ = case
    return DR.receive(tfg, n_id, cp, ports, n_rb, cfi, dur, res, sizes_of(case), dl_mask_of(case), 7, mi_of(case))


# ---------------------------------------------------------------- the host twin (tests/host/pdcch_host.cpp)
ROOT = PC.ROOT
TWIN_SRC = os.path.join(ROOT, "tests", "host", "pdcch_host.cpp")
TWIN_LIB = os.path.join(ROOT, "tests", "host", "libpdcch_host.so")
SAN = os.path.join(ROOT, "tests", "host", "pdcch_host_san")
_dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
_ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
_up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))


def stale(target):
    dep = [TWIN_SRC] + [os.path.join(PC.CSRC, h) for h in ("pdcch.h", "pcfich.h", "cell_meas.h", "tdd_config.h", "lte_device.h")] + [os.path.join(ROOT, "include", "lcs.h")]
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in dep)


def load_twin(capi):
    """pdcch.h and the length-n decoder compiled for the host (built where missing or older than its sources)"""
    if stale(TWIN_LIB):
        subprocess.check_call(PC.HIPCC + ["-O2", "-fPIC", "-shared", "-o", TWIN_LIB, TWIN_SRC])
    h = C.CDLL(TWIN_LIB)
    ip = C.POINTER(C.c_int32)
    h.pdcch_host.argtypes = [C.POINTER(C.c_double)] + [C.c_int] * 7 + [C.POINTER(C.c_uint32), C.POINTER(capi.PdcchCfg), ip, C.POINTER(C.c_double), C.POINTER(capi.PdcchInfo)]
    h.pdcch_host.restype = None
    h.pdcch_host_map.argtypes = [C.c_int] * 8 + [ip, ip, ip, ip, ip, ip, C.c_int, ip]
    h.pdcch_host_interleave.argtypes = [C.c_int, ip]
    h.pdcch_host_interleave.restype = None
    h.pdcch_host_derm.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int16)]
    h.pdcch_host_scramble.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    h.pdcch_host_scramble.restype = None
    h.pdcch_host_slot.argtypes = [C.c_int, C.c_int, ip, ip]
    h.pdcch_host_rnti_x.argtypes = [C.c_uint64, C.c_int]
    h.pdcch_host_rnti_x.restype = C.c_uint32
    h.pdcch_host_vit.argtypes = [C.POINTER(C.c_double), C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    return h


def twin_map(H, n_rb, ports, cp, n_id, dur, res, mi, cfi):
    """-> None where refused, else dict(n_reg, n_cce, re [576], pcfich / phich / order as lists of (k', l'))"""
    cap = 1400
    n_reg, n_cce, lists = C.c_int32(), C.c_int32(), np.zeros(3, np.int32)
    re, a, b, o = np.zeros(576, np.int32), np.zeros(4, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    ok = H.pdcch_host_map(n_rb, ports, cp, n_id, dur, res, mi, cfi, C.byref(n_reg), C.byref(n_cce), _ip(re), _ip(a), _ip(b), _ip(o), cap, _ip(lists))
    if not ok:
        assert n_reg.value == 0 and n_cce.value == 0 and (re == -1).all()
        return None
    un = lambda v, n: [(int(x) >> 2, int(x) & 3) for x in v[:n]]
    return dict(n_reg=n_reg.value, n_cce=n_cce.value, re=re, pcfich=un(a, lists[0]), phich=un(b, lists[1]), order=un(o, lists[2]))


def make_cfg(capi, case, **kw):
    return capi.PdcchCfg.make(sizes_of(case), phich_duration=case[4], phich_resource=case[5], phich_mi=case[6], **kw)


def twin_record(H, capi, case, tfg, cfi, cfg=None, mask=None, want_llr=False):
    n_id, cp, ports, n_rb = case[:4]
    tfg = np.ascontiguousarray(tfg, np.complex128)
    jump = PC.jump_tables(n_rb)
    cfg = make_cfg(capi, case) if cfg is None else cfg
    o = capi.PdcchInfo()
    o.sizes = tuple(cfg.size[:cfg.n_sizes])
    cfi = np.ascontiguousarray(np.concatenate([np.asarray(cfi, np.int32), np.zeros(72, np.int32)])[:72])
    llr = np.zeros((PR.n_sf_of(tfg.shape[0], cp), 1152)) if want_llr else None
    H.pdcch_host(_dp(tfg.view(np.float64)), tfg.shape[0], PR.n_symb_of(cp), n_rb, n_id, cp, ports, dl_mask_of(case) if mask is None else mask, _up(jump),
                 C.byref(cfg), _ip(cfi), _dp(llr) if want_llr else None, C.byref(o))
    return (o, llr) if want_llr else o


def assert_record_against_numpy(rec, ref, planted, tol, what=""):
    """rec: capi.PdcchInfo; ref: pdcch_ref.receive's dict.  cfi, n_reg, n_cce and which entries are decoded: equal.  Every planted
    entry: bits, rnti_x, flags equal and equal to what was planted.  Every other entry: equal unless numpy's best and second-best
    start states lie within 1e-9 (relative to sum |coded bit|), which a planted entry may never do.  quality within tol.
    -> (worst quality difference, decodes compared, decodes excused)"""
    n = ref["n_sf"]
    assert rec.n_sf == n and np.array_equal(rec.cfi, ref["cfi"]) and np.array_equal(rec.n_reg, ref["n_reg"]) and np.array_equal(rec.n_cce, ref["n_cce"]), what
    assert rec.n_read == ref["n_read"], what
    got = {(g, s, i): d for g, s, i, d in rec.entries()}
    assert set(got) == {k for k, d in ref["dec"].items() if d["flags"] & 1}, what
    plant = {(p["g"], p["slot"], p["i"]): p for p in planted}
    worst, excused = 0.0, 0
    for key, d in got.items():
        r = ref["dec"][key]
        if key in plant:
            p = plant[key]
            accepted = 2 if p["rnti"] in (0xFFFF, 0xFFFE) or 1 <= p["rnti"] <= 60 else 0
            assert r["gap"] > 1e-9, (what, key)
            assert (d.bits, d.rnti_x, d.flags) == (p["bits"], p["rnti"], 1 | accepted) == (r["bits"], r["rnti_x"], r["flags"]), (what, key, hex(d.bits), hex(d.rnti_x), d.flags)
        elif r["gap"] <= 1e-9:
            excused += 1
            continue
        else:
            assert (d.bits, d.rnti_x, d.flags) == (r["bits"], r["rnti_x"], r["flags"]), (what, key)
        assert abs(d.quality - r["quality"]) <= tol, (what, key, d.quality, r["quality"])
        worst = max(worst, abs(d.quality - r["quality"]))
    return worst, len(got), excused


# ---------------------------------------------------------------- captures with the generator's PCFICH and PDCCH in them
CAP_ID = (41, 2)                 # n_id_1, n_id_2
CAP_T0 = 100.0                   # 1.92 Msps samples into frame 0 at which the capture starts: the grid starts at frame 1
CAP_SHAPES = [(1, 6, 1, 2), (2, 15, 1, 2), (2, 15, 2, 4)]      # (R, n_rb, CP type, ports)
CAP_FC = 739e6


def capture_cfi(frame, sf):
    return 2 + (frame + sf) % 2


def fields_1a(frame, sf, n_rb):
    start = (3 * sf + frame) % n_rb
    return dict(flag_1a=1, distributed=0, rb_start=start, n_rb_alloc=1 + sf % (n_rb - start), mcs=(3 * sf + frame) % 32, harq=sf % 8, ndi=sf & 1, rv=sf % 4, tpc=(sf + 1) % 4)


def pack_1a(f, n_rb):
    """the payload bits of format 1A (FDD) from its fields, in the order sent (36.212 5.3.3.1.3), padded to the table's size"""
    L, S = f["n_rb_alloc"], f["rb_start"]
    riv = n_rb * (L - 1) + S if L - 1 <= n_rb // 2 else n_rb * (n_rb - L + 1) + (n_rb - 1 - S)
    out = []
    for v, n in ((f["flag_1a"], 1), (f["distributed"], 1), (riv, (n_rb * (n_rb + 1) // 2 - 1).bit_length()), (f["mcs"], 5), (f["harq"], 3), (f["ndi"], 1), (f["rv"], 2), (f["tpc"], 2)):
        out += [(v >> (n - 1 - i)) & 1 for i in range(n)]
    size = load_pkg().capi.dci_common_sizes(n_rb)[0]
    return out + [0] * (size - len(out))


def capture_plan(n_rb, cp, ports):
    """(frame, subframe) -> the DCIs of that subframe: a 1A with SI- or P-RNTI from CCE 0 (L = 8 in every third subframe where eight
    CCEs exist), and a 1C with an RA-RNTI at L = 4 from CCE 8 where twelve exist"""
    pkg = load_pkg()
    n_id = CAP_ID[1] + 3 * CAP_ID[0]

    def plan(frame, sf):
        n_cce = pkg.synth.pdcch_layout(n_id, n_rb, ports, cp == 1, capture_cfi(frame, sf))[1]
        out = []
        if n_cce >= 4:
            out.append(dict(rnti=0xFFFF if sf % 2 == 0 else 0xFFFE, bits=pack_1a(fields_1a(frame, sf, n_rb), n_rb), L=8 if n_cce >= 8 and sf % 3 == 0 else 4, cce=0))
        if n_cce >= 12:
            bits = np.random.default_rng(100 * frame + sf).integers(0, 2, pkg.capi.dci_common_sizes(n_rb)[1])
            out.append(dict(rnti=1 + (7 * sf + frame) % 60, bits=[int(b) for b in bits], L=4, cce=8))
        return out
    return plan


@functools.lru_cache(maxsize=None)
def pdcch_capture(R, n_rb, cp, ports, snr_db=10.0):
    """synth.make_wideband_cell: one cell of n_rb resource blocks at 1.92e6 R on the capture's centre, three frames in noise 10 dB
    below a resource element, with capture_cfi and capture_plan planted and every other CCE filled with probability 1/2
    -> (complex64 samples, frame_start of the cell's frame 1 in them)"""
    pkg = load_pkg()
    cell = dict(n_id_1=CAP_ID[0], n_id_2=CAP_ID[1], cp_normal=cp == 1, n_ports=ports, f_off=0.0, t0=CAP_T0, sfn0=8, n_rb_dl=n_rb,
                cfi=capture_cfi, pdcch=capture_plan(n_rb, cp, ports), pdcch_fill=0.5)
    x, _, _ = pkg.synth.make_wideband_cell(40 + R + cp + ports, CAP_FC, R, [(CAP_FC, R, n_rb, cell)], snr_db=snr_db, n_in=3 * 19200 * R)
    x.setflags(write=False)
    return x, (19200.0 - CAP_T0) * R


def capture_planted(n_rb, cp, ports, n_sf):
    """what capture_plan put into grid subframes g < n_sf of a grid that starts at frame 1: dicts as crafted()'s"""
    sizes = load_pkg().capi.dci_common_sizes(n_rb)
    out = []
    for g in range(n_sf):
        for d in capture_plan(n_rb, cp, ports)(1 + g // 10, g % 10):
            slot = d["cce"] // 4 if d["L"] == 4 else 4 + d["cce"] // 8
            out.append(dict(g=g, slot=slot, i=sizes.index(len(d["bits"])), L=d["L"], cce=d["cce"], rnti=d["rnti"], bits=sum(int(b) << t for t, b in enumerate(d["bits"]))))
    return out
