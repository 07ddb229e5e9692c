"""Inputs the blind-search tests share (tests/test_pdcch_scan_host.py, tests/test_gpu_pdcch_scan.py): crafted grids of six subframes
with planted PCFICH and PDCCH, and the host twin's loader.  Scaffolding as pdcch_cases.crafted: per-port gains, a linear phase and an
amplitude slope across the band, a slow drift over the rows, CRS of every port, the PCFICH of the subframe's CFI, noise 20 dB below a
resource element.

Plan of a case (subframes that are read, in order): the recurring RNTI `a` has one DCI in every subframe but the silent one, inside
its own search space, at L = 1, 2, 4, 8 in turn (the next level that exists, fits the rate rule and has a free start); the recurring
RNTI `b` has one in the first two such subframes at the level after `a`'s; RNTI `once` has a single DCI; RNTI `out` has a single DCI
at a start OUTSIDE its search space; an SI DCI sits at L = 4 from CCE 0 and a paging DCI at L = 8 from CCE 8 where those exist.
Subframe SILENT_SF carries no PDCCH (noise alone); FILL_SF has every unused CCE filled with random bits."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import pcfich_cases as PC
import pcfich_ref as PR
import pdcch_ref as DR
import pdcch_scan_ref as SR
from conftest import load_pkg

# (n_id_cell, CP type, ports, n_rb, PHICH duration, PHICH resource, TDD m_i or None, CFI per subframe)
CASES = [
    (0, 1, 1, 6, 1, 1, None, (1, 2, 3, 3, 2, 1)),            # N_CCE 2 .. 6: wrap-around spaces, no L = 8
    (503, 2, 2, 6, 1, 3, None, (3, 3, 2, 3, 3, 2)),
    (141, 1, 2, 15, 1, 1, None, (3, 2, 3, 1, 3, 2)),
    (68, 1, 4, 15, 2, 2, None, (3, 3, 3, 3, 3, 3)),          # four ports, the extended PHICH duration
    (7, 1, 2, 25, 1, 3, None, (3, 2, 3, 3, 3, 1)),           # N_CCE 20 at CFI 3
    (141, 1, 2, 25, 1, 3, (0, 1, None, None, 1, 0, 1, None, None, 1), (3, 3, 3, 3, 3, 3)),   # TDD configuration 1
    (329, 1, 2, 50, 1, 3, None, (3, 3, 2, 3, 3, 3)),         # N_CCE 41: CCEs beyond 15 and beyond 32
    (256, 1, 2, 100, 1, 3, None, (3, 3, 3, 3, 3, 3)),        # N_CCE 84: quadruplets beyond 576, the third mask word
]
N_SF = 6
SILENT_SF, FILL_SF = 3, 4
SNR_DB = 20.0
RNTI_A, RNTI_B, RNTI_ONCE, RNTI_OUT = 0x4A31, 0x0107, 0xC0DE, 0x2F05
MIN_QUALITY = None          # None: the bindings' default


def case_id(case):
    return "id%d-cp%d-p%d-rb%d-d%d-r%d%s" % (case[:6] + ("-tdd" if case[6] else "",))


def sizes_of(case):
    """the sizes of formats 0/1A, 1, 2A (two ports and more) and 1C of the cell"""
    capi = load_pkg().capi
    tdd = case[6] is not None
    ue = capi.dci_ue_sizes(case[3], case[2], tdd)
    out = [ue["0/1A"], ue["1"]] + ([ue["2A"]] if "2A" in ue else []) + [capi.dci_common_sizes(case[3], tdd)[1]]
    return tuple(dict.fromkeys(out))


def mi_of(case):
    return None if case[6] is None else [0 if m is None else m for m in case[6]]


def dl_mask_of(case):
    return 0x3FF if case[6] is None else sum(1 << i for i, m in enumerate(case[6]) if m is not None)


def min_quality():
    return load_pkg().capi.PDCCH_SCAN_MIN_QUALITY if MIN_QUALITY is None else MIN_QUALITY


@functools.lru_cache(maxsize=None)
def crafted(case, snr_db=SNR_DB, fill=None, seed=0, plan=None):
    """-> (tfg [6 subframes], cfi [6], planted: list of dict(g, L, cce, i, bits (int), rnti, kind)); kind is "a", "b", "once", "out"
    or "common".  tools/pdcch_scan_accuracy.py asks for other noise, a fill in every subframe and further seeds.  plan(g, sf, n_cce,
    put) replaces the module's plan: it calls put(rnti, L, cce, size index, kind, bits) for every DCI of the subframe."""
    n_id, cp, ports, n_rb, dur, res, _, cfis = case
    c_no = CASES.index(case)
    synth = load_pkg().synth
    n, nc = PR.n_symb_of(cp), 12 * n_rb
    n_ofdm = 2 * N_SF * n
    rng = np.random.default_rng(9000 + c_no + 100 * seed)
    gain = np.exp(2j * np.pi * rng.random(4)) * (0.7 + 0.6 * rng.random(4))
    tau = 0.2 + 0.5 * rng.random(4)
    sizes, mi, mask = sizes_of(case), mi_of(case), dl_mask_of(case)

    def chan(p, row, cols):
        cols = np.asarray(cols)
        return gain[p] * np.exp(-2j * np.pi * tau[p] * (cols - nc / 2) / (128.0 * n_rb / 6)) * (1.0 + 0.3 * (cols / nc - 0.5)) * np.exp(2j * np.pi * 0.002 * row)

    k = np.arange(nc)
    qpsk = lambda m: ((1 - 2.0 * rng.integers(0, 2, m)) + 1j * (1 - 2.0 * rng.integers(0, 2, m))) / np.sqrt(2.0)
    tfg = np.stack([qpsk(nc) * chan(0, r, k) for r in range(n_ofdm)])
    cfi = np.array(cfis, np.int32)
    planted, turn, n_b, singles = [], 0, 0, ["once", "out"]
    for g in range(N_SF):
        sf, row = g % 10, 2 * g * n
        tfg[row:row + 4] = 0
        for p in range(ports):
            r = row + (0 if p < 2 else 1)
            idx = PR.shift_of(p, n_id, 2 * sf) + 6 * np.arange(2 * n_rb)
            tfg[r, idx] = PR.rs_row(n_id, cp, n_rb, 2 * sf, 0 if p < 2 else 1) * chan(p, r, idx)
        cols = PR.columns(n_id, n_rb)
        x = synth._tx_diversity(synth.pcfich_symbols(n_id, sf, cfi[g]), ports)
        tfg[row, cols] = sum(x[p] * chan(p, row, cols) for p in range(ports))
        if not DR.is_read(g, n_ofdm, cp, n_rb, mask, dur, mi is not None):
            continue
        lay = DR.layout(n_id, cp, ports, n_rb, int(cfi[g]), dur, res, 1 if mi is None else mi[sf])
        n_cce = lay["n_cce"]
        used = np.zeros(n_cce, bool)
        dcis = []

        def put(rnti, L, cce, i, kind, bits=None):
            bits = rng.integers(0, 2, sizes[i]) if bits is None else np.asarray(bits)
            assert bits.size == sizes[i] and not used[cce:cce + L].any()
            used[cce:cce + L] = True
            dcis.append(dict(rnti=rnti, bits=bits, L=L, cce=cce))
            planted.append(dict(g=g, L=L, cce=cce, i=i, bits=sum(int(b) << t for t, b in enumerate(bits)), rnti=rnti, kind=kind))

        def place(rnti, first_level, kind, inside=True):
            """the first level from first_level on (cyclically) with a size that fits the rate rule and a free start inside (or outside)
            the RNTI's space"""
            for dl in range(4):
                L = SR.LEVELS[(first_level + dl) % 4]
                fit = [i for i, a in enumerate(sizes) if SR.rate_ok(a + 16, L)]
                space = SR.search_space(rnti, sf, n_cce, L)
                starts = list(dict.fromkeys(space)) if inside else [c for c in range(0, n_cce - L + 1, L) if c not in space]
                starts = [c for c in starts if not used[c:c + L].any()]
                if fit and starts:
                    put(rnti, L, starts[-1] if inside else starts[0], fit[(g + turn) % len(fit)], kind)
                    return True
            return False

        if plan is not None:
            plan(g, sf, n_cce, put)
        elif g != SILENT_SF and n_cce:
            if n_cce >= 4:
                put(0xFFFF, 4, 0, 0, "common")
            if n_cce >= 16 and g % 2 == 0:
                put(0xFFFE, 8, 8, 0, "common")
            place(RNTI_A, turn, "a")
            if n_b < 2 and place(RNTI_B, turn + 1, "b"):
                n_b += 1
            if singles and place(RNTI_ONCE if singles[0] == "once" else RNTI_OUT, turn + 2, singles[0], inside=singles[0] == "once"):
                singles.pop(0)
            turn += 1
        DR.plant(tfg, g, n_id, cp, ports, n_rb, int(cfi[g]), dur, res, dcis, chan, fill=(1.0 if g == FILL_SF and plan is None else 0.0) if fill is None else fill, rng=rng,
                 mi=1 if mi is None else mi[sf])
    sigma = 10 ** (-snr_db / 20) / np.sqrt(2.0)
    tfg += sigma * (rng.standard_normal(tfg.shape) + 1j * rng.standard_normal(tfg.shape))
    tfg.setflags(write=False)
    return tfg, cfi, planted


@functools.lru_cache(maxsize=None)
def reference(case, min_repeat=2):
    """pdcch_scan_ref.receive on the case's grid with the planted CFI: computed once, shared by the tests"""
    tfg, cfi, _ = crafted(case)
    n_id, cp, ports, n_rb, dur, res = case[:6]
    return SR.receive(tfg, n_id, cp, ports, n_rb, cfi, dur, res, sizes_of(case), min_quality(), min_repeat, dl_mask_of(case), 7, mi_of(case))


def rereading(m, planted):
    """is the message (dict with subframe, L, cce, size_index, bits, rnti) a planted DCI or a re-reading of one: the same subframe, RNTI,
    size and bits on CCEs that overlap the planted ones"""
    return any(p["g"] == m["subframe"] and p["rnti"] == m["rnti"] and p["i"] == m["size_index"] and p["bits"] == m["bits"] and
               m["cce"] < p["cce"] + p["L"] and p["cce"] < m["cce"] + m["L"] for p in planted)


# ---------------------------------------------------------------- the host twin (tests/host/pdcch_scan_host.cpp)
ROOT = PC.ROOT
TWIN_SRC = os.path.join(ROOT, "tests", "host", "pdcch_scan_host.cpp")
TWIN_LIB = os.path.join(ROOT, "tests", "host", "libpdcch_scan_host.so")
SAN = os.path.join(ROOT, "tests", "host", "pdcch_scan_host_san")
_dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
_ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
_up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))


def stale(target, src=TWIN_SRC):
    dep = [src] + [os.path.join(PC.CSRC, h) for h in ("pdcch_scan.h", "pdcch.h", "pcfich.h", "cell_meas.h", "tdd_config.h", "lte_device.h")] + [os.path.join(ROOT, "include", "lcs.h")]
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in dep)


def declare_twin(h, capi):
    ip = C.POINTER(C.c_int32)
    h.pscan_host.argtypes = [C.POINTER(C.c_double)] + [C.c_int] * 7 + [C.POINTER(C.c_uint32), C.POINTER(capi.PdcchScanCfg), ip, C.c_int, C.POINTER(C.c_double),
                                                                     C.POINTER(capi.PdcchScanDec), C.POINTER(capi.PdcchScanInfo)]
    h.pscan_host.restype = None
    h.pscan_host_map.argtypes = [C.c_int] * 8 + [ip, ip, ip, ip]
    h.pscan_host_scramble.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    h.pscan_host_scramble.restype = None
    h.pscan_host_cand.argtypes = [C.c_int, C.c_int, ip, ip]
    h.pscan_host_spaces.argtypes = [C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_int8)]
    h.pscan_host_spaces.restype = None
    h.pscan_host_rnti_x.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_uint32)]
    h.pscan_host_rnti_x.restype = C.c_uint32
    h.pscan_host_decode.argtypes = [C.POINTER(C.c_double)] + [C.c_int] * 6 + [C.POINTER(capi.PdcchScanDec), ip, ip]
    return h


def load_twin(capi):
    """pdcch_scan.h compiled for the host (built where missing or older than its sources)"""
    if stale(TWIN_LIB):
        subprocess.check_call(PC.HIPCC + ["-O2", "-fPIC", "-shared", "-o", TWIN_LIB, TWIN_SRC])
    return declare_twin(C.CDLL(TWIN_LIB), capi)


def make_cfg(capi, case, **kw):
    kw.setdefault("min_quality", MIN_QUALITY)
    return capi.PdcchScanCfg.make(sizes_of(case), phich_duration=case[4], phich_resource=case[5], phich_mi=case[6], **kw)


def twin_record(H, capi, case, tfg, cfi, cfg=None, mask=None, want_llr=False, msg_cap=1024):
    """-> (PdcchScanInfo, decode table [n_sf][165][6] of PdcchScanDec as a ctypes array, llr or None)"""
    n_id, cp, ports, n_rb = case[:4]
    tfg = np.ascontiguousarray(tfg, np.complex128)
    jump = np.ascontiguousarray(PC.jump_tables(n_rb)[:32])
    cfg = make_cfg(capi, case) if cfg is None else cfg
    o = capi.PdcchScanInfo()
    o.sizes = tuple(cfg.size[:cfg.n_sizes])
    n_sf = PR.n_sf_of(tfg.shape[0], cp)
    cfi = np.ascontiguousarray(np.concatenate([np.asarray(cfi, np.int32), np.zeros(72, np.int32)])[:72])
    llr = np.zeros((n_sf, 6336)) if want_llr else None
    tab = (capi.PdcchScanDec * (n_sf * 165 * 6))()
    H.pscan_host(_dp(tfg.view(np.float64)), tfg.shape[0], PR.n_symb_of(cp), n_rb, n_id, cp, ports, dl_mask_of(case) if mask is None else mask, _up(jump),
                 C.byref(cfg), _ip(cfi), msg_cap, _dp(llr) if want_llr else None, tab, C.byref(o))
    return o, tab, llr


def table_of(tab, g, n_cand, n_sizes):
    """the entries of subframe g in candidate and size order, as lcs_pdcch_scan_decodes returns them"""
    return [tab[(g * 165 + i) * 6 + si] for i in range(n_cand) for si in range(n_sizes)]


DEC_FIELDS = ("bits", "rnti_x", "flags", "n_err", "n_obs", "n_repeat")


# ---------------------------------------------------------------- a capture with C-RNTI grants in it
CAP_SHAPE = (2, 15, 1, 2)        # (R, n_rb, CP type, ports), as pdcch_cases.CAP_SHAPES[1]
CAP_RNTIS = (0x4A31, 0x0107)
CAP_N_SF = 20


def cap_sizes():
    ue = load_pkg().capi.dci_ue_sizes(CAP_SHAPE[1], CAP_SHAPE[3])
    return (ue["0/1A"], ue["1"], ue["2A"])


def cap_plan():
    """(frame, subframe) -> the DCIs of that subframe: RNTI 0 in every subframe at L = 2, 4, 8 in turn (where the level exists), RNTI 1
    in every other one at the level after it, each at the last start of its own search space that is free; sizes in turn.
    No L = 1: the 15 RB sizes go out at rate 0.53 there with 45 of 117 coded bits punctured, which the rule does not find every time
    at this noise (tools/pdcch_scan_accuracy.py: 94 % at 5 dB; on this capture two of five such DCIs came back with 9 and 11 of 72
    observed coded bits wrong), and this test asks for every planted DCI.  L = 1 is pinned at 20 dB on the crafted grids."""
    import pdcch_cases as DC
    pkg = load_pkg()
    R, n_rb, cp, ports = CAP_SHAPE
    n_id = DC.CAP_ID[1] + 3 * DC.CAP_ID[0]
    sizes = cap_sizes()

    def plan(frame, sf):
        n_cce = pkg.synth.pdcch_layout(n_id, n_rb, ports, cp == 1, DC.capture_cfi(frame, sf))[1]
        out, used = [], set()
        for j, rnti in enumerate(CAP_RNTIS):
            if j == 1 and (frame + sf) % 2:
                continue
            L = (2, 4, 8)[(sf + frame + j) % 3]
            fit = [a for a in sizes if SR.rate_ok(a + 16, L)]
            starts = [c for c in dict.fromkeys(SR.search_space(rnti, sf, n_cce, L)) if not used & set(range(c, c + L))]
            if not starts or not fit:
                continue
            a = fit[(sf + j) % len(fit)]
            bits = np.random.default_rng(1000 * frame + 10 * sf + j).integers(0, 2, a)
            out.append(dict(rnti=rnti, bits=[int(b) for b in bits], L=L, cce=starts[-1]))
            used |= set(range(starts[-1], starts[-1] + L))
        return out
    return plan


@functools.lru_cache(maxsize=None)
def scan_capture(snr_db=10.0):
    """synth.make_wideband_cell with cap_plan planted and every other CCE filled with probability 1/2, three frames
    -> (complex64 samples, frame_start of the cell's frame 1 in them)"""
    import pdcch_cases as DC
    pkg = load_pkg()
    R, n_rb, cp, ports = CAP_SHAPE
    cell = dict(n_id_1=DC.CAP_ID[0], n_id_2=DC.CAP_ID[1], cp_normal=cp == 1, n_ports=ports, f_off=0.0, t0=DC.CAP_T0, sfn0=8, n_rb_dl=n_rb,
                cfi=DC.capture_cfi, pdcch=cap_plan(), pdcch_fill=0.5)
    x, _, _ = pkg.synth.make_wideband_cell(77, DC.CAP_FC, R, [(DC.CAP_FC, R, n_rb, cell)], snr_db=snr_db, n_in=3 * 19200 * R)
    x.setflags(write=False)
    return x, (19200.0 - DC.CAP_T0) * R


def cap_planted():
    """what cap_plan put into grid subframes g < CAP_N_SF of a grid that starts at frame 1"""
    sizes = cap_sizes()
    out = []
    for g in range(CAP_N_SF):
        for d in cap_plan()(1 + g // 10, g % 10):
            out.append(dict(g=g, i=sizes.index(len(d["bits"])), L=d["L"], cce=d["cce"], rnti=d["rnti"], bits=sum(int(b) << t for t, b in enumerate(d["bits"]))))
    return out
