"""Inputs the tests of distributed allocations and format 1C share (tests/test_pdsch_dvrb_host.py, tests/test_gpu_pdsch_dvrb.py): crafted
grids of 13 subframes built as tests/pdsch_cases.py builds its own, at the smallest bandwidths at which the rule can go wrong, and
the host twin's loader (tests/host/pdsch_dvrb_host.cpp).

The cases: 6 RB (N_null = 2, one port); 15 RB (N_null = 2, P = 2, an odd n_rb: the central 72 columns cut a resource block in half, and
subframes 0 and 5 carry an allocation through the centre); 25 RB (N_null = 0; four ports, extended CP; once under a TDD table, which leaves few downlink subframes, and once FDD, so that every kind
of grant of the plan is read at N_null = 0 too); 50 RB (both gaps, by
1A's NDI and by 1C's gap bit; N_step = 4; an allocation that crosses an interleaving unit).

The plan of grid subframe g (plan_of): 0 a distributed 1A SI grant over every VRB; 1 a 1C paging grant of N_step VRBs; 2 a 1C SI grant;
3 a distributed 1A RA grant whose VRBs reach beyond N_VRB (a plain one at 6 RB, where N_VRB = n_rb); 4 a 1C grant whose RIV is out of
range; 5 a 1C SI grant over every VRB (SIB1's place); 6 two grants, a distributed 1A paging grant and a 1C RA grant; 7 a localized 1A
grant; 8 a distributed 1A grant (gap 2 by the NDI bit at 50 RB); 9 a 1C grant (gap 2 by the gap bit and across an interleaving unit at
50 RB); 10 a 1C SI grant outside subframe 5; 11 a distributed 1A paging grant; 12 a 1C grant whose rows leave the grid.  A 1C SI
grant is sent with the redundancy version the rule assumes for SFN0 and SI_WINDOW."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import pcfich_cases as PC
import pcfich_ref as PR
import pdcch_cases as DC
import pdcch_ref as DR
import pdsch_cases as SC
import pdsch_dvrb_ref as VR
import pdsch_ref as SR
from conftest import load_pkg

# (n_id_cell, CP type, ports, n_rb, PHICH resource, TDD m_i or None)
CASES = [(0, 1, 1, 6, 1, None), (141, 1, 2, 15, 1, None), (329, 2, 4, 25, 1, (0, 1, None, None, 1, 0, 1, None, None, 1)), (5, 1, 2, 50, 3, None),
         (503, 2, 4, 25, 1, None)]
SFN0, SI_WINDOW = 6, 10
SETTINGS = {"sfn": (3, SFN0, SI_WINDOW), "nosfn": (3, -1, 0)}      # flags, sfn0, si_window
SNR_DB = 20.0
N_SF = 13
BEYOND_SF, RIV_SF, TWO_SF, LOCAL_SF, ROWS_SF = 3, 4, 6, 7, 12

case_id = SC.case_id
pdcch_case = SC.pdcch_case
tdd_of = SC.tdd_of


def plan_of(case, g):
    """the grants of grid subframe g: [dict(format, rb_start, n_prb (VRBs), gap, distributed, rnti, riv (a raw 1C RIV, or None))]"""
    n_rb = case[3]
    step, nv = VR.n_step_of(n_rb), VR.sizes(n_rb, 0)["n_vrb"]
    a = lambda s, n, rnti, **kw: dict(dict(format="1a", rb_start=s, n_prb=n, gap=0, distributed=1, rnti=rnti, riv=None), **kw)
    c = lambda s, n, rnti, **kw: dict(dict(format="1c", rb_start=s, n_prb=n, gap=0, distributed=1, rnti=rnti, riv=None), **kw)
    n1 = nv // step
    if g == 0:
        return [a(0, nv, 0xFFFF)]
    if g == 1:
        return [c(0, step, 0xFFFE)]
    if g == 2:
        return [c(step, 2 * step, 0xFFFF)]
    if g == BEYOND_SF:
        return [a(nv - 1, 2, 23)] if nv < n_rb else [a(1, 3, 23)]
    if g == RIV_SF:
        return [c(0, step, 0xFFFE, riv=n1 * (n1 + 1) // 2)]
    if g == 5:
        return [c(0, n1 * step, 0xFFFF)]
    if g == TWO_SF:
        return [a(0, 2, 0xFFFE), c(2 * step, step, 41)]
    if g == LOCAL_SF:
        return [a(1, 3, 0xFFFF, distributed=0)]
    if g == 8:
        return [a(3, 5, 7, gap=1)] if n_rb >= 50 else [a(1, 3, 7)]
    if g == 9:
        return [c(12, 12, 0xFFFE, gap=1)] if n_rb >= 50 else [c(step, step, 0xFFFE)]
    if g == 10:
        return [c(0, 2 * step, 0xFFFF)]
    if g == 11:
        return [a(2, nv - 3, 0xFFFE)]
    return [c(0, step, 0xFFFF)]


def comb_plan_of(case, g):
    """the combining's grid (27 subframes of the 15 RB case): one SI transport block of 488 bits (mcs 13, TBS column 2: K = 512) sent in
    subframes 5 and 25 by distributed 1A grants of two VRBs each, rv 0 and 2, as tests/pdsch_comb_cases.py's "rate-one-rv023" sends its
    own on two resource blocks: G is about K in each, so each alone fails its CRC and the sum decodes"""
    a = lambda s, rv: dict(format="1a", rb_start=s, n_prb=2, gap=0, distributed=1, rnti=0xFFFF, riv=None, fixed=dict(mcs=13, tpc=0, rv=rv), msg="sib")
    return [a(0, 0)] if g == 5 else [a(4, 2)] if g == 25 else []


PLANS = {"main": (N_SF, plan_of), "comb": (27, comb_plan_of)}


def _grant_fields(case, g, f, n_ctrl):
    """the transport block size and the fields that say it, so that the code rate stays below 1 / 2"""
    capi = load_pkg().capi
    n_id, cp, ports, n_rb = case[:4]
    tdd = tdd_of(case)
    if "fixed" in f:
        return dict(f["fixed"], tbs=capi.tbs_1a(f["fixed"]["mcs"], f["fixed"]["tpc"]))
    inside = f["rb_start"] + f["n_prb"] <= (VR.sizes(n_rb, f["gap"])["n_vrb"] if f["distributed"] else n_rb)
    if f["distributed"] and inside:
        G = 2 * len(VR.elements(n_id, cp, ports, n_rb, g % 10, n_ctrl, f["gap"], f["rb_start"], f["n_prb"], tdd))
    else:
        G = 2 * len(SR.elements(n_id, cp, ports, n_rb, g % 10, n_ctrl, f["rb_start"], min(f["n_prb"], n_rb - f["rb_start"]), tdd))
    if f["format"] == "1c":
        i = max([i for i in range(32) if VR.TBS_1C[i] + 24 <= G // 2] or [0])
        i = min(i, 9 + g)                      # (small blocks: the decoder is not what these grids are about)
        return dict(i_tbs=i, mcs=i, tbs=VR.TBS_1C[i], tpc=0, rv=VR.rv_1c(SR.kind_of(f["rnti"]), g, SFN0, SI_WINDOW))
    tpc = g % 2
    m = max([m for m in range(27) if capi.tbs_1a(m, tpc) + 24 <= G // 2] or [0])
    m = min(m, 8 + g)
    return dict(mcs=m, tbs=capi.tbs_1a(m, tpc), tpc=tpc, rv=g % 4)


@functools.lru_cache(maxsize=None)
def crafted(case, snr_db=SNR_DB, plan="main"):
    """-> (tfg, cfi [n_sf], planted: list of dict(plan_of's keys, g, slot, size index i, mcs, tbs, tpc, rv, bits (the transport block, or None
    where none is sent)))"""
    n_id, cp, ports, n_rb, res, mi = case
    pkg = load_pkg()
    synth, capi = pkg.synth, pkg.capi
    c_no = CASES.index(case)
    n, nc = PR.n_symb_of(cp), 12 * n_rb
    n_sf, plan_fn = PLANS[plan]
    n_ofdm = 2 * (n_sf - 1) * n + (4 if n_rb <= 10 else 3)
    rng = np.random.default_rng(9100 + c_no + 10 * sorted(PLANS).index(plan))
    gain = np.exp(2j * np.pi * rng.random(4)) * (0.7 + 0.6 * rng.random(4))
    tau = 0.2 + 0.5 * rng.random(4)
    tdd = mi is not None
    mask = DC.dl_mask_of(pdcch_case(case))
    mis = DC.mi_of(pdcch_case(case))

    def chan(p, row, cols):
        cols = np.asarray(cols)
        return gain[p] * np.exp(-2j * np.pi * tau[p] * (cols - nc / 2) / (128.0 * n_rb / 6)) * (1.0 + 0.3 * (cols / nc - 0.5)) * np.exp(2j * np.pi * 0.002 * row)

    k = np.arange(nc)
    qpsk = lambda m: ((1 - 2.0 * rng.integers(0, 2, m)) + 1j * (1 - 2.0 * rng.integers(0, 2, m))) / np.sqrt(2.0)
    tfg = np.stack([qpsk(nc) * chan(0, r, k) for r in range(n_ofdm)])
    cfi = np.zeros(n_sf, np.int32)
    planted = []
    for g in range(n_sf):
        sf, row = g % 10, 2 * g * n
        cfi[g] = 3 if g == TWO_SF else 2 + (g + n_id) % 2           # (a control region of one symbol holds no candidate at 15 resource blocks)
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
        n_ctrl = DR.n_ctrl_of(int(cfi[g]), n_rb)
        dcis = []
        for j, f in enumerate(plan_fn(case, g)):
            free = [c for c in cand if all(c[2] + c[1] <= d["cce"] or c[2] >= d["cce"] + d["L"] for d in dcis)]
            if not free:                   # the control region of 6 resource blocks holds one candidate: the second grant of a subframe is not sent there
                assert n_rb == 6 and j == 1, (case, g, j)
                break
            slot, L, cce = free[(g + c_no) % len(free)] if j == 0 else free[0]
            f = dict(f, **_grant_fields(case, g, f, n_ctrl))
            if f["format"] == "1c":
                bits = VR.pack_1c(f["gap"], f["rb_start"], f["n_prb"], f["i_tbs"], n_rb, f["riv"])
            else:
                bits = SC.pack_1a(dict(f, ndi=f["gap"]), n_rb, tdd)
            dcis.append(dict(rnti=f["rnti"], bits=np.array(bits), L=L, cce=cce))
            limit = VR.sizes(n_rb, f["gap"])["n_vrb"] if f["distributed"] else n_rb
            sent = f["riv"] is None and f["rb_start"] + f["n_prb"] <= limit and SR.whole(g, n_ofdm, cp) and not (tdd and sf in (1, 6))
            tb = (np.random.default_rng(sum(map(ord, f["msg"]))) if "msg" in f else rng).integers(0, 2, f["tbs"]).astype(np.uint8) if sent else None
            planted.append(dict(f, g=g, slot=slot, i=1 if f["format"] == "1c" else 0, bits=tb))
            if sent:
                SR.plant(tfg, g, n_id, cp, ports, n_rb, int(cfi[g]), dict(f, bits=tb), chan, tdd)
        DR.plant(tfg, g, n_id, cp, ports, n_rb, int(cfi[g]), 1, res, dcis, chan, rng=rng, mi=1 if mis is None else mis[sf])
    sigma = 10 ** (-snr_db / 20) / np.sqrt(2.0)
    tfg += sigma * (rng.standard_normal(tfg.shape) + 1j * rng.standard_normal(tfg.shape))
    tfg.setflags(write=False)
    return tfg, cfi, planted


@functools.lru_cache(maxsize=None)
def pdcch_reference(case):
    tfg, cfi, _ = crafted(case)
    n_id, cp, ports, n_rb, res, mi = case
    pc = pdcch_case(case)
    return DR.receive(tfg, n_id, cp, ports, n_rb, cfi, 1, res, DC.sizes_of(pc), DC.dl_mask_of(pc), 7, DC.mi_of(pc))


@functools.lru_cache(maxsize=None)
def reference(case, setting):
    """pdsch_dvrb_ref.receive's blocks on the case's grid under SETTINGS[setting]: computed once, shared"""
    tfg, _, _ = crafted(case)
    n_id, cp, ports, n_rb, res, mi = case
    flags, sfn0, w = SETTINGS[setting]
    return VR.receive(tfg, n_id, cp, ports, n_rb, pdcch_reference(case), flags, sfn0, w, 0, tdd_of(case), DC.dl_mask_of(pdcch_case(case)), 1)


# ---------------------------------------------------------------- the host twin (tests/host/pdsch_dvrb_host.cpp)
TWIN_SRC = os.path.join(PC.ROOT, "tests", "host", "pdsch_dvrb_host.cpp")
TWIN_LIB = os.path.join(PC.ROOT, "tests", "host", "libpdsch_dvrb_host.so")
_ip, _dp, _up = SC._ip, SC._dp, SC._up


def stale(target):
    dep = [TWIN_SRC, SC.TWIN_SRC] + [os.path.join(PC.CSRC, h) for h in ("pdsch.h", "pdcch.h", "pcfich.h", "cell_meas.h", "tdd_config.h", "lte_device.h")] + \
          [os.path.join(PC.ROOT, "include", "lcs.h")]
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in dep)


def load_twin(capi):
    """pdsch.h compiled for the host with the setting's entry points (built where missing or older than its sources)"""
    if stale(TWIN_LIB):
        subprocess.check_call(PC.HIPCC + ["-O2", "-fPIC", "-shared", "-o", TWIN_LIB, TWIN_SRC])
    h = C.CDLL(TWIN_LIB)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    h.pdsch_dvrb_host.argtypes = [dp] + [C.c_int] * 7 + [C.POINTER(C.c_uint32), C.c_int, C.c_int, C.POINTER(capi.PdcchInfo), C.POINTER(capi.PdschCfg),
                                                         C.POINTER(capi.PdschAllocCfg), dp, C.c_int, C.POINTER(capi.PdschAlloc), C.POINTER(capi.PdschInfo)]
    h.pdsch_dvrb_host.restype = None
    h.pdsch_dvrb_host_params.argtypes = [C.c_int, C.c_int, ip]
    h.pdsch_dvrb_host_params.restype = None
    h.pdsch_dvrb_host_prb.argtypes = [C.c_int] * 4
    h.pdsch_dvrb_host_1c.argtypes = [C.c_uint64, C.c_int, ip]
    h.pdsch_dvrb_host_1c.restype = None
    h.pdsch_dvrb_host_1c_rv.argtypes = [C.c_int] * 4
    h.pdsch_dvrb_host_elements.argtypes = [C.c_int] * 10 + [ip, C.c_int]
    return h


def alloc_cfg(capi, setting):
    flags, sfn0, w = SETTINGS[setting] if isinstance(setting, str) else setting
    return capi.PdschAllocCfg.make(distributed=bool(flags & 1), format_1c=bool(flags & 2), sfn0=sfn0, si_window=w)


def twin_record(H, capi, case, tfg, pdc_rec, setting, cfg=None, want_soft=False, mask=None):
    """the twin's record from the grid and a PDCCH record -> (record, [alloc dict per block]) and the soft bits [2 n_sf][stride] where asked"""
    n_id, cp, ports, n_rb = case[:4]
    pc = pdcch_case(case)
    tfg = np.ascontiguousarray(tfg, np.complex128)
    cfg = SC.make_cfg(capi) if cfg is None else cfg
    al = alloc_cfg(capi, setting)
    n_sf = PR.n_sf_of(tfg.shape[0], cp)
    stride = 2 * 12 * n_rb * 14
    llr = np.zeros((2 * n_sf, stride)) if want_soft else None
    allocs = (capi.PdschAlloc * 32)()
    o = capi.PdschInfo()
    H.pdsch_dvrb_host(_dp(tfg.view(np.float64)), tfg.shape[0], PR.n_symb_of(cp), n_rb, n_id, cp, ports, DC.dl_mask_of(pc) if mask is None else mask,
                      _up(SC.jump_tables(n_rb)), 1, 1 if tdd_of(case) else 0, C.byref(pdc_rec), C.byref(cfg), C.byref(al), _dp(llr) if want_soft else None, stride, allocs, C.byref(o))
    al_out = [allocs[i].as_dict() for i in range(o.n_blocks)]
    return (o, al_out, llr) if want_soft else (o, al_out)


def slots_of(blocks):
    """the grant slot (2 subframe + place among the subframe's) of every block of a numpy list"""
    per_sf, out = {}, []
    for b in blocks:
        u = per_sf.get(b["subframe"], 0)
        per_sf[b["subframe"]] = u + 1
        out.append(2 * b["subframe"] + u)
    return out
