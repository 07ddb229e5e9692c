"""Inputs the tests of the combined redundancy versions share (tests/test_pdsch_comb_ref.py, tests/test_pdsch_comb_host.py,
tests/test_gpu_pdsch_comb.py): crafted grids of 46 to 61 subframes, made as tests/pdsch_cases.py makes its own -- per-port complex gains,
a linear phase and an amplitude slope across the band, a slow drift over the rows, the CRS of every port, load on every other element,
the PCFICH of a CFI that changes from subframe to subframe --, with SI grants planted (format 1A on the PDCCH and the transport block
behind it) or forced.  The dl_mask of a scenario holds only the subframes it uses.  Noise is 20 dB below a resource element; the
elements of a grant may carry more (its `snr`, fixed here on the CPU so that the numpy rule fails the block alone where the scenario
needs that): the control region and the reference elements stay readable, so every scenario's grants are found.

A scenario: dict(case = (n_id_cell, CP type, ports, n_rb, PHICH resource, TDD m_i or None) as pdsch_cases.CASES, n_sf, grants = [dict(g,
rb_start, n_prb, mcs, tpc, rv, msg, rnti, snr, silent, distributed)], forced: the grants go into the configuration instead of the
PDCCH, si_window, sib1).  Grants with one `msg` carry the same transport block."""
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
import pdsch_comb_ref as CR
import pdsch_ref as SR
from conftest import load_pkg

SI, PAGING, RA = 0xFFFF, 0xFFFE, 17
TDD_MI = (0, 1, None, None, 1, 0, 1, None, None, 1)


def G(g, rb_start, n_prb, mcs, tpc, rv, msg, rnti=SI, snr=20.0, silent=False, distributed=0):
    return dict(g=g, rb_start=rb_start, n_prb=n_prb, mcs=mcs, tpc=tpc, rv=rv, msg=msg, rnti=rnti, snr=snr, silent=silent, distributed=distributed)


def S(name, case, n_sf, grants, forced=False, si_window=0, sib1=True, snr_all=None, seed=0):
    """snr_all, seed (tools/pdsch_comb_accuracy.py): one noise level on every element of the grid, the reference elements included; further draws"""
    return dict(name=name, case=case, n_sf=n_sf, grants=tuple(tuple(sorted(g.items())) for g in grants), forced=forced, si_window=si_window, sib1=sib1, snr_all=snr_all, seed=seed)


# tbs 296 (column 0, mcs 9; K = 320) on one resource block: fewer coded bits than information bits in every transmission.  Such a
# transmission is sent with rv 0 or 1 here.  With rv 2 or 3 and G well below K it holds parity bits only and none that the known ends of
# the trellis reach: the stage's decoder then sees a zero (or never negative) posterior at every step, decides all zeros, and CRC24A of
# all zeros is zero -- the block ends `ok` with a zero payload (tests/test_pdsch_comb_ref.py::test_parity_only_transmission_is_a_false_ok
# says where that was seen and where not).  "more-info-rv023" keeps the literal sizes and redundancy versions of the issue's first case
# and shows what the rule then gives; "rate-one-rv023" is that case at the sizes at which the numpy rule meets its conditions with rv 0, 2,
# 3: tbs 488 (column 0, mcs 13; K = 512) on two resource blocks of 15, G = 528 = 1.03 K -- every member alone ends crc, the sum decodes.
SCENARIOS = [
    S("more-info-than-coded", (0, 1, 1, 6, 1, None), 46, [G(5, 0, 1, 9, 0, 0, "a"), G(25, 0, 1, 9, 0, 1, "a"), G(45, 0, 1, 9, 0, 0, "a")]),
    S("more-info-than-coded-forced", (503, 2, 2, 6, 3, None), 46, [G(5, 5, 1, 7, 0, 0, "a"), G(25, 4, 1, 7, 0, 1, "a"), G(45, 5, 1, 7, 0, 0, "a")], forced=True),      # (tbs 208, K = 232; 72 elements)
    S("rate-one-rv023", (141, 1, 2, 15, 1, None), 46, [G(5, 0, 2, 13, 0, 0, "a"), G(25, 0, 2, 13, 0, 2, "a"), G(45, 0, 2, 13, 0, 3, "a")]),
    S("more-info-rv023", (0, 1, 1, 6, 1, None), 46, [G(5, 0, 1, 9, 0, 0, "a"), G(25, 0, 1, 9, 0, 2, "a"), G(45, 0, 1, 9, 0, 3, "a")]),
    # tbs 256 as (column 0, mcs 8) and (column 1, mcs 6); the second member lies across the PSS / SSS columns; rv 0 / 2 / 3; the noise on
    # the grants' elements is 1.5 dB ABOVE a resource element: the numpy rule fails every member and decodes the sum
    S("different-grants", (141, 1, 2, 15, 1, None), 46, [G(5, 0, 2, 8, 0, 0, "a", snr=-1.5), G(25, 6, 3, 6, 1, 2, "a", snr=-1.5), G(45, 11, 2, 8, 0, 3, "a", snr=-1.5)]),
    S("member-decodes", (68, 1, 4, 6, 2, None), 46, [G(5, 0, 3, 8, 0, 0, "a"), G(25, 1, 1, 8, 0, 1, "a"), G(45, 2, 3, 8, 0, 3, "a")]),
    S("changed-content-ok", (256, 2, 4, 15, 4, None), 46, [G(5, 0, 4, 5, 0, 0, "a"), G(25, 3, 4, 5, 0, 2, "b")]),
    S("changed-content-crc", (329, 1, 1, 15, 3, None), 46, [G(5, 0, 1, 9, 0, 0, "a"), G(25, 0, 1, 9, 0, 1, "b")]),
    S("parity", (0, 1, 1, 6, 1, None), 61, [G(5, 0, 1, 9, 0, 0, "a"), G(15, 1, 1, 9, 0, 0, "b"), G(25, 2, 1, 9, 0, 1, "a"), G(35, 3, 1, 9, 0, 1, "b"),
                                            G(45, 4, 1, 9, 0, 0, "a"), G(55, 5, 1, 9, 0, 0, "b")]),
    S("parity-tdd", (142, 1, 2, 25, 3, TDD_MI), 46, [G(5, 0, 1, 9, 0, 0, "a"), G(15, 1, 1, 9, 0, 0, "b"), G(25, 9, 1, 9, 0, 1, "a"), G(35, 3, 1, 9, 0, 1, "b")]),
    # rule 2: blocks outside subframe 5; 4, 14 and 24 of one tbs (24 is 20 from the first: a new group), another tbs at 9 in between
    S("window-off", (141, 1, 2, 15, 1, None), 46, [G(4, 0, 1, 9, 0, 0, "a"), G(9, 0, 3, 3, 0, 0, "c"), G(14, 2, 1, 9, 0, 1, "a"), G(24, 4, 1, 9, 0, 0, "a")]),
    S("window-20", (141, 1, 2, 15, 1, None), 46, [G(4, 0, 1, 9, 0, 0, "a"), G(9, 0, 3, 3, 0, 0, "c"), G(14, 2, 1, 9, 0, 1, "a"), G(24, 4, 1, 9, 0, 0, "a")], si_window=20),
    S("window-no-sib1", (0, 1, 1, 6, 1, None), 46, [G(5, 0, 1, 9, 0, 0, "a"), G(25, 0, 1, 9, 0, 1, "a"), G(45, 0, 1, 9, 0, 0, "a")], si_window=41, sib1=False),
    # never members: paging and RA, and SI blocks that are silent, distributed, mcs 27 or whose rows leave the grid
    S("never-members", (256, 2, 4, 15, 4, None), 46, [G(5, 0, 1, 9, 0, 0, "a", rnti=PAGING), G(5, 2, 1, 9, 0, 0, "a", rnti=RA), G(15, 0, 1, 9, 0, 0, "b", silent=True),
                                                      G(25, 0, 1, 9, 0, 1, "a", distributed=1), G(35, 0, 1, 27, 0, 1, "b"), G(45, 0, 1, 9, 0, 0, "a")]),
    S("rows", (0, 1, 1, 6, 1, None), 46, [G(25, 0, 1, 9, 0, 0, "a"), G(45, 0, 1, 9, 0, 1, "a")]),      # (the grid is cut inside subframe 45)
    # limits: six members of one key (the fifth opens a second group)
    S("fifth-member", (141, 1, 2, 15, 1, None), 46, [G(5, 0, 1, 9, 0, 0, "a"), G(5, 1, 1, 9, 0, 1, "a"), G(25, 2, 1, 9, 0, 0, "a"), G(25, 3, 1, 9, 0, 1, "a"),
                                                     G(45, 4, 1, 9, 0, 0, "a"), G(45, 5, 1, 9, 0, 1, "a")]),
    # ten blocks of ten sizes under rule 2: ten groups of one member, eight listed
    S("ninth-group", (141, 1, 2, 15, 1, None), 51, [G(4 + 10 * (i // 2) + 5 * (i % 2), 0, 3, i, 0, 0, "m%d" % i) for i in range(10)], si_window=5),
    # a sum that is silent: two members whose soft bits cancel -- the second subframe repeats the first with the grant's elements negated
    S("silent-sum", (0, 1, 1, 6, 1, None), 46, [G(5, 0, 1, 9, 0, 0, "a"), G(25, 0, 1, 9, 0, 0, "a")]),
]
ROWS_CUT = {"rows": 45}                # scenario -> the subframe inside which its grid ends
NEGATED = {"silent-sum": (5, 25)}      # scenario -> (g, its negated copy)


def by_name(name):
    return next(s for s in SCENARIOS if s["name"] == name)


def grants_of(sc):
    return [dict(g) for g in sc["grants"]]


def mask_of(sc):
    return sum(1 << sf for sf in {g["g"] % 10 for g in grants_of(sc)})


def comb_cfg(capi, sc):
    return capi.PdschCombCfg.make(si_window=sc["si_window"], sib1=sc["sib1"])


def cfi_of(sc, g):
    """a CFI that changes with the subframe and leaves room for the subframe's DCIs (two of them need three control symbols)"""
    two = sum(x["g"] == g for x in grants_of(sc)) > 1
    return 3 if two else 2 + (g + sc["case"][0]) % 2


def forced_list(sc):
    capi = load_pkg().capi
    return [(g["g"], g["rnti"], g["rb_start"], g["n_prb"], capi.tbs_1a(g["mcs"], g["tpc"]), g["rv"]) for g in grants_of(sc)] if sc["forced"] else None


def _key(sc):
    return tuple(sorted((k, v) for k, v in sc.items()))


@functools.lru_cache(maxsize=None)
def _crafted(key):
    sc = dict(key)
    case = sc["case"]
    n_id, cp, ports, n_rb, res, mi = case
    pkg = load_pkg()
    synth, capi = pkg.synth, pkg.capi
    n, nc, n_sf = PR.n_symb_of(cp), 12 * n_rb, sc["n_sf"]
    cut = ROWS_CUT.get(sc["name"])
    n_ofdm = 2 * n * n_sf if cut is None else 2 * n * cut + (4 if n_rb <= 10 else 3)
    rng = np.random.default_rng(7000 + sum(map(ord, sc["name"])) + 100000 * sc.get("seed", 0))
    gain = np.exp(2j * np.pi * rng.random(4)) * (0.7 + 0.6 * rng.random(4))
    tau = 0.2 + 0.5 * rng.random(4)
    tdd = mi is not None
    pc = SC.pdcch_case(case)
    mask, mis = mask_of(sc), DC.mi_of(pc)

    def chan(p, row, cols):
        cols = np.asarray(cols)
        return gain[p] * np.exp(-2j * np.pi * tau[p] * (cols - nc / 2) / (128.0 * n_rb / 6)) * (1.0 + 0.3 * (cols / nc - 0.5)) * np.exp(2j * np.pi * 0.0005 * row)

    k = np.arange(nc)
    qpsk = lambda m: ((1 - 2.0 * rng.integers(0, 2, m)) + 1j * (1 - 2.0 * rng.integers(0, 2, m))) / np.sqrt(2.0)
    tfg = np.stack([qpsk(nc) * chan(0, r, k) for r in range(n_ofdm)])
    cfi = np.zeros(n_sf, np.int32)
    grants = grants_of(sc)
    msgs = {}
    snr_all = sc.get("snr_all")
    sigma = np.full(tfg.shape, 10 ** (-(20.0 if snr_all is None else snr_all) / 20) / np.sqrt(2.0))
    planted = []
    for g in range(n_sf):
        sf, row = g % 10, 2 * g * n
        cfi[g] = cfi_of(sc, g)
        if row >= n_ofdm:
            continue
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
        for f in (x for x in grants if x["g"] == g):
            tbs = capi.tbs_1a(f["mcs"], f["tpc"]) if f["mcs"] <= 26 else 0
            sent = not f["distributed"] and f["mcs"] <= 26 and SR.whole(g, n_ofdm, cp) and not (tdd and sf in (1, 6))
            if sent and (f["msg"], tbs) not in msgs:
                msgs[(f["msg"], tbs)] = np.random.default_rng(sum(map(ord, f["msg"])) + 1000 * tbs).integers(0, 2, tbs).astype(np.uint8)
            bits = msgs[(f["msg"], tbs)] if sent else None
            if not sc["forced"]:
                free = [c for c in cand if all(c[2] + c[1] <= d["cce"] or c[2] >= d["cce"] + d["L"] for d in dcis)]
                assert free, (sc["name"], g)
                slot, L, cce = free[0]
                dcis.append(dict(rnti=f["rnti"], bits=np.array(SC.pack_1a(f, n_rb, tdd)), L=L, cce=cce))
            planted.append(dict(f, tbs=tbs, bits=bits))
            if sent:
                gr = dict(rnti=f["rnti"], rb_start=f["rb_start"], n_prb=f["n_prb"], rv=f["rv"], bits=bits)
                SR.plant(tfg, g, n_id, cp, ports, n_rb, int(cfi[g]), gr, chan, tdd, silent=f["silent"])
                for l, cc, _ in synth.pdsch_region(n_id, n_rb, ports, cp == 1, sf, int(cfi[g]), gr, tdd):
                    sigma[row + l, cc] = 0.0 if f["silent"] else 10 ** (-(f["snr"] if snr_all is None else snr_all) / 20) / np.sqrt(2.0)
        DR.plant(tfg, g, n_id, cp, ports, n_rb, int(cfi[g]), 1, res, dcis, chan, rng=rng, mi=1 if mis is None else mis[sf])
    tfg += sigma * (rng.standard_normal(tfg.shape) + 1j * rng.standard_normal(tfg.shape))
    if sc["name"] in NEGATED:               # the second subframe: the first's received rows, with the grant's elements negated
        a, b = NEGATED[sc["name"]]
        tfg[2 * b * n:2 * (b + 1) * n] = tfg[2 * a * n:2 * (a + 1) * n]
        f = next(x for x in grants if x["g"] == b)
        gr = dict(rnti=f["rnti"], rb_start=f["rb_start"], n_prb=f["n_prb"], rv=f["rv"], bits=planted[0]["bits"])
        for l, cc, _ in synth.pdsch_region(n_id, n_rb, ports, cp == 1, b % 10, int(cfi[b]), gr, tdd):
            tfg[2 * b * n + l, cc] = -tfg[2 * b * n + l, cc]
    tfg.setflags(write=False)
    return tfg, cfi, planted


def crafted(sc):
    """-> (tfg, cfi [n_sf], planted: the scenario's grants with tbs and bits (None where nothing is sent))"""
    return _crafted(_key(sc))


@functools.lru_cache(maxsize=None)
def _reference(key):
    sc = dict(key)
    tfg, cfi, _ = crafted(sc)
    n_id, cp, ports, n_rb, res, mi = sc["case"]
    pc = SC.pdcch_case(sc["case"])
    mask = mask_of(sc)
    pdc = DR.receive(tfg, n_id, cp, ports, n_rb, cfi, 1, res, DC.sizes_of(pc), mask, 7, DC.mi_of(pc))
    blocks = SR.receive(tfg, n_id, cp, ports, n_rb, pdc, 0, SC.tdd_of(sc["case"]), mask, 1, forced=forced_list(sc))
    return pdc, blocks, CR.combine(blocks, sc["si_window"], sc["sib1"])


def reference(sc):
    """(pdcch_ref.receive's dict, pdsch_ref.receive's blocks, pdsch_comb_ref.combine's dict): computed once, shared"""
    return _reference(_key(sc))


# ---------------------------------------------------------------- the host twin (tests/host/pdsch_comb_host.cpp)
ROOT = PC.ROOT
TWIN_SRC = os.path.join(ROOT, "tests", "host", "pdsch_comb_host.cpp")
TWIN_LIB = os.path.join(ROOT, "tests", "host", "libpdsch_comb_host.so")
SAN = os.path.join(ROOT, "tests", "host", "pdsch_comb_host_san")
_dp = SC._dp


def stale(target):
    dep = [TWIN_SRC, SC.TWIN_SRC] + [os.path.join(PC.CSRC, h) for h in ("pdsch_comb.h", "pdsch.h", "pdcch.h", "pcfich.h", "cell_meas.h", "tdd_config.h", "lte_device.h")] + \
          [os.path.join(ROOT, "include", "lcs.h")]
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in dep)


def load_twin(capi):
    """pdsch_comb.h compiled for the host (built where missing or older than its sources)"""
    if stale(TWIN_LIB):
        subprocess.check_call(PC.HIPCC + ["-O2", "-fPIC", "-shared", "-o", TWIN_LIB, TWIN_SRC])
    h = C.CDLL(TWIN_LIB)
    dp = C.POINTER(C.c_double)
    h.pdsch_comb_host.argtypes = [dp] + [C.c_int] * 7 + [C.POINTER(C.c_uint32), C.c_int, C.c_int, C.POINTER(capi.PdcchInfo), C.POINTER(capi.PdschCfg),
                                                         C.POINTER(capi.PdschCombCfg), dp, C.POINTER(capi.PdschInfo), C.POINTER(capi.PdschCombInfo)]
    h.pdsch_comb_host.restype = None
    h.pdsch_comb_host_groups.argtypes = [C.POINTER(capi.PdschInfo), dp, C.c_int, C.c_int, C.POINTER(capi.PdschCombCfg), dp, C.POINTER(capi.PdschCombInfo)]
    h.pdsch_comb_host_groups.restype = None
    return h


def pdsch_cfg(capi, sc):
    return SC.make_cfg(capi, forced=forced_list(sc) or ())


def twin_records(H, capi, sc, tfg, pdc_rec, want_d=False):
    """the twin's PDSCH record and combined record from a grid and a PDCCH record (the PDCCH twin's, or the device's)"""
    n_id, cp, ports, n_rb = sc["case"][:4]
    tfg = np.ascontiguousarray(tfg, np.complex128)
    cfg, ccfg = pdsch_cfg(capi, sc), comb_cfg(capi, sc)
    d = np.zeros((8, 3, 2244)) if want_d else None
    o, oc = capi.PdschInfo(), capi.PdschCombInfo()
    H.pdsch_comb_host(_dp(tfg.view(np.float64)), tfg.shape[0], PR.n_symb_of(cp), n_rb, n_id, cp, ports, mask_of(sc), SC._up(SC.jump_tables(n_rb)), 1,
                      1 if SC.tdd_of(sc["case"]) else 0, C.byref(pdc_rec), C.byref(cfg), C.byref(ccfg), _dp(d) if want_d else None, C.byref(o), C.byref(oc))
    return (o, oc, d) if want_d else (o, oc)


def pdcch_twin_record(capi, sc, tfg, cfi):
    return DC.twin_record(DC.load_twin(capi), capi, SC.pdcch_case(sc["case"]), tfg, cfi, mask=mask_of(sc))


def assert_groups_against_numpy(rec, ref, what=""):
    """rec: capi.PdschCombInfo; ref: pdsch_comb_ref.combine's dict.  Every field of every group equal; no decoded group's numpy
    posterior may have come within 1e-9 of zero (relative)"""
    assert (rec.n_groups, rec.n_overflow) == (len(ref["groups"]), ref["n_overflow"]), (what, rec.n_groups, rec.n_overflow)
    for i, r in enumerate(ref["groups"]):
        g = rec.group[i]
        assert r["margin"] > 1e-9, (what, i, r["margin"])
        got = (g.n_members, list(g.member), g.rule, g.tbs, g.K, g.F, g.rv_mask, g.n_ok_members, g.n_same, g.n_iter, g.status)
        want = (len(r["members"]), r["members"] + [-1] * (4 - len(r["members"])), r["rule"], r["tbs"], r["K"], r["F"], r["rv_mask"], r["n_ok_members"], r["n_same"],
                r["n_iter"], r["status"])
        assert got == want, (what, i, got, want)
        assert np.array_equal(np.ctypeslib.as_array(g.payload), r["payload"]), (what, i)
    st = [sum(r["status"] == s for r in ref["groups"]) for s in range(5)]
    assert list(rec.n_status) == st and rec.n_members == sum(len(r["members"]) for r in ref["groups"])
    assert rec.n_decoded == sum(r["status"] in (2, 3) and r["n_iter"] > 0 for r in ref["groups"])
