"""CPU tests of what the stages on the full-bandwidth grid share before a launch (lte-cell-scanner_amd/csrc/wide_call.h, compiled for
the host by tests/host/wide_call_host.cpp): the row plans against the numpy statements of the stages' rules (pcfich_ref, pdcch_ref,
phich_ref, pdsch_ref) over their whole domain, what the PHICH configuration and the m_i resolve to over the cfg and cell
combinations of the stages' cases, the exact text of every refusal, and the twin as a stand-alone program under
-fsanitize=address,undefined."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import pcfich_cases as PC
import pcfich_ref as PR
import pdcch_cases as DC
import pdcch_ref as DR
import pdcch_scan_cases as SC
import pdsch_ref as SR
import phich_cases as HC
import phich_ref as HR
from conftest import ROOT, load_pkg

CSRC = os.path.join(ROOT, "lte-cell-scanner_amd", "csrc")
TWIN_SRC = os.path.join(ROOT, "tests", "host", "wide_call_host.cpp")
TWIN_LIB = os.path.join(ROOT, "tests", "host", "libwide_call_host.so")
SAN = os.path.join(ROOT, "tests", "host", "wide_call_host_san")
MAX_SF, MAX_OFDM = 72, 854
KEEP = (2, 4, 3, 4)                      # PCFICH, PDCCH (and the scan), PHICH, PDSCH
MASKS = (0x3FF, 0x021, 0x001, 0x200)
MI = (2, 1, 0, 1, 1, 2, 1, 0, 1, 1)      # the m_i of the sweep: every value, so every entry of UNITS
UNITS = (0, 3, -1)                       # map-unit counts of m_i = 0, 1, 2: none, some, a refused map


def stale(target):
    dep = [TWIN_SRC] + [os.path.join(CSRC, h) for h in ("wide_call.h", "phich.h", "pdcch.h", "pcfich.h", "cell_meas.h", "tdd_config.h", "lte_device.h")]
    dep.append(os.path.join(ROOT, "include", "lcs.h"))
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in dep)


def load_twin():
    """wide_call.h compiled for the host (built where it is missing or older than its sources), as phich_cases.load_twin"""
    if stale(TWIN_LIB):
        subprocess.check_call(PC.HIPCC + ["-O2", "-fPIC", "-shared", "-o", TWIN_LIB, TWIN_SRC])
    h = C.CDLL(TWIN_LIB)
    ip = C.POINTER(C.c_int32)
    h.wide_host_refusal.argtypes = [C.c_int] * 4
    h.wide_host_refusal.restype = C.c_char_p
    h.wide_host_resolve.argtypes = [C.c_int] * 4 + [ip] + [C.c_int] * 4 + [ip]
    h.wide_host_resolve.restype = C.c_char_p
    h.wide_host_plan.argtypes = [C.c_int] * 8 + [ip, ip, C.c_int, ip, ip, ip, ip, ip]
    h.wide_host_plan.restype = C.c_int
    h.wide_host_sweep.argtypes = [ip]
    h.wide_host_sweep.restype = C.c_uint64
    return h


@pytest.fixture(scope="module")
def H():
    load_pkg()
    assert (MAX_SF, MAX_OFDM) == (load_pkg().capi.PCFICH_MAX_SF, 854)
    return load_twin()


_ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))


def plan(H, stage, cp, n_ofdm, ports, n_rb, mask, dur, tdd, with_list):
    """-> (n_sf, rows [n_sf][keep], first [n_sf], sfrow [n_sf], list or None)"""
    rows, first, sfrow, lst = np.full(4 * MAX_SF, -7, np.int32), np.full(MAX_SF, -7, np.int32), np.full(MAX_SF, -7, np.int32), np.full(MAX_OFDM, -7, np.int32)
    n_list = np.zeros(1, np.int32)
    n_sf = H.wide_host_plan(stage, PR.n_symb_of(cp), n_ofdm, ports, n_rb, mask, dur, int(tdd), _ip(np.array(MI, np.int32)), _ip(np.array(UNITS, np.int32)), int(with_list),
                            _ip(rows), _ip(first), _ip(sfrow), _ip(lst), _ip(n_list))
    k = KEEP[stage]
    assert (rows[k * n_sf:] == -7).all() and (first[n_sf:] == -7).all() and (lst[n_list[0]:] == -7).all(), "written beyond the plan"
    return n_sf, rows[:k * n_sf].reshape(n_sf, k), first[:n_sf], sfrow[:n_sf], (lst[:n_list[0]] if with_list else None)


def need_of(stage, g, cp, n_ofdm, ports, n_rb, mask, dur, tdd):
    """the numpy statements of the rules -> (leading rows of subframe g in the grid, rows of it that are recorded, is it there whole)"""
    n = PR.n_symb_of(cp)
    r0 = 2 * g * n
    if stage == 0:                       # the mask rule of pcfich_ref.decode
        read = bool((mask >> (g % 10)) & 1) and not (r0 >= n_ofdm or (ports == 4 and r0 + 1 >= n_ofdm))
        k = (2 if ports == 4 else 1) if read else 0
        return k, k, False
    if stage == 2:
        read = HR.subframe_read(g, n_ofdm, cp, ports, dur, tdd, mask) and UNITS[MI[g % 10]] >= 0
        k = HR.rows_needed(ports, dur) if read else 0
        return k, k, False
    n_max = 4 if n_rb <= 10 else 3
    if not DR.is_read(g, n_ofdm, cp, n_rb, mask, dur, tdd):
        return 0, 0, False
    if stage == 1:
        return n_max, n_max, False
    whole = SR.whole(g, n_ofdm, cp) and not (tdd and g % 10 in (1, 6))      # a TDD special subframe carries no PDSCH the stage follows
    return (2 * n if whole else n_max), n_max, whole


# ---------------------------------------------------------------- the row plans
@pytest.mark.parametrize("cp", [1, 2])
def test_row_plans_against_the_numpy_rules_over_their_domain(H, cp):
    n, n_checked = PR.n_symb_of(cp), 0
    for ports, n_rb, dur, tdd, mask in itertools.product((1, 2, 4), (6, 15, 25), (1, 2), (False, True), MASKS):
        for n_ofdm in list(range(2 * n, 4 * n + 5)) + [122 * n]:
            for stage in range(4):
                what = (stage, cp, ports, n_rb, dur, tdd, hex(mask), n_ofdm)
                k = KEEP[stage]
                want = [need_of(stage, g, cp, n_ofdm, ports, n_rb, mask, dur, tdd) for g in range(PR.n_sf_of(n_ofdm, cp))]
                # without a list: the rows themselves
                n_sf, rows, first, sfrow, _ = plan(H, stage, cp, n_ofdm, ports, n_rb, mask, dur, tdd, False)
                assert n_sf == len(want) == PR.n_sf_of(n_ofdm, cp), what
                for g, (need, rec, whole) in enumerate(want):
                    assert list(rows[g]) == [2 * g * n + l if l < rec else -1 for l in range(k)], (what, g)
                    assert first[g] == (2 * g * n if need else -1), (what, g)
                    assert sfrow[g] == (2 * g * n if whole else -1), (what, g)
                # with a list: places in the rows a transform is asked for
                n_sf, rows, first, sfrow, lst = plan(H, stage, cp, n_ofdm, ports, n_rb, mask, dur, tdd, True)
                assert n_sf == len(want), what
                assert list(lst) == [2 * g * n + l for g, (need, _, _) in enumerate(want) for l in range(need)], what
                assert (np.diff(lst) > 0).all() and (lst.size == 0 or (lst[0] >= 0 and lst[-1] < n_ofdm)), what
                for g, (need, rec, whole) in enumerate(want):
                    assert (rows[g][rec:] == -1).all() and (rows[g][:rec] >= 0).all() and (rows[g][:rec] < lst.size).all(), (what, g)
                    assert list(lst[rows[g][:rec]]) == [2 * g * n + l for l in range(rec)], (what, g)
                    assert (first[g] == -1) if not need else (lst[first[g]] == 2 * g * n), (what, g)
                    assert (sfrow[g] == first[g]) if whole else (sfrow[g] == -1), (what, g)
                    if whole:
                        assert list(lst[first[g]:first[g] + 2 * n]) == list(range(2 * g * n, 2 * (g + 1) * n)), (what, g)
                n_checked += 1
    assert n_checked == 3 * 3 * 2 * 2 * 4 * (2 * n + 6) * 4


def test_the_domain_reaches_every_branch_of_the_rules(H):
    """what the sweep above must have met: a last subframe cut at every row, both values of n_ctrl_max, subframes 1 and 6 left out in
    TDD at the extended duration, a refused PHICH map, whole and cut PDSCH subframes, a special subframe that is read but not whole"""
    n_sf, rows, first, sfrow, lst = plan(H, 3, 1, 31, 2, 15, 0x3FF, 1, True, True)
    assert n_sf == 3 and list(sfrow) == [0, -1, -1] and list(first) == [0, 14, 17] and lst.size == 14 + 3 + 3 and list(rows[2]) == [17, 18, 19, -1]
    n_sf, rows, first, sfrow, lst = plan(H, 3, 1, 32, 2, 6, 0x3FF, 2, True, True)
    assert list(first) == [0, -1, 14] and list(rows[2]) == [14, 15, 16, 17] and list(sfrow) == [0, -1, -1]
    n_sf, rows, first, _, lst = plan(H, 2, 2, 27, 4, 15, 0x3FF, 1, False, True)
    assert list(first) == [-1, 0, 2] and list(lst) == [12, 13, 24, 25]          # subframe 0: m_i 2, whose map is refused
    n_sf, rows, first, _, lst = plan(H, 0, 2, 25, 4, 15, 0x3FF, 1, False, True)
    assert list(first) == [0, 2, -1] and list(lst) == [0, 1, 12, 13]            # symbol 1 of subframe 2 is row 25: outside


# ---------------------------------------------------------------- what the configurations resolve to
def resolve(H, cell, cfg, mi, rnti_mask=0, cfi_force=0, n_rb=25, own=0):
    out = np.full(16, -7, np.int32)
    arr = None if mi is None else np.array(mi, np.int32)
    what = H.wide_host_resolve(cell[0], cell[1], cfg[0], cfg[1], None if arr is None else _ip(arr), rnti_mask, cfi_force, n_rb, own, _ip(out))
    return (None if what is None else what.decode()), out


def test_shared_fields_resolve_as_the_stages_resolvers_gave_them(H):
    """the fields the launchers read (PdcchPlan / PdcchScanPlan / PhichPlan: phich_duration, phich_resource, mi, rnti_mask, cfi_force, and
    tdd for the planners and the PDSCH) over the cases of the three stages: all in cfg, all deferred to the cell, cfg over a cell that
    says otherwise; an m_i of -1 reads 1; no m_i at all is FDD"""
    cases = [(c[4], c[5], DC.mi_of(c)) for c in DC.CASES] + [(c[4], c[5], SC.mi_of(c)) for c in SC.CASES]
    cases += [(c["duration"], c["resource"], c["mi"]) for c in HC.CORNERS.values()]
    assert any(m is not None for _, _, m in cases) and {d for d, _, _ in cases} == {1, 2} and {r for _, r, _ in cases} == {1, 2, 3, 4}
    n = 0
    for dur, res, mi in cases:
        for cell, cfg in (((0, 0), (dur, res)), ((dur, res), (0, 0)), ((3 - dur, 5 - res), (dur, res)), ((dur, 0), (0, res)), ((0, res), (dur, 0))):
            for given in (mi, None if mi is None else [-1 if i % 3 == 0 else m for i, m in enumerate(mi)], None if mi is not None else [-1] * 10):
                for rnti_mask, cfi_force in ((0, 0), (5, 3), (7, 0), (1, 3)):
                    what, out = resolve(H, cell, cfg, given, rnti_mask, cfi_force)
                    assert what is None, (dur, res, given, what)
                    want_mi = [1] * 10 if given is None else [1 if m < 0 else m for m in given]
                    tdd = given is not None and any(m >= 0 for m in given)
                    assert list(out[:15]) == [dur, res] + want_mi + [int(tdd), rnti_mask or 7, cfi_force], (dur, res, given, rnti_mask, cfi_force, list(out))
                    n += 1
    assert n > 1000


# the texts as the entry points gave them before the stages shared this code
TEXT = {
    "cell": "needs a cell with n_id_1, n_id_2 and a known cp_type",
    "n_ofdm": "n_ofdm is outside 2 n_symb .. 122 n_symb (14 .. 854 normal CP, 12 .. 732 extended)",
    "mask": "needs a dl_mask with at least one of the bits 0 .. 9 and none above",
    "lte": "n_rb is not an LTE bandwidth (6, 15, 25, 50, 75 or 100)",
    "contra": "n_rb contradicts the cell's n_rb_dl",
    "unknown": "the PHICH configuration is unknown: neither cfg nor the cell says it",
    "duration": "phich_duration is outside 1 (normal) .. 2 (extended)",
    "resource": "phich_resource is outside 1 (Ng = 1/6) .. 4 (Ng = 2)",
    "cfi": "cfi_force is outside 0 .. 3",
    "cfi_ext": "the extended PHICH duration needs three control symbols: cfi_force gives fewer",
    "mi": "an m_i is outside 0 .. 2 (-1: FDD's 1)",
    "rnti": "rnti_mask is outside 0 .. 7",
}


def test_refusal_table_one_broken_rule_at_a_time(H):
    ref = lambda *a: (lambda t: None if t is None else t.decode())(H.wide_host_refusal(*a))
    # the cell
    assert ref(0, 0, 0, 1) is None and ref(0, 167, 2, 2) is None
    for bad in ((-1, 0, 1), (168, 0, 1), (0, -1, 1), (0, 3, 1), (0, 0, 0), (0, 0, 3), (0, 0, -1)):
        assert ref(0, *bad) == TEXT["cell"], bad
    # n_ofdm
    for n_symb in (6, 7):
        assert ref(1, 2 * n_symb, n_symb, 0) is None and ref(1, 122 * n_symb, n_symb, 0) is None
        assert ref(1, 2 * n_symb - 1, n_symb, 0) == ref(1, 122 * n_symb + 1, n_symb, 0) == ref(1, 0, n_symb, 0) == ref(1, -5, n_symb, 0) == TEXT["n_ofdm"]
    # the mask
    assert all(ref(2, m, 0, 0) is None for m in (1, 0x200, 0x3FF, 0x021))
    assert all(ref(2, m, 0, 0) == TEXT["mask"] for m in (0, -1, 0x400, 0x7FF, 1 << 20))
    # the bandwidth: LTE's, and the cell's where the cell says one
    for n_rb in range(0, 112):
        lte = n_rb in PR.BANDWIDTHS
        assert ref(3, 0, n_rb, 0) == (None if lte else TEXT["lte"]), n_rb
        assert ref(3, -1, n_rb, 0) == ref(3, 7, n_rb, 0) == ref(3, 0, n_rb, 0), n_rb            # a cell without a bandwidth says nothing
        for cell_rb in PR.BANDWIDTHS:
            assert ref(3, cell_rb, n_rb, 0) == (TEXT["lte"] if not lte else None if cell_rb == n_rb else TEXT["contra"]), (cell_rb, n_rb)
    # the resolver
    ok = dict(cell=(1, 3), cfg=(0, 0), mi=None)
    assert resolve(H, **ok)[0] is None
    assert resolve(H, (0, 3), (0, 0), None)[0] == resolve(H, (1, 0), (0, 0), None)[0] == resolve(H, (0, 0), (0, 0), None)[0] == TEXT["unknown"]
    assert resolve(H, (1, 3), (3, 0), None)[0] == resolve(H, (-1, 3), (0, 0), None)[0] == resolve(H, (1, 3), (-1, 0), None)[0] == TEXT["duration"]
    assert resolve(H, (1, 3), (0, 5), None)[0] == resolve(H, (1, -2), (0, 0), None)[0] == TEXT["resource"]
    assert resolve(H, cfi_force=4, **ok)[0] == resolve(H, cfi_force=-1, **ok)[0] == TEXT["cfi"]
    # 25 resource blocks: a CFI is that many symbols; up to 10 it is one more
    assert resolve(H, (2, 3), (0, 0), None, cfi_force=2)[0] == resolve(H, (1, 3), (2, 0), None, cfi_force=1)[0] == TEXT["cfi_ext"]
    assert resolve(H, (2, 3), (0, 0), None, cfi_force=3)[0] is None and resolve(H, (2, 3), (0, 0), None, cfi_force=2, n_rb=6)[0] is None
    assert resolve(H, (2, 3), (0, 0), None, cfi_force=1, n_rb=6)[0] == TEXT["cfi_ext"]
    for i in range(10):
        for bad in (-2, 3):
            assert resolve(H, (1, 3), (0, 0), [bad if k == i else 1 for k in range(10)])[0] == TEXT["mi"], (i, bad)
    assert resolve(H, rnti_mask=8, **ok)[0] == resolve(H, rnti_mask=-1, **ok)[0] == TEXT["rnti"]
    # the stage's own refusal stands behind the PHICH configuration's and before the rest, where the PDCCH checked its sizes
    assert resolve(H, own=1, **ok)[0] == "the stage's own" == resolve(H, (1, 3), (0, 0), [3] * 10, 9, 9, own=1)[0]
    assert resolve(H, (0, 0), (0, 0), None, own=1)[0] == TEXT["unknown"]


def test_every_text_stands_once_in_the_sources():
    """each string exists once: in wide_call.h, and nowhere in the entry points"""
    api = open(os.path.join(CSRC, "lcs_api.hip")).read()
    hdr = open(os.path.join(CSRC, "wide_call.h")).read()
    for key, text in TEXT.items():
        assert hdr.count('"' + text + '"') == 1 and api.count('"' + text) == 0, key


# ---------------------------------------------------------------- the sanitizer
def test_stand_alone_program_under_address_and_undefined_sanitizers(H):
    """the same source with its own main, built with -fsanitize=address,undefined: a clean exit, and the digest of every plan of the
    domain that the library form gives"""
    if stale(SAN):
        subprocess.check_call(PC.HIPCC + ["-O1", "-g", "-DWIDE_CALL_HOST_MAIN", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                                          "-fno-sanitize-recover=undefined", "-o", SAN, TWIN_SRC])
    p = subprocess.run([SAN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
    n = np.zeros(1, np.int32)
    digest = H.wide_host_sweep(_ip(n))
    assert digest != 0 and n[0] == 3 * 3 * 2 * 2 * 4 * ((2 * 6 + 6) + (2 * 7 + 6)) * 4 * 2
    tok = p.stdout.split()
    assert (int(tok[0]), int(tok[1])) == (int(n[0]), int(digest)) and int(tok[2]) > 0
