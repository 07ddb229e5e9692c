"""pdcch.h and the length-n tail-biting decoder compiled for the HOST -- the __host__ __device__ code k_pdcch_llr, k_pdcch_dec and
k_pdcch_fin run, and the very functions that build the kernels' tables -- against the numpy statement of the rule
(tests/pdcch_ref.py) on crafted grids with planted PCFICH and PDCCH (tests/pdcch_cases.py).

Bars: soft bits to 1e-12 of the subframe's largest |soft bit| (the project's bar for a host twin of an fp64 sum); maps, lists and
every integer equal; quality to 1e-12 (a ratio of order one).  Every planted candidate decodes to its bits, its RNTI and `accepted`.
An unplanted candidate (noise, fill) is compared bit for bit unless numpy's best and second-best start states lie within 1e-9 of
sum |coded bit|: at most 1 % of the unplanted decodes, and never a planted one.  The length-n decoder at n = 40 returns the PBCH
forms' bits and end metrics exactly, on the de-rate-matched PBCH bits of tests/pbch_cases.py.  The same source is built once more as
a stand-alone program with -fsanitize=address,undefined: nothing is loaded into Python under a sanitizer."""
import ctypes as C
import itertools
import subprocess

import numpy as np
import pytest

import pcfich_cases as PC
import pcfich_ref as PR
import pdcch_cases as DC
import pdcch_ref as DR
from conftest import load_pkg

TOL = 1e-12
_dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))


@pytest.fixture(scope="module")
def capi():
    return load_pkg().capi


@pytest.fixture(scope="module")
def H(capi):
    return DC.load_twin(capi)


def test_the_case_set_covers_what_it_says():
    cases = DC.CASES
    assert {c[0] % 6 for c in cases} == set(range(6)) and {c[2] for c in cases} == {1, 2, 4} and {c[1] for c in cases} == {1, 2}
    assert {c[3] for c in cases} == {6, 15, 25} and {c[5] for c in cases} == {1, 2, 3, 4} and {c[4] for c in cases} == {1, 2}
    seen, kinds, cfis, beyond = set(), set(), set(), False
    for case in cases:
        tfg, cfi, planted = DC.crafted(case)
        ref = DC.reference(case)
        assert ref["n_sf"] == DC.N_SF and tfg.shape[1] == 12 * case[3]
        cfis |= {(case[3] <= 10, int(c)) for c in ref["cfi"] if c}
        beyond = beyond or any(case[0] > n > 0 for n in ref["n_reg"])
        for p in planted:
            seen.add((p["slot"], p["i"]))
            kinds.add("si" if p["rnti"] == 0xFFFF else "paging" if p["rnti"] == 0xFFFE else "ra" if p["rnti"] <= 60 else "other")
        assert not any(p["g"] == DC.SILENT_SF for p in planted)
    assert seen == set(itertools.product(range(6), range(2))), "a DCI of both sizes in every slot (so at both levels)"
    assert kinds == {"si", "paging", "ra", "other"} and beyond
    assert {c for small, c in cfis if not small} == {1, 2, 3} and {c for small, c in cfis if small} >= {2, 3}


def test_maps_equal_numpy_for_every_configuration(H):
    """REG sets, PHICH positions, the PDCCH's order, N_REG against the closed form, the quadruplet -> element table; refused alike"""
    n_maps = 0
    for n_rb, ports, cp, cfi, res, dur in itertools.product(PR.BANDWIDTHS, (1, 2, 4), (1, 2), (1, 2, 3), (1, 2, 3, 4), (1, 2)):
        for n_id, mi in ((0, 1), (503, 1), (257, 2 if res < 4 else 0)):
            if n_id and n_rb in (50, 75):
                continue                                     # (every bandwidth with id 0; the other ids at the smallest and the largest)
            lay = DR.layout(n_id, cp, ports, n_rb, cfi, dur, res, mi)
            m = DC.twin_map(H, n_rb, ports, cp, n_id, dur, res, mi, cfi)
            what = (n_rb, ports, cp, cfi, res, dur, n_id, mi)
            assert (lay is None) == (m is None), what
            if lay is None:
                assert dur == 2 and DR.n_ctrl_of(cfi, n_rb) < 3 or (n_rb == 6 and mi == 2), what
                continue
            n_maps += 1
            assert m["pcfich"] == lay["pcfich"] and m["phich"] == lay["phich"] and m["order"] == lay["order"], what
            assert (m["n_reg"], m["n_cce"]) == (lay["n_reg"], lay["n_cce"]) and lay["n_reg"] == DR.n_reg_closed_form(cp, ports, n_rb, cfi, res, mi), what
            # the three kinds are disjoint REGs of the enumeration, and together they are all of it
            every = {(k, l) for l in range(DR.n_ctrl_of(cfi, n_rb)) for k in DR.symbol_regs(l, n_rb, ports, cp)}
            parts = lay["pcfich"] + lay["phich"] + lay["order"]
            assert len(set(parts)) == len(parts) and set(parts) == every, what
            # the table: element j of quadruplet q sits where numpy puts it
            q = DR.quad_of_reg(lay["n_reg"], n_id)
            assert sorted(q) == list(range(lay["n_reg"])), what
            want = np.full(576, -1, np.int64)
            for i, (k, l) in enumerate(lay["order"]):
                if q[i] < min(144, 9 * lay["n_cce"]):
                    want[4 * q[i]:4 * q[i] + 4] = [(l << 16) | c for c in DR.reg_columns(k, l, n_id, ports, cp)]
            assert np.array_equal(m["re"], want), what
            cols = m["re"][m["re"] >= 0]
            assert len(set(cols)) == cols.size and ((cols & 0xFFFF) < 12 * n_rb).all() and ((cols >> 16) < DR.n_ctrl_of(cfi, n_rb)).all(), what
    print("maps compared:", n_maps)
    # known figures of the standard: 2 ports, normal CP, Ng = 1
    for n_rb, want in ((50, (8, 25, 41)), (100, (17, 50, 84))):
        assert tuple(DC.twin_map(H, n_rb, 2, 1, 0, 1, 3, 1, cfi)["n_cce"] for cfi in (1, 2, 3)) == want


def test_interleaver_is_a_bijection_and_equals_numpy(H):
    for n in (1, 23, 31, 32, 33, 58, 64, 113, 160, 799, 800):
        w = np.zeros(n, np.int32)
        H.pdcch_host_interleave(n, w.ctypes.data_as(C.POINTER(C.c_int32)))
        assert sorted(w) == list(range(n)) and np.array_equal(w, DR.interleave(n)), n
    assert list(DR.interleave(32)) == DR.PERM


def test_candidate_slots(H):
    for n_cce in range(0, 90):
        got = []
        for s in range(6):
            L, cce = C.c_int32(), C.c_int32()
            if H.pdcch_host_slot(s, n_cce, C.byref(L), C.byref(cce)):
                got.append((s, L.value, cce.value))
        assert got == DR.candidates(n_cce), n_cce
    # 15 RB, Ng = 1/6, CFI 3: 12 CCE -> three L = 4 candidates and one L = 8; 6 RB, CFI 1: 2 CCE -> none
    m = DC.twin_map(H, 15, 2, 1, 0, 1, 1, 1, 3)
    assert m["n_cce"] == 12 and [(L, c) for _, L, c in DR.candidates(12)] == [(4, 0), (4, 4), (4, 8), (8, 0)]
    m = DC.twin_map(H, 6, 2, 1, 0, 1, 3, 1, 1)
    assert m["n_cce"] == 2 and DR.candidates(2) == []


def test_derm_lists_equal_numpy(H):
    for A in (8, 13, 21, 22, 25, 27, 31, 48):
        for E in (288, 576):
            K = A + 16
            out = np.full((3 * K, 8), -7, np.int16)
            assert H.pdcch_host_derm(K, E, 8, out.ctypes.data_as(C.POINTER(C.c_int16))) == 1
            for b, pos in enumerate(DR.derm_lists(K, E)):
                assert np.array_equal(out[b, :pos.size], pos) and (out[b, pos.size:] == -1).all(), (A, E, b)
    out = np.zeros((72, 7), np.int16)
    assert H.pdcch_host_derm(24, 576, 7, out.ctypes.data_as(C.POINTER(C.c_int16))) == 0          # eight positions do not fit seven


def test_scrambling_and_rnti(H):
    pn = load_pkg().synth._pn
    jump = PC.jump_tables(6)[32:].copy()
    for n_id, sf in ((0, 0), (1, 3), (277, 9), (503, 5)):
        words = np.zeros(36, np.uint32)
        H.pdcch_host_scramble(sf, n_id, jump.ctypes.data_as(C.POINTER(C.c_uint32)), words.ctypes.data_as(C.POINTER(C.c_uint32)))
        assert [(int(words[i >> 5]) >> (i & 31)) & 1 for i in range(1152)] == list(pn(sf * 512 + n_id, 1152))
    rng = np.random.default_rng(3)
    synth = load_pkg().synth
    for A, rnti in ((8, 0xFFFF), (21, 0xFFFE), (27, 0x0001), (48, 0x8001), (31, 0x003C)):
        a = rng.integers(0, 2, A)
        c = np.concatenate([a, synth.crc16(a) ^ np.array([(rnti >> (15 - t)) & 1 for t in range(16)], np.uint8)])
        assert H.pdcch_host_rnti_x(sum(int(b) << t for t, b in enumerate(c)), A) == rnti          # the RNTI's MSB on the first parity bit


def test_length_n_decoder_at_40_steps_is_the_pbch_decoder_bit_for_bit(H):
    import pbch_cases as BC
    names = [n for n in BC.NAMES if BC.CASES[n]["kind"] == "crafted"]
    n_run = 0
    for name in names:
        d_all = BC.oracle_soft(name)[1]
        for k in range(0, d_all.shape[0], 3):
            d = np.ascontiguousarray(d_all[k], np.float64).reshape(-1)
            res = []
            for form in (0, 1):
                end, bits, e2 = np.zeros(64), C.c_uint64(), C.c_double()
                ss = H.pdcch_host_vit(_dp(d), 40, form, _dp(end), C.byref(bits), C.byref(e2))
                res.append((ss, bits.value, e2.value, end.tobytes()))
            assert res[0] == res[1], (name, k)
            n_run += 1
    assert n_run >= 40
    # ... and at every other length it returns a codeword's bits with the end metric -sum |d|, ties and all-zero input included
    synth, rng = load_pkg().synth, np.random.default_rng(11)
    for n in range(24, 65):
        c = rng.integers(0, 2, n)
        d = (1.0 - 2.0 * synth.conv_encode_tailbite(c)) * (0.5 + rng.random((3, n)))
        end, bits, e2 = np.zeros(64), C.c_uint64(), C.c_double()
        ss = H.pdcch_host_vit(_dp(np.ascontiguousarray(d).reshape(-1)), n, 0, _dp(end), C.byref(bits), C.byref(e2))
        assert [(bits.value >> t) & 1 for t in range(n)] == list(c) and ss == int(sum(int(b) << (5 - j) for j, b in enumerate(c[-6:][::-1]))), n
        assert abs(e2.value + np.abs(d).sum()) <= 1e-12 * np.abs(d).sum() and e2.value == end[ss] == end.min(), n
        nb, ne = DR.viterbi_tailbite(d)
        assert list(nb) == list(c) and np.allclose(ne, end, rtol=1e-12, atol=1e-12), n
        ss = H.pdcch_host_vit(_dp(np.zeros(3 * n)), n, 0, _dp(end), C.byref(bits), C.byref(e2))
        assert (ss, bits.value, e2.value) == (0, 0, 0.0) and not end.any(), n


@pytest.mark.parametrize("case", DC.CASES, ids=DC.case_id)
def test_twin_against_numpy_on_crafted_grids(H, capi, case):
    tfg, cfi, planted = DC.crafted(case)
    ref = DC.reference(case)
    o, llr = DC.twin_record(H, capi, case, tfg, cfi, want_llr=True)
    worst_llr = 0.0
    for g, want in ref["llr"].items():
        scale = np.abs(want).max()
        assert scale > 0
        worst_llr = max(worst_llr, np.abs(llr[g] - want).max() / scale)
    assert worst_llr <= TOL, worst_llr
    worst, n, excused = DC.assert_record_against_numpy(o, ref, planted, TOL, DC.case_id(case))
    assert (o.n_accepted, o.n_si, o.n_paging, o.n_ra) == (ref["n_accepted"], ref["n_si"], ref["n_paging"], ref["n_ra"]) or excused
    assert (o.dl_mask, o.n_rb, o.n_ports) == (DC.dl_mask_of(case), case[3], case[2])
    assert len(planted) >= 3 and ref["n_read"] >= 3          # (the TDD case with the extended duration reads subframes 0, 5, 10 alone)
    # messages(): every planted DCI of the set once, with its fields
    msgs = {(m["subframe"], m["cce"], m["size"], m["bits"], m["rnti"]) for m in o.messages()}
    sizes = DC.sizes_of(case)
    for p in planted:
        if p["rnti"] != 0x1234:
            assert (p["g"], p["cce"], sizes[p["i"]], p["bits"], p["rnti"]) in msgs, p
    print(DC.case_id(case), "worst soft bit %.2e, worst quality %.2e, %d decodes, %d excused, %d planted" % (worst_llr, worst, n, excused, len(planted)))


def test_numpy_ties_stay_under_one_percent_of_the_unplanted_decodes():
    n_un, n_tie = 0, 0
    for case in DC.CASES:
        planted = {(p["g"], p["slot"], p["i"]) for p in DC.crafted(case)[2]}
        for key, d in DC.reference(case)["dec"].items():
            if key in planted:
                assert d["gap"] > 1e-9, (case, key)
            elif d["flags"] & 1:
                n_un += 1
                n_tie += d["gap"] <= 1e-9
    print("unplanted decodes %d, of them within 1e-9: %d" % (n_un, n_tie))
    assert n_un > 500 and n_tie <= 0.01 * n_un


def test_a_silent_candidate_decodes_to_zeros_and_is_never_accepted(H, capi):
    case = DC.CASES[4]
    cfg = DC.make_cfg(capi, case, cfi_force=3)
    o = DC.twin_record(H, capi, case, np.zeros((44, 180), np.complex128), np.zeros(4, np.int32), cfg=cfg)
    ent = list(o.entries())
    assert o.n_sf == 4 and o.n_read == 3 and o.n_accepted == 0 and len(ent) == 3 * 4 * 2          # 12 CCE: three L = 4 slots and one L = 8
    assert all((d.bits, d.rnti_x, d.flags, d.quality) == (0, 0, 1, 0.0) for _, _, _, d in ent) and o.messages() == []
    # values that are not finite: no entry at all
    o = DC.twin_record(H, capi, case, np.full((44, 180), np.nan + 0j), np.zeros(4, np.int32), cfg=cfg)
    assert o.n_read == 3 and list(o.entries()) == []
    # without cfi_force and without a PCFICH decision nothing is read
    o = DC.twin_record(H, capi, case, np.zeros((44, 180), np.complex128), np.zeros(4, np.int32))
    assert o.n_read == 0 and not o.cfi.any() and list(o.entries()) == []


def test_record_size_and_layout(H, capi):
    P = capi.PdcchInfo
    assert C.sizeof(P) == 21640 == H.pdcch_host_record_bytes() and C.sizeof(capi.PdcchCfg) == 68 == H.pdcch_host_cfg_bytes()
    want = dict(n_sf=0, n_read=4, n_accepted=8, n_si=12, n_paging=16, n_ra=20, dl_mask=24, n_rb=28, n_ports=32, _cfi=40, _n_reg=328, _n_cce=616, dec=904)
    assert {k: getattr(P, k).offset for k in want} == want
    assert {k: getattr(capi.PdcchDec, k).offset for k in ("bits", "rnti_x", "flags", "quality")} == dict(bits=0, rnti_x=8, flags=12, quality=16)
    # messages(): a DCI found at L = 8 and at L = 4 from the same first CCE is listed once, the better quality kept
    o = P()
    o.n_sf, o.sizes = 2, (21, 8)
    for slot, q in ((2, 0.5), (5, 0.75)):
        d = o.dec[1][slot][0]
        d.bits, d.rnti_x, d.flags, d.quality = 0x155, 0xFFFF, 3, q
    o.dec[1][0][1].bits, o.dec[1][0][1].rnti_x, o.dec[1][0][1].flags = 3, 0x1234, 1
    m = o.messages()
    assert m == [dict(subframe=1, L=8, cce=8, kind="si", rnti=0xFFFF, size=21, bits=0x155, quality=0.75)]


def test_stand_alone_program_under_address_and_undefined_sanitizers(H, capi, tmp_path):
    """the same source with its own main, built with -fsanitize=address,undefined: a clean exit, and the record the library form gives"""
    if DC.stale(DC.SAN):
        subprocess.check_call(PC.HIPCC + ["-O1", "-g", "-DPDCCH_HOST_MAIN", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                                          "-fno-sanitize-recover=undefined", "-o", DC.SAN, DC.TWIN_SRC])
    runs = [(DC.CASES[i], None) for i in (0, 2, 5, 9, 13)] + [(DC.CASES[4], np.full((45, 180), np.nan + 0j))]
    for case, grid in runs:
        tfg, cfi, _ = DC.crafted(case)
        tfg = tfg if grid is None else grid
        n_id, cp, ports, n_rb = case[:4]
        cfg = DC.make_cfg(capi, case)
        cfi72 = np.concatenate([cfi, np.zeros(72, np.int32)])[:72].astype(np.int32)
        path = tmp_path / "grid.bin"
        with open(path, "wb") as f:
            f.write(np.array([tfg.shape[0], PR.n_symb_of(cp), n_rb, n_id, cp, ports, DC.dl_mask_of(case), 0], np.int32).tobytes() + PC.jump_tables(n_rb).tobytes() +
                    bytes(cfg) + cfi72.tobytes() + np.ascontiguousarray(tfg, np.complex128).tobytes())
        r = subprocess.run([DC.SAN, str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
        v = r.stdout.split()
        o = DC.twin_record(H, capi, case, tfg, cfi)
        assert [int(x) for x in v[:6]] == [o.n_sf, o.n_read, o.n_accepted, o.n_si, o.n_paging, o.n_ra]
        per = [x for g in range(o.n_sf) for s in range(6) for i in range(2) for x in (float(o.dec[g][s][i].bits), float(o.dec[g][s][i].rnti_x), float(o.dec[g][s][i].flags), o.dec[g][s][i].quality)]
        assert [float(x) for x in v[6:]] == per
