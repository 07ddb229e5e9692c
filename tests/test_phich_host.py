"""CPU tests of the PHICH rule (include/lcs.h: lcs_phich_info): phich.h compiled for the host (tests/host/phich_host.cpp) against the
numpy statement of the rule (tests/phich_ref.py) and against what the generator planted (synth.phich_region).

Noise-free crafted grids pin the rule itself: every planted indicator of amplitude 1 reads +-1 to 1e-12 with its sign at every
corner -- which fails for the j-sequences projected on the wrong axis, the PDCCH's 4-port pair rule, extended-CP odd groups on
elements 0, 1, and the PDCCH's c_init -- and a silent group beside a full one reads 0.  Noisy grids hold the twin to numpy (values
and sigma to 1e-12 of the subframe's largest, decisions equal off the thresholds), which with unequal gains per repetition fails for
repetition weights dropped from `value`.  The statistics of value / sigma, phich_index, phich_for_grants, the bindings' layout, the
generator's bit-equality without PHICH, and the twin as a stand-alone program under -fsanitize=address,undefined."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import pcfich_cases as PC
import pcfich_ref as PR
import phich_cases as HC
import phich_ref as HR
from conftest import ROOT, load_pkg

SAN = os.path.join(ROOT, "tests", "host", "phich_host_san")
TOL = 1e-12
NOISE_FREE = ["6rb_one_unit", "15rb", "25rb_4ports", "ext_cp", "ext_cp_4ports", "ext_duration", "ext_duration_4ports", "100rb_ng2_mi2", "tdd_mi_012"]


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def capi(pkg):
    return pkg.capi


@pytest.fixture(scope="module")
def H(capi):
    return HC.load_twin(capi)


# ---------------------------------------------------------------- layout
def test_record_sizes_and_offsets_agree_between_the_header_ctypes_and_the_twin(H, capi):
    o = (C.c_int32 * 12)()
    H.phich_host_layout(o)
    want = [C.sizeof(capi.PhichCfg), C.sizeof(capi.PhichSf), C.sizeof(capi.PhichHi), C.sizeof(capi.PhichInfo), capi.PhichInfo.sf.offset, capi.PhichInfo.hi.offset,
            capi.PhichHi.value.offset, capi.PhichCfg.min_amp.offset, capi.PhichSf.noise.offset, capi.PhichInfo.dl_mask.offset, capi.PHICH_MAX_ENTRIES, capi.PHICH_MAX_HI]
    assert list(o) == want == [72, 32, 24, 26928, 48, 48 + 32 * capi.PCFICH_MAX_SF, 8, 56, 24, 28, 400, 1024]
    assert (H.phich_host_default(0), H.phich_host_default(1)) == (capi.PHICH_MIN_AMP, capi.PHICH_MIN_SIGMA)
    assert capi.PHICH_MAX_GROUP == 100 and capi.PHICH_MAX_ENTRIES == 8 * 50
    cfg = capi.PhichCfg.make()
    assert (cfg.min_amp, cfg.min_sigma, list(cfg.phich_mi), cfg.tdd) == (capi.PHICH_MIN_AMP, capi.PHICH_MIN_SIGMA, [-1] * 10, False)
    assert capi.PhichCfg.make(phich_mi=capi.tdd_phich_mi(1)).tdd


# ---------------------------------------------------------------- the units
@pytest.mark.parametrize("n_rb", PR.BANDWIDTHS)
def test_unit_list_is_the_generator_s_phich_list(H, pkg, n_rb):
    """the twin's table (pdc_build_map_t's list through phi_build_map) against synth.pdcch_layout's, element by element: every Ng, both
    durations, m_i 0 / 1 / 2, 1 / 2 / 4 ports, both CPs, every n_id_cell mod 6"""
    synth, n = pkg.synth, 0
    for n_id in (0, 7, 68, 141, 256, 329):
        assert sorted(i % 6 for i in (0, 7, 68, 141, 256, 329)) == list(range(6))
        for res in (1, 2, 3, 4):
            for dur in (1, 2):
                for mi in (0, 1, 2):
                    for ports in (1, 2, 4):
                        for cp in (1, 2):
                            what = (n_rb, n_id, res, dur, mi, ports, cp)
                            n_unit, re = HC.twin_map(H, n_rb, ports, cp, n_id, dur, res, mi)
                            try:
                                _, _, regs, cols = synth.pdcch_layout(n_id, n_rb, ports, cp == 1, 3, dur == 2, res - 1, mi)
                            except ValueError:
                                assert n_unit == -1, what
                                continue
                            assert n_unit == len(regs) // 3 == HR.n_units(n_rb, res, mi), what
                            assert n_unit * (1 if cp == 1 else 2) == pkg.capi.phich_n_group(n_rb, res, cp == 1, mi) == synth.phich_n_group(n_rb, res - 1, cp == 1, mi), what
                            want = np.array([[(l << 16) | int(c) for c in cols(k, l)] for k, l in regs], np.int32).reshape(-1, 3, 4)
                            assert np.array_equal(re, want), what
                            n += 1
    assert n > 500


# ---------------------------------------------------------------- noise-free crafted grids
@pytest.mark.parametrize("name", NOISE_FREE)
def test_every_planted_indicator_reads_plus_or_minus_one(H, capi, name):
    """every (group, seq) of every subframe at amplitude 1 with a pseudo-random ACK pattern: orthogonality, scrambling, the
    extended-CP alignment, the 4-port pair rule, the axis of the j-sequences"""
    tfg, planted = HC.crafted(name, "all")
    rec, values, sigma = HC.twin_record(H, capi, name, tfg)
    ref = HC.ref_record(name, tfg)
    n_checked = 0
    for g, pat in enumerate(planted):
        if rec.sf[g].n_unit < 0:
            continue
        if pat is None:
            assert rec.sf[g].n_unit == 0 and rec.sf[g].n_present == 0, (name, g)      # U = 0: read with nothing in it
            continue
        n = pat.size
        assert rec.sf[g].n_unit * 8 == n and rec.sf[g].n_group == pat.shape[0], (name, g)
        assert np.abs(values[g][:n] - pat.reshape(-1)).max() <= TOL, (name, g, np.abs(values[g][:n] - pat.reshape(-1)).max())
        assert np.abs(ref["values"][g] - pat).max() <= TOL, (name, g)
        assert rec.sf[g].n_present == n and rec.sf[g].n_ack == int((pat < 0).sum()) and rec.sf[g].n_nack == int((pat > 0).sum()), (name, g)
        assert rec.sf[g].noise <= 1e-24, (name, g, rec.sf[g].noise)
        n_checked += n
    assert n_checked > 0
    got = [(h["subframe"], h["group"], h["seq"], h["ack"]) for h in rec.indicators()]
    want = [(g, a, b, bool(pat[a, b] < 0)) for g, pat in enumerate(planted) if pat is not None and rec.sf[g].n_unit > 0 for a in range(pat.shape[0]) for b in range(pat.shape[1])]
    assert got == want[:capi.PHICH_MAX_HI] and rec.n_dropped == len(want) - len(got) and rec.n_present == len(want)
    assert rec.ack_rate() == rec.n_ack / rec.n_present


@pytest.mark.parametrize("name", ["15rb", "25rb_4ports", "ext_cp", "ext_duration"])
def test_a_full_group_leaves_its_silent_neighbours_at_zero(H, capi, name):
    tfg, planted = HC.crafted(name, "one_group")
    rec, values, _ = HC.twin_record(H, capi, name, tfg)
    for g, pat in enumerate(planted):
        if pat is None or rec.sf[g].n_unit < 0:
            continue
        assert pat.shape[0] >= 2 and (pat[0] != 0).all() and not pat[1:].any()
        assert np.abs(values[g][:pat.size] - pat.reshape(-1)).max() <= TOL, (name, g)
        assert rec.sf[g].n_present == pat.shape[1], (name, g)


def test_the_list_is_capped_and_the_rest_counted(H, capi):
    tfg, planted = HC.crafted("100rb_ng2_mi2", "all")
    rec, _, _ = HC.twin_record(H, capi, "100rb_ng2_mi2", tfg)
    assert rec.n_present == 1600 and rec.n_hi == capi.PHICH_MAX_HI and rec.n_dropped == 1600 - 1024 and len(rec.indicators()) == 1024
    last = rec.indicators()[-1]
    assert (last["subframe"], last["group"], last["seq"]) == (2, 27, 7)      # 1024 = 2 x 400 + 224: entry 223 of subframe 2


def test_masks_grid_ends_and_refused_maps(H, capi):
    for name in ("15rb", "25rb_4ports", "ext_duration"):
        tfg, planted = HC.crafted(name, "half", n_sub=12, ragged=1)
        for mask in HC.MASKS:
            rec, values, sigma = HC.twin_record(H, capi, name, tfg, mask)
            ref = HC.ref_record(name, tfg, mask)
            HC.assert_record_close(rec, values, sigma, ref, TOL, (name, hex(mask)))
            read = [rec.sf[g].n_unit >= 0 for g in range(rec.n_sf)]
            need = HR.rows_needed(HC.CORNERS[name]["n_ports"], HC.CORNERS[name]["duration"])
            assert read == [bool((mask >> (g % 10)) & 1) and (g < 12 or need == 1) for g in range(13)], (name, hex(mask), read)
    # a map that the rule refuses: 6 resource blocks hold 8 free REGs in symbol 0, Ng = 2 with m_i 2 asks for 4 units = 12
    HC.CORNERS["refused"] = dict(n_rb=6, n_ports=2, cp=1, duration=1, resource=4, mi=[2, 1] * 5, n_id=7)
    assert HC.twin_map(H, 6, 2, 1, 7, 1, 4, 2)[0] == -1 and HC.twin_map(H, 6, 2, 1, 7, 1, 4, 1)[0] == 2
    tfg, planted = HC.crafted("refused", "all")
    rec, values, sigma = HC.twin_record(H, capi, "refused", tfg)
    assert [rec.sf[g].n_unit for g in range(4)] == [-1, 2, -1, 2] and rec.n_read == 2 and rec.n_present == 32
    HC.assert_record_close(rec, values, sigma, HC.ref_record("refused", tfg), TOL, "refused")
    # TDD at the extended duration leaves subframes 1 and 6 out
    HC.CORNERS["tdd_ext"] = dict(HC.CORNERS["ext_duration"], mi=[1] * 10)
    tfg, _ = HC.crafted("tdd_ext", "all", n_sub=8, ragged=0)
    rec, values, sigma = HC.twin_record(H, capi, "tdd_ext", tfg)
    assert [rec.sf[g].n_unit >= 0 for g in range(8)] == [True, False, True, True, True, True, False, True]
    HC.assert_record_close(rec, values, sigma, HC.ref_record("tdd_ext", tfg), TOL, "tdd_ext")


def test_grids_without_a_value(H, capi):
    for fill in (0.0, np.nan):
        tfg = np.full((30, 300), fill + 0j)
        rec, values, sigma = HC.twin_record(H, capi, "25rb_4ports", tfg)
        assert rec.n_read == 3 and rec.n_present == 0 and not values.any() and not sigma.any()
        assert all(rec.sf[g].noise == 0.0 and rec.sf[g].n_unit == 4 for g in range(3))
        HC.assert_record_close(rec, values, sigma, HC.ref_record("25rb_4ports", tfg), TOL, fill)


# ---------------------------------------------------------------- the twin against numpy on noisy grids
@pytest.mark.parametrize("name", NOISE_FREE)
def test_twin_against_numpy_on_noisy_grids(H, capi, name):
    """half of the entries planted, a channel that is not flat (the gains of the three repetitions differ: dropping the repetition
    weights from `value` moves it by far more than the tolerance), 5 dB per element"""
    near = total = 0
    for seed, amp in ((11, 1.0), (12, 0.5)):
        tfg, planted = HC.crafted(name, "half", 5.0, seed=seed, ripple=True, amp=amp)
        rec, values, sigma = HC.twin_record(H, capi, name, tfg)
        ref = HC.ref_record(name, tfg)
        assert ref["n_present"] > 0
        w, k, n = HC.assert_record_close(rec, values, sigma, ref, TOL, (name, seed))
        near, total = near + k, total + n
        # numpy alone: a planted entry is nowhere near a threshold
        for g, pat in enumerate(planted):
            if pat is None or ref["values"][g] is None:
                continue
            v, s = ref["values"][g][pat != 0], ref["sigma"][g][pat != 0]
            assert (np.abs(np.abs(v) - capi.PHICH_MIN_AMP) > 1e-9).all() and (np.abs(np.abs(v) - capi.PHICH_MIN_SIGMA * s) > 1e-9).all(), (name, seed, g)
    assert near <= 0.01 * total, (name, near, total)


# ---------------------------------------------------------------- statistics
def test_value_over_sigma_has_unit_variance_on_silent_units_in_white_noise():
    """50 resource blocks, Ng = 2: 13 units, 104 entries per subframe, so the t distribution's nu / (nu - 2) is 1.0097; 24 960 entries.
    The sampling error of a variance over that many is 0.9 %."""
    HC.CORNERS["silent50"] = dict(n_rb=50, n_ports=2, cp=1, duration=1, resource=4, mi=None, n_id=33)
    r = []
    for seed in range(4):
        tfg, planted = HC.crafted("silent50", "none", 5.0, 60, 0, seed)
        ref = HC.ref_record("silent50", tfg)
        r += [(ref["values"][g] / ref["sigma"][g]).reshape(-1) for g in range(60)]
    r = np.concatenate(r)
    assert r.size >= 20000 and np.isfinite(r).all()
    print("variance of value / sigma over %d silent entries: %.4f" % (r.size, r.var()))
    assert abs(r.var() - 1.0) <= 0.05 and abs(r.mean()) < 0.03


# ---------------------------------------------------------------- 36.213 9.1.2
def test_phich_index_by_hand_and_over_its_domain(capi):
    # 25 RB, Ng = 1: 4 groups.  I_PRB 10, n_DMRS 3: group (10 + 3) mod 4 = 1, seq (floor(10 / 4) + 3) mod 8 = 5
    assert capi.phich_index(10, 3, 4, True) == (1, 5)
    assert capi.phich_index(0, 0, 4, True) == (0, 0)
    assert capi.phich_index(24, 7, 4, True) == (3, 5)                 # (31 mod 4, (6 + 7) mod 8)
    assert capi.phich_index(24, 7, 4, True, 1) == (7, 5)              # I_PHICH = 1: the second set of groups
    assert capi.phich_index(10, 3, 8, False) == (5, 0)                # extended CP, 2 N_SF = 4: (13 mod 8, (1 + 3) mod 4)
    assert capi.phich_index(99, 7, 13, True) == (2, 6)                # 100 RB, Ng = 1: (106 mod 13, (7 + 7) mod 8)
    for cp in (True, False):
        for n_group in (1, 2, 3, 4, 7, 13, 25, 26, 50):
            for rb in range(0, 100):
                for dm in range(8):
                    grp, seq = capi.phich_index(rb, dm, n_group, cp)
                    assert 0 <= grp < n_group and 0 <= seq < (8 if cp else 4)
    for bad in ((0, 8, 4), (-1, 0, 4), (0, 0, 0)):
        with pytest.raises(ValueError):
            capi.phich_index(*bad, True)
    assert capi.phich_n_group(25, 3, True) == 4 and capi.phich_n_group(100, 4, False, 2) == 100 and capi.phich_n_group(6, 1, True) == 1
    assert capi.phich_n_group(50, 2, True) == 4 and capi.phich_n_group(15, 3, True, 0) == 0


def test_phich_for_grants_on_a_record_made_by_hand(capi):
    n_rb = 25
    size = capi.dci_1a_size(n_rb, False)
    grants = [(0, 0x1234, 10, 3), (1, 0x2345, 0, 0), (2, 0x1234, 24, 7), (5, 0x0999, 3, 1)]      # (subframe, rnti, rb_start, cyclic shift)
    scan = capi.PdcchScanInfo()
    scan.n_sf, scan.n_ports, scan.n_sizes, scan.sizes = 14, 2, 1, (size,)
    for i, (g, rnti, rb, cs) in enumerate(grants):
        m = scan.msg[i]
        m.g, m.L, m.cce, m.size_index = g, 2, 4 * i, 0
        m.d.bits, m.d.rnti_x, m.d.flags, m.d.quality = HC.format0_bits(n_rb, rb, 1, cs, size), rnti, capi.SCAN_DECODED | capi.SCAN_ACCEPTED | capi.SCAN_IN_SPACE, 0.9
        assert capi.dci_0_fields(m.d.bits, n_rb)["rb_start"] == rb and capi.dci_0_fields(m.d.bits, n_rb)["cyclic_shift"] == cs
    # a format 1A message of the same size is no uplink grant
    scan.msg[4].g, scan.msg[4].L, scan.msg[4].cce = 3, 1, 0
    scan.msg[4].d.bits, scan.msg[4].d.rnti_x, scan.msg[4].d.flags, scan.msg[4].d.quality = 1, 0x1234, 7, 0.9
    scan.n_msg = 5
    ph = capi.PhichInfo()
    ph.n_sf = 12
    for g in range(12):
        ph.sf[g].n_unit, ph.sf[g].n_group = (4, 4) if g != 9 else (-1, 0)
    for i, (g, grp, seq, fl) in enumerate([(8, 1, 5, 3), (10, 3, 5, 1)]):      # the ACK for grant 0, a NACK for grant 2
        ph.hi[i].g, ph.hi[i].group, ph.hi[i].seq, ph.hi[i].flags, ph.hi[i].value = g, grp, seq, fl, (-1.0 if fl & 2 else 1.0)
    ph.n_hi = ph.n_present = 2
    rows = capi.phich_for_grants(scan, ph, n_rb)
    assert [(r["subframe"], r["rnti"], r["phich_subframe"], r["group"], r["seq"], r["status"]) for r in rows] == [
        (0, 0x1234, 8, 1, 5, "ack"), (1, 0x2345, 9, None, None, "outside"), (2, 0x1234, 10, 3, 5, "nack"), (5, 0x0999, 13, None, None, "outside")]
    ph.sf[9].n_unit, ph.sf[9].n_group = 4, 4
    assert capi.phich_for_grants(scan, ph, n_rb)[1]["status"] == "absent" and capi.phich_for_grants(scan, ph, n_rb)[1]["group"] == 0
    ph.tdd = True
    with pytest.raises(ValueError, match="FDD only"):
        capi.phich_for_grants(scan, ph, n_rb)


# ---------------------------------------------------------------- the generator
def test_waveforms_without_phich_are_bit_equal_to_the_parent_commit_s(pkg):
    """cell_waveform_wide with phich=None at one small shape, with and without a control region: the SHA-256 of the samples as the
    commit before the PHICH produced them"""
    synth = pkg.synth
    w = synth.cell_waveform_wide(1, 52, 1, 1, 6, True, n_ports=2, rng=np.random.default_rng(5))
    assert hashlib.sha256(np.ascontiguousarray(w).tobytes()).hexdigest() == PARENT_SHA["plain"]
    dci = lambda fr, sf: [dict(rnti=0xFFFF, bits=[1, 0] * 10 + [1], L=2, cce=0)] if sf == 5 else []
    w = synth.cell_waveform_wide(1, 52, 1, 1, 6, False, n_ports=4, rng=np.random.default_rng(6), cfi=2, pdcch=dci, pdcch_fill=0.3)
    assert hashlib.sha256(np.ascontiguousarray(w).tobytes()).hexdigest() == PARENT_SHA["control"]
    # and with it the generator draws no more from rng: the load outside the PHICH's groups is the same
    a = synth.cell_waveform_wide(1, 52, 1, 2, 15, True, n_ports=2, rng=np.random.default_rng(7), cfi=1, load=0.0)
    b = synth.cell_waveform_wide(1, 52, 1, 2, 15, True, n_ports=2, rng=np.random.default_rng(7), cfi=1, load=0.0, phich=lambda fr, sf: [])
    assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        synth.cell_waveform_wide(1, 52, 1, 2, 15, phich=lambda fr, sf: [])
    with pytest.raises(ValueError):
        synth.phich_region(157, 15, 2, True, 0, 1, [dict(group=2, seq=0, ack=1)])       # 15 RB at Ng = 1 has groups 0 and 1


PARENT_SHA = {"plain": "67dc0d899cacbd97e55a45ed249496f59083e69e13d22d42e92688f5ec0dce18", "control": "667e4e302ea97ec18b0ebc7a3eac8853889c124110a85a9cb42af7823e9f015a"}


# ---------------------------------------------------------------- the sanitizer
def test_stand_alone_program_under_address_and_undefined_sanitizers(H, capi, tmp_path):
    """the same source with its own main, built with -fsanitize=address,undefined: a clean exit, and the record the library form gives"""
    if HC.stale(SAN):
        subprocess.check_call(HC.HIPCC + ["-O1", "-g", "-DPHICH_HOST_MAIN", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                                          "-fno-sanitize-recover=undefined", "-o", SAN, HC.TWIN_SRC])
    cases = [("100rb_ng2_mi2", HC.crafted("100rb_ng2_mi2", "all")[0]), ("ext_cp_4ports", HC.crafted("ext_cp_4ports", "half", 5.0, seed=11, ripple=True)[0]),
             ("ext_duration", np.full((30, 300), np.nan + 0j)), ("tdd_mi_012", HC.crafted("tdd_mi_012", "all")[0])]
    for name, tfg in cases:
        c = HC.CORNERS[name]
        tfg = np.ascontiguousarray(tfg, np.complex128)
        path = tmp_path / "grid.bin"
        hdr = np.array([tfg.shape[0], PR.n_symb_of(c["cp"]), c["n_rb"], c["n_id"], c["cp"], c["n_ports"], 0x3FF, c["duration"], c["resource"], int(c["mi"] is not None)]
                       + HC.mi_of(c), np.int32)
        with open(path, "wb") as fh:
            fh.write(hdr.tobytes()); fh.write(PC.jump_tables(c["n_rb"]).tobytes()); fh.write(tfg.tobytes())
        p = subprocess.run([SAN, str(path)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and not p.stderr, (name, p.returncode, p.stderr[-2000:])
        rec, _, _ = HC.twin_record(H, capi, name, tfg)
        tok = p.stdout.split()
        assert [int(t) for t in tok[:7]] == [rec.n_sf, rec.n_read, rec.n_present, rec.n_ack, rec.n_nack, rec.n_hi, rec.n_dropped], name
        for g in range(rec.n_sf):
            assert (int(tok[7 + 3 * g]), int(tok[8 + 3 * g]), float(tok[9 + 3 * g])) == (rec.sf[g].n_unit, rec.sf[g].n_present, rec.sf[g].noise), (name, g)
