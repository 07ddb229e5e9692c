"""The PDCCH rule's reference pinned where it shares arithmetic with the PBCH -- whose decoder the oracle checks -- and plant and
recover on the CPU: the generator's PDCCH (synth.cell_waveform_wide(pdcch=...)) through synth.make_wideband_cell at 10 dB, the numpy
grid (tests/meas_wide_ref.py) and the numpy statement of the rule (tests/pdcch_ref.py).  The decoder's reference is checked against
planted values, not against itself; the generator (synth.pdcch_layout, its own enumeration) against pdcch_ref.layout.

Pins: the generic de-rate-matching list at K = 40 equals the PBCH's table (tests/test_pbch_host.py pins that to the oracle);
CRC + encoder + rate matching at A = 24, RNTI 0 give synth.pbch_symbols' bit stream; the Gold bits equal the oracle's; the PCFICH's
four REGs are REGs of the enumeration.  The DCI sizes against their formula."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import meas_wide_ref as WR
import oracle as O
import pcfich_ref as PR
import pdcch_cases as DC
import pdcch_ref as DR
from conftest import load_pkg

FS = 1.92e6


@pytest.fixture(scope="module")
def H():
    return DC.load_twin(load_pkg().capi)


@pytest.mark.parametrize("n_e", [1920, 1728])
def test_generic_derm_list_at_40_steps_is_the_pbch_table(H, n_e):
    lib = os.path.join(DC.ROOT, "tests", "host", "libpbch_host.so")
    if not os.path.exists(lib):                              # (tests/test_pbch_host.py's build of its twin)
        import pcfich_cases as PC
        subprocess.check_call(PC.HIPCC + ["-O2", "-fPIC", "-shared", "-o", lib, os.path.join(DC.ROOT, "tests", "host", "pbch_host.cpp")])
    P = C.CDLL(lib)
    P.pbch_host_derm_inv.argtypes = [C.c_int, C.POINTER(C.c_int16)]
    want, got = np.full((120, 16), -7, np.int16), np.full((120, 16), -9, np.int16)
    assert P.pbch_host_derm_inv(n_e, want.ctypes.data_as(C.POINTER(C.c_int16))) == 1
    assert H.pdcch_host_derm(40, n_e, 16, got.ctypes.data_as(C.POINTER(C.c_int16))) == 1
    assert np.array_equal(got, want)


def test_dci_coding_at_24_bits_and_rnti_0_is_the_pbch_bit_stream():
    synth = load_pkg().synth
    for n_id, cp_normal in ((0, True), (277, False)):
        a = synth.mib_bits(25, 1, 2, 372)
        n_e = 1920 if cp_normal else 1728
        # pdcch_ref's and synth's DCI coders agree with each other on 72 L bits, and their chain with the PBCH's on its length
        for L in (4, 8):
            assert np.array_equal(DR.dci_codeword(a, 0, L), synth.dci_bits(a, 0, L))
        c = np.concatenate([a, np.array([(DR.crc16_int(a) >> (15 - t)) & 1 for t in range(16)], np.uint8)])
        e = synth.conv_ratematch(synth.conv_encode_tailbite(c), n_e) ^ synth._pn(n_id, n_e)
        s = synth.pbch_symbols(n_id, 1, 25, 1, 2, 372, cp_normal)
        bits = np.empty(n_e, np.uint8)
        bits[0::2], bits[1::2] = s.real < 0, s.imag < 0
        assert np.array_equal(bits, e)
        assert np.array_equal(DR.dci_codeword(a, 0, 4), synth.conv_ratematch(synth.conv_encode_tailbite(c), 288))
    # the RNTI goes on the parity bits MSB first
    a = np.array([1, 0, 1, 1, 0, 0, 1, 0], np.uint8)
    for rnti in (0x8000, 0x0001, 0xFFFE):
        d = synth.crc16(a) ^ np.array([(rnti >> (15 - t)) & 1 for t in range(16)], np.uint8)
        assert DR.crc16_int(a) ^ sum(int(b) << (15 - t) for t, b in enumerate(d)) == rnti


def test_gold_bits_match_the_oracle():
    for n_id, sf in ((0, 0), (503, 9), (141, 4)):
        assert np.array_equal(DR.scrambling(n_id, sf, 1152), np.asarray(O.lte_pn(sf * 512 + n_id, 1152)).astype(np.int64))


def test_pcfich_regs_are_regs_of_the_enumeration_and_the_generator_agrees():
    synth = load_pkg().synth
    for n_rb in PR.BANDWIDTHS:
        for n_id in (0, 7, 68, 141, 256, 329, 503):
            cols = PR.columns(n_id, n_rb)
            regs0 = DR.symbol_regs(0, n_rb, 2, 1)
            for i in range(4):
                k = int(cols[4 * i]) // 6 * 6
                assert k in regs0 and list(cols[4 * i:4 * i + 4]) == DR.reg_columns(k, 0, n_id, 2, 1)
                assert (k, 0) in DR.layout(n_id, 1, 2, n_rb, 1, 1, 3)["pcfich"]
    for n_id, cp, ports, n_rb, cfi, dur, res in ((7, 1, 2, 6, 2, 1, 3), (503, 2, 4, 15, 3, 2, 1), (256, 1, 1, 25, 1, 1, 4), (68, 2, 4, 6, 3, 2, 2), (141, 1, 4, 100, 2, 1, 2)):
        regs, n_cce, phich, cols = synth.pdcch_layout(n_id, n_rb, ports, cp == 1, cfi, dur - 1, res - 1)
        lay = DR.layout(n_id, cp, ports, n_rb, cfi, dur, res)
        assert regs == lay["order"] and n_cce == lay["n_cce"] and phich == lay["phich"]
        assert all(list(cols(k, l)) == DR.reg_columns(k, l, n_id, ports, cp) for k, l in regs)
        assert np.array_equal(synth.pdcch_interleave(len(regs)), DR.interleave(len(regs)))
    # m_i of a TDD subframe: no PHICH at all, and twice FDD's
    for mi in (0, 2):
        regs, n_cce, phich, _ = synth.pdcch_layout(141, 25, 2, True, 2, 0, 2, mi)
        lay = DR.layout(141, 1, 2, 25, 2, 1, 3, mi)
        assert regs == lay["order"] and phich == lay["phich"] and len(phich) == 3 * 4 * mi and n_cce == lay["n_cce"]


def test_dci_sizes_and_the_tdd_table():
    capi = load_pkg().capi
    amb = (12, 14, 16, 20, 24, 26, 32, 40, 44, 56)
    for n_rb, row in zip(PR.BANDWIDTHS, ((21, 23, 8), (22, 25, 10), (25, 27, 12), (27, 29, 13), (27, 30, 14), (28, 31, 15))):
        for tdd in (False, True):
            a = 15 + int(np.ceil(np.log2(n_rb * (n_rb + 1) / 2))) + (3 if tdd else 0)
            a += a in amb
            assert capi.dci_common_sizes(n_rb, tdd) == (a, row[2]) == (row[1 if tdd else 0], row[2]) and capi.dci_1a_size(n_rb, tdd) == a
    gap = {6: 3, 15: 8, 25: 12, 50: 27, 75: 32, 100: 48}
    for n_rb in PR.BANDWIDTHS:
        v = 2 * min(gap[n_rb], n_rb - gap[n_rb]) // (2 if n_rb < 50 else 4)
        assert capi.dci_common_sizes(n_rb)[1] == (1 if n_rb >= 50 else 0) + int(np.ceil(np.log2(v * (v + 1) / 2))) + 5
    up = {0: (2, 3, 4, 7, 8, 9), 1: (2, 3, 7, 8), 2: (2, 7), 3: (2, 3, 4), 4: (2, 3), 5: (2,), 6: (2, 3, 4, 7, 8)}
    for cfg in range(7):
        mi = capi.tdd_phich_mi(cfg)
        assert len(mi) == 10 and tuple(i for i, m in enumerate(mi) if m is None) == up[cfg] and all(m in (0, 1, 2) for m in mi if m is not None)
    assert capi.tdd_phich_mi(0)[:2] == [2, 1] and capi.PdcchCfg.make((21, 8), phich_mi=capi.tdd_phich_mi(0)).phich_mi[2] == 0
    # the fields of 1A, there and back
    for n_rb in PR.BANDWIDTHS:
        for frame, sf in ((0, 0), (1, 3), (2, 9), (5, 6)):
            f = DC.fields_1a(frame, sf, n_rb)
            got = capi.dci_1a_fields(sum(b << t for t, b in enumerate(DC.pack_1a(f, n_rb))), n_rb)
            assert {k: got[k] for k in f} == f, (n_rb, frame, sf)


@pytest.mark.parametrize("shape", DC.CAP_SHAPES, ids=str)
def test_planted_dcis_are_recovered_through_the_samples(shape):
    R, n_rb, cp, ports = shape
    capi = load_pkg().capi
    x, frame_start = DC.pdcch_capture(*shape)
    n, n_id = PR.n_symb_of(cp), DC.CAP_ID[1] + 3 * DC.CAP_ID[0]
    n_sf = 15
    n_ofdm = 2 * n * n_sf
    rows = [2 * g * n + l for g in range(n_sf) for l in range(4)]
    tfg = WR.grid(x, frame_start, 0.0, cp, DC.CAP_FC, DC.CAP_FC, FS * R, 128 * R, n_rb, n_ofdm, rows)[0]
    cfi = PR.decode(tfg, n_id, cp, ports, n_rb)["cfi"]
    assert list(cfi) == [DC.capture_cfi(1 + g // 10, g % 10) for g in range(n_sf)]
    sizes = capi.dci_common_sizes(n_rb)
    ref = DR.receive(tfg, n_id, cp, ports, n_rb, cfi, 1, 3, sizes)
    planted = DC.capture_planted(n_rb, cp, ports, n_sf)
    assert len(planted) >= 7
    extra = sum(bool(d["flags"] & 2) for d in ref["dec"].values())
    for p in planted:
        d = ref["dec"][(p["g"], p["slot"], p["i"])]
        assert (d["bits"], d["rnti_x"], d["flags"]) == (p["bits"], p["rnti"], 3), (shape, p, d)
        extra -= 1
        if p["i"] == 0:
            f = capi.dci_1a_fields(d["bits"], n_rb)
            assert {k: f[k] for k in DC.fields_1a(1 + p["g"] // 10, p["g"] % 10, n_rb)} == DC.fields_1a(1 + p["g"] // 10, p["g"] % 10, n_rb)
    print(shape, "planted %d, all found; other accepted decodes (L = 4 inside an L = 8, fill, noise): %d of %d" % (len(planted), extra, len(ref["dec"]) - len(planted)))
    # another cell's identity finds none of them
    other = DR.receive(tfg, n_id + 6, cp, ports, n_rb, cfi, 1, 3, sizes)
    assert not any(other["dec"].get((p["g"], p["slot"], p["i"]), dict(flags=0))["flags"] & 2 and other["dec"][(p["g"], p["slot"], p["i"])]["bits"] == p["bits"] for p in planted)


def test_generator_without_pdcch_is_what_it_was():
    synth = load_pkg().synth
    args = (2, 41, 2, 2, 15)
    for cp_normal, n_ports, tdd in ((True, 2, None), (False, 4, None), (True, 1, (1, 9))):
        a = synth.cell_waveform_wide(*args, cp_normal, n_ports=n_ports, rng=np.random.default_rng(5), tdd=tdd, cfi=DC.capture_cfi)
        b = synth.cell_waveform_wide(*args, cp_normal, n_ports=n_ports, rng=np.random.default_rng(5), tdd=tdd, cfi=DC.capture_cfi, pdcch=None, pdcch_fill=0.7)
        assert a.tobytes() == b.tobytes()
    with pytest.raises(ValueError):
        synth.cell_waveform_wide(*args, pdcch=lambda f, s: [])
