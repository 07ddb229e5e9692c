"""The host twin of the stage that combines redundancy versions (tests/host/pdsch_comb_host.cpp: pdsch_comb.h compiled for the host,
the code the kernels run) against the numpy statement of the rule (tests/pdsch_comb_ref.py), on the CPU: groups, members, statuses,
iterations, payloads and the summed streams on every scenario of tests/pdsch_comb_cases.py."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import pcfich_cases as PC
import pdsch_cases as SC
import pdsch_comb_cases as CC
from conftest import load_pkg


@pytest.fixture(scope="module")
def H():
    return CC.load_twin(load_pkg().capi)


def test_layouts(H):
    capi = load_pkg().capi
    assert H.pdsch_comb_host_record_bytes() == C.sizeof(capi.PdschCombInfo) == 2800
    assert H.pdsch_comb_host_cfg_bytes() == C.sizeof(capi.PdschCombCfg) == 16 and H.pdsch_comb_host_group_bytes() == C.sizeof(capi.PdschCombGroup) == 344


@pytest.mark.parametrize("sc", CC.SCENARIOS, ids=lambda s: s["name"])
def test_records_against_numpy(H, sc):
    """the PDSCH record as the stage's own twin test holds it; groups, members, statuses, n_iter and payloads equal; the summed
    stream values to 1e-12 of the group's largest (the bar of test_pdsch_host.py); no numpy decision near a tie"""
    capi = load_pkg().capi
    tfg, cfi, _ = CC.crafted(sc)
    _, blocks, comb = CC.reference(sc)
    pdc = CC.pdcch_twin_record(capi, sc, tfg, cfi)
    rec, crec, d = CC.twin_records(H, capi, sc, tfg, pdc, want_d=True)
    assert SC.assert_blocks_against_numpy(rec, blocks, sc["name"]) == (len(blocks), 0)
    CC.assert_groups_against_numpy(crec, comb, sc["name"])
    for i, g in enumerate(comb["groups"]):
        if g["d"] is not None:
            assert np.abs(d[i, :, :g["K"] + 4] - g["d"]).max() <= 1e-12 * max(np.abs(g["d"]).max(), 1e-300), (sc["name"], i)
    assert [x["bytes"] for x in crec.groups()] == [bytes(g["payload"][:(g["tbs"] + 7) // 8]) if g["status"] != 4 else b"" for g in comb["groups"]]
    assert [x["members"] for x in crec.groups()] == [g["members"] for g in comb["groups"]]


def test_the_stage_alone_is_the_pdsch_twins(H):
    """the PDSCH record the combining twin returns is pdsch_host's, byte for byte"""
    capi = load_pkg().capi
    sc = CC.by_name("different-grants")
    tfg, cfi, _ = CC.crafted(sc)
    pdc = CC.pdcch_twin_record(capi, sc, tfg, cfi)
    rec, _ = CC.twin_records(H, capi, sc, tfg, pdc)
    alone = SC.twin_record(SC.load_twin(capi), capi, sc["case"], tfg, pdc, cfg=CC.pdsch_cfg(capi, sc), mask=CC.mask_of(sc))
    assert bytes(rec) == bytes(alone)


def test_stand_alone_program_under_address_and_undefined_sanitizers(H, tmp_path):
    """the same source with its own main, built with -fsanitize=address,undefined: a clean exit, and what the library form gives"""
    capi = load_pkg().capi
    if CC.stale(CC.SAN):
        subprocess.check_call(PC.HIPCC + ["-O1", "-g", "-DPDSCH_COMB_HOST_MAIN", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                                          "-fno-sanitize-recover=undefined", "-o", CC.SAN, CC.TWIN_SRC])
    SH = SC.load_twin(capi)
    for name in ("different-grants", "fifth-member", "ninth-group", "silent-sum", "never-members"):
        sc = CC.by_name(name)
        tfg, cfi, _ = CC.crafted(sc)
        pdc = CC.pdcch_twin_record(capi, sc, tfg, cfi)
        rec, llr, _ = SC.twin_record(SH, capi, sc["case"], tfg, pdc, cfg=CC.pdsch_cfg(capi, sc), mask=CC.mask_of(sc), want_soft=True)
        _, want = CC.twin_records(H, capi, sc, tfg, pdc)
        path = tmp_path / "comb.bin"
        with open(path, "wb") as f:
            f.write(np.array([llr.shape[1], 8, llr.shape[0], 0], np.int32).tobytes() + bytes(CC.comb_cfg(capi, sc)) + bytes(rec) + np.ascontiguousarray(llr).tobytes())
        r = subprocess.run([CC.SAN, str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
        lines = [[int(x) for x in l.split()] for l in r.stdout.splitlines()]
        assert lines[0] == [want.n_groups, want.n_overflow, want.n_members, want.n_decoded]
        assert lines[1:] == [[g.n_members, g.rule, g.status, g.n_iter, g.n_ok_members, g.n_same, int(np.ctypeslib.as_array(g.payload).sum())]
                             for g in (want.group[i] for i in range(want.n_groups))]
