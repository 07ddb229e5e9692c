"""GPU tests of what the stages on the full-bandwidth grid share in lcs_api.hip (one source type, one prologue, one row planner,
one jump-table helper): every stage from samples against the same stage on lcs_extract_tfg_wide's grid, the stages beside each other
on one context, and a call that breaks two rules at once.  Every case is a synthetic cell of 6 resource blocks at n_fft = 128.

Records are compared byte for byte, as tests/test_gpu_pcfich.py's from-samples test compares: every stage's own GPU test already
holds its sample entry to its host-grid entry that way, so the stages are reproducible from run to run."""
import ctypes as C

import numpy as np
import pytest

import meas_wide_cases as WC
import phich_cases as HC
from conftest import load_pkg

pytestmark = pytest.mark.gpu
FS, FC, N_FFT, N_RB = 1.92e6, WC.FC, 128, 6
# (CP type, ports, n_ofdm, mask): two whole subframes with the normal CP; a third subframe cut after three rows with the extended
# CP; each under the full mask and under subframe 0's bit alone; four ports once, so that symbol 1 is planned
CASES = [(1, 2, 28, 0x3FF), (1, 2, 28, 0x001), (2, 2, 27, 0x3FF), (2, 2, 27, 0x001), (1, 4, 28, 0x3FF)]


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def S(pkg):
    s = pkg.Searcher(0)
    yield s
    s.close()


_dev = {}


def dev(cp, ports):
    """a capture with the generator's PCFICH and PHICH in every subframe (phich_cases.phich_capture), on the device"""
    import torch
    if (cp, ports) not in _dev:
        _dev[cp, ports] = torch.from_numpy(np.ascontiguousarray(HC.phich_capture(1, N_RB, cp, ports))).cuda()
    return _dev[cp, ports]


def _cell(pkg, cp, ports, n_rb_dl=N_RB):
    c = pkg.new_cell(n_id_1=WC.CELL_ID[0], n_id_2=WC.CELL_ID[1], cp_type=cp, n_ports=ports, freq_fine=0.0, frame_start=float(WC.FRAME_START))
    c.n_rb_dl = n_rb_dl
    c.phich_duration, c.phich_resource = 1, 3
    return c


def _scan_cfg(capi, ports):
    ue = capi.dci_ue_sizes(N_RB, ports)
    return capi.PdcchScanCfg.make((ue["0/1A"], ue["1"]))


def _same(a, b, what):
    a, b = bytes(a), bytes(b)
    assert a == b, (what, np.flatnonzero(np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8))[:8])


# ---------------------------------------------------------------- case 1: the sample entry against the host-grid entry
@pytest.mark.parametrize("case", CASES, ids=["cp%d-p%d-n%d-m%03x" % c for c in CASES])
def test_every_stage_from_samples_equals_the_stage_on_the_extracted_grid(pkg, S, case):
    cp, ports, n_ofdm, mask = case
    capi, d, cell = pkg.capi, dev(cp, ports), _cell(pkg, cp, ports)
    wide = (cell, d, FC, FC, FS, N_FFT, N_RB, n_ofdm, mask)
    tfg, ts = S.extract_tfg_wide(*wide[:-1])
    assert tfg.shape == (n_ofdm, 12 * N_RB) and np.isfinite(tfg.view(np.float64)).all() and (np.diff(ts) > 0).all()
    n_sf = -(-n_ofdm // (12 if cp == 2 else 14))
    pc = S.pcfich_wide(*wide)
    _same(pc, S.pcfich(cell, tfg, N_RB, mask), ("pcfich", case))
    read = [bool((mask >> g) & 1) for g in range(n_sf)]
    assert pc.n_sf == n_sf and [c > 0 for c in pc.cfi[:n_sf]] == read, (case, list(pc.cfi[:n_sf]))
    pd = S.pdcch_wide(*wide)
    _same(pd, S.pdcch(cell, tfg, N_RB, mask), ("pdcch", case))
    # 6 resource blocks: four control symbols, so the cut subframe (three rows) is not read
    assert pd.n_sf == n_sf and [c > 0 for c in pd.cfi[:n_sf]] == [r and 2 * g * (6 if cp == 2 else 7) + 3 < n_ofdm for g, r in enumerate(read)], (case, list(pd.cfi[:n_sf]))
    cfg = _scan_cfg(capi, ports)
    sc = S.pdcch_scan_wide(*wide, cfg)
    tables = [b"".join(bytes(x) for x in S.pdcch_scan_decodes(g)) for g in range(n_sf)]
    _same(sc, S.pdcch_scan(cell, tfg, N_RB, mask, cfg), ("pdcch_scan", case))
    assert tables == [b"".join(bytes(x) for x in S.pdcch_scan_decodes(g)) for g in range(n_sf)] and sc.n_sf == n_sf
    ph = S.phich_wide(*wide)
    values = [S.phich_values(g).tobytes() for g in range(n_sf)]
    _same(ph, S.phich(cell, tfg, N_RB, mask), ("phich", case))
    assert values == [S.phich_values(g).tobytes() for g in range(n_sf)]
    assert ph.n_sf == n_sf and [ph.sf[g].n_unit >= 0 for g in range(n_sf)] == read and (ph.n_present > 0 or mask != 0x3FF), case
    ps, pdc = S.pdsch_wide(*wide, want_pdcch=True)
    ps2, pdc2 = S.pdsch(cell, tfg, N_RB, mask, want_pdcch=True)
    _same(ps, ps2, ("pdsch", case))
    _same(pdc, pdc2, ("pdsch's pdcch", case))
    _same(pdc, pd, ("pdsch's pdcch against the pdcch stage", case))
    cb = S.pdsch_comb_wide(*wide)
    cb2 = S.pdsch_comb(cell, tfg, N_RB, mask)
    _same(cb[0], cb2[0], ("pdsch_comb", case))
    _same(cb[1], cb2[1], ("pdsch_comb's groups", case))
    _same(cb[0], ps, ("pdsch_comb's blocks against pdsch", case))


# ---------------------------------------------------------------- case 2: the stages do not disturb each other
def test_stages_beside_each_other_leave_each_other_s_tables_alone(pkg):
    """pcfich, pdcch, phich, pdsch, pdcch_scan, then pcfich at another bandwidth, then the first call again, on a fresh context: every
    stage keeps the jump tables of its own bandwidth in a block of its own, so the first record comes back byte for byte"""
    capi = pkg.capi
    cell = _cell(pkg, 1, 2)
    wide = (cell, dev(1, 2), FC, FC, FS, N_FFT, N_RB, 28, 0x3FF)
    other = np.ones((28, 12 * 15), np.complex128)
    with pkg.Searcher(0) as s:
        first = s.pcfich_wide(*wide)
        pd, ph, ps = s.pdcch_wide(*wide), s.phich_wide(*wide), s.pdsch_wide(*wide)
        sc = s.pdcch_scan_wide(*wide, _scan_cfg(capi, 2))
        assert s.pcfich(_cell(pkg, 1, 2, n_rb_dl=15), other, 15).n_rb == 15
        last = s.pcfich_wide(*wide)
        _same(first, last, "pcfich after the other stages and another bandwidth")
        assert first.n_decoded == 2
        # ... and so do the others after a call of each at the other bandwidth
        c15 = _cell(pkg, 1, 2, n_rb_dl=15)
        s.pdcch(c15, other, 15), s.phich(c15, other, 15), s.pdsch(c15, other, 15)
        s.pdcch_scan(c15, other, 15, 0x3FF, capi.PdcchScanCfg.make((capi.dci_ue_sizes(15, 2)["0/1A"],)))
        _same(pd, s.pdcch_wide(*wide), "pdcch")
        _same(ph, s.phich_wide(*wide), "phich")
        _same(ps, s.pdsch_wide(*wide), "pdsch")
        _same(sc, s.pdcch_scan_wide(*wide, _scan_cfg(capi, 2)), "pdcch_scan")


# ---------------------------------------------------------------- case 3: two rules broken at once
def test_a_host_grid_call_that_breaks_two_rules_names_one_and_launches_nothing(pkg, S):
    cell = _cell(pkg, 1, 2)
    wide = (cell, dev(1, 2), FC, FC, FS, N_FFT, N_RB, 28, 0x3FF)
    before = S.pcfich_wide(*wide)
    grid = np.ones((28, 120), np.complex128)
    rec = pkg.PcfichInfo()
    no_rb = _cell(pkg, 1, 2, n_rb_dl=-1)
    # 10 resource blocks are no LTE bandwidth, and a mask of 0 names no subframe
    rc = S._lib.lcs_pcfich(S._h, C.byref(no_rb), grid.ctypes.data_as(C.POINTER(C.c_double)), 28, 10, 0, C.byref(rec))
    assert rc == -2 and pkg.capi.ERRORS[rc] == "LCS_ERR_BAD_ARG"
    text = S._lib.lcs_last_error(S._h).decode()
    assert text.startswith("lcs_pcfich: ") and ("not an LTE bandwidth" in text or "needs a dl_mask" in text), text
    cfg = pkg.capi.PdcchCfg.make(pkg.capi.dci_common_sizes(N_RB))          # the bindings have no default for a bandwidth that is none
    for call in (lambda: S.pdcch(no_rb, grid, 10, 0, cfg), lambda: S.phich(no_rb, grid, 10, 0), lambda: S.pdsch(no_rb, grid, 10, 0, cfg),
                 lambda: S.pdcch_scan(no_rb, grid, 10, 0, _scan_cfg(pkg.capi, 2))):
        with pytest.raises(pkg.SearcherError, match="not an LTE bandwidth|needs a dl_mask"):
            call()
    _same(before, S.pcfich_wide(*wide), "the next valid call")
