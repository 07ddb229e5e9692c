"""GPU tests of the PHICH stage (lcs_phich_wide, lcs_phich, lcs_phich_values; k_phich, k_phich_fin).

The stage on crafted grids: the record and the table of every subframe bit-equal to the host twin (tests/host/phich_host.cpp) and
within 1e-9 of the numpy statement of the rule (tests/phich_ref.py), the project's bar for a device fp64 stage against numpy.  From
samples: captures with the generator's PHICH in them (three frames, 20 dB) read every planted indicator with its sign and nothing
among the silent ones, and the record is lcs_phich's on lcs_extract_tfg_wide's grid of the same call.  The link: format 0 grants
found by the blind search are answered eight subframes later as planted.  Refusals, isolation from the other stages, and
sweep.measure_wideband(phich=True)."""
import ctypes as C

import numpy as np
import pytest

import meas_wide_cases as WC
import pcfich_cases as PC
import pcfich_ref as PR
import phich_cases as HC
import phich_ref as HR
from conftest import load_pkg

pytestmark = pytest.mark.gpu
FS = 1.92e6
FC = WC.FC
CORNERS = ["6rb_one_unit", "15rb", "25rb_4ports", "ext_cp", "ext_cp_4ports", "ext_duration", "ext_duration_4ports", "100rb_ng2_mi2", "tdd_mi_012"]
# (R, n_rb, CP type, ports): the issue's shape, then four ports and the extended CP
SAMPLE_CASES = [(2, 15, 1, 2), (4, 25, 1, 4), (2, 15, 2, 2)]


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def S(pkg):
    s = pkg.Searcher(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def H(pkg):
    return HC.load_twin(pkg.capi)


_dev = {}


def dev(key, make):
    import torch
    if key not in _dev:
        _dev[key] = torch.from_numpy(np.ascontiguousarray(make())).cuda()
    return _dev[key]


def _cell(pkg, cp, R, n_ports, n_rb_dl=-1, **kw):
    c = pkg.new_cell(n_id_1=WC.CELL_ID[0], n_id_2=WC.CELL_ID[1], cp_type=cp, n_ports=n_ports, freq_fine=kw.pop("freq_fine", 0.0),
                     frame_start=kw.pop("frame_start", WC.FRAME_START * R), **kw)
    c.n_rb_dl = n_rb_dl
    c.phich_duration, c.phich_resource = 1, 3
    return c


def _same_bytes(a, b, what):
    assert bytes(a) == bytes(b), (what, np.flatnonzero(np.frombuffer(bytes(a), np.uint8) != np.frombuffer(bytes(b), np.uint8))[:8])


def _check(pkg, S, H, name, tfg, mask=0x3FF, **thr):
    """the device on a grid of corner `name` against the twin (bytes) and numpy (1e-9) -> the record"""
    capi = pkg.capi
    cell, cfg = HC.cell_of(pkg, name), HC.cfg_of(capi, name, **thr)
    got = S.phich(cell, tfg, HC.CORNERS[name]["n_rb"], mask, cfg)
    twin, tv, ts = HC.twin_record(H, capi, name, tfg, mask, thr.get("min_amp"), thr.get("min_sigma"))
    _same_bytes(got, twin, (name, hex(mask)))
    values = np.zeros_like(tv)
    for g in range(got.n_sf):
        v = S.phich_values(g)
        n = max(got.sf[g].n_unit, 0) * 8
        assert v.size == n and v.shape[1:] == (HR.n_seq_of(HC.CORNERS[name]["cp"]),), (name, g, v.shape)
        assert v.tobytes() == tv[g][:n].tobytes(), (name, g)
        values[g][:n] = v.reshape(-1)
    ref = HC.ref_record(name, tfg, mask, thr.get("min_amp"), thr.get("min_sigma"))
    HC.assert_record_close(got, values, None, ref, 1e-9, (name, hex(mask)), thr.get("min_amp"), thr.get("min_sigma"))
    return got


# ---------------------------------------------------------------- the stage on crafted grids
@pytest.mark.parametrize("name", CORNERS)
def test_stage_against_the_host_twin_and_numpy_on_crafted_grids(pkg, S, H, name):
    """noise-free with every entry planted (the grid ends two rows into a subframe), then 5 dB with half of them through a channel
    that is not flat"""
    tfg, planted = HC.crafted(name, "all")
    got = _check(pkg, S, H, name, tfg)
    assert got.n_present == sum(p.size for g, p in enumerate(planted) if p is not None and got.sf[g].n_unit > 0)
    noisy, _ = HC.crafted(name, "half", 5.0, seed=11, ripple=True)
    assert _check(pkg, S, H, name, noisy).n_present > 0


def test_masks_a_grid_that_ends_inside_a_subframe_empty_and_refused_subframes(pkg, S, H):
    for name in ("15rb", "25rb_4ports", "ext_duration"):
        tfg, _ = HC.crafted(name, "half", n_sub=12, ragged=1)
        for mask in HC.MASKS:
            got = _check(pkg, S, H, name, tfg, mask)
            need = HR.rows_needed(HC.CORNERS[name]["n_ports"], HC.CORNERS[name]["duration"])
            assert [got.sf[g].n_unit >= 0 for g in range(13)] == [bool((mask >> (g % 10)) & 1) and (g < 12 or need == 1) for g in range(13)], (name, hex(mask))
    # U = 0: subframes of m_i 0 are read with nothing in them
    tfg, _ = HC.crafted("tdd_mi_012", "all")
    got = _check(pkg, S, H, "tdd_mi_012", tfg)
    assert [got.sf[g].n_unit for g in range(4)] == [8, 4, 0, 0] and got.n_read == 4 and S.phich_values(2).size == 0
    # a refused map: m_i 2 at 6 resource blocks and Ng = 2 does not fit symbol 0
    HC.CORNERS["refused"] = dict(n_rb=6, n_ports=2, cp=1, duration=1, resource=4, mi=[2, 1] * 5, n_id=7)
    tfg, _ = HC.crafted("refused", "all")
    got = _check(pkg, S, H, "refused", tfg)
    assert [got.sf[g].n_unit for g in range(4)] == [-1, 2, -1, 2] and got.n_read == 2 and got.n_present == 32
    # thresholds of the caller's, grids without a value, and the cap of the list
    tfg, _ = HC.crafted("25rb_4ports", "half", 0.0, seed=3, ripple=True)
    loose, strict = _check(pkg, S, H, "25rb_4ports", tfg, min_amp=0.0, min_sigma=1.0), _check(pkg, S, H, "25rb_4ports", tfg, min_amp=0.9, min_sigma=6.0)
    assert loose.n_present > strict.n_present
    for fill in (0.0, np.nan):
        got = _check(pkg, S, H, "25rb_4ports", np.full((30, 300), fill + 0j))
        assert got.n_read == 3 and got.n_present == 0
    tfg, _ = HC.crafted("100rb_ng2_mi2", "all")
    got = S.phich(HC.cell_of(pkg, "100rb_ng2_mi2"), tfg, 100, 0x3FF, HC.cfg_of(pkg.capi, "100rb_ng2_mi2"))
    assert (got.n_present, got.n_hi, got.n_dropped) == (1600, 1024, 576)


# ---------------------------------------------------------------- from samples
@pytest.mark.parametrize("case", SAMPLE_CASES, ids=[str(c) for c in SAMPLE_CASES])
def test_from_samples_finds_every_planted_indicator_and_equals_the_stage_on_the_extracted_grid(pkg, S, case):
    R, n_rb, cp, n_ports = case
    n = PR.n_symb_of(cp)
    n_ofdm = 50 * n + 3                                       # two and a half frames and the head of a subframe
    d = dev(("phich",) + case, lambda: HC.phich_capture(*case))
    cell = _cell(pkg, cp, R, n_ports, n_rb_dl=n_rb)
    got = S.phich_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm)
    n_group, n_seq = pkg.capi.phich_n_group(n_rb, 3, cp == 1), HR.n_seq_of(cp)
    assert got.n_sf == 26 and got.n_read == 26            # the last subframe has three rows: enough at the normal duration
    want = []
    for g in range(26):
        pat = HC.capture_pattern(g // 10, g % 10, n_group, n_seq)
        assert got.sf[g].n_group == n_group
        want += [(g, a, b, bool(pat[a, b] < 0)) for a in range(n_group) for b in range(n_seq) if pat[a, b]]
    found = [(h["subframe"], h["group"], h["seq"], h["ack"]) for h in got.indicators()]
    print(case, "%d planted; |value| %.3f .. %.3f, noise %.2e .. %.2e" % (len(want), min(abs(h["value"]) for h in got.indicators()),
                                                                         max(abs(h["value"]) for h in got.indicators()), got.noise.min(), got.noise.max()))
    assert found == want and got.n_dropped == 0 and got.n_ack == sum(w[3] for w in want)
    assert all(0.7 < abs(h["value"]) < 1.3 for h in got.indicators())
    tfg, _ = S.extract_tfg_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm)
    _same_bytes(got, S.phich(cell, tfg, n_rb), case)
    # a mask, a frequency offset and a grid of one subframe
    off = _cell(pkg, cp, R, n_ports, freq_fine=137.0)
    one = S.phich_wide(off, d, FC, FC, FS * R, 128 * R, n_rb, 2 * n, 0x001)
    tfg1, _ = S.extract_tfg_wide(off, d, FC, FC, FS * R, 128 * R, n_rb, 2 * n)
    assert (one.n_sf, one.n_read) == (1, 1)
    _same_bytes(one, S.phich(off, tfg1, n_rb, 0x001), case)


# ---------------------------------------------------------------- the link to the uplink grants
def test_grants_of_the_blind_search_are_answered_as_planted(pkg, S):
    capi = pkg.capi
    R, n_rb, cp, n_ports = HC.LINK_SHAPE
    d = dev(("link",), HC.link_capture)
    cell = _cell(pkg, cp, R, n_ports, n_rb_dl=n_rb)
    n_ofdm = 29 * 2 * 7                                        # 29 subframes: the capture's last row lies beyond its end
    scan = S.pdcch_scan_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm, 0x3FF, capi.PdcchScanCfg.make((capi.dci_1a_size(n_rb),), phich_duration=1, phich_resource=3))
    ph = S.phich_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm)
    rows = capi.phich_for_grants(scan, ph, n_rb)
    # the control region is silent but for the grants, and the blind search may accept a recurring decode of noise as a UE grant: such
    # a grant is the one thing here that no indicator answers
    assert all(r["status"] in ("absent", "outside") for r in rows if r["rnti"] not in HC.LINK_RNTIS)
    got = sorted((r["subframe"], r["rnti"], r["rb_start"], r["cyclic_shift"], r["status"]) for r in rows if r["rnti"] in HC.LINK_RNTIS)
    want = sorted((g, rnti, rb, cs, answer if g + 8 < 29 else "outside") for g, rnti, rb, n_prb, cs, answer in HC.LINK_GRANTS)
    assert got == want, (got, want)
    assert ph.n_present == 4 and ph.n_ack == 2 and ph.ack_rate() == 0.5
    for r in rows:
        if r["status"] != "outside":
            assert (r["group"], r["seq"]) == capi.phich_index(r["rb_start"], r["cyclic_shift"], 2, True) and r["phich_subframe"] == r["subframe"] + 8
    tdd = S.phich_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm, cfg=capi.PhichCfg.make(phich_mi=[1] * 10))
    with pytest.raises(ValueError, match="FDD only"):
        capi.phich_for_grants(scan, tdd, n_rb)


# ---------------------------------------------------------------- refusals
def test_refusals_launch_nothing_and_leave_the_context_usable(pkg, S):
    capi = pkg.capi
    R, n_rb, cp, n_ports = SAMPLE_CASES[0]
    d = dev(("phich",) + SAMPLE_CASES[0], lambda: HC.phich_capture(*SAMPLE_CASES[0]))
    n = d.numel()
    ok = dict(cell=_cell(pkg, cp, R, n_ports), ptr=d.data_ptr(), n_cap=n, fs=FS * R, n_fft=256, n_rb=15, n_ofdm=280, mask=0x3FF, cfg=None)
    before = S.phich_wide(ok["cell"], d, FC, FC, FS * R, 256, 15, 280)
    assert before.n_read == 20 and before.n_present > 0
    unknown = _cell(pkg, cp, R, n_ports)
    unknown.phich_duration = unknown.phich_resource = 0
    mk = capi.PhichCfg.make
    bad_reserved = mk()
    bad_reserved.reserved[1] = 1
    cases = [(dict(ptr=0), "null pointer"), (dict(ptr=d.data_ptr() + 4), "not aligned"), (dict(n_fft=384), "n_fft is not"),
             (dict(fs=FS * R * 1.0011), "15 kHz x n_fft"), (dict(n_rb=5), "n_rb is outside"), (dict(n_rb=10), "not an LTE bandwidth"),
             (dict(cell=_cell(pkg, cp, R, n_ports, n_rb_dl=25)), "contradicts the cell's n_rb_dl"),
             (dict(n_ofdm=13), "n_ofdm is outside"), (dict(n_ofdm=122 * 7 + 1), "n_ofdm is outside"), (dict(mask=0), "dl_mask"), (dict(mask=0x400), "dl_mask"),
             (dict(cell=pkg.new_cell(n_id_2=1, cp_type=cp)), "n_id_1, n_id_2 and a known cp_type"),
             (dict(n_cap=int(ok["cell"].frame_start) + 19200 * R), "does not hold the last requested row"),
             (dict(cell=unknown), "PHICH configuration is unknown"), (dict(cfg=mk(phich_duration=3)), "phich_duration is outside"),
             (dict(cfg=mk(phich_resource=5)), "phich_resource is outside"), (dict(cfg=mk(phich_mi=[1] * 9 + [3])), "an m_i is outside"),
             (dict(cfg=mk(min_amp=-0.1)), "min_amp"), (dict(cfg=mk(min_amp=float("nan"))), "min_amp"), (dict(cfg=mk(min_sigma=float("inf"))), "min_sigma"),
             (dict(cfg=bad_reserved), "reserved")]
    for change, text in cases:
        a = dict(ok, **change)
        with pytest.raises(pkg.SearcherError, match=text):
            S.phich_wide(a["cell"], a["ptr"], FC, FC, a["fs"], a["n_fft"], a["n_rb"], a["n_ofdm"], a["mask"], a["cfg"], n_cap=a["n_cap"])
    grid = np.ones((280, 180), np.complex128)
    host_cases = [(dict(n_rb=10, grid=np.ones((280, 120), np.complex128)), "not an LTE bandwidth"), (dict(grid=grid[:13]), "n_ofdm is outside"), (dict(mask=0x400), "dl_mask"),
                  (dict(cell=unknown), "PHICH configuration is unknown"), (dict(cfg=mk(min_sigma=-1.0)), "min_sigma"),
                  (dict(cell=pkg.new_cell(n_id_1=5, cp_type=cp)), "n_id_1, n_id_2 and a known cp_type")]
    for change, text in host_cases:
        a = dict(dict(cell=ok["cell"], grid=grid, n_rb=15, mask=0x3FF, cfg=None), **change)
        with pytest.raises(pkg.SearcherError, match=text):
            S.phich(a["cell"], a["grid"], a["n_rb"], a["mask"], a["cfg"])
    with pytest.raises(ValueError):
        S.phich(ok["cell"], grid, 25)
    # through the C ABI: the return value is LCS_ERR_BAD_ARG and the text says who
    lib, cell, rec = S._lib, ok["cell"], capi.PhichInfo()
    assert lib.lcs_phich_wide(S._h, C.byref(cell), C.c_void_p(d.data_ptr()), n, FC, FC, FS * R, 256, 15, 280, 0x3FF, None, None) == -2
    assert b"lcs_phich_wide: a null pointer" in lib.lcs_last_error(S._h)
    assert lib.lcs_phich(S._h, C.byref(cell), None, 280, 15, 0x3FF, None, C.byref(rec)) == -2
    assert lib.lcs_phich(S._h, C.byref(cell), grid.ctypes.data_as(C.POINTER(C.c_double)), 280, 15, 0x3FF, C.byref(mk(phich_resource=9)), C.byref(rec)) == -2
    assert b"lcs_phich: phich_resource is outside" in lib.lcs_last_error(S._h)
    buf = np.zeros(400)
    dp = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.lcs_phich_values(S._h, 20, dp, 400) == -2 and b"outside the subframes" in lib.lcs_last_error(S._h)
    assert lib.lcs_phich_values(S._h, 0, dp, 15) == -2 and b"cap is below" in lib.lcs_last_error(S._h)
    assert lib.lcs_phich_values(S._h, 0, None, 400) == -2
    with pkg.Searcher(0) as fresh:
        assert fresh._lib.lcs_phich_values(fresh._h, 0, dp, 400) == -2 and b"no PHICH call" in fresh._lib.lcs_last_error(fresh._h)
    assert lib.lcs_phich_values(S._h, 0, dp, 400) == 16
    after = S.phich_wide(ok["cell"], d, FC, FC, FS * R, 256, 15, 280)
    _same_bytes(after, before, "after the refusals")


# ---------------------------------------------------------------- isolation
def test_the_other_wide_stages_are_left_alone(pkg):
    """the PCFICH, PDCCH and blind-search records and the chain's cells before and after the stage: byte-equal"""
    import cell_meas_cases as CS
    capi = pkg.capi
    R, n_rb, cp, n_ports = HC.LINK_SHAPE
    d = dev(("link",), HC.link_capture)
    cell = _cell(pkg, cp, R, n_ports, n_rb_dl=n_rb)
    args = (cell, d, FC, FC, FS * R, 128 * R, n_rb, 283)
    scan_cfg = capi.PdcchScanCfg.make((capi.dci_1a_size(n_rb),), phich_duration=1, phich_resource=3)
    with pkg.Searcher(0) as s:
        others = lambda: [bytes(s.pcfich_wide(*args)), bytes(s.pdcch_wide(*args)), bytes(s.pdcch_scan_wide(*args, 0x3FF, scan_cfg)), bytes(s.cell_meas_wide(*args)),
                          [bytes(c) for c in s.search_capbuf(CS.cap(1), CS.GRID, CS.FC, CS.FC, FS)[0]]]
        want = others()
        first = s.phich_wide(*args)
        assert first.n_read == 21                             # 283 rows: 20 subframes and symbol 0 of one more, which two ports need no more of
        assert others() == want
        _same_bytes(s.phich_wide(*args), first, "between the other stages")
        s.stream_open(pkg.FMT_IQ_U8, 153600, CS.FC, CS.FC, FS)
        _same_bytes(s.phich_wide(*args), first, "beside an open stream")
        s.stream_close()


# ---------------------------------------------------------------- the sweep
def test_measure_wideband_reads_the_phich_from_the_measurement_s_buffer(pkg):
    import torch
    K, fc = 8, 1.8425e9
    n_group = pkg.capi.phich_n_group(25, 3, True)

    def phich(frame, subframe):
        pat = HC.capture_pattern(frame, subframe, n_group, 8)
        return [dict(group=int(a), seq=int(b), ack=int(pat[a, b] < 0)) for a, b in zip(*np.nonzero(pat))]

    wide = dict(n_id_1=52, n_id_2=1, n_ports=2, port_gains=[1.0, 0.7j], f_off=1200.0, t0=4321.0, sfn0=8, phich=phich)
    x, _, _ = pkg.synth.make_wideband_cell(11, fc, K, [(fc, 4, 25, wide)], snr_db=20.0, n_in=153600 * K, cfi=PC.planted_cfi)
    d = torch.from_numpy(x).cuda()
    carriers = np.array([fc])
    with pkg.Searcher(0) as s:
        cells = pkg.sweep.search_wideband(s, d.data_ptr(), pkg.FMT_C64, x.size, FS * K, K, fc, carriers, np.array([-5e3, 0.0, 5e3]), n_out=153584, meas=True)
        big = [c for c in cells[0] if c["n_id_cell"] == 52 * 3 + 1 and c["n_rb_dl"] == 25]
        assert len(big) == 1, [(c["n_id_cell"], c["n_rb_dl"]) for c in cells[0]]
        calls = []
        chan = s.channelize
        s.channelize = lambda *a, **k: (calls.append(a), chan(*a, **k))[1]
        today = pkg.sweep.measure_wideband(s, d.data_ptr(), pkg.FMT_C64, x.size, FS * K, fc, K, cells, carriers)
        assert all("phich" not in c for c in cells[0])
        n_today = len(calls)
        both = pkg.sweep.measure_wideband(s, d.data_ptr(), pkg.FMT_C64, x.size, FS * K, fc, K, cells, carriers, phich=True)
        assert len(calls) == 2 * n_today                     # the PHICH reads the measurement's buffer: no channelizer call of its own
        del s.channelize
    for c, t, b in zip(cells[0], today[0], both[0]):
        if c["n_rb_dl"] == -1:
            assert t is None and b is None and "phich" not in c
            continue
        assert isinstance(t, pkg.CellMeasWide) and bytes(b[0]) == bytes(t) and b[1] is c["phich"]
    rec = big[0]["phich"]
    assert rec.n_sf == 61 and rec.n_read == 61 and rec.n_rb == 25 and rec.n_ports == 2 and rec.n_present > 200
    # the grid starts at the frame the search found: which of the capture's frames that is, the planted pattern tells
    found = {(h["subframe"], h["group"], h["seq"]): h["ack"] for h in rec.indicators()}
    match = []
    for f0 in range(0, 3):
        want = {}
        for g in range(61):
            pat = HC.capture_pattern(f0 + g // 10, g % 10, n_group, 8)
            want.update({(g, a, b): bool(pat[a, b] < 0) for a, b in zip(*np.nonzero(pat))})
        match.append(want == found)
    assert sum(match) == 1, match
