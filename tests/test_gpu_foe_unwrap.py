"""GPU tests of the unwrapped frequency estimate (lcs_set_foe_unwrap): the PSS-only coarse estimate as a stage
(lcs_pss_foe_coarse), pss_sss_foe with the mode on, and the chain on the reference's 5 kHz grid in TDD through every entry point.

The reference is tests/pss_coarse_ref.py -- the numpy restatement of the arithmetic of include/lcs.h on top of
tests/sss_duplex_ref.py -- with the oracle for everything behind the two stages.  Bars: C to 1e-9 of sum_k |A_k| |B_k|, f_coarse and
freq_fine to 1e-6 Hz stage by stage; through the fused chain those of tests/test_gpu_tdd.py (frame_start 1e-6, frequencies 1e-3 Hz,
integers equal).  The chain cases and the batch of six use whole 153600-sample buffers (a MIB needs them); so do the two buffers
that carry the u8 and complex<float> source formats through the batch."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle as O
import pss_coarse_ref as PC
import sss_duplex_ref as R
import foe_unwrap_cases as K
from conftest import ROOT, iq_u8_to_capbuf, load_pkg

pytestmark = pytest.mark.gpu
FS, FC, GRID5, TDD, FDD = K.FS, K.FC, K.GRID5, R.GEO["tdd"], R.GEO["fdd"]
INT_FIELDS = ("ind", "n_id_2", "n_id_1", "cp_type", "n_ports", "n_rb_dl", "phich_duration", "phich_resource", "sfn")


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module", autouse=True)
def _oracle_mode():
    O.set_legacy(False)
    O.set_threads(min(16, os.cpu_count() or 1))


@pytest.fixture(scope="module")
def T(pkg):
    """a searcher set to TDD, unwrap off"""
    s = pkg.Searcher(0)
    s.set_duplex(pkg.DUPLEX_TDD)
    yield s
    s.close()


@pytest.fixture(scope="module")
def TU(pkg):
    """a searcher set to TDD with the unwrap on"""
    s = pkg.Searcher(0)
    s.set_duplex(pkg.DUPLEX_TDD)
    s.set_foe_unwrap(True)
    yield s
    s.close()


@pytest.fixture(scope="module")
def F(pkg):
    """a searcher left in FDD, unwrap off"""
    s = pkg.Searcher(0)
    yield s
    s.close()


# ---------------------------------------------------------------- 4. stage parity of the coarse estimate
def stage_t0(peak, cp_normal, tdd, half=0):
    """the timing that puts the peak of a PSS occurrence (the start of its cyclic prefix) at sample `peak`"""
    P = (2204 if cp_normal else 2272) if tdd else 832
    return float((P - (peak + 9) + 9600 * half) % 19200)


# (id, n_cap, TDD?, normal CP?, the peak record's ind, its freq, planted f_off, occurrences, dongle parameters?)
STAGE_SHAPES = [
    ("24000 samples, two occurrences, TDD normal CP", 24000, True, True, 6000, 0.0, 2200.0, 2, False),
    ("24000 samples, TDD extended CP, hypothesis 2500 Hz", 24000, True, False, 3000, 2500.0, 4400.0, 3, False),
    ("57600 samples, TDD normal CP, hypothesis 5000 Hz", 57600, True, True, 5000, 5000.0, 2700.0, 6, False),
    ("57600 samples, TDD extended CP", 57600, True, False, 7000, 0.0, -2300.0, 6, False),
    ("24000 samples, FDD normal CP", 24000, False, True, 4000, 0.0, 2400.0, 3, False),
    ("57600 samples, FDD extended CP, hypothesis 5000 Hz", 57600, False, False, 2000, 5000.0, 3000.0, 6, False),
    ("peak at 300: moved by the TDD room rule", 24000, True, True, 300, 0.0, -2400.0, 2, False),
    ("dongle parameters, TDD extended CP, hypothesis 2500 Hz", 57600, True, False, 5000, 2500.0, 500.0, 6, True),
    ("dongle parameters, TDD normal CP", 24000, True, True, 2000, 0.0, 2400.0, 3, True),
]
DONGLE = dict(fc_programmed=FC * (1 - 31e-6), fs_programmed=FS * 1.00002)


def stage_case(pkg, n_cap, tdd, cp_normal, ind, freq, f_off, dongle):
    """-> (capture, the cell behind the reference's SSS detection, (fc_requested, fc_programmed, fs_programmed), geometry)"""
    fcp, fsp = (DONGLE["fc_programmed"], DONGLE["fs_programmed"]) if dongle else (FC, FS)
    cell = dict(K.BASE, cp_normal=cp_normal, f_off=f_off, t0=stage_t0(ind, cp_normal, tdd), tdd=(2, 10) if tdd else None)
    cap = iq_u8_to_capbuf(pkg.synth.make_capbuf(21, FC, [cell], snr_db=15.0, n_cap=n_cap, fc_programmed=fcp, fs_programmed=fsp)[0])
    geo = TDD if tdd else FDD
    pk = O.new_cell(pss_pow=1.0, ind=ind, freq=freq, n_id_2=cell["n_id_2"], fc_requested=FC, fc_programmed=fcp)
    det, _ = R.sss_detect(pk, cap, 3.0, FC, fcp, fsp, geo)
    assert (det.n_id_1, det.cp_type) == (cell["n_id_1"], 1 if cp_normal else 2), "the reference finds the planted cell"
    return cap, det, (FC, fcp, fsp), geo


@pytest.mark.parametrize("name, n_cap, tdd, cp_normal, ind, freq, f_off, n_occ, dongle", STAGE_SHAPES, ids=[s[0] for s in STAGE_SHAPES])
def test_coarse_stage_parity(pkg, T, F, name, n_cap, tdd, cp_normal, ind, freq, f_off, n_occ, dongle):
    cap, det, prm, geo = stage_case(pkg, n_cap, tdd, cp_normal, ind, freq, f_off, dongle)
    if name.startswith("peak at"):
        assert R.sss_geometry(det, n_cap, prm[0], prm[1], geo)[0] != ind and ind + 9 < 482
    ref = PC.coarse(det, cap, *prm, geo)
    assert ref["n_occ"] == n_occ
    f_coarse, C, n = (T if tdd else F).pss_foe_coarse(pkg.new_cell(**{k: getattr(det, k) for k, _ in O.Cell._fields_ if hasattr(pkg.LcsCell, k)}), cap, *prm)
    print(name, "C error / scale %.2e" % (abs(C - ref["C"]) / ref["scale"]), "f_coarse", f_coarse, "reference", ref["f_coarse"], "planted residual", f_off - freq)
    assert n == ref["n_occ"]
    assert abs(C - ref["C"]) <= 1e-9 * ref["scale"]
    assert abs(f_coarse - ref["f_coarse"]) <= 1e-6
    assert abs(ref["f_coarse"] - (f_off - freq)) < 1000.0, "the estimate means something: within 1 kHz of the planted residual at 15 dB"


# ---------------------------------------------------------------- 5. pss_sss_foe with the mode on
def _lcs(pkg, c):
    return pkg.new_cell(**{k: getattr(c, k) for k, _ in O.Cell._fields_ if hasattr(pkg.LcsCell, k)})


@pytest.mark.parametrize("name, snr, cp_normal, f_off, n, native_ok", K.CRAFTED, ids=[c[0] for c in K.CRAFTED])
def test_pss_sss_foe_with_the_mode_on(pkg, T, TU, name, snr, cp_normal, f_off, n, native_ok):
    r = K.crafted_ref(snr, cp_normal, f_off)
    assert r["n"] == n
    det = _lcs(pkg, r["detected"])
    on = TU.pss_sss_foe(det, r["cap"], FC, FC, FS)
    off = T.pss_sss_foe(det, r["cap"], FC, FC, FS)
    print(name, "on", on.freq_fine, "off", off.freq_fine, "reference", r["unwrapped"].freq_fine, r["native"].freq_fine)
    assert abs(off.freq_fine - r["native"].freq_fine) <= 1e-6
    assert abs(on.freq_fine - r["unwrapped"].freq_fine) <= 1e-6
    if n == 0:
        assert on.freq_fine == off.freq_fine      # the same double
    for k, _ in pkg.LcsCell._fields_:
        if k != "freq_fine":
            assert getattr(on, k) == getattr(off, k) or (getattr(on, k) != getattr(on, k) and getattr(off, k) != getattr(off, k)), k
    # the stage of the coarse estimate does not depend on the setting
    assert T.pss_foe_coarse(det, r["cap"], FC, FC, FS) == TU.pss_foe_coarse(det, r["cap"], FC, FC, FS)


# ---------------------------------------------------------------- 6. the chain on the 5 kHz grid
def _key(c):
    return tuple(getattr(c, k) for k in INT_FIELDS)


def _cells_match(got, exp):
    assert [_key(c) for c in got] == [_key(c) for c in exp], ([_key(c) for c in got], [_key(c) for c in exp])
    for a, b in zip(got, exp):
        assert a.freq == b.freq
        assert abs(a.frame_start - b.frame_start) < 1e-6, (a.frame_start, b.frame_start)
        assert abs(a.freq_fine - b.freq_fine) < 1e-3 and abs(a.freq_superfine - b.freq_superfine) < 1e-3


CHAIN = [c for c in K.CRAFTED if not c[5]][:4]      # the +- 2400 / -2300 Hz cells that do not decode natively: n = +1, +1, -1, -1
SIX = CHAIN + [K.CRAFTED[1], K.CRAFTED[5]]            # ... one that does (n = 0), and the -6 dB cell the peak search finds at 5 kHz


@pytest.fixture(scope="module")
def chain(pkg, T, TU):
    """the chain cases one by one (search_capbuf) in both modes, with the reference chain run on the GPU's own peak lists"""
    out = []
    for name, snr, cp_normal, f_off, n, _ in CHAIN:
        cap = iq_u8_to_capbuf(K.crafted_u8(snr, cp_normal, f_off))
        on, peaks = TU.search_capbuf(cap, GRID5, FC, FC, FS)
        off, peaks_off = T.search_capbuf(cap, GRID5, FC, FC, FS)
        assert [bytes(p) for p in peaks] == [bytes(p) for p in peaks_off]
        out.append(dict(name=name, on=on, off=off, f_off=f_off, cp_normal=cp_normal,
                        ref_on=PC.search_peaks(peaks, cap, FC, FC, FS, TDD, unwrap_on=True),
                        ref_off=PC.search_peaks(peaks, cap, FC, FC, FS, TDD, unwrap_on=False)))
    return out


def test_chain_on_the_5_khz_grid_single_buffers(chain):
    assert [c[4] for c in CHAIN] == [1, 1, -1, -1]
    for c in chain:
        print(c["name"], "off", [_key(x) for x in c["off"]], "on", [(x.n_id_cell(), x.freq_fine, x.freq_superfine) for x in c["on"]])
        assert c["ref_off"] == [] and c["off"] == [], "natively the cell is absent, as in the reference"
        _cells_match(c["on"], c["ref_on"])
        assert [(x.n_id_cell(), x.cp_type, x.n_ports, x.n_rb_dl) for x in c["on"]] == [(77 * 3 + 2, 1 if c["cp_normal"] else 2, 2, 25)]
        assert abs(c["on"][0].freq_superfine - c["f_off"]) < 100.0


@pytest.fixture(scope="module")
def six(pkg, TU):
    import torch
    bufs = [K.crafted_u8(c[1], c[2], c[3]) for c in SIX]
    single = [TU.search_capbuf(iq_u8_to_capbuf(b), GRID5, FC, FC, FS)[0] for b in bufs]
    d = torch.from_numpy(np.stack(bufs)).cuda()
    return dict(bufs=bufs, d=d, single=single, batch=TU.search_batch(d.data_ptr(), pkg.FMT_IQ_U8, 6, 153600, GRID5, FC, FC, FS, pkg.STAGE_FULL))


def test_batch_of_six_equals_the_single_calls_and_contexts_keep_their_settings(pkg, T, TU, F, six, chain):
    for b in range(6):
        _cells_match(six["batch"][b], six["single"][b])
        assert [c.n_id_cell() for c in six["batch"][b]] == [77 * 3 + 2], SIX[b][0]
        assert abs(six["batch"][b][0].freq_superfine - SIX[b][3]) < 100.0
    for b in range(4):
        _cells_match(six["single"][b], chain[b]["ref_on"])
    # a second context in FDD, and a third in TDD without the unwrap, on the same buffers -- then the first again
    fdd = F.search_batch(six["d"].data_ptr(), pkg.FMT_IQ_U8, 6, 153600, GRID5, FC, FC, FS, pkg.STAGE_FULL)
    assert fdd == [[], [], [], [], [], []]
    native = T.search_batch(six["d"].data_ptr(), pkg.FMT_IQ_U8, 6, 153600, GRID5, FC, FC, FS, pkg.STAGE_FULL)
    assert [len(c) for c in native] == [0, 0, 0, 0, 1, 0]
    assert bytes(native[4][0]) == bytes(six["batch"][4][0]), "n = 0: the same record in both modes"
    again = TU.search_batch(six["d"].data_ptr(), pkg.FMT_IQ_U8, 6, 153600, GRID5, FC, FC, FS, pkg.STAGE_FULL)
    assert [[bytes(c) for c in b] for b in again] == [[bytes(c) for c in b] for b in six["batch"]]
    assert (F.duplex, F.foe_unwrap, T.duplex, T.foe_unwrap, TU.duplex, TU.foe_unwrap) == (0, False, 1, False, 1, True)


def test_source_formats_through_the_batch(pkg, TU):
    """u8 and complex<float> buffers through the batch (the int8 pairs and the caller's floats are what k_foe_fin_unwrap reads there),
    against the stages on the same context fed the same samples as complex<double>"""
    import torch
    bufs = [K.crafted_u8(c[1], c[2], c[3]) for c in CHAIN[:2]]
    caps = [iq_u8_to_capbuf(b) for b in bufs]
    d8 = torch.from_numpy(np.stack(bufs)).cuda()
    d32 = torch.from_numpy(np.stack([0.5 * c for c in caps]).astype(np.complex64)).cuda()      # halved: no dongle data any more, exact in fp32
    for fmt, d, scale in ((pkg.FMT_IQ_U8, d8, 1.0), (pkg.FMT_C64, d32, 0.5)):
        got = TU.search_batch(d.data_ptr(), fmt, 2, 153600, GRID5, FC, FC, FS, pkg.STAGE_FULL)
        for b in range(2):
            assert [c.n_id_cell() for c in got[b]] == [77 * 3 + 2]
            c = got[b][0]
            pk = pkg.new_cell(pss_pow=c.pss_pow, ind=c.ind, freq=c.freq, n_id_2=c.n_id_2, fc_requested=FC, fc_programmed=FC)
            det, _ = TU.sss_detect(pk, scale * caps[b], 3.0, FC, FC, FS)
            st = TU.pss_sss_foe(det, scale * caps[b], FC, FC, FS)
            print("fmt", fmt, "buffer", b, "batch", c.freq_fine, "stages", st.freq_fine)
            assert abs(c.freq_fine - st.freq_fine) < 1e-3 and abs(c.frame_start - det.frame_start) < 1e-6
            assert abs(c.freq_fine - CHAIN[b][3]) < 100.0 and abs(c.freq_fine - c.freq) > 2330.0      # unwrapped: outside the native range


def test_streaming_mode_and_hypothesis_split_with_the_mode_on(pkg, chain):
    buf = K.crafted_u8(*CHAIN[0][1:4])
    want = chain[0]["ref_on"]
    with pkg.Searcher(0) as s:
        s.set_duplex(pkg.DUPLEX_TDD)
        for on in (False, True):
            s.set_foe_unwrap(on)
            s.stream_open(pkg.FMT_IQ_U8, 153600, FC, FC, FS)
            s.stream_push(buf, 0.0)
            cells, dup, _ = s.stream_collect()
            s.stream_close()
            assert dup == 0 and [c.n_id_cell() for c in cells] == ([77 * 3 + 2] if on else [])
        assert (cells[0].cp_type, cells[0].n_ports, cells[0].n_rb_dl, cells[0].sfn) == (want[0].cp_type, want[0].n_ports, want[0].n_rb_dl, want[0].sfn)
        assert abs(cells[0].frame_start - want[0].frame_start) < 1e-6 and abs(cells[0].freq_superfine - want[0].freq_superfine) < 1e-3
        assert abs(cells[0].freq_fine - want[0].freq_fine) < 1e-3
        got, _ = pkg.sweep.search_capbuf_foe_split_dev(s, iq_u8_to_capbuf(buf), GRID5, FC, FC, FS)
        assert [(c["n_id_1"], c["n_id_2"], c["cp_type"], c["n_ports"], c["n_rb_dl"], c["sfn"]) for c in got] == \
               [(c.n_id_1, c.n_id_2, c.cp_type, c.n_ports, c.n_rb_dl, c.sfn) for c in want]
        assert abs(got[0]["frame_start"] - want[0].frame_start) < 1e-6 and abs(got[0]["freq_superfine"] - want[0].freq_superfine) < 1e-3
        s.set_foe_unwrap(False)
        assert pkg.sweep.search_capbuf_foe_split_dev(s, iq_u8_to_capbuf(buf), GRID5, FC, FC, FS)[0] == []


# ---------------------------------------------------------------- 7. mode-off invariance
def test_mode_off_is_what_it_was(pkg):
    import torch
    grids = {True: np.arange(-15, 16) * 2.5e3, False: np.arange(-15, 16) * 5e3}
    with pkg.Searcher(0) as never, pkg.Searcher(0) as toggled:
        for tdd, fc0, f_off_max in ((True, 1.9e9, 37.5e3), (False, 739e6, 60e3)):
            fcs = fc0 + 100e3 * np.arange(6)
            d = torch.from_numpy(pkg.synth.make_batch_u8(6, 77, fcs, tdd=tdd, f_off_max=f_off_max)).cuda()
            run = lambda s: s.search_batch(d.data_ptr(), pkg.FMT_IQ_U8, 6, 153600, grids[tdd], fcs, fcs, FS, pkg.STAGE_FULL)
            for s in (never, toggled):
                s.set_duplex(pkg.DUPLEX_TDD if tdd else pkg.DUPLEX_FDD)
            toggled.set_foe_unwrap(True)
            with_mode = run(toggled)
            toggled.set_foe_unwrap(False)
            a, b = run(never), run(toggled)
            assert sum(len(x) for x in a) >= 1, "the batch holds a cell"
            assert [[bytes(c) for c in x] for x in a] == [[bytes(c) for c in x] for x in b]
            # (on these grids nothing aliases: the mode decides n = 0 everywhere and hands the native doubles on)
            assert [[bytes(c) for c in x] for x in with_mode] == [[bytes(c) for c in x] for x in a]


# ---------------------------------------------------------------- 8. the setter's contract
def test_setter_contract(pkg):
    with pkg.Searcher(0) as s:
        assert s.foe_unwrap is False
        s.set_foe_unwrap(True)
        assert s.foe_unwrap is True
        s.set_foe_unwrap(False)
        assert s.foe_unwrap is False
        for bad in (2, -1, 7):
            rc = s._lib.lcs_set_foe_unwrap(s._h, bad)
            assert pkg.capi.ERRORS[rc] == "LCS_ERR_BAD_ARG" and b"foe_unwrap" in s._lib.lcs_last_error(s._h)
        assert s.foe_unwrap is False
        s.stream_open(pkg.FMT_IQ_U8, 153600, FC, FC, FS)
        with pytest.raises(pkg.SearcherError, match="LCS_ERR_BAD_ARG.*stream"):
            s.set_foe_unwrap(True)
        s.set_foe_unwrap(False)      # no change: accepted
        assert s.foe_unwrap is False
        s.stream_close()
        s.set_foe_unwrap(True)
        assert s.foe_unwrap is True
        cap = np.zeros(24000, np.complex128)
        with pytest.raises(pkg.SearcherError, match="LCS_ERR_BAD_ARG.*n_id_1"):
            s.pss_foe_coarse(pkg.new_cell(ind=100, freq=0.0, n_id_2=1, n_id_1=-1, cp_type=1, frame_start=0.0), cap, FC, FC, FS)
        with pytest.raises(pkg.SearcherError, match="LCS_ERR_BAD_ARG"):
            s.pss_foe_coarse(pkg.new_cell(ind=100, freq=0.0, n_id_2=1, n_id_1=5, frame_start=0.0), cap, FC, FC, FS)      # no CP type
        # an all-zero buffer: C = 0, nothing usable, and the mode hands the native value on
        z = pkg.new_cell(ind=100, freq=0.0, n_id_2=1, n_id_1=5, cp_type=1, frame_start=300.0, fc_requested=FC, fc_programmed=FC)
        n_occ = PC.coarse(z, cap, FC, FC, FS, FDD)["n_occ"]
        assert n_occ >= 2 and s.pss_foe_coarse(z, cap, FC, FC, FS) == (0.0, 0j, n_occ)
        on = s.pss_sss_foe(z, cap, FC, FC, FS)
        s.set_foe_unwrap(False)
        assert bytes(on) == bytes(s.pss_sss_foe(z, cap, FC, FC, FS))      # (a NaN: the native weights are 0 / 0 there)


# ---------------------------------------------------------------- 9. CLI
def test_cellsearch_foe_unwrap(pkg, tmp_path):
    exe = os.path.join(ROOT, "host", "CellSearch")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])
    h = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--foe-unwrap" in h
    cap = iq_u8_to_capbuf(K.crafted_u8(*CHAIN[0][1:4]))      # f_off = +2400 Hz
    pkg.itfile.write_it(str(tmp_path / "capbuf_0000.it"), {"capbuf": cap, "fc": np.array([int(FC)], np.int32)})
    for extra in (["--foe-unwrap"], []):      # the 5 kHz grid with the unwrap, and -x tdd alone on its 2.5 kHz grid
        r = subprocess.run([exe, "-s", str(int(FC)), "-p", "2", "-x", "tdd"] + extra + ["-l", "-d", str(tmp_path)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert re.search(r"cell.ID..%d\b" % (77 * 3 + 2), r.stdout), r.stdout
