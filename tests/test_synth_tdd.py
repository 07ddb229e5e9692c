"""The TDD (36.211 frame structure type 2) form of the synthetic generator, and the recovery of a planted TDD cell on the CPU.

Structure: cell_waveform(..., tdd=(ul_dl_config, dwpts_symbols)) puts the PSS into symbol 2 of slots 2 / 12, the SSS into the last
symbol of slots 1 / 11, keeps uplink subframes and the tail of a special subframe exactly zero, and tdd=None is the generator as
it was (tests/golden/synth_fdd_seeded.npz holds two seeded FDD buffers written by the generator before it knew TDD).

Recovery: the peak comes from the oracle's xcorr_pss + peak_search, SSS detection and the PSS/SSS frequency estimate from the numpy
restatement in TDD mode (tests/sss_duplex_ref.py, pinned to the oracle in FDD by test_sss_duplex_ref.py), the rest -- extract_tfg,
tfoec, decode_mib -- from the oracle, which takes a cell record and does not care about duplex.  Every case must decode.

frame_start follows the reference's convention: two samples in front of the frame boundary (the DFT windows start two samples
inside the cyclic prefix, src/searcher.cpp:578), so the planted value is boundary - 2."""
import os

import numpy as np
import pytest

import oracle as O
import sss_duplex_ref as R
from conftest import GOLDEN, load_pkg

FS = 1.92e6
FC = 2.35e9          # band 40
F_SET = np.array([-2.5e3, 0.0, 2.5e3])


@pytest.fixture(scope="module")
def synth():
    return load_pkg().synth


@pytest.fixture(scope="module", autouse=True)
def _oracle_mode():
    O.set_legacy(False)
    O.set_threads(min(16, os.cpu_count() or 1))


# ---------------------------------------------------------------- structure
def test_fdd_buffers_of_a_seed_are_unchanged(synth):
    g = np.load(os.path.join(GOLDEN, "synth_fdd_seeded.npz"))
    a, _ = synth.make_capbuf(41, 739e6, [dict(n_id_1=92, n_id_2=1, f_off=1200.0, t0=1000.3, sfn0=17)], snr_db=10.0, n_cap=9600)
    b, _ = synth.make_capbuf(42, 739e6, [dict(n_id_1=33, n_id_2=0, cp_normal=False, n_ports=4, n_rb_dl=15, f_off=-3e3),
                                         dict(n_id_1=5, n_id_2=2, n_ports=1, gain_db=-3.0)], snr_db=3.0, n_cap=9600)
    assert np.array_equal(a, g["a"]) and np.array_equal(b, g["b"])
    # the keyword itself: None is the default
    w0 = synth.cell_waveform(1, 7, 1, rng=np.random.default_rng(5))
    w1 = synth.cell_waveform(1, 7, 1, rng=np.random.default_rng(5), tdd=None)
    assert np.array_equal(w0, w1)


def _symbols(w, cp_normal):
    """one frame -> {(slot, sym): (start of the symbol's CP, CP length)}"""
    pos, out = 0, {}
    for slot in range(20):
        for sym in range(7 if cp_normal else 6):
            cp = (10 if sym == 0 else 9) if cp_normal else 32
            out[(slot, sym)] = (pos, cp)
            pos += cp + 128
    assert pos == 19200
    return out


def _bins62(w, start, cp):
    X = np.fft.fft(w[start + cp:start + cp + 128]) / np.sqrt(128.0)
    return np.concatenate([X[97:128], X[1:32]])


@pytest.mark.parametrize("cfg, dwpts, cp_normal", [(0, 3, True), (2, 10, True), (5, 11, True), (1, 9, False), (6, 8, False), (3, 12, False)])
def test_tdd_frame_structure(synth, cfg, dwpts, cp_normal):
    n_id_1, n_id_2, n_frames = 55, 2, 2
    w = synth.cell_waveform(n_frames, n_id_1, n_id_2, cp_normal=cp_normal, n_ports=1, port_gains=[1.0], rng=np.random.default_rng(1),
                            tdd=(cfg, dwpts))
    assert w.size == n_frames * 19200
    n_symb = 7 if cp_normal else 6
    kinds = synth.TDD_SUBFRAMES[cfg]
    assert kinds == ("DSUUUDSUUU", "DSUUDDSUUD", "DSUDDDSUDD", "DSUUUDDDDD", "DSUUDDDDDD", "DSUDDDDDDD", "DSUUUDSUUD")[cfg]
    pss = np.asarray(O.pss_fd(n_id_2))
    for fr in range(n_frames):
        f = w[fr * 19200:(fr + 1) * 19200]
        where = _symbols(f, cp_normal)
        for (slot, sym), (start, cp) in where.items():
            kind = kinds[slot >> 1]
            silent = kind == "U" or (kind == "S" and (slot & 1) * n_symb + sym >= dwpts)
            seg = f[start:start + cp + 128]
            if silent:
                assert not seg.any(), (slot, sym)
            else:
                assert np.abs(seg).max() > 0, (slot, sym)
                assert np.allclose(seg[:cp], seg[128:], atol=1e-12), "cyclic prefix"
        for half in (0, 10):
            assert np.allclose(_bins62(f, *where[(2 + half, 2)]), pss, atol=1e-12)
            sss = np.asarray(O.sss_fd(n_id_1, n_id_2, half), np.float64)
            assert np.allclose(_bins62(f, *where[(1 + half, n_symb - 1)]), sss, atol=1e-12)
            # and the FDD positions carry no synchronisation signal
            assert not np.allclose(_bins62(f, *where[(half, n_symb - 1)]), pss, atol=1e-3)


def test_tdd_key_reaches_make_signal_and_bad_dwpts_is_refused(synth):
    sig, _, truth = synth.make_signal(np.random.default_rng(2), FC, [dict(n_id_1=1, n_id_2=0, t0=0.0, tdd=(0, 3), port_gains=[1.0], n_ports=1)], n_cap=19200)
    assert truth[0]["tdd"] == (0, 3)
    # configuration 0: subframes 2-4 are uplink -- samples 2 * 1920 + guard .. 5 * 1920 - guard of the resampled signal are silent
    assert np.abs(sig[2 * 1920 + 40:5 * 1920 - 40]).max() < 1e-3 * np.abs(sig[:1920]).max()
    with pytest.raises(ValueError):
        synth.cell_waveform(1, 1, 0, tdd=(0, 2))


# ---------------------------------------------------------------- recovery of a planted cell
def _t0(peak, cp_normal, half=0):
    """the timing that puts a PSS occurrence's peak (the start of its cyclic prefix, `ind`) at sample `peak` of the buffer"""
    P = 2204 if cp_normal else 2272
    return float((P - (peak + 9) + 9600 * half) % 19200)


# (name, cell keys, SNR dB, expected ind of the first peak or None)
CASES = [
    ("config 2, DwPTS 10, normal CP", dict(tdd=(2, 10), t0=5000.0), 5, None),
    ("config 0, DwPTS 3, extended CP", dict(tdd=(0, 3), cp_normal=False, t0=7777.0), 5, None),
    ("config 0, DwPTS 3, normal CP, peak at 95", dict(tdd=(0, 3), t0=_t0(95, True)), 5, 95),
    ("config 1, DwPTS 9, normal CP, -3 dB", dict(tdd=(1, 9), t0=12000.0), -3, None),
    ("config 6, DwPTS 8, extended CP", dict(tdd=(6, 8), cp_normal=False, t0=333.0), 5, None),
    ("config 5, DwPTS 11, normal CP, 2200 Hz", dict(tdd=(5, 11), t0=15000.0, f_off=2200.0), 5, None),
    ("peak at 468: moved by the room rule", dict(tdd=(2, 10), t0=_t0(468, True)), 5, 468),
    ("peak at 473: not moved", dict(tdd=(2, 10), t0=_t0(473, True, 1)), 5, 473),
    ("extended CP, peak at 198", dict(tdd=(1, 9), cp_normal=False, t0=_t0(198, False)), 5, 198),
    ("extended CP, peak at 458", dict(tdd=(1, 9), cp_normal=False, t0=_t0(458, False, 1)), 5, 458),
    ("ind comes out as -1", dict(tdd=(2, 10), t0=_t0(-1, True)), 5, -1),
    ("one port", dict(tdd=(2, 10), n_ports=1, t0=4000.5), 5, None),
    ("four ports", dict(tdd=(1, 9), n_ports=4, t0=14000.25), 5, None),
]


@pytest.mark.parametrize("name, keys, snr, ind", CASES, ids=[c[0] for c in CASES])
def test_planted_tdd_cell_is_recovered(synth, name, keys, snr, ind):
    cell = dict(n_id_1=77, n_id_2=2, cp_normal=True, n_ports=2, n_rb_dl=25, sfn0=500, f_off=300.0)
    cell.update(keys)
    cap, _ = synth.make_capbuf(3, FC, [cell], snr_db=snr, quantise=False, n_cap=153600)
    peaks = [p for p in R.oracle_peaks(cap, F_SET, FC, FC, FS) if p.n_id_2 == cell["n_id_2"]]
    assert peaks, "no PSS peak"
    pk = peaks[0]
    if ind is not None:
        assert abs(pk.ind - ind) <= 1, pk.ind
        moved = pk.ind + 9 < 482
        assert moved == (ind < 473)
    assert abs(cell["f_off"] - pk.freq) < (2330.0 if cell["cp_normal"] else 2000.0)      # inside the estimate's unambiguous range
    c = R.per_peak(pk, cap, FC, FC, FS, R.GEO["tdd"])
    assert c is not None, "the planted cell did not decode"
    assert (c.n_id_1, c.n_id_2, c.cp_type) == (cell["n_id_1"], cell["n_id_2"], 1 if cell["cp_normal"] else 2)
    assert (c.n_ports, c.n_rb_dl) == (cell["n_ports"], cell["n_rb_dl"])
    planted = (-cell["t0"]) % 19200 - 2
    d = (c.frame_start - planted + 9600) % 19200 - 9600
    assert abs(d) <= 1.0, (c.frame_start, planted)
    # the SFN of the frame that starts at the reported frame_start
    assert c.sfn == (cell["sfn0"] + int(round((cell["t0"] + c.frame_start + 2) / 19200))) % 1024
    assert abs(c.freq_superfine - cell["f_off"]) < 100.0, c.freq_superfine
    # the same peak through the FDD geometry reads the wrong window: no cell (what the library did before it had a duplex mode)
    if snr >= 5 and ind is None:
        assert R.per_peak(pk, cap, FC, FC, FS, R.GEO["fdd"]) is None
