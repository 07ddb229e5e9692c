"""Plant and recover on the CPU: the generator's PCFICH (synth.cell_waveform_wide(cfi=...)) through the numpy grid
(tests/meas_wide_ref.py) and the numpy statement of the rule (tests/pcfich_ref.py) -- the decoder's reference is checked against
planted values, not against itself -- and the generator's new argument against the generator without it.

The seeds are those of pcfich_cases.pcfich_capture: with them the numpy rule reads every planted subframe at 20 dB with a margin of
at least 0.2 (the smallest seen is printed)."""
import numpy as np
import pytest

import meas_wide_cases as WC
import meas_wide_ref as WR
import pcfich_cases as PC
import pcfich_ref as PR
from conftest import load_pkg

FS = 1.92e6
N_ID = WC.CELL_ID[1] + 3 * WC.CELL_ID[0]


def _grid(R, n_rb, cp, n_ports, n_ofdm):
    n = PR.n_symb_of(cp)
    rows = [r for g in range(PR.n_sf_of(n_ofdm, cp)) for r in (2 * g * n, 2 * g * n + 1) if r < n_ofdm]
    cap = PC.pcfich_capture(R, n_rb, cp, n_ports)
    return WR.grid(cap, WC.FRAME_START * R, 0.0, cp, WC.FC, WC.FC, FS * R, 128 * R, n_rb, n_ofdm, rows)[0]


@pytest.mark.parametrize("shape", [(1, 6), (2, 15)], ids=str)
@pytest.mark.parametrize("cp", [1, 2])
@pytest.mark.parametrize("n_ports", PC.PORTS)
def test_planted_cfi_is_recovered_and_a_wrong_identity_is_not(shape, cp, n_ports):
    R, n_rb = shape
    n_ofdm = 40 * PR.n_symb_of(cp) + 3                       # two frames and the head of a subframe
    tfg = _grid(R, n_rb, cp, n_ports, n_ofdm)
    ref = PR.decode(tfg, N_ID, cp, n_ports, n_rb)
    print(shape, cp, n_ports, "margins %.3f .. %.3f" % (ref["margin"].min(), ref["margin"].max()))
    assert ref["n_sf"] == 21 and ref["n_decoded"] == 21
    assert np.array_equal(ref["cfi"], PC.planted_of_grid(21))
    assert ref["min_margin"] >= 0.2
    assert ref["n_cfi"] == [9, 6, 6] and ref["mean_n_ctrl_sym"] == (9 + 12 + 18) / 21 + (n_rb <= 10)
    # another cell's identity on the same grid: other elements, another scrambling, another reference sequence
    other = PR.decode(tfg, N_ID + 7, cp, n_ports, n_rb)
    assert other["margin"][other["cfi"] > 0].mean() < ref["min_margin"]
    # the mask picks subframes, and leaves the others' entries zero
    part = PR.decode(tfg, N_ID, cp, n_ports, n_rb, 0x021)
    assert list(np.flatnonzero(part["cfi"])) == [0, 5, 10, 15, 20] and np.array_equal(part["corr"][5], ref["corr"][5]) and not part["corr"][1].any()


def test_generator_without_cfi_is_what_it_was_and_with_it_changes_the_pcfich_elements_alone():
    synth = load_pkg().synth
    args = (2, 41, 2, 2, 15)
    # cfi = None: the call existing tests pin, draw for draw
    for cp_normal, n_ports, tdd in ((True, 2, None), (False, 4, None), (True, 1, (1, 9))):
        a = synth.cell_waveform_wide(*args, cp_normal, n_ports=n_ports, rng=np.random.default_rng(5), tdd=tdd)
        b = synth.cell_waveform_wide(*args, cp_normal, n_ports=n_ports, rng=np.random.default_rng(5), tdd=tdd, cfi=None)
        assert a.tobytes() == b.tobytes()
    # without load and with the gains given, no value depends on a draw: the PCFICH elements are all that cfi changes
    n_id, R, n_rb = 2 + 3 * 41, 2, 15
    cols = PR.columns(n_id, n_rb)
    assert np.array_equal(cols, synth.pcfich_columns(n_id, n_rb))
    for cp_normal, n_ports in ((True, 1), (False, 2), (True, 4)):
        kw = dict(n_ports=n_ports, load=0.0, per_port=True, rng=np.random.default_rng(1))
        a = synth.cell_waveform_wide(1, 41, 2, R, n_rb, cp_normal, **kw)
        b = synth.cell_waveform_wide(1, 41, 2, R, n_rb, cp_normal, cfi=PC.planted_cfi, **dict(kw, rng=np.random.default_rng(1)))
        n_symb, n_fft = (7, 256) if cp_normal else (6, 256)
        pos = 0
        for slot in range(20):
            for sym in range(n_symb):
                cp = R * ((10 if sym == 0 else 9) if cp_normal else 32)
                seg = slice(pos + cp, pos + cp + n_fft)
                fa, fb = (np.fft.fft(x[:, seg], axis=-1) / np.sqrt(n_fft) for x in (a, b))
                fa, fb = (np.concatenate([f[:, n_fft - 6 * n_rb:], f[:, 1:6 * n_rb + 1]], axis=1) for f in (fa, fb))
                pos += cp + n_fft
                if sym or slot & 1:
                    assert np.abs(fa - fb).max() < 1e-12
                    continue
                rest = np.setdiff1d(np.arange(12 * n_rb), cols)
                assert np.abs(fa[:, rest] - fb[:, rest]).max() < 1e-12 and np.abs(fa[:, cols]).max() < 1e-12
                want = synth._tx_diversity(synth.pcfich_symbols(n_id, slot >> 1, PC.planted_cfi(0, slot >> 1)), n_ports)
                assert np.abs(fb[:, cols] - want / np.sqrt(n_ports)).max() < 1e-12
                # the bits behind the symbols: the codeword of 36.212 table 5.3.4-1 under the subframe's scrambling
                s = synth.pcfich_symbols(n_id, slot >> 1, PC.planted_cfi(0, slot >> 1))
                bits = np.empty(32, np.int64)
                bits[0::2], bits[1::2] = s.real < 0, s.imag < 0
                assert np.array_equal(bits ^ PR.scrambling(n_id, slot >> 1), PR.CODEWORDS[PC.planted_cfi(0, slot >> 1) - 1])


def test_make_wideband_cell_passes_cfi_through():
    synth = load_pkg().synth
    cell = dict(n_id_1=41, n_id_2=2, n_ports=2, f_off=0.0, t0=100.0, sfn0=4, load=0.0, port_gains=[1.0, 1.0])
    kw = dict(snr_db=None, n_in=2 * 19200 * 2 // 10)
    a = synth.make_wideband_cell(3, 739e6, 2, [(739e6, 2, 15, dict(cell))], **kw)[0]
    b = synth.make_wideband_cell(3, 739e6, 2, [(739e6, 2, 15, dict(cell))], cfi=2, **kw)[0]
    c = synth.make_wideband_cell(3, 739e6, 2, [(739e6, 2, 15, dict(cell, cfi=2))], **kw)[0]
    assert np.array_equal(b, c) and not np.array_equal(a, b)
