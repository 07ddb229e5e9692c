"""What the cell measurement tests share (tests/test_cell_meas_ref.py and test_cell_meas_host.py on the CPU,
tests/test_gpu_cell_meas.py on the GPU): crafted grids whose answer is planted, and planted capture buffers.

crafted(...) is modelled on tdd_config_ref.crafted_grid -- RS_DL of every port times a smooth channel, QPSK data, noise, the same
D / S / U kinds per subframe -- and returns the planted truth beside the grid; flat=True leaves out the amplitude ripple, so that the
rule's premise (a channel that hardly changes over 6 subcarriers) holds exactly and its outputs can be held against the truth.

The buffers are 80 ms of dongle bytes from the generator: the cell n_id_1 = 77, n_id_2 = 2 (normal CP, 2 ports, 25 RB) at 739 MHz at
15 / 8 / 2 / -3 dB, that cell with a weaker second one (extended CP, 1 port) beside it, and a 4-port cell through EPA fading; for TDD,
tdd_config_cases.BUFFERS as they are.  recovered(b) runs FDD buffer b through the oracle chain."""
import functools

import numpy as np

import oracle as O
import sss_duplex_ref as R
import tdd_config_ref as TR
from conftest import iq_u8_to_capbuf, load_pkg

FS = 1.92e6
FC = 739e6
GRID = np.arange(-5e3, 5e3 + 1, 5e3)
SEED = 7
_BASE = dict(n_id_1=77, n_id_2=2, cp_normal=True, n_ports=2, n_rb_dl=25, sfn0=500, f_off=300.0, t0=3000.0)
_SECOND = dict(n_id_1=3, n_id_2=0, cp_normal=False, n_ports=1, n_rb_dl=25, sfn0=500, f_off=300.0, gain_db=-4.0, t0=11111.0)
SNR_SERIES = (15.0, 8.0, 2.0, -3.0)
# (snr_db, cells) per buffer: 0..3 the SNR series of the base cell, 4 two cells, 5 four ports through EPA
BUFFERS = [(snr, [dict(_BASE)]) for snr in SNR_SERIES] + [
    (8.0, [dict(_BASE), dict(_SECOND)]),
    (8.0, [dict(_BASE, n_ports=4, channel="EPA", doppler_hz=5.0)]),
]


@functools.lru_cache(maxsize=None)
def u8(b):
    snr, cells = BUFFERS[b]
    return load_pkg().synth.make_capbuf(SEED, FC, cells, snr_db=snr, n_cap=153600)[0]


def cap(b):
    return iq_u8_to_capbuf(u8(b))


@functools.lru_cache(maxsize=None)
def recovered(b):
    """[(decoded cell, its raw grid, its tfoec-compensated grid)] of FDD buffer b, in peak order (the oracle chain)"""
    x = cap(b)
    out = []
    for pk in R.oracle_peaks(x, GRID, FC, FC, FS):
        c, _ = R.sss_detect(R.oracle_cell(pk), x, 3.0, FC, FC, FS, R.GEO["fdd"])
        if c.n_id_1 == -1:
            continue
        c = R.pss_sss_foe(c, x, FC, FC, FS, R.GEO["fdd"])
        tfg, ts = O.extract_tfg(c, x, FC, FC, FS)
        c, tfgc, _ = O.tfoec(c, tfg, ts, FC, FC)
        c = O.decode_mib(c, tfgc)
        if c.n_rb_dl != -1:
            out.append((c, tfg, tfgc))
    return out


# ---------------------------------------------------------------------------------------------------------------- crafted grids
def crafted(n_id_cell, cp_type, kinds, dwpts, n_ofdm, seed=0, snr_db=15.0, n_ports=1, flat=False, uplink="qpsk", uplink_gain=1.5):
    """-> (tfg [n_ofdm][72], truth).  Downlink rows (D subframes, the first `dwpts` symbols of S ones) carry RS_DL of the first
    n_ports ports times a channel -- a common phase per row that turns like a frequency offset, a phase ramp over the subcarriers
    like a timing offset, per-port complex gains, and unless `flat` a 25 % amplitude ripple over the subcarriers --, QPSK data of
    0.7 times port 0's amplitude elsewhere, and complex noise of variance 10^(-snr_db / 10); the other rows hold nothing
    (uplink="none") or QPSK of uplink_gain.  truth: rs_power [4] = |gain_p|^2 (the mean over the ripple is not folded in: it is the
    truth of flat grids), noise_var, row_power = the expected |.|^2 of a downlink row that carries port 0's reference signals."""
    rng = np.random.default_rng(seed)
    rs, sh = TR._rs(n_id_cell, cp_type)
    n = TR.n_symb_of(cp_type)
    k = np.arange(72)
    qpsk = lambda size: ((1 - 2.0 * rng.integers(0, 2, size)) + 1j * (1 - 2.0 * rng.integers(0, 2, size))) / np.sqrt(2.0)
    noise_var = 10 ** (-snr_db / 10)
    sigma = np.sqrt(noise_var / 2.0)
    tau, f_row = 0.37 + 0.2 * rng.random(), 0.013 * (rng.random() - 0.5)
    port_gain = np.exp(2j * np.pi * rng.random(4)) * (0.8 + 0.4 * rng.random(4))
    tfg = np.zeros((n_ofdm, 72), np.complex128)
    for r in range(n_ofdm):
        sym, slot = r % n, (r // n) % 20
        kind = kinds[slot >> 1]
        down = kind == "D" or (kind == "S" and (slot & 1) * n + sym < dwpts)
        if not down:
            if uplink == "qpsk":
                tfg[r] = uplink_gain * qpsk(72)
            continue
        ramp = np.exp(-2j * np.pi * tau * (k - 35.5) / 128) * np.exp(2j * np.pi * f_row * r)
        ripple = np.ones(72) if flat else 1.0 + 0.25 * np.cos(2 * np.pi * k / 72 + r / 57.0)
        row = 0.7 * qpsk(72) * ramp * ripple * port_gain[0]
        row20 = slot * n + sym
        for port in range(4):
            if not sh[row20, port] >= 0:      # (the oracle marks "no reference signal of this port here" with NaN)
                continue
            idx = int(sh[row20, port]) + 6 * np.arange(12)
            row[idx] = rs[row20] * ramp[idx] * ripple[idx] * port_gain[port] if port < n_ports else 0.0
        tfg[r] = row + sigma * (rng.standard_normal(72) + 1j * rng.standard_normal(72))
    g2 = np.abs(port_gain) ** 2
    rs_power = np.where(np.arange(4) < n_ports, g2, 0.0)
    row_power = 48 * 0.49 * g2[0] + 12 * rs_power[0] + 12 * rs_power[1] + 72 * noise_var
    return tfg, dict(rs_power=rs_power, noise_var=noise_var, row_power=float(row_power))


# the stage's shapes on the GPU and the host twin's on the CPU: every n_id_cell mod 6, both CP types, whole grids, two frames, a
# partial last slot, 1 / 2 / 4 ports
SHAPES = [(96, 1, 854, 1), (97, 2, 732, 4), (98, 1, 280, 2), (99, 2, 240, 4), (100, 1, 283, 1), (101, 2, 245, 2), (503, 1, 854, 4), (0, 2, 732, 1)]
MASKS = [0x3FF, 0x021, 0x200, 0x339]      # all, the TDD default, one subframe, tdd_dl_mask(2)


@functools.lru_cache(maxsize=None)
def shape_grid(shape):
    n_id, cp, n_ofdm, ports = shape
    return crafted(n_id, cp, "DDDDDDDDDD", 0, n_ofdm, seed=n_id, n_ports=ports)[0]
