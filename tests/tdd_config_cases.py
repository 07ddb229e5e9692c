"""The planted TDD cells the uplink-downlink configuration tests share (tests/test_tdd_config_ref.py on the CPU,
tests/test_gpu_tdd_config.py on the GPU): six 80 ms buffers of dongle bytes from the generator, configurations 0, 1, 2, 4, 5, 6 on
buffers of one cell and configuration 3 beside a second cell, both CP types, 1 / 2 / 4 ports, every DwPTS class, EPA fading on two.
All at 8 dB: tools/tdd_config_accuracy.py (profiles/tdd/tdd_config_accuracy.json) shows cells at 5 dB and above with a margin far
over 0.1, which test_tdd_config_ref.py asserts for each of these.

recovered(b) runs buffer b through the CPU chain -- the oracle's xcorr_pss and peak_search, sss_detect and pss_sss_foe from the numpy
restatement in TDD mode, the oracle's extract_tfg / tfoec / decode_mib -- and the numpy rule on the oracle's UNCORRECTED grid."""
import functools

import numpy as np

import oracle as O
import sss_duplex_ref as R
import tdd_config_ref as TR
from conftest import iq_u8_to_capbuf, load_pkg

FS = 1.92e6
FC = 1.9e9            # band 39
GRID = np.arange(-5e3, 5e3 + 1, 2.5e3)
SNR_DB = 8.0
_BASE = dict(n_id_1=77, n_id_2=2, cp_normal=True, n_ports=2, n_rb_dl=25, sfn0=500, f_off=300.0)


def _cell(**kw):
    c = dict(_BASE)
    c.update(kw)
    return c


# (seed, cells) per buffer
BUFFERS = [
    (51, [_cell(tdd=(0, 3), cp_normal=False, n_id_1=12, n_id_2=0, t0=7777.0)]),
    (52, [_cell(tdd=(1, 9), t0=3000.0, channel="EPA", doppler_hz=5.0)]),
    (53, [_cell(tdd=(2, 10), t0=5000.0), _cell(tdd=(3, 10), cp_normal=False, n_id_1=3, n_id_2=0, t0=11111.0, f_off=-2700.0, gain_db=-2.0)]),
    (54, [_cell(tdd=(4, 12), n_id_1=150, n_id_2=1, n_ports=4, t0=14000.25, f_off=-900.0)]),
    (55, [_cell(tdd=(5, 8), cp_normal=False, n_id_1=40, n_id_2=1, t0=333.0, channel="EPA", doppler_hz=5.0)]),
    (56, [_cell(tdd=(6, 6), n_id_1=101, n_id_2=0, n_ports=1, t0=9000.5)]),
]


def planted(b):
    """{n_id_cell: (configuration, DwPTS class, cp_type)} of buffer b"""
    out = {}
    for c in BUFFERS[b][1]:
        cp = 1 if c["cp_normal"] else 2
        out[c["n_id_2"] + 3 * c["n_id_1"]] = (c["tdd"][0], TR.dwpts_rows(c["tdd"][1], cp), cp)
    return out


@functools.lru_cache(maxsize=None)
def u8(b):
    seed, cells = BUFFERS[b]
    return load_pkg().synth.make_capbuf(seed, FC, cells, snr_db=SNR_DB, n_cap=153600)[0]


def cap(b):
    return iq_u8_to_capbuf(u8(b))


@functools.lru_cache(maxsize=None)
def recovered(b):
    """[(decoded cell, its uncorrected grid, the numpy rule's record)] of buffer b, in peak order"""
    x = cap(b)
    out = []
    for pk in R.oracle_peaks(x, GRID, FC, FC, FS):
        c = R.per_peak(pk, x, FC, FC, FS, R.GEO["tdd"])
        if c is None:
            continue
        tfg, _ = O.extract_tfg(c, x, FC, FC, FS)
        out.append((c, tfg, TR.estimate(c.n_id_2 + 3 * c.n_id_1, c.cp_type, tfg)))
    return out
