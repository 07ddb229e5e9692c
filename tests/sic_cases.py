"""The captures of the cancellation tests: a strong cell S and a cell W 6 dB below it with the same n_id_2, three samples later."""
import numpy as np

from conftest import load_pkg

FC = 739e6
FS = 1.92e6
F_SET = np.array([-5e3, 0.0, 5e3])
SNR_DB = 15.0
RMS = 0.15
SEED = 1

S = dict(n_id_1=10, n_id_2=1, t0=5000.0, sfn0=8, port_gains=[1, 0.7j], f_off=300.0, load=0.5)
W = dict(n_id_1=77, n_id_2=1, t0=5003.0, sfn0=100, port_gains=[0.9j, -0.8], gain_db=-6.0, f_off=300.0, load=0.5)
ID_S, ID_W = 31, 232

PORT_GAINS = {1: [1], 2: [1, 0.7j], 4: [1, 0.7j, -0.6, 0.5 - 0.5j]}


def variant(cells, **kw):
    return [dict(c, **kw) for c in cells]


def s_ports(n_ports):
    return dict(S, n_ports=n_ports, port_gains=PORT_GAINS[n_ports])


def capture(cells, seed=SEED, quantise=False):
    """-> complex128 capture (quantise: what the receiver computes from the dongle's bytes, and the bytes)"""
    synth = load_pkg().synth
    rng = np.random.default_rng(seed)
    sig, ref_pow, _ = synth.make_signal(rng, FC, cells)
    x = synth.add_noise_and_quantise(rng, sig, ref_pow, SNR_DB, RMS, quantise=quantise)
    if quantise:
        return synth.iq_u8_to_complex(x), x
    return x


_cache = {}


def cached(name, cells, quantise=False):
    key = (name, quantise)
    if key not in _cache:
        _cache[key] = capture(cells, quantise=quantise)
    return _cache[key]


def pair():
    return cached("pair", [S, W])


def pair_u8():
    return cached("pair", [S, W], quantise=True)


def s_alone():
    return cached("s", [S])


def s_alone_u8():
    return cached("s", [S], quantise=True)


def noise_only():
    return cached("noise", [])


def tdd_pair():
    return cached("tdd", variant([S, W], tdd=(2, 9)))


def ext_pair():
    return cached("ext", variant([S, W], cp_normal=False))
