"""sweep.search_wideband(meas=True) and sweep.meas_with_gain: the measurement of a band search from one wideband capture with two
planted carriers, on complex<float> carriers and on 8-bit ones, on one power scale.

The two paths differ by the 8-bit quantisation of the carriers (Searcher.channelize_u8: component rms in (16, 32] codes, so rounding
to a code adds noise of 1/12 code^2 per component, 8e-5 to 3.3e-4 of the carrier's power).  The test measures that effect on the
float path first -- the complex<float> carriers quantised on the host by the channelizer's own rule (chan_u8_ref.quantise_ref) and
measured by the same stage on the same record: how far rsrp[0] and rssi move (relative) and 10 log10 rsrq and port 0's SINR (dB), the
worst of the two carriers -- and the bar on search_wideband's two outputs is twice that figure, quantity by quantity.
Measured on one MI355X, on the float path: rsrp 4.19e-4, rssi 1.54e-4, rsrq 0.0021 dB, SINR 0.0083 dB; search_wideband's two outputs
differ by 4.19e-4, 1.54e-4, 0.0021 dB and 0.0083 dB -- the device's bytes are the host rule's."""
import numpy as np
import pytest

import chan_ref as R
import chan_u8_ref as U
from conftest import load_pkg

pytestmark = pytest.mark.gpu
FS_OUT = 1.92e6
PLACED = R.WB_PLACED[1:]      # 740.5 MHz: extended CP, 2 ports; 742.6 MHz: normal CP, 4 ports, 3 dB up
CARRIERS = np.array([c for c, _ in PLACED])
N_OUT = R.WB["n_out"]


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def wb(pkg):
    import torch
    iq, _ = pkg.synth.make_wideband(R.WB["seed"], R.WB["fc_centre"], R.WB["decim"], PLACED, R.WB["snr_db"], pkg.FMT_IQ_S16)
    return dict(d=torch.from_numpy(iq).cuda(), n_in=iq.size // 2, fs_in=R.WB["decim"] * FS_OUT, D=R.WB["decim"])


def _diff(a, b):
    return dict(rsrp=abs(a.rsrp[0] / b.rsrp[0] - 1), rssi=abs(a.rssi / b.rssi - 1), rsrq_db=abs(a.rsrq_db - b.rsrq_db), sinr_db=abs(a.sinr_db[0] - b.sinr_db[0]))


def _worst(ds):
    return {k: max(d[k] for d in ds) for k in ds[0]}


def _capbuf(codes):
    c = codes.astype(np.float64)
    return (c[:, 0] - 127.0) / 128.0 + 1j * ((c[:, 1] - 127.0) / 128.0)


def test_float_and_8_bit_carriers_agree_within_the_quantisation(pkg, wb):
    import torch
    with pkg.Searcher(0) as s:
        args = (s, wb["d"].data_ptr(), pkg.FMT_IQ_S16, wb["n_in"], wb["fs_in"], wb["D"], R.WB["fc_centre"], CARRIERS, R.WB_GRID)
        f = pkg.sweep.search_wideband(*args, n_out=N_OUT, out="c64", meas=True)
        assert s.cell_meas_mode is False, "the mode is put back"
        plain = pkg.sweep.search_wideband(*args, n_out=N_OUT, out="c64")
        u = pkg.sweep.search_wideband(*args, n_out=N_OUT, out="u8", meas=True)
        # the float path: the same carriers quantised on the host, the same record, the same stage
        y = torch.zeros((len(CARRIERS), N_OUT), dtype=torch.complex64, device="cuda")
        s.channelize_rational(wb["d"].data_ptr(), pkg.FMT_IQ_S16, wb["n_in"], wb["fs_in"], 1, wb["D"], CARRIERS - R.WB["fc_centre"], y.data_ptr(), N_OUT)
        s.sync()
        y = y.cpu().numpy().astype(np.complex128)
        codes, gain, _ = U.quantise_ref(y)
        on_float = []
        for k, fc in enumerate(CARRIERS):
            c = plain[k][0]
            # (a code stands for (code - 127) / gain on the float carrier's scale: _capbuf's dongle convention divides by 128 more)
            m = [s.cell_meas(c, s.extract_tfg(c, x, fc, fc, FS_OUT)[0]) for x in (y[k], _capbuf(codes[k]) * 128.0 / gain[k])]
            on_float.append(_diff(m[0], m[1]))
    got = []
    for k in range(len(CARRIERS)):
        assert len(f[k]) == len(u[k]) == len(plain[k]) == 1
        want_id = PLACED[k][1][0]["n_id_2"] + 3 * PLACED[k][1][0]["n_id_1"]
        assert f[k][0]["n_id_1"] * 3 + f[k][0]["n_id_2"] == u[k][0]["n_id_1"] * 3 + u[k][0]["n_id_2"] == plain[k][0].n_id_cell() == want_id
        # an 8-bit capture stands for code / 128 (the dongle convention): one power scale over the 8-bit carriers is the float
        # carriers' scale divided by 128^2, again a power of two
        a, b = f[k][0]["meas"], pkg.sweep.meas_with_gain([[u[k][0]["meas"]]], [1.0 / 128])[0][0]
        assert a.status == b.status == 0 and (a.n_rows, a.n_ports, a.dl_mask) == (b.n_rows, b.n_ports, b.dl_mask) and a.dl_mask == 0x3FF
        got.append(_diff(a, b))
        # one power scale: the float records and the scaled 8-bit ones agree in pss_pow as they do in rsrp
        assert abs(u[k][0]["pss_pow"] * 128.0 ** 2 / f[k][0]["pss_pow"] - 1) < 0.01
    print("quantisation on the float path:", _worst(on_float))
    print("search_wideband c64 against u8:", _worst(got))
    bar = _worst(on_float)
    assert all(0 < v < 0.05 for v in bar.values()), bar      # (a figure of zero would make the bar empty: the quantisation does move every quantity)
    for k, v in _worst(got).items():
        assert v <= 2 * bar[k], (k, v, bar[k])


def test_meas_with_gain_is_exact_on_crafted_records(pkg):
    def rec(status, scale):
        m = pkg.CellMeas()
        m.status, m.n_rows, m.n_ports, m.dl_mask = status, 285, 2, 0x3FF
        m.rsrp[0], m.rsrp[1], m.noise[0], m.noise[1] = 0.3 * scale, 0.1 * scale, 0.013 * scale, -1e-5 * scale
        m.rssi, m.rsrq = 7.7 * scale, 6 * 0.3 / 7.7
        for i, v in enumerate((1.5, -2.25, 1e-3, 1e3)):
            m.a_re_im[i] = v * scale
        return m
    gains = np.array([1.0, 64.0, 0.125, 2.0 ** 20])
    per = [[rec(0, g * g), rec(-1, g * g), rec(pkg.MEAS_NOT_MEASURED, 1.0)] for g in gains]
    out = pkg.sweep.meas_with_gain(per, gains)
    one = rec(0, 1.0)
    for k, g in enumerate(gains):
        a = out[k][0]
        assert bytes(a) == bytes(one), "divided by gain^2 exactly: a power of two"
        assert a.sinr == one.sinr and a.rsrq == one.rsrq and a.sinr[1] == float("inf")
        assert bytes(out[k][1]) == bytes(per[k][1]) and bytes(out[k][2]) == bytes(per[k][2]), "records without a measurement pass unchanged"
        assert bytes(per[k][0]) == bytes(rec(0, g * g)), "the input is not touched"
    with pytest.raises(ValueError, match="4 carriers, 3 gains"):
        pkg.sweep.meas_with_gain(per, gains[:3])
