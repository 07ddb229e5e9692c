"""GPU test of sweep.measure_wideband behind sweep.search_wideband: one 30.72 Msps capture (K = 16) of synth.make_wideband_cell with
a 25 RB cell (measured at R = 4) on the centre carrier and a 6 RB cell 5 MHz above it.

Every decoded cell gets a record.  Restricted to 6 RB the wide record is the narrow one: the same capture through the same
decimation, so it is held to the two filters' passband ripple, 2 x 0.0034 dB (include/lcs.h: lcs_channelize), plus the quantity's own
1e-9.  The full record's rsrp is the generator's: scale^2 |g_0|^2 / n_ports per reference element at the cell's own rate.  Its bar, 0.1
dB, is the sum of what can differ: the measurement filter's ripple (0.0034 dB); the estimate's own scatter -- 244 rows x 49 pair
products at 20 dB SNR, relative standard deviation sqrt((2 / snr + 1 / snr^2) / 11956) = 1.3e-3, four of them 0.023 dB; and the loss of
a reference element to a timing error of the search of up to one 1.92 Msps sample beyond the cyclic prefix's slack, 4 of 512 samples
of a symbol leaking at most 0.07 dB."""
import numpy as np
import pytest

from conftest import load_pkg

pytestmark = pytest.mark.gpu
FS = 1.92e6
K = 16
FC_CENTRE = 1.8425e9
NEIGHBOUR = FC_CENTRE + 5.0e6
GAINS = [1.0, 0.7j]
N_OUT = 153584


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def capture(pkg):
    wide = dict(n_id_1=52, n_id_2=1, n_ports=2, port_gains=GAINS, f_off=1200.0, t0=4321.0, sfn0=8)
    narrow = dict(n_id_1=120, n_id_2=2, n_ports=1, n_rb_dl=6, f_off=-800.0, t0=15000.0, gain_db=-3.0, sfn0=20)
    x, truth, scale = pkg.synth.make_wideband_cell(11, FC_CENTRE, K, [(FC_CENTRE, 4, 25, wide)], [(NEIGHBOUR, [narrow])], snr_db=20.0, n_in=153600 * K)
    return x, truth, scale


@pytest.fixture(scope="module")
def searched(pkg, capture):
    import torch
    x, truth, scale = capture
    d = torch.from_numpy(x).cuda()
    s = pkg.Searcher(0)
    carriers = np.array([FC_CENTRE, NEIGHBOUR])
    cells = pkg.sweep.search_wideband(s, d.data_ptr(), pkg.FMT_C64, x.size, FS * K, K, FC_CENTRE, carriers, np.array([-5e3, 0.0, 5e3]), n_out=N_OUT, meas=True)
    yield s, d, carriers, cells
    s.close()


def test_every_decoded_cell_gets_a_record_and_the_full_one_reads_the_generator(pkg, capture, searched):
    x, truth, scale = capture
    s, d, carriers, cells = searched
    ids = [[c["n_id_cell"] for c in row if c["n_rb_dl"] != -1] for row in cells]
    assert 52 * 3 + 1 in ids[0] and 120 * 3 + 2 in ids[1], ids
    recs = pkg.sweep.measure_wideband(s, d.data_ptr(), pkg.FMT_C64, x.size, FS * K, FC_CENTRE, K, cells, carriers)
    assert [len(r) for r in recs] == [len(c) for c in cells]
    for row, rr in zip(cells, recs):
        for c, r in zip(row, rr):
            if c["n_rb_dl"] == -1:
                assert r is None and "meas_wide" not in c
                continue
            assert r is c["meas_wide"] and r.status == 0 and r.n_rb == c["n_rb_dl"] and r.n_fft == 128 * pkg.sweep.meas_rate(c["n_rb_dl"])
            assert r.dl_mask == c["meas"].dl_mask == 0x3FF and r.n_rows == 244
            assert abs(r.rsrq - r.n_rb * r.rsrp[0] / r.rssi) <= 1e-12 * r.rsrq      # rsrq uses n_rb
    big = next(c for c in cells[0] if c["n_id_cell"] == 52 * 3 + 1)
    assert (big["n_rb_dl"], big["n_ports"], big["meas_wide"].n_rb, big["meas_wide"].n_fft) == (25, 2, 25, 512)
    for p in range(2):
        want = 10 * np.log10(scale ** 2 * abs(GAINS[p]) ** 2 / 2)
        print("port %d: rsrp_db %.4f, the generator's %.4f" % (p, big["meas_wide"].rsrp_db[p], want))
        assert abs(big["meas_wide"].rsrp_db[p] - want) <= 0.1
    prof = 10 * np.log10(big["meas_wide"].rsrp_rb[0] / big["meas_wide"].rsrp[0])
    print("profile over the 25 RB, dB about the whole: %.3f .. %.3f; sinr %.2f dB, rsrq %.2f dB" % (prof.min(), prof.max(), big["meas_wide"].sinr_db[0], big["meas_wide"].rsrq_db))
    assert np.abs(prof).max() < 0.5
    # the narrow measurement of the same cell sees 6 of the 25 RB at a quarter of the rate: its bins hold a quarter of the power
    assert abs(big["meas"].rsrp_db[0] + 10 * np.log10(4) - big["meas_wide"].rsrp_db[0]) <= 0.1 + 2 * 0.0034


def test_restricted_to_six_resource_blocks_it_is_the_narrow_measurement(pkg, capture, searched):
    x, _, _ = capture
    s, d, carriers, cells = searched
    recs = pkg.sweep.measure_wideband(s, d.data_ptr(), pkg.FMT_C64, x.size, FS * K, FC_CENTRE, K, cells, carriers, n_rb=6)
    n = 0
    for row, rr in zip(cells, recs):
        for c, r in zip(row, rr):
            if r is None:
                continue
            m = c["meas"]
            assert (r.status, r.n_rb, r.n_fft, r.n_rows, r.n_ports, r.dl_mask) == (0, 6, 128, m.n_rows, m.n_ports, m.dl_mask)
            bar = 2 * 0.0034 + 1e-9
            print("cell %d: narrow rsrp_db %.6f, wide at 6 RB %.6f" % (c["n_id_cell"], m.rsrp_db[0], r.rsrp_db[0]))
            assert abs(r.rsrp_db[0] - m.rsrp_db[0]) <= bar and abs(r.rsrq_db - m.rsrq_db) <= bar
            n += 1
    assert n >= 2


def test_what_measure_wideband_refuses_and_the_capture_in_place(pkg, capture, searched):
    import torch
    x, _, _ = capture
    s, d, carriers, cells = searched
    args = lambda **kw: dict(dict(searcher=s, d_wide_ptr=d.data_ptr(), fmt=pkg.FMT_C64, n_in=x.size, fs_in=FS * K, fc_centre=FC_CENTRE, decim_search=K,
                                  cells_per_carrier=cells, carriers=carriers), **kw)
    with pytest.raises(ValueError, match="in place"):
        pkg.sweep.measure_wideband(**args(n_rb=100))                       # K / R = 1 on the neighbour's carrier, off the centre
    with pytest.raises(ValueError, match="in place"):
        pkg.sweep.measure_wideband(**args(n_rb=100, fmt=pkg.FMT_IQ_S16, cells_per_carrier=cells[:1], carriers=carriers[:1]))
    with pytest.raises(ValueError, match="rational"):
        pkg.sweep.measure_wideband(**args(fs_in=20e6))
    with pytest.raises(ValueError, match="integer decimation"):
        pkg.sweep.measure_wideband(**args(fs_in=FS * 12, n_rb=50))         # K = 12, R = 8
    with pytest.raises(ValueError, match="cell lists"):
        pkg.sweep.measure_wideband(**args(carriers=carriers[:1]))
    # a complex64 capture centred on the carrier is measured in place at K = R
    rec = pkg.sweep.measure_wideband(**args(n_rb=100, cells_per_carrier=cells[:1], carriers=carriers[:1]))[0]
    big = next(r for c, r in zip(cells[0], rec) if c["n_id_cell"] == 52 * 3 + 1)
    assert (big.status, big.n_rb, big.n_fft) == (0, 100, 2048)
    # the 25 RB of the cell sit in the middle of the hundred (RB 37.5 .. 62.5); below them there is noise only, and the profile of
    # the received power shows the neighbour's 6 RB 5 MHz = 27.8 RB above the centre (RB 74.8 .. 80.8), where this cell has nothing
    mid, below = big.rsrp_rb[0][38:62], big.rsrp_rb[0][:30]
    assert mid.min() > 20 * below.max()
    assert big.rssi_rb[76:80].min() > 5 * big.rssi_rb[:30].max() and big.rsrp_rb[0][76:80].max() < mid.min() / 3
