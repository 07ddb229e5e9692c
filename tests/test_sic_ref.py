"""The cancellation rule on the CPU: sic_ref (numpy, fp64) between two runs of the oracle's search.

A cell 6 dB under a neighbour with the same n_id_2 and almost the same timing is invisible to peak_search (the +-274 rule);
after the neighbour's PSS, SSS, CRS and PBCH are rebuilt and subtracted it is an ordinary detection."""
import numpy as np
import pytest

import oracle as O
import sic_cases as K
import sic_ref as R
import sss_duplex_ref as D


def ids(cells):
    return [c.n_id_cell() for c in cells]


def search(x, tdd=False):
    O.set_threads(8)
    if not tdd:
        return O.search_capbuf(x, K.F_SET, K.FC, K.FC, K.FS)[0]
    return D.search_peaks(D.oracle_peaks(x, K.F_SET, K.FC, K.FC, K.FS), x, K.FC, K.FC, K.FS, D.GEO["tdd"])


def uncovered(x, tdd=False):
    found = search(x, tdd)
    assert ids(found) == [K.ID_S]
    res, info = R.cancel(x, found, K.FC, K.FC, K.FS, duplex=R.TDD if tdd else R.FDD)
    after = search(res, tdd)
    assert K.ID_W in ids(after) and K.ID_S not in ids(after)
    w = after[ids(after).index(K.ID_W)]
    assert (w.n_ports, w.sfn) == (2, K.W["sfn0"] + 1)      # sfn0 is the frame the transmitter was in at t0 before the capture
    return found, info


def test_pair_float():
    found, info = uncovered(K.pair())
    assert found[0].sfn == K.S["sfn0"] + 1                 # decode_mib's rule: the record's sfn is the grid's first frame
    assert abs(abs(info[0]["gain"]) - np.sqrt(2.0)) < 0.15 # synth sends the sync signals at sqrt(n_ports) on port 0


def test_pair_u8():
    uncovered(K.pair_u8()[0])


def test_s_alone_leaves_nothing():
    x = K.s_alone()
    found = search(x)
    assert ids(found) == [K.ID_S]
    res, info = R.cancel(x, found, K.FC, K.FC, K.FS)
    assert search(res) == []
    # the yardstick of the device (test_gpu_sic.py): with noise 15 dB below the sync symbols no more than ~15 dB + the
    # estimator's averaging gain can go; measured 17.6 dB
    assert 15.0 < info[0]["suppression_db"] < 20.0
    assert info[0]["n_sym"] == 1119                        # 80 ms of 7-symbol slots, less the cut symbols at both ends


def test_tdd_pair():
    uncovered(K.tdd_pair(), tdd=True)


def test_tdd_configuration_widens_the_mask():
    """with the configuration known (2: DSUDDDSUDD) CRS and PBCH go in subframes 0, 3, 4, 5, 8, 9 and in symbol 0 of 1 and 6 too: 26
    reference symbols per frame instead of 8 -- 3.25 times the CRS energy by count, somewhat less in fact, because the estimate from
    two subframes is the noisier one and its noise is energy too (so the bounds are 2.7 .. 3.4); the sync and PBCH energies move
    by a few per cent with the estimate; and W is still uncovered"""
    x = K.tdd_pair()
    found = search(x, tdd=True)
    assert ids(found) == [K.ID_S]
    _, a = R.cancel(x, found, K.FC, K.FC, K.FS, duplex=R.TDD)
    res, b = R.cancel(x, found, K.FC, K.FC, K.FS, duplex=R.TDD, ul_dl_config=[2])
    assert abs(b[0]["power"][0] / a[0]["power"][0] - 1) < 0.1 and 2.7 < b[0]["power"][2] / a[0]["power"][2] < 3.4
    assert R.dl_mask_for(R.TDD, 2) == (0x339, True) and R.dl_mask_for(R.TDD, -1) == (0x021, False) and R.dl_mask_for(R.FDD, 2) == (0x3ff, False)
    after = search(res, tdd=True)
    assert K.ID_W in ids(after) and K.ID_S not in ids(after)
    geo = R.geometry(found[0], x.size, K.FC, K.FC, K.FS)
    used = {(t // 7 % 20) >> 1 for t in range(geo["t_lo"], geo["t_hi"] + 1) if R.usable(geo, t, 0x339, True)}
    assert used == {0, 1, 3, 4, 5, 6, 8, 9}
    assert not R.usable(geo, 7 * 2 + 1, 0x339, True) and R.usable(geo, 7 * 2, 0x339, True) and not R.usable(geo, 7 * 3, 0x339, True)


def test_extended_cp_pair():
    found, info = uncovered(K.ext_pair())
    assert found[0].cp_type == 2 and info[0]["n_sym"] == 959


def test_mask_selects_components():
    x = K.s_alone()
    found = search(x)
    _, a = R.cancel(x, found, K.FC, K.FC, K.FS, mask=R.PSS | R.SSS)
    assert a[0]["power"][2] == 0 and a[0]["power"][3] == 0 and a[0]["power"][0] > 0


@pytest.mark.parametrize("normal, frame_start, ppm", [(True, 14198.0, 0.0), (True, 3.3, 120.0), (False, 19190.7, -120.0), (False, 9000.5, 40.0)])
def test_owner_tiles(normal, frame_start, ppm):
    """every sample of the covered stretch has exactly one owner, in symbol order, and its offset continues the window periodically"""
    c = O.new_cell(frame_start=frame_start, freq_fine=-ppm * 1e-6 * K.FC, freq_superfine=0.0, cp_type=1 if normal else 2)
    geo = R.geometry(c, 153600, K.FC, K.FC, K.FS)
    n = np.arange(153600)
    sym, off = R.owner(geo, n)
    t = np.arange(geo["t_lo"], geo["t_hi"] + 1)
    a = geo["a"](np.append(t, geo["t_hi"] + 1))
    a[-1] = geo["w"](geo["t_hi"]) + 128
    walk = np.full(153600, geo["t_lo"] - 1)
    for i, tt in enumerate(t):
        walk[a[i]:a[i + 1]] = tt
    assert np.array_equal(sym, walk)
    assert np.all(np.diff(a) > 128) and a[0] >= 0 and a[-1] <= 153600
    inside = sym >= geo["t_lo"]
    assert np.array_equal(off[inside], (n[inside] - geo["w"](sym[inside])) % 128)
