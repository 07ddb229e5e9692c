"""GPU tests of the cancellation stage (lcs_sic_cancel_dev, lcs_search_capbuf_sic, lcs_search_batch_sic_dev; csrc/sic.hip).

The captures are those of tests/sic_cases.py: S, and W 6 dB below it with the same n_id_2 three samples later.  The plain search lists
S alone; with one cancellation round W is found.  The device residual is compared with tests/sic_ref.py (numpy, fp64) on the same
capture and the same records -- the reference is sic_ref, never the device."""
import numpy as np
import pytest

import sic_cases as K
import sic_ref as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu

# max |device residual - sic_ref residual| / rms(capture).  Measured on the first run (MI355X): 1.281e-7 on the S + W capture as
# complex64, 1.883e-7 with a 1-port S, 1.154e-7 with a 4-port S, 1.717e-7 on the TDD pair (the residual and the per-symbol table
# are complex64: 6e-8 relative to samples of a few rms; the transforms themselves run in fp64).  The bound is 10 x the value
# measured on the S + W capture, the margin for other seeds.
RESIDUAL_TOL = 1.281e-6


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def S(pkg):
    s = pkg.Searcher(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def S_tdd(pkg):
    s = pkg.Searcher(0)
    s.set_duplex(pkg.DUPLEX_TDD)
    yield s
    s.close()


def ids(cells):
    return [c.n_id_cell() for c in cells]


def plain(S, x):
    return S.search_capbuf(x, K.F_SET, K.FC, K.FC, K.FS)[0]


def with_sic(S, x, **kw):
    return S.search_capbuf_sic(x, K.F_SET, K.FC, K.FC, K.FS, **kw)


def dev_c64(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x.astype(np.complex64))).to("cuda:0")


def dev_u8(iq):
    import torch
    return torch.from_numpy(np.ascontiguousarray(iq)).to("cuda:0")


def cancel_c64(pkg, S, x, cells, mask=R.ALL):
    """-> (device residual complex64 as complex128, info, the capture as the device saw it)"""
    import torch
    d = dev_c64(x)
    res = torch.empty(x.size, dtype=torch.complex64, device="cuda:0")
    info = S.sic_cancel(d.data_ptr(), pkg.FMT_C64, 1, x.size, [cells], K.FC, K.FC, K.FS, res.data_ptr(), mask)[0]
    torch.cuda.synchronize()
    return res.cpu().numpy().astype(np.complex128), info, d.cpu().numpy().astype(np.complex128)


def residual_error(pkg, S, x, duplex=R.FDD):
    cells = plain(S, x)
    assert K.ID_S in ids(cells)
    got, info, seen = cancel_c64(pkg, S, x, cells)
    want, ref_info = R.cancel(seen, cells, K.FC, K.FC, K.FS, duplex=duplex)
    err = np.abs(got - want).max() / np.sqrt(np.mean(np.abs(seen) ** 2))
    return err, info, ref_info


def assert_same_record(u, v):
    for name, kind in type(u)._fields_:
        p, q = getattr(u, name), getattr(v, name)
        if isinstance(p, float):
            assert abs(p - q) <= 1e-6 * abs(q) + (1e-3 if name.startswith("freq") else 0.0), (name, p, q)
        else:
            assert p == q, (name, p, q)


def assert_info_close(got, ref):
    for c in range(4):
        assert abs(got.power[c] - ref["power"][c]) <= 1e-6 * ref["power"][c], (c, got.power[c], ref["power"][c])
    assert abs(got.gain - ref["gain"]) < 1e-8 and got.n_sym == ref["n_sym"]
    assert abs(got.pss_before - ref["pss_before"]) <= 1e-6 * ref["pss_before"] and abs(got.pss_after - ref["pss_after"]) <= 1e-4 * ref["pss_after"]


def test_hidden_cell_is_uncovered(pkg, S):
    x = K.pair()
    before = plain(S, x)
    assert ids(before) == [K.ID_S]
    cells, rounds, info = with_sic(S, x)
    assert sorted(ids(cells)) == [K.ID_S, K.ID_W] and rounds == [0, 1]
    assert bytes(cells[0]) == bytes(before[0])                       # round 0 is the plain call: field for field
    w = cells[1]
    assert (w.n_ports, w.n_rb_dl, w.sfn, w.cp_type) == (2, 50, K.W["sfn0"] + 1, 1)
    assert info[0].cancelled and info[0].n_sym == 1119 and info[0].n_pss == 16 and not info[1].cancelled
    assert abs(abs(info[0].gain) - np.sqrt(2.0)) < 0.15              # synth sends the sync signals at sqrt(n_ports)
    assert S.last_sic_stats() == dict(rounds=2, cancellations=1, added=1, dropped=0)
    # a third round cancels both and finds nothing new
    cells3, rounds3, info3 = with_sic(S, x, max_rounds=3)
    assert ids(cells3) == ids(cells) and rounds3 == [0, 1] and info3[1].cancelled
    assert S.last_sic_stats()["rounds"] == 3 and S.last_sic_stats()["added"] == 1


def test_residual_against_sic_ref(pkg, S):
    """measured on the first run: max |device - sic_ref| / rms = 1.281e-7; asserted: 10 x that (RESIDUAL_TOL)"""
    err, info, ref = residual_error(pkg, S, K.pair())
    print("residual: max |device - sic_ref| / rms = %.3e" % err)
    assert err < RESIDUAL_TOL
    for c in range(4):
        assert abs(info[0].power[c] - ref[0]["power"][c]) <= 1e-6 * ref[0]["power"][c]
    assert abs(info[0].gain - ref[0]["gain"]) < 1e-9
    assert info[0].n_sym == ref[0]["n_sym"]


@pytest.mark.parametrize("n_ports", [1, 4])
def test_residual_one_and_four_ports(pkg, S, n_ports):
    x = K.cached("s%d" % n_ports, [K.s_ports(n_ports), K.W])
    err, info, ref = residual_error(pkg, S, x)
    print("residual, %d-port S: max |device - sic_ref| / rms = %.3e" % (n_ports, err))
    assert err < RESIDUAL_TOL
    assert info[0].power[3] > 0 and abs(info[0].power[3] - ref[0]["power"][3]) <= 1e-6 * ref[0]["power"][3]


def test_suppression_on_s_alone(pkg, S):
    import torch
    x, (xq, iq) = K.s_alone(), K.s_alone_u8()
    cells = plain(S, x)
    assert ids(cells) == [K.ID_S]
    _, ref = R.cancel(x, cells, K.FC, K.FC, K.FS)
    _, info, _ = cancel_c64(pkg, S, x, cells)
    cells_q = plain(S, xq)
    d = dev_u8(iq)
    res = torch.empty(xq.size, dtype=torch.complex64, device="cuda:0")
    info_q = S.sic_cancel(d.data_ptr(), pkg.FMT_IQ_U8, 1, xq.size, [cells_q], K.FC, K.FC, K.FS, res.data_ptr())[0]
    # the same bytes as complex64: the two input formats of one capture
    _, info_qc, _ = cancel_c64(pkg, S, xq, cells_q)
    print("PSS suppression on S alone: sic_ref %.2f dB, device %.2f dB (complex64), %.2f dB (u8), %.2f dB (the u8 capture as complex64)"
          % (ref[0]["suppression_db"], info[0].suppression_db, info_q[0].suppression_db, info_qc[0].suppression_db))
    assert abs(info[0].suppression_db - ref[0]["suppression_db"]) < 1.0
    assert abs(info_q[0].suppression_db - ref[0]["suppression_db"]) < 1.0
    assert abs(info_q[0].suppression_db - info_qc[0].suppression_db) < 1.0
    # (u8 - 127) / 128 is exact in complex64: the two routes subtract from the same numbers
    assert np.array_equal(res.cpu().numpy(), cancel_c64(pkg, S, xq, cells_q)[0].astype(np.complex64))


def test_s_alone_and_noise_add_nothing(pkg, S):
    x = K.s_alone()
    before = plain(S, x)
    cells, rounds, info = with_sic(S, x)
    assert [bytes(c) for c in cells] == [bytes(c) for c in before] and ids(cells) == [K.ID_S] and rounds == [0]
    assert S.last_sic_stats() == dict(rounds=2, cancellations=1, added=0, dropped=0)
    cells, rounds, info = with_sic(S, K.noise_only(), max_rounds=4)
    assert cells == [] and rounds == [] and info == []
    assert S.last_sic_stats() == dict(rounds=1, cancellations=0, added=0, dropped=0)      # no decoded cell: nothing more is launched


def test_batch_equals_single_calls(pkg, S, S_tdd):
    import torch
    caps = [K.pair(), K.s_alone(), K.noise_only()]
    d = torch.stack([dev_c64(x) for x in caps])
    cells, rounds, info = S.search_batch_sic(d.data_ptr(), pkg.FMT_C64, 3, caps[0].size, K.F_SET, K.FC, K.FC, K.FS)
    assert [sorted(ids(c)) for c in cells] == [[K.ID_S, K.ID_W], [K.ID_S], []] and rounds == [[0, 1], [0], []]
    assert S.last_sic_stats() == dict(rounds=2, cancellations=1, added=1, dropped=0)
    for b, x in enumerate(caps):
        one = dev_c64(x)
        c1, r1, i1 = S.search_batch_sic(one.data_ptr(), pkg.FMT_C64, 1, x.size, K.F_SET, K.FC, K.FC, K.FS)
        assert [bytes(c) for c in c1[0]] == [bytes(c) for c in cells[b]] and r1[0] == rounds[b]
        assert [bytes(i) for i in i1[0]] == [bytes(i) for i in info[b]]
        # ... and the single-buffer entry point on the same numbers (the capture as the batch saw it, rounded to complex64):
        # record for record -- every integer field equal, every double to 1e-6 relative (frequencies: 1e-3 Hz)
        c2, r2, _ = with_sic(S, x.astype(np.complex64).astype(np.complex128))
        assert r2 == rounds[b] and len(c2) == len(cells[b])
        for u, v in zip(c2, cells[b]):
            assert_same_record(u, v)
    # the u8 route of round 0 is kept: the same capture as dongle bytes
    xq, iq = K.pair_u8()
    dq = dev_u8(iq)
    cq, rq, _ = S.search_batch_sic(dq.data_ptr(), pkg.FMT_IQ_U8, 1, xq.size, K.F_SET, K.FC, K.FC, K.FS)
    plain_q = S.search_batch(dq.data_ptr(), pkg.FMT_IQ_U8, 1, xq.size, K.F_SET, K.FC, K.FC, K.FS, pkg.STAGE_FULL)[0]
    assert sorted(ids(cq[0])) == [K.ID_S, K.ID_W] and rq[0] == [0, 1] and bytes(cq[0][0]) == bytes(plain_q[0]) and len(plain_q) == 1
    # the TDD pair on a TDD context, a batch of its own
    xt = K.tdd_pair()
    assert ids(S_tdd.search_capbuf(xt, K.F_SET, K.FC, K.FC, K.FS)[0]) == [K.ID_S]
    dt = dev_c64(xt)
    ct, rt, it = S_tdd.search_batch_sic(dt.data_ptr(), pkg.FMT_C64, 1, xt.size, K.F_SET, K.FC, K.FC, K.FS)
    assert sorted(ids(ct[0])) == [K.ID_S, K.ID_W] and rt[0] == [0, 1]
    c2, r2, _ = S_tdd.search_capbuf_sic(xt, K.F_SET, K.FC, K.FC, K.FS)
    assert ids(c2) == ids(ct[0]) and r2 == rt[0]
    got, info_t, seen = cancel_c64(pkg, S_tdd, xt, ct[0][:1])
    want, _ = R.cancel(seen, ct[0][:1], K.FC, K.FC, K.FS, duplex=R.TDD)
    err = np.abs(got - want).max() / np.sqrt(np.mean(np.abs(seen) ** 2))
    print("residual, TDD pair: max |device - sic_ref| / rms = %.3e" % err)
    assert err < RESIDUAL_TOL


def test_masks(pkg, S):
    x = K.pair()
    cells, rounds, info = with_sic(S, x, mask=pkg.SIC_PSS | pkg.SIC_SSS)
    assert sorted(ids(cells)) == [K.ID_S, K.ID_W] and rounds == [0, 1]      # the sync signals alone hide W
    assert info[0].power[0] > 0 and info[0].power[1] > 0 and info[0].power[2] == 0 and info[0].power[3] == 0
    for bad in (0, 16, -1):
        with pytest.raises(pkg.SearcherError, match="LCS_ERR_BAD_ARG"):
            with_sic(S, x, mask=bad)
    with pytest.raises(pkg.SearcherError, match="LCS_ERR_BAD_ARG"):
        with_sic(S, x, max_rounds=5)
    # a record without a MIB stays in the capture
    got, info, seen = cancel_c64(pkg, S, x, [pkg.new_cell(n_id_1=10, n_id_2=1, cp_type=1, frame_start=14198.0, freq_fine=300.0, freq_superfine=300.0)])
    assert not info[0].cancelled and np.array_equal(got, seen)


def test_wideband_band_search_with_rounds(pkg, S):
    """sweep.search_wideband(..., sic_rounds=2): the pair on one carrier of a 3.84 Msps capture, nothing on the other; off by default"""
    import torch
    carriers = np.array([K.FC - 0.9e6, K.FC + 0.9e6])
    wide, _ = pkg.synth.make_wideband(K.SEED, K.FC, 2, [(carriers[0], [K.S, K.W])], snr_db=K.SNR_DB, fmt=pkg.FMT_C64)
    d = torch.from_numpy(np.ascontiguousarray(wide)).to("cuda:0")
    args = (S, d.data_ptr(), pkg.FMT_C64, wide.size, 2 * K.FS, 2, K.FC, carriers, K.F_SET)
    plain_cells = pkg.sweep.search_wideband(*args)
    assert [ids(c) for c in plain_cells] == [[K.ID_S], []]
    cells, rounds = pkg.sweep.search_wideband(*args, sic_rounds=2)
    assert [sorted(ids(c)) for c in cells] == [[K.ID_S, K.ID_W], []] and rounds == [[0, 1], []]
    assert bytes(cells[0][0]) == bytes(plain_cells[0][0])
    with pytest.raises(ValueError):
        pkg.sweep.search_wideband(*args, sic_rounds=2, meas=True)


def test_two_cells_and_a_compacted_round(pkg, S):
    """The subtraction's loop over two cells of one buffer, and a round whose active buffers are not the batch's first ones: the noise
    buffer goes first, so rounds 1 and 2 work on the compacted batch [buffer 1]; round 2 cancels S and W from buffer 1 of the caller's
    array, and what it reports for both equals sic_ref's cancellation of [S, W] from that capture."""
    import torch
    caps = [K.noise_only(), K.pair()]
    d = torch.stack([dev_c64(x) for x in caps])
    cells, rounds, info = S.search_batch_sic(d.data_ptr(), pkg.FMT_C64, 2, caps[0].size, K.F_SET, K.FC, K.FC, K.FS, max_rounds=3)
    assert [sorted(ids(c)) for c in cells] == [[], [K.ID_S, K.ID_W]] and rounds == [[], [0, 1]]
    assert S.last_sic_stats()["rounds"] == 3 and S.last_sic_stats()["cancellations"] == 2
    seen = d[1].cpu().numpy().astype(np.complex128)
    want, ref = R.cancel(seen, cells[1], K.FC, K.FC, K.FS)
    for got, r in zip(info[1], ref):
        assert got.cancelled
        assert_info_close(got, r)
    # the same two cells through the cancellation alone: the residual itself
    got, info2, seen2 = cancel_c64(pkg, S, caps[1], cells[1])
    err = np.abs(got - want).max() / np.sqrt(np.mean(np.abs(seen) ** 2))
    print("residual, S and W both cancelled: max |device - sic_ref| / rms = %.3e" % err)
    assert np.array_equal(seen, seen2) and err < RESIDUAL_TOL
    assert [bytes(i)[:72] for i in info2] == [bytes(i)[:72] for i in info[1]]      # the compacted round ran the same launch sequence


def test_tdd_configuration_feeds_the_mask(pkg):
    """A TDD context with set_tdd_config(True): every cell is cancelled with the uplink-downlink configuration its round's chain found
    (tdd=(2, 9): configuration 2) -- CRS and PBCH in subframes 0, 3, 4, 5, 8, 9 and symbol 0 of 1 and 6 -- and the device residual with
    that mask equals sic_ref's."""
    xt = K.tdd_pair()
    with pkg.Searcher(0) as s:
        s.set_duplex(pkg.DUPLEX_TDD)
        s.set_tdd_config(True)
        cells, rounds, info = s.search_capbuf_sic(xt, K.F_SET, K.FC, K.FC, K.FS)
        assert sorted(ids(cells)) == [K.ID_S, K.ID_W] and rounds == [0, 1]
        assert info[0].ul_dl_config == 2 and info[1].ul_dl_config == pkg.TDD_NOT_ESTIMATED      # W was found, not cancelled
        tdd = s.last_sic_tdd_info(1, pkg.MAX_PEAKS)[0]
        assert [t.ul_dl_config for t in tdd[:2]] == [2, 2] and tdd[2].ul_dl_config == pkg.TDD_NOT_ESTIMATED
        # subframes 0 and 5 alone without the configuration, the wider mask with it: against sic_ref both ways
        import torch
        d = dev_c64(xt)
        res = torch.empty(xt.size, dtype=torch.complex64, device="cuda:0")
        seen = d.cpu().numpy().astype(np.complex128)
        crs = []
        for cfg in (None, [[2]]):
            inf = s.sic_cancel(d.data_ptr(), pkg.FMT_C64, 1, xt.size, [cells[:1]], K.FC, K.FC, K.FS, res.data_ptr(), ul_dl_config=cfg)[0]
            want, ref = R.cancel(seen, cells[:1], K.FC, K.FC, K.FS, duplex=R.TDD, ul_dl_config=cfg[0] if cfg else None)
            err = np.abs(res.cpu().numpy().astype(np.complex128) - want).max() / np.sqrt(np.mean(np.abs(seen) ** 2))
            print("residual, TDD pair, configuration %s: max |device - sic_ref| / rms = %.3e" % (cfg, err))
            assert err < RESIDUAL_TOL
            assert_info_close(inf[0], ref[0])
            assert inf[0].ul_dl_config == (2 if cfg else pkg.TDD_NOT_ESTIMATED)
            crs.append(inf[0].power[2])
        assert 2.7 < crs[1] / crs[0] < 3.4      # 26 reference symbols per frame instead of 8 (tests/test_sic_ref.py says why not 3.25)
        assert bytes(inf[0])[:64] == bytes(info[0])[:64]      # the round of search_capbuf_sic used that mask: the same energies and gain
