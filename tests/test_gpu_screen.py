"""The batch screen (lcs_set_batch_screen): a batch with the screen on returns the records of the same batch with the
screen off byte for byte, its debug arrays are completed to the same bits on demand, and lcs_last_screen_stats tells what was
flagged.  Inputs are small: 8 buffers or fewer; one template group (n_f = 5) on captures of 2 and 3 combining windows, and n_f = 31 on
full 153600-sample captures for two cases only.  Premises about where a peak lies and how it compares with its threshold are taken
from the CPU oracle here and asserted before the GPU result is looked at.

lcs_last_screen_stats hands out counts, not the flags themselves: that the tile of a peak is flagged is checked on one-buffer batches
whose peak sits beside a tile edge (the count then must include the neighbour), together with the records being the exact path's."""
import numpy as np
import pytest

import oracle as O
from conftest import f_search_set_for, golden, load_pkg

pytestmark = pytest.mark.gpu

FS, FC = 1.92e6, 739e6
N2, N3, NFULL = 236 + 2 * 9600, 236 + 3 * 9600, 153600
F5 = np.arange(-2, 3) * 5000.0
F31 = f_search_set_for(FC, 100)
TILE, N_TILES = 512, 19
EDGE_LAGS = (511, 512, 513, 0, 9599)


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def S(pkg):
    with pkg.Searcher(0) as s:
        yield s


def oracle_arrays(pkg, iq, f, n_cap):
    cap = pkg.synth.iq_u8_to_complex(iq)[:n_cap]
    r = O.xcorr_pss(cap, f, 2, FC, FC, FS)
    return r, O.z_th1(r["sp_incoherent"], r["n_comb_xc"])


def oracle_peaks(pkg, iq, f, n_cap):
    r, z = oracle_arrays(pkg, iq, f, n_cap)
    return O.peak_search(r["pow"], r["frq"], z, f, FC, FC, r["single"], 2), r, z


def noise(seed, n_cap):
    return np.clip(np.rint(np.random.default_rng(seed).normal(127.0, 19.0, 2 * n_cap)), 0, 255).astype(np.uint8)


def run(pkg, s, host, f, n_cap, stage, screen, readback=()):
    import torch
    host = np.ascontiguousarray(host[:, :2 * n_cap])
    B = host.shape[0]
    d = torch.from_numpy(host).to("cuda:0")
    s.set_batch_screen(screen)
    assert s.get_batch_screen() == screen
    fcs = np.full(B, FC)
    s.batch_enqueue(d.data_ptr(), pkg.FMT_IQ_U8, B, n_cap, f, fcs, fcs, FS, stage)
    rec, cnt = s.batch_collect_raw(B, 16)
    out = dict(rec=rec, cnt=cnt, stats=s.last_screen_stats(), kernel=s.last_xcorr_info()[0])
    out["rb"] = {b: s.batch_readback(b, f.size) for b in readback}
    out["repairs"] = s.last_frq_repair_stats() if readback else None
    s.sync()
    return out


def digest(r):
    """Bytes of the valid records (every field, NaNs included) behind the counts."""
    return b"".join([r["cnt"].tobytes()] + [r["rec"][b, :r["cnt"][b]].tobytes() for b in range(len(r["cnt"]))])


def both(pkg, s, host, f, n_cap, stage, readback=()):
    off = run(pkg, s, host, f, n_cap, stage, False, readback)
    on = run(pkg, s, host, f, n_cap, stage, True, readback)
    assert off["stats"] == (0, 0, 0, 0) and on["stats"][1] == host.shape[0] * N_TILES and on["stats"][2] == on["stats"][0] * ((3 * f.size + 15) // 16)
    assert on["kernel"] == off["kernel"] == "k_xcorr_i8x3"
    assert digest(on) == digest(off), (on["cnt"], off["cnt"])
    for b in readback:
        for k in off["rb"][b]:
            assert np.array_equal(on["rb"][b][k].view(np.uint8), off["rb"][b][k].view(np.uint8)), (b, k)
    assert on["repairs"] == off["repairs"]
    return on, off


@pytest.fixture(scope="module")
def short_inputs(pkg):
    """3-window captures, n_f = 5: a cell whose oracle peak lag is each of EDGE_LAGS (the tile edge at 512, the circular wrap), two
    cells of different PSS at one lag, noise only, a silent buffer."""
    base, _ = pkg.synth.make_capbuf(11, FC, [dict(n_id_1=77, n_id_2=1, f_off=3000.0, t0=4000.0)], snr_db=6.0, n_cap=N3)
    pk, _, _ = oracle_peaks(pkg, base, F5, N3)
    assert pk and pk[0].n_id_2 == 1
    p0 = pk[0].ind
    placed = {}
    for lag in EDGE_LAGS:
        iq = np.roll(base, 2 * ((lag - p0) % 9600))
        for _ in range(2):                                           # the roll's seam may move the refined index by a sample
            got = oracle_peaks(pkg, iq, F5, N3)[0][0].ind
            if got == lag:
                break
            iq = np.roll(iq, 2 * (lag - got))
        assert oracle_peaks(pkg, iq, F5, N3)[0][0].ind == lag        # the premise: the oracle's peak lies where the case says
        placed[lag] = iq
    two, _ = pkg.synth.make_capbuf(12, FC, [dict(n_id_1=10, n_id_2=0, f_off=-4000.0, t0=7000.0),
                                           dict(n_id_1=20, n_id_2=2, f_off=-4000.0, t0=7000.0)], snr_db=6.0, n_cap=N3)
    pk2 = oracle_peaks(pkg, two, F5, N3)[0]
    assert {p.n_id_2 for p in pk2[:2]} == {0, 2} and abs(pk2[0].ind - pk2[1].ind) <= 1
    silent = np.full(2 * N3, 127, np.uint8)
    return dict(placed=placed, two=two, noise=noise(100, N3), silent=silent)


@pytest.mark.parametrize("n_cap", [N2, N3])
def test_records_and_debug_arrays_are_the_exact_paths_on_short_captures(pkg, S, short_inputs, n_cap):
    si = short_inputs
    host = np.stack([si["noise"]] + [si["placed"][l] for l in EDGE_LAGS] + [si["two"], si["silent"]])
    on, off = both(pkg, S, host, F5, n_cap, pkg.STAGE_PSS, readback=range(8))
    assert (off["cnt"][1:7] >= 1).all() and off["cnt"][0] == 0       # the planted cells are found, the noise buffer holds none
    print(f"n_cap {n_cap}: flagged {on['stats'][0]} of {on['stats'][1]} tiles, flag-everything buffers {on['stats'][3]}")
    assert on["stats"][3] == 1 and on["stats"][0] >= N_TILES + 6     # the silent buffer flags everything; every occupied one something


def test_a_peak_beside_a_tile_edge_flags_the_neighbour_too(pkg, S, short_inputs):
    """ind +- 2 around a recorded peak is read by the collapse, the repair and the peak search: a peak at 511, 512 or 513 needs tiles
    0 and 1, one at 0 or 9599 tiles 0 and 18 (circular)."""
    for lag in EDGE_LAGS:
        host = short_inputs["placed"][lag][None, :]
        on, off = both(pkg, S, host, F5, N3, pkg.STAGE_PSS, readback=[0])
        inds = off["rec"]["ind"][0, :off["cnt"][0]]
        assert lag in inds.tolist()
        assert 2 <= on["stats"][0] <= 6 and on["stats"][3] == 0, (lag, on["stats"])


def test_noise_only_buffers_flag_nothing(pkg, S):
    bufs = [noise(100 + k, N3) for k in range(4)]
    for iq in bufs:                                                  # the premise, on the oracle's values
        r, z = oracle_arrays(pkg, iq, F5, N3)
        assert r["pow"].max() < 0.8 * z.min()
    on, off = both(pkg, S, np.stack(bufs), F5, N3, pkg.STAGE_PSS, readback=[0, 3])
    assert on["cnt"].sum() == 0 and on["stats"] == (0, 4 * N_TILES, 0, 0)


def test_a_silent_buffer_flags_everything_and_returns_the_exact_records(pkg, S, short_inputs):
    host = np.stack([short_inputs["silent"], short_inputs["placed"][512]])
    on, off = both(pkg, S, host, F5, N3, pkg.STAGE_PSS, readback=[0, 1])
    assert on["stats"][3] == 1 and on["stats"][0] >= N_TILES + 2


def test_a_weak_cell_crossing_its_threshold_is_recorded_exactly_when_the_exact_path_records_it(pkg, S):
    """Eight gains of one weak cell, chosen here with the oracle so that its peak / Z_th1 runs from about 0.9 to about 1.1."""
    rng = np.random.default_rng(5)
    sig, ref_pow, _ = pkg.synth.make_signal(rng, FC, [dict(n_id_1=77, n_id_2=1, f_off=3000.0, t0=4000.0)], N3)

    def at(snr):
        iq = pkg.synth.add_noise_and_quantise(np.random.default_rng(9), sig, ref_pow, snr_db=float(snr))
        r, z = oracle_arrays(pkg, iq, F5, N3)
        return iq, float((r["pow"][1] / z[None, :]).max())           # the cell's PSS against its threshold, lag by lag

    grid = np.arange(-16.0, 6.0, 0.5)
    ratios = np.array([at(s)[1] for s in grid])
    lo, hi = grid[np.argmax(ratios >= 0.9)], grid[np.argmax(ratios >= 1.1)]
    assert ratios.min() < 0.9 and ratios.max() >= 1.1 and lo < hi
    sweep = [at(s) for s in np.linspace(lo - 0.25, hi + 0.25, 8)]
    rr = np.array([r for _, r in sweep])
    print("oracle peak / Z_th1 over the sweep:", np.round(rr, 3).tolist())
    assert rr.min() < 0.95 and rr.max() > 1.05 and 0.8 < rr.min() and rr.max() < 1.3     # the crossing lies inside the sweep
    on, off = both(pkg, S, np.stack([iq for iq, _ in sweep]), F5, N3, pkg.STAGE_PSS, readback=range(8))
    found = [bool((off["rec"]["n_id_2"][b, :off["cnt"][b]] == 1).any()) for b in range(8)]
    assert not found[0] and found[-1], found


@pytest.fixture(scope="module")
def full_inputs(pkg):
    g = golden("capbuf_0000")["iq_u8"]
    occ, _ = pkg.synth.make_capbuf(21, FC, [dict(n_id_1=50, n_id_2=2, f_off=21000.0), dict(n_id_1=90, n_id_2=0, f_off=-33000.0, gain_db=-3.0)], snr_db=5.0)
    return np.stack([g, noise(7, NFULL), occ, np.full(2 * NFULL, 127, np.uint8)])


def test_full_size_batch_full_chain(pkg, S, full_inputs):
    """153600 samples, n_f = 31, every stage: the golden capture, noise, two planted cells, a silent buffer."""
    on, off = both(pkg, S, full_inputs, F31, NFULL, pkg.STAGE_FULL, readback=[0, 2])
    assert off["cnt"][0] >= 1 and off["cnt"][2] >= 1
    tiles = set()
    for b in (0, 2):                                                 # the oracle's peaks: their tiles are among the flagged
        for p in oracle_peaks(pkg, full_inputs[b], F31, NFULL)[0]:
            tiles.add((b, p.ind // TILE))
    print(f"full size: flagged {on['stats'][0]} of {on['stats'][1]} tiles; oracle peak tiles {len(tiles)}")
    assert on["stats"][3] == 1 and N_TILES + len(tiles) <= on["stats"][0] < 4 * N_TILES


def test_dense_batch(pkg, S):
    """Every buffer holds 2-3 cells: the same records, and how much of the batch the exact kernel redoes.  A batch that flags more
    than a fifth of its tiles is a poor bargain: the context's next batches run unscreened (same records) until lcs_set_batch_screen
    is called again or 63 of them have passed."""
    import torch
    fcs = FC + 100e3 * np.arange(8)
    host = pkg.synth.make_batch_u8(8, 77, fcs, occupied_every=1, n_distinct=4, cells_cycle=(2, 3))
    on, off = both(pkg, S, host, F31, NFULL, pkg.STAGE_FULL, readback=[1])
    assert off["cnt"].sum() >= 4
    print(f"dense: flagged {on['stats'][0]} of {on['stats'][1]} tiles = {on['stats'][0] / on['stats'][1]:.3f}")
    assert on["stats"][0] >= 8
    if 5 * on["stats"][0] > on["stats"][1]:
        d = torch.from_numpy(host).to("cuda:0")
        for _ in range(2):                                           # the screen is still on, and the next batches take the exact kernel alone
            assert S.get_batch_screen()
            S.batch_enqueue(d.data_ptr(), pkg.FMT_IQ_U8, 8, NFULL, F31, np.full(8, FC), np.full(8, FC), FS, pkg.STAGE_FULL)
            rec, cnt = S.batch_collect_raw(8, 16)
            assert S.last_screen_stats() == (0, 0, 0, 0)
            assert digest(dict(rec=rec, cnt=cnt)) == digest(off)
        again = run(pkg, S, host, F31, NFULL, pkg.STAGE_FULL, True)  # set_batch_screen forgets the count
        assert again["stats"] == on["stats"] and digest(again) == digest(off)
