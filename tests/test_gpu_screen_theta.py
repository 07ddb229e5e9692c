"""The batch screen refines down to theta -- the smallest lower bound of an entry that is hot against the threshold of its OWN lag --
not to the buffer's smallest threshold (k_screen_flag, csrc/screen_bound.h): records stay the unscreened batch's byte for
byte, the debug arrays are completed to the same bits, and the flagged counts follow the CPU model of the rule
(tests/screen_theta_model.py: the header's functions compiled for the host) on the oracle's arrays.  Small inputs: 3-window captures at
n_f = 5 in batches of <= 8 buffers; one test runs four full-size buffers at n_f = 31.  Premises are asserted on the oracle first."""
import numpy as np
import pytest

import screen_theta_model as M
from conftest import golden, load_pkg
from test_gpu_screen import F5, F31, FC, N3, NFULL, N_TILES, both, noise, oracle_peaks, run

pytestmark = pytest.mark.gpu

WAVE_AND_TILE_EDGES = (127, 128, 129, 511, 512, 0, 9599)


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def S(pkg):
    with pkg.Searcher(0) as s:
        yield s


def model(n_comb, r, z, sc):
    """Both rules on the oracle's arrays (they stand in for the screened ones: ~1e-5 apart)."""
    vs, _ = M.collapse(r["single"])
    return vs, M.theta_rule(n_comb, sc, z, vs), M.zmin_rule(n_comb, sc, z, vs)


def test_loud_and_quiet_halves(pkg, S):
    """The two crafted buffers (A: both cells recorded; B: a loud-half entry below its own threshold outranks the recordable quiet-half
    cell), a silent buffer and a noise buffer."""
    crafted = M.pick_crafted(pkg, F5, FC, N3)
    nz = noise(100, N3)
    r, z, pk = M.oracle_of(pkg, nz, F5, FC, N3)
    sc = M.buffer_scale(F5, FC)
    assert not pk and model(3, r, z, sc)[1]["mode"] == M.MODE_NONE   # the premise: the noise buffer flags nothing
    host = np.stack([crafted["A"][0], crafted["B"][0], np.full(2 * N3, 127, np.uint8), nz])
    on, off = both(pkg, S, host, F5, N3, pkg.STAGE_PSS, readback=range(4))
    assert on["stats"][3] == 1                                        # the silent buffer, and only it, flags everything
    lo = hi = 0
    for k in "AB":
        _, r, z, pk, _ = crafted[k]
        _, th, zm = model(3, r, z, sc)
        need = int(M.tiles_of([c.ind for c in pk]).sum())
        print(f"crafted {k}: tiles of the oracle's peaks {need}, theta rule {int(th['flags'].sum())}, Zmin rule {int(zm['flags'].sum())}")
        lo, hi = lo + need, hi + int(zm["flags"].sum())
    got = on["stats"][0] - N_TILES
    print(f"flagged by the two crafted buffers: {got}")
    assert lo <= got <= hi, (lo, got, hi)
    for b, k in enumerate("AB"):                                     # and the records are the oracle's cells: in B the quiet-half cell is not among them
        rec = set(zip(off["rec"]["n_id_2"][b, :off["cnt"][b]].tolist(), off["rec"]["ind"][b, :off["cnt"][b]].tolist()))
        assert rec == {(c.n_id_2, c.ind) for c in crafted[k][3]}, (k, rec)


def test_a_weak_cell_in_the_quiet_half_crossing_its_threshold(pkg, S):
    """Eight gains of the quiet-half cell, chosen with the oracle so that its peak / Z_th1 runs from about 0.9 to about 1.1, while the
    loud half stays as it is.  The loud half's extra power is an out-of-band carrier here, not noise, and it holds no cell: its thresholds
    stand >= 3 x above the quiet half's, but nothing in it outranks the cell (noise that loud, or a strong cell's sidelobes, would -- the
    crafted buffer B -- and the cell would never be recorded near its threshold).  So the exact path's record appears inside the sweep,
    and the screened batch must record the cell exactly when the exact path does."""
    def at(g):
        iq = M.crafted(pkg, FC, N3, float(g), gain_s_db=None, tone_hz=800e3)
        r, z, pk = M.oracle_of(pkg, iq, F5, FC, N3)
        quiet = z < 1.5 * z.min()
        return iq, float((r["pow"][1] / z)[quiet].max()), float(z.max() / z.min()), any(c.n_id_2 == 1 for c in pk)

    grid = np.arange(-14.0, -6.0, 0.5)
    ratios = np.array([at(g)[1] for g in grid])
    lo, hi = grid[np.argmax(ratios >= 0.9)], grid[np.argmax(ratios >= 1.1)]
    assert ratios.min() < 0.9 and ratios.max() >= 1.1 and lo < hi
    sweep = [at(g) for g in np.linspace(lo - 0.25, hi + 0.25, 8)]
    rr = np.array([r for _, r, _, _ in sweep])
    by_oracle = [rec for _, _, _, rec in sweep]
    print("oracle peak / Z_th1 of the quiet-half cell over the sweep:", np.round(rr, 3).tolist(), "; the oracle records it:", by_oracle)
    assert rr.min() < 0.95 and rr.max() > 1.05 and 0.8 < rr.min() and rr.max() < 1.3     # the crossing lies inside the sweep
    assert min(zr for _, _, zr, _ in sweep) >= 3.0                   # the loud half is loud in every one of them
    assert not by_oracle[0] and by_oracle[-1]                        # and the oracle's record appears inside the sweep
    on, off = both(pkg, S, np.stack([iq for iq, _, _, _ in sweep]), F5, N3, pkg.STAGE_PSS, readback=range(8))
    found = [bool((off["rec"]["n_id_2"][b, :off["cnt"][b]] == 1).any()) for b in range(8)]
    print("the exact path records the quiet-half cell:", found, "; tiles flagged:", on["stats"][0])
    assert not found[0] and found[-1], found


def test_peaks_at_wave_tile_and_circular_edges(pkg, S):
    """A peak at lags 127, 128, 129 (the 128-lag grain inside a tile), 511, 512 (the tile edge), 0 and 9599 (the wrap), one buffer each."""
    base, _ = pkg.synth.make_capbuf(11, FC, [dict(n_id_1=77, n_id_2=1, f_off=3000.0, t0=4000.0)], snr_db=6.0, n_cap=N3)
    p0 = oracle_peaks(pkg, base, F5, N3)[0][0].ind
    bufs, need = [], 0
    for lag in WAVE_AND_TILE_EDGES:
        iq = np.roll(base, 2 * ((lag - p0) % 9600))
        for _ in range(2):                                           # the roll's seam may move the refined index by a sample
            got = oracle_peaks(pkg, iq, F5, N3)[0][0].ind
            if got == lag:
                break
            iq = np.roll(iq, 2 * (lag - got))
        pk = oracle_peaks(pkg, iq, F5, N3)[0]
        assert pk[0].ind == lag and pk[0].n_id_2 == 1                # the premise: the oracle's peak lies where the case says
        need += int(M.tiles_of([c.ind for c in pk]).sum())
        bufs.append(iq)
    on, off = both(pkg, S, np.stack(bufs), F5, N3, pkg.STAGE_PSS, readback=range(len(bufs)))
    for b, lag in enumerate(WAVE_AND_TILE_EDGES):
        assert lag in off["rec"]["ind"][b, :off["cnt"][b]].tolist(), lag
    print(f"edges: flagged {on['stats'][0]} tiles, the oracle's peaks need {need}")
    assert on["stats"][3] == 0 and need <= on["stats"][0] <= 6 * len(bufs)


def test_full_size(pkg, S):
    """The first two occupied buffers that the benchmark's generator draws for its seed (make_batch_u8(., 1234, .); here on one carrier,
    not on the benchmark's 100 kHz raster, and with the circular shifts of an 8-buffer batch), noise and the golden capture through the
    whole chain; then those two buffers alone, for their flagged count against the model's."""
    bench = pkg.synth.make_batch_u8(8, 1234, np.full(8, FC))          # buffers 0 and 4 are the occupied ones
    g = golden("capbuf_0000")["iq_u8"]
    host = np.stack([bench[0], bench[4], noise(7, NFULL), g])
    on, off = both(pkg, S, host, F31, NFULL, pkg.STAGE_FULL, readback=[0, 3])
    assert off["cnt"][0] >= 1 and off["cnt"][1] >= 1 and off["cnt"][3] >= 1 and on["stats"][3] == 0
    two = run(pkg, S, host[:2], F31, NFULL, pkg.STAGE_PSS, True)
    sc = M.buffer_scale(F31, FC)
    lo = hi = want = 0
    for b in range(2):
        r, z, pk = M.oracle_of(pkg, host[b], F31, FC, NFULL)
        vs, th, zm = model(r["n_comb_xc"], r, z, sc)
        assert th["mode"] == M.MODE_BY_T and pk
        # entries within 1e-4 of T(theta) may fall either way on values that differ from the oracle's in the fifth digit
        sure = M.tiles_of(np.nonzero((vs >= th["T"] * (1 + 1e-4)).any(0))[0])
        maybe = M.tiles_of(np.nonzero((vs >= th["T"] * (1 - 1e-4)).any(0))[0])
        assert (sure | ~M.tiles_of([c.ind for c in pk])).all()
        lo, hi, want = lo + int(sure.sum()), hi + int(maybe.sum()), want + int(th["flags"].sum())
        print(f"benchmark buffer {b}: theta rule {int(th['flags'].sum())} tiles (Zmin rule {int(zm['flags'].sum())}), theta / Zmin {th['theta'] / z.min():.3f}")
    print(f"flagged by the two benchmark buffers: {two['stats'][0]}; model {want} ({lo} .. {hi}); all four buffers: {on['stats'][0]}")
    assert lo <= two["stats"][0] <= hi, (lo, two["stats"][0], hi)
    assert two["stats"][0] <= on["stats"][0] < 3 * N_TILES
