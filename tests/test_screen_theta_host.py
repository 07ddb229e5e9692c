"""The theta rule of the batch screen (csrc/screen_bound.h: lcs_screen_lower, _in_s, _decide, _hot), compiled for the
host in tests/host/screen_theta_host.cpp -- the text k_screen_flag runs.

1. L_e against brute-force integer correlations (the adversarial captures of test_screen_bound_host.py): the exact power never lies
   below L_e(screened power) -- per element, box-filtered, and as the maximum over columns.
2. The equivalence the rule promises, on the oracle's arrays: every element of `single` moved by the full bound B_e (all up, all down,
   random signs) is a legitimate "screened" array; the rule flags tiles on its collapse; the mixed arrays (exact where the whole box
   lies in flagged tiles, screened elsewhere) must give the oracle's peak search the very cells the exact arrays give it.
3. The counts of the model that motivated the rule, as a regression pin: on the eight distinct occupied buffers of the benchmark batch
   the theta rule flags at most half the tiles the Zmin rule flags, never more per buffer, and always the tiles of the oracle's peaks."""
import numpy as np
import pytest

import oracle as O
import screen_theta_model as M
from conftest import f_search_set_for, golden, load_pkg
from test_screen_bound_host import DS, K, LAGS, QMAX, capture, columns, correlate, digits, powers

FC = 739e6
N3, NFULL = 236 + 3 * 9600, 153600
F5 = np.arange(-2, 3) * 5000.0
F31 = f_search_set_for(FC, 100)


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.mark.parametrize("n_win", [2, 3, 15])
def test_the_exact_power_never_lies_below_the_lower_bound(n_win):
    B = M.lib()
    rng = np.random.default_rng(70 + n_win)
    t = columns(rng)
    t_hi = t - digits(t)[0]
    sc = np.array([1.0 / (128.0 * QMAX / m) for m in (0.11, 0.10, 0.09)])
    lower = np.vectorize(lambda s, v: B.theta_lower(n_win, DS, float(s), float(v)))
    const = np.tile(np.array([[-128, 127]], np.int64), ((n_win - 1) * 180 + K + LAGS, 1))
    cases = [const, -const - 1, capture(n_win, t[1], LAGS // 2, rng), capture(n_win, t[2], LAGS // 2, rng), capture(n_win, None, 0, rng)]
    closest = 0.0
    for a in cases:
        x, xs = correlate(a, t, n_win), correlate(a, t_hi, n_win)
        for v, vs, s in zip(powers(x, sc, n_win), powers(xs, sc, n_win), (sc[None, :], sc[None, :], sc.max())):
            lo = lower(np.broadcast_to(s, vs.shape), vs)
            assert (lo <= v).all(), (lo / v).max()
            up = vs > v                                              # where the screen overshoots: v' - v against the v' - L_e(v') granted
            if up.any():
                closest = max(closest, float(((vs - v) / (vs - lo))[up].max()))
    print(f"n_win {n_win}: the screened value's overshoot reaches {closest:.3f} of what L_e allows for")
    assert closest <= 1.0
    # zero, tiny and NaN arguments: 0 (the caller then flags everything), never negative, never above the argument
    e = 1.4142135623730951 * 128 * 274 * 128 * sc[0]
    for v in (0.0, 0.5 * e * e, e * e, float("nan"), -1.0):
        assert B.theta_lower(n_win, DS, float(sc[0]), v) == 0.0
    vv = e * e * np.geomspace(1.0001, 1e12, 300)
    ll = lower(sc[0], vv)
    assert (ll >= 0).all() and (ll < vv).all() and (np.diff(ll) > 0).all()


def test_the_decision_refuses_what_it_cannot_stand_on():
    import ctypes as C
    B = M.lib()
    sc = 1.0 / (128.0 * QMAX / 0.1)
    e = 1.4142135623730951 * 128 * 274 * 128 * sc
    th, T = C.c_float(0), C.c_double(0)
    assert B.theta_decide(15, DS, sc, float("inf"), C.byref(th), C.byref(T)) == M.MODE_NONE       # S is empty
    for lmin in (0.0, -1.0, float("nan"), 0.5 * e * e, e * e, 5.8 * e * e, 1e39):
        assert B.theta_decide(15, DS, sc, lmin, C.byref(th), C.byref(T)) == M.MODE_ALL, lmin
        assert th.value == 0.0 and T.value == -1.0
    for lmin in e * e * np.geomspace(7.0, 1e10, 50):
        assert B.theta_decide(15, DS, sc, float(lmin), C.byref(th), C.byref(T)) == M.MODE_BY_T
        assert 0 < th.value <= lmin and th.value >= lmin * (1 - 2.0 ** -23) and 0 < T.value < th.value      # theta is rounded DOWN
    assert B.theta_in_s(15, DS, sc, 0.5 * e * e, 1e-30) == 1 and B.theta_in_s(15, DS, sc, float("nan"), 1.0) == 1   # no usable T(z): in S
    assert B.theta_hot(1.0, float("nan")) == 1 and B.theta_hot(1.0, 1.0) == 1 and B.theta_hot(1.0, 0.999) == 0


def cells_bytes(cells):
    return [bytes(c) for c in cells]


def equivalence(name, r, z, f, fc, sc, n_comb):
    """The three screened variants of one buffer's oracle arrays -> the tile counts they flag."""
    exact = O.peak_search(r["pow"], r["frq"], z, f, fc, fc, r["single"], DS)
    e = np.sqrt(2.0) * 128 * 274 * 128 * sc * (1 + 1e-15)
    v = r["single"].astype(np.float64)
    bound = 2 * e * np.sqrt(v) + e * e
    rng = np.random.default_rng(17)
    counts = []
    for variant, sign in (("up", 1.0), ("down", -1.0), ("random", np.where(rng.integers(0, 2, v.shape) == 1, 1.0, -1.0))):
        single_s = np.maximum(v + sign * bound, 0.0).astype(np.float32)
        vs, frq_s = M.collapse(single_s)
        rule = M.theta_rule(n_comb, sc, z, vs)
        idx = np.arange(M.N_IDX)
        tf = rule["flags"]
        whole = tf[idx // M.TILE] & tf[((idx - DS) % M.N_IDX) // M.TILE] & tf[((idx + DS) % M.N_IDX) // M.TILE]
        pow_m = np.where(whole[None, :], r["pow"], vs.astype(np.float64))
        frq_m = np.where(whole[None, :], r["frq"], frq_s).astype(np.int32)
        single_m = np.where(tf[idx // M.TILE][None, :, None], r["single"], single_s)
        mixed = O.peak_search(pow_m, frq_m, z, f, fc, fc, single_m, DS)
        assert cells_bytes(mixed) == cells_bytes(exact), (name, variant, [(c.n_id_2, c.ind) for c in mixed], [(c.n_id_2, c.ind) for c in exact])
        assert (rule["flags"] | ~M.tiles_of([c.ind for c in exact])).all(), (name, variant)
        counts.append(int(tf.sum()))
    print(f"{name}: {len(exact)} cells; tiles flagged up / down / random: {counts}")
    return exact, counts


@pytest.fixture(scope="module")
def bench_occupied(pkg):
    """The eight distinct occupied buffers of the benchmark batch (bench.py: make_batch_u8(B, 1234, FC + 100 kHz * b); every fourth
    buffer is occupied and the first eight of them are distinct) with the oracle's arrays."""
    fcs = FC + 100e3 * np.arange(32)
    host = pkg.synth.make_batch_u8(32, 1234, fcs)
    out = []
    for b in range(0, 32, 4):
        r, z, pk = M.oracle_of(pkg, host[b], F31, float(fcs[b]), NFULL)
        out.append(dict(b=b, fc=float(fcs[b]), iq=host[b], r=r, z=z, peaks=pk, sc=M.buffer_scale(F31, float(fcs[b]))))
    return out


def test_the_peak_search_sees_the_same_cells_on_full_size_buffers(pkg, bench_occupied):
    g = golden("capbuf_0000")
    fc = float(g["fc"][0])
    f = f_search_set_for(fc, 100)
    r, z, _ = M.oracle_of(pkg, g["iq_u8"], f, fc, NFULL)
    # The golden capture says little here, and is kept because it is the project's reference input: strong cells put entries that reach
    # their own threshold into its quietest stretch as well (theta = 0.99 Zmin on the unperturbed arrays, |S| > 2000), so the rule
    # flags all 19 tiles -- by its threshold, not by the flag-everything branch -- and the mixed arrays are the exact ones.  The
    # buffers below leave most tiles unrefined (6, 2, 0 of 19; the crafted ones 4 and 11).
    exact, counts = equivalence("golden", r, z, f, fc, M.buffer_scale(f, fc), r["n_comb_xc"])
    assert len(exact) >= 1 and counts == [M.N_TILES] * 3
    for o in bench_occupied[:2]:
        exact, counts = equivalence(f"bench buffer {o['b']}", o["r"], o["z"], F31, o["fc"], o["sc"], o["r"]["n_comb_xc"])
        assert len(exact) >= 1 and 0 < min(counts) and max(counts) <= M.N_TILES // 2      # most of the buffer stays screened: the comparison can fail
    noise = np.clip(np.rint(np.random.default_rng(7).normal(127.0, 19.0, 2 * NFULL)), 0, 255).astype(np.uint8)
    r, z, _ = M.oracle_of(pkg, noise, F31, FC, NFULL)
    assert r["pow"].max() < 0.8 * z.min()                            # the premise: noise only
    exact, counts = equivalence("noise", r, z, F31, FC, M.buffer_scale(F31, FC), r["n_comb_xc"])
    assert not exact and counts == [0, 0, 0]


def test_the_peak_search_sees_the_same_cells_on_the_crafted_loud_and_quiet_buffers(pkg):
    """pick_crafted asserts the premises: the thresholds of the loud half lie >= 3 x above the quiet half's; in A both cells are recorded,
    in B a loud-half entry below its own threshold outranks the recordable quiet-half cell and the reference stops before it."""
    sc = M.buffer_scale(F5, FC)
    for k, (iq, r, z, pk, i_w) in M.pick_crafted(pkg, F5, FC, N3).items():
        exact, counts = equivalence("crafted " + k, r, z, F5, FC, sc, r["n_comb_xc"])
        assert cells_bytes(exact) == cells_bytes(pk)
        if k == "B":
            assert r["pow"][1, i_w] >= z[i_w] and all(c.n_id_2 != 1 for c in exact)


def test_the_models_counts(bench_occupied):
    theta, zmin = [], []
    for o in bench_occupied:
        vs, _ = M.collapse(o["r"]["single"])                         # the exact arrays stand in for the screened ones (they differ by ~1e-5)
        n = o["r"]["n_comb_xc"]
        a, b = M.theta_rule(n, o["sc"], o["z"], vs), M.zmin_rule(n, o["sc"], o["z"], vs)
        assert a["mode"] == M.MODE_BY_T and not b["all"]
        assert not (a["flags"] & ~b["flags"]).any()                  # theta >= Zmin: a subset
        assert (a["flags"] | ~M.tiles_of([c.ind for c in o["peaks"]])).all()
        theta.append(int(a["flags"].sum()))
        zmin.append(int(b["flags"].sum()))
        print(f"buffer {o['b']}: theta / Zmin = {a['theta'] / o['z'].min():.3f}, |S| = {a['n_s']}, tiles {theta[-1]} against {zmin[-1]}")
    print("tiles per buffer, theta rule:", theta, "Zmin rule:", zmin)
    assert all(t <= zz for t, zz in zip(theta, zmin)) and 2 * sum(theta) <= sum(zmin), (theta, zmin)
