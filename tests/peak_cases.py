"""Crafted (pow, frq, sp) arrays for the peak search of the fused chain (tests/test_gpu_peak_search_cases.py puts them in front of
k_peak_search_reg through lcs_foe_partial / lcs_foe_finish) and a plain model of the reference's loop (src/searcher.cpp:436-509).
tests/test_peak_cases_host.py checks on the CPU that the oracle, the model and every premise below agree on every case.

All cases: n_f = 7 hypotheses 5 kHz apart, ds_comb_arm = 2, n_comb = 2 (the seed buffer's: two combining windows).
Only numpy and the oracle's threshold recipe."""
import functools

import numpy as np

import oracle as O

N = 9600
CANCEL = 274
MAX_REC = 104                       # LCS_MAX_PEAKS
N_F, DS, N_COMB = 7, 2, 2
F_SET = np.arange(-3, 4) * 5e3
FLOOR = 10.0 ** (-12.0 / 10.0)      # the -12 dB floor; the host's std::pow may give a neighbouring double (floor case)
Z_MARGIN = 1e-6                     # room for the two chi2cdf_inv implementations (tests/test_tables_abi.py bounds their difference
                                    # by 1e-9 k absolute on a value above k: below 1e-9 relative)
REFINE_MARGIN = 1e-4                # best two refinement candidates in the oracle's `single` (the GPU's is within 1e-5 of it)
SHARES = [(0, 0), (0, N_F), (2, 3)]          # (first, count): owns nothing, everything, the middle
_FRQ_CYCLE = (1, 2, 4, 5, 3, 0, 6)           # planted cells walk over both edges of the middle share


# ---------------------------------------------------------------------------------------------------- the model
def model(pow64, frq, Z, f, single, ds, trace=None):
    """The reference's loop on float64 -> [(n_id_2, ind, freq, pss_pow)], at most MAX_REC records.  `single`: [3][9600][n_f].
    trace (a list): one (row, col, value, Z[col], passed) per iteration, the stopping one included."""
    w = np.array(pow64, np.float64).reshape(-1).copy()
    frq = np.asarray(frq).reshape(3, N)
    out = []
    while len(out) < MAX_REC:
        i = int(np.argmax(w))                     # the first maximum of the flattened array
        r, c = divmod(i, N)
        p = float(w[i])
        passed = not p < Z[c]
        if trace is not None:
            trace.append((r, c, p, float(Z[c]), passed))
        if not passed:
            break
        fi = int(frq[r, c])
        ind = -1
        if c - ds >= 0:                           # uint16 loop variable of the reference: no pass at all when c < ds
            best = -np.inf
            for t in range(c - ds, c + ds + 1):
                v = float(single[r, t % N, fi])
                if v > best:
                    best, ind = v, t % N
        out.append((r, ind, float(f[fi]), p))
        w[r * N + (c + np.arange(-CANCEL, CANCEL + 1)) % N] = 0.0
        w[w < p * FLOOR] = 0.0
    return out


def refine_candidates(c, ds=DS):
    """columns the refinement of a peak at column c reads (empty: the wrap quirk)"""
    return [t % N for t in range(c - ds, c + ds + 1)] if c - ds >= 0 else []


# ---------------------------------------------------------------------------------------------------- the packed form
def pack(pow32, frq, sp, n_comb=N_COMB):
    """-> (words int64 [3 * 9600], meta float64 [9601]) as k_foe_pack leaves them"""
    bits = np.ascontiguousarray(pow32, np.float32).reshape(-1).view(np.uint32).astype(np.uint64)
    low = (np.uint64(0xFFFFFFFF) - np.asarray(frq).reshape(-1).astype(np.uint64))
    words = ((bits << np.uint64(32)) | low).view(np.int64)
    meta = np.concatenate([np.asarray(sp, np.float64), [float(n_comb)]])
    return words, meta


def z_of(sp):
    return O.z_th1(np.asarray(sp, np.float64), N_COMB, DS)


@functools.lru_cache(maxsize=None)
def _z_per_sp():
    return float(z_of(np.ones(1))[0])


def sp_for(z):
    """the sp_incoherent that gives a threshold of (nearly) z"""
    return np.asarray(z, np.float64) / _z_per_sp()


def f32_below(x):
    """largest float32 strictly below the double x"""
    v = np.float32(x)
    return v if float(v) < x else np.nextafter(v, np.float32(-np.inf))


def f32_at_or_above(x):
    """smallest float32 at or above the double x"""
    v = np.float32(x)
    return v if float(v) >= x else np.nextafter(v, np.float32(np.inf))


class _Case:
    def __init__(self, name, z, background=0.0):
        self.name = name
        self.sp = sp_for(np.broadcast_to(np.asarray(z, np.float64), (N,)).copy())
        self.pow32 = np.zeros((3, N), np.float32) + np.float32(background)
        c = np.arange(N)
        self.frq = ((c[None, :] * 3 + np.arange(3)[:, None] * 5 + c[None, :] // 7) % N_F).astype(np.int32)
        self.planted = []
        self.extra = {}

    def plant(self, row, col, value, frq=None):
        col %= N
        self.pow32[row, col] = np.float32(value)
        self.frq[row, col] = _FRQ_CYCLE[len(self.planted) % len(_FRQ_CYCLE)] if frq is None else frq
        self.planted.append((row, col))

    def done(self, **extra):
        d = dict(name=self.name, pow32=self.pow32, frq=self.frq, sp=self.sp, f=F_SET.copy(), planted=tuple(self.planted))
        d.update(self.extra)
        d.update(extra)
        for a in (d["pow32"], d["frq"], d["sp"], d["f"]):
            a.setflags(write=False)
        return d


# ---------------------------------------------------------------------------------------------------- the cases
def _dense(name, offsets, seed):
    """34 cells per row, 275 apart (the cancellation reaches 274): every one is a peak, 102 in all"""
    k = _Case(name, 0.05)
    rng = np.random.default_rng(seed)
    k.pow32[:] = rng.uniform(0.0, 0.04, (3, N)).astype(np.float32)       # below Z
    vals = np.linspace(0.2, 1.0, 102).astype(np.float32)
    assert np.unique(vals).size == 102
    rng.shuffle(vals)
    for r in range(3):
        for j in range(34):
            k.plant(r, offsets[r] + 275 * j, vals[r * 34 + j])
    return k.done(n_peaks=102)


def _plateau():
    k = _Case("plateau", 0.05, background=0.75)
    exp = [(r, c) for r in range(3) for c in range(0, 9076, 275)]
    return k.done(n_peaks=102, positions=exp)


def _ties():
    """pairs (and two triples) of EQUAL maxima; every group its own value, descending, so the list's order is the groups' order and,
    inside a group, ascending linear index"""
    k = _Case("ties", 0.01, background=1e-3)
    groups = [
        [(0, 1000), (0, 1512)],                    # two registers of one thread (tid 232), one row
        [(0, 8000), (1, 8256)],                    # two registers of one thread (tid 64), two rows
        [(0, 2088), (0, 2565)],                    # two lanes of wave 0 (40 and 5): the lower index in the higher lane
        [(2, 2053), (2, 2600)],                    # two lanes of wave 0 (5 and 40): the lower index in the lower lane
        [(1, 3272), (1, 3850)],                    # two waves (tid 200 and 10): the lower index in the higher wave
        [(2, 3082), (2, 3784)],                    # two waves (tid 10 and 200): the lower index in the lower wave
        [(0, 5000), (1, 5000), (2, 5000)],         # one column, the three rows
        [(0, 9599), (1, 0)],                       # the last column of a row against the first of the next
        [(0, 6274), (1, 6274), (2, 7188)],         # three ways: two registers of thread 130 (wave 2) and thread 20 (wave 0)
    ]
    for g, cells in enumerate(groups):
        for r, c in cells:
            k.plant(r, c, np.float32(1.0) - np.float32(0.01) * np.float32(g))
    exp = [rc for cells in groups for rc in sorted(cells)]
    return k.done(n_peaks=len(exp), positions=exp)


def _ties_pad():
    """a column of the half-padded last register (9590: register 37, thread 118) against column 100 of the next row, whose linear
    index is the one a padded element of threads 128..255 would alias; and the very last element against the very first"""
    k = _Case("ties_pad", 0.01, background=1e-3)
    groups = [[(0, 9590), (1, 100)], [(1, 5000), (2, 9599)], [(0, 4000), (2, 9199)]]
    for g, cells in enumerate(groups):
        for r, c in cells:
            k.plant(r, c, np.float32(1.0) - np.float32(0.01) * np.float32(g))
    exp = [rc for cells in groups for rc in sorted(cells)]
    return k.done(n_peaks=len(exp), positions=exp)


CANCEL_COLS = (0, 100, 274, 275, 4800, 9325, 9326, 9599)


def _cancel(j, c):
    """a peak at column c; at c +- 274 of its row smaller cells that vanish, at c +- 275 cells that come back as peaks; at c +- 274
    of another row cells that survive"""
    k = _Case(f"cancel_{c}", 0.01, background=1e-3)
    r, o = j % 3, (j + 1) % 3
    # the hypotheses: the three peaks of the row inside the middle share (one of them may sit at a column below ds_comb_arm, never
    # all), the two of the other row on either side of it
    k.plant(r, c, 1.0, 3)
    k.plant(r, c - 274, 0.5, 1)
    k.plant(r, c + 274, 0.45, 5)
    k.plant(r, c - 275, 0.4, 2)
    k.plant(r, c + 275, 0.35, 4)
    k.plant(o, c - 274, 0.3, 1)
    k.plant(o, c + 274, 0.25, 5)
    exp = [(r, c % N), (r, (c - 275) % N), (r, (c + 275) % N), (o, (c - 274) % N), (o, (c + 274) % N)]
    return k.done(n_peaks=5, positions=exp, vanish=((r, (c - 274) % N), (r, (c + 274) % N)))


def floor_pair(p):
    """-> (largest float32 below p * FLOOR, smallest at or above it), both clear of the threshold by more than 2 double ulps: the
    host's std::pow(10, -1.2) and Python's may differ in the last place"""
    t = float(p) * FLOOR
    lo, hi = f32_below(t), f32_at_or_above(t)
    u = 2 * np.spacing(t)
    assert float(lo) < t - u and float(hi) >= t + u, (p, lo, hi, t)
    return lo, hi


FLOOR_PEAKS = (1.0, 0.8125, 0.3337)


def _floor(j, p):
    """Z far below every value.  After the peak p the largest float32 below p * 10^-1.2 is zeroed and never returned, the smallest
    at or above it stays and is the next peak.  (One pair per case: whatever a later, smaller peak's floor would remove is gone.)"""
    k = _Case(f"floor_{j}", 1e-9)
    p = np.float32(p)
    lo, hi = floor_pair(p)
    r = j % 3
    k.plant(r, 1000, p)
    k.plant((r + 1) % 3, 2000, lo)
    k.plant((r + 2) % 3, 3000, hi)
    return k.done(n_peaks=2, positions=[(r, 1000), ((r + 2) % 3, 3000)], vanish=(((r + 1) % 3, 2000),))


def _stop(two_first):
    """the loop ends at the first global maximum below ITS column's threshold, although a smaller value elsewhere is above its own"""
    z = np.full(N, 0.01)
    z[4000:4100] = 1.0
    k = _Case("stop_after_two" if two_first else "stop", z, background=1e-3)
    exp = []
    if two_first:
        k.plant(2, 1000, 0.9)
        k.plant(0, 7000, 0.8)
        exp = [(2, 1000), (0, 7000)]
    k.plant(1, 4050, 0.5)
    k.plant(0, 2000, 0.3)
    return k.done(n_peaks=len(exp), positions=exp, vanish=((1, 4050), (0, 2000)))


def _smooth_z(rng, lo, hi):
    x = np.arange(N) / N
    s = sum(rng.uniform(0, 1) * np.sin(2 * np.pi * (h * x + rng.uniform())) for h in (1, 2, 3, 5))
    s = (s - s.min()) / (s.max() - s.min())
    return lo + (hi - lo) * s


def _near_z():
    """cells a relative 1e-6 above their column's Z (peaks) and one 1e-6 below the smallest Z of all (the stop): a factor missing
    from or added to the Z_th1 the device forms moves one of them to the other side"""
    rng = np.random.default_rng(5)
    k = _Case("near_z", _smooth_z(rng, 0.02, 0.03))
    Z = z_of(k.sp)
    cols = [(0, int(np.argmax(Z))), (1, 1234), (2, 8000), (1, 6100), (0, 9599), (2, 1)]
    exp = []
    for r, c in cols:
        k.plant(r, c, f32_at_or_above(Z[c] * (1 + Z_MARGIN)))
        exp.append((r, c))
    exp.sort(key=lambda rc: (-float(k.pow32[rc]), rc))
    cb = int(np.argmin(Z))
    k.plant(2, cb, f32_below(Z[cb] * (1 - Z_MARGIN)))
    return k.done(n_peaks=len(exp), positions=exp, vanish=((2, cb),), exact_margin=True)


def _empty():
    rng = np.random.default_rng(6)
    k = _Case("empty", _smooth_z(rng, 0.02, 0.03))
    k.pow32[:] = rng.uniform(0.0, 0.019, (3, N)).astype(np.float32)
    return k.done(n_peaks=0, positions=[])


def _edges():
    """with dense (9597..9599) and dense_low (0..2): columns 3 and 9596, so that every ds_comb_arm of 0..3 meets the wrap quirk from
    both sides in the stage kernel's run; and the first column of the padded register"""
    k = _Case("edges", 0.01, background=1e-3)
    for j, (r, c) in enumerate([(0, 3), (1, 9596), (2, 9472), (0, 5000), (1, 4000), (2, 9195)]):
        k.plant(r, c, 1.0 - 0.05 * j)
    return k.done(n_peaks=6)


def _random(seed):
    """exponential background (a few elements above Z by themselves), 0..40 cells at random places with heights from a small pool
    (equal values), a smooth threshold"""
    rng = np.random.default_rng(1000 + seed)
    k = _Case(f"random_{seed}", _smooth_z(rng, 0.02, 0.04))
    k.pow32[:] = rng.exponential(0.03 / 8.0, (3, N)).astype(np.float32)
    n = int(rng.integers(0, 41))
    pool = rng.uniform(0.05, 1.5, max(1, n // 2)).astype(np.float32)
    for _ in range(n):
        k.plant(int(rng.integers(0, 3)), int(rng.integers(0, N)), pool[int(rng.integers(0, pool.size))])
    return k.done()


@functools.lru_cache(maxsize=None)
def cases():
    """-> tuple of dicts (name, pow32 [3][9600] float32, frq [3][9600] int32, sp [9600], f [7], ...), built once, read-only"""
    out = [_dense("dense", (522, 523, 524), 1),            # last cells at 9597, 9598, 9599: the padded register of every row
           _dense("dense_low", (0, 1, 2), 2),              # first cells at 0, 1, 2
           _plateau(), _ties(), _ties_pad()]
    out += [_cancel(j, c) for j, c in enumerate(CANCEL_COLS)]
    out += [_floor(j, p) for j, p in enumerate(FLOOR_PEAKS)] + [_stop(False), _stop(True), _near_z(), _empty(), _edges()]
    out += [_random(s) for s in range(20)]
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c["name"] == name)


NAMES = ("dense", "dense_low", "plateau", "ties", "ties_pad") + tuple(f"cancel_{c}" for c in CANCEL_COLS) + \
        tuple(f"floor_{j}" for j in range(len(FLOOR_PEAKS))) + ("stop", "stop_after_two", "near_z", "empty", "edges") + tuple(f"random_{s}" for s in range(20))


def crafted_single(seed=99):
    """xc_incoherent_single for the stage kernel's run: eight levels only, so that most five-candidate windows hold exact ties"""
    rng = np.random.default_rng(seed)
    s = (rng.integers(1, 9, (3, N, N_F)) / 8.0).astype(np.float32)
    s.setflags(write=False)
    return s
