"""The PDSCH stage at every turbo block size and at 50 / 75 / 100 resource blocks, on the CPU: what tests/test_pdsch_host.py checks
at a handful of sizes, over the whole table.

The kernel's shape changes with the block size K: ceil(K / 32) windows, a last window of 8, 16, 24 or 32 steps, one wave up to
K = 2048 and two beyond; four dummy columns in the sub-block interleaver where K = 24 (mod 32); up to 63 fillers.  The scrambling
sequence of a block is reached by jumping 160 2^b clocks for every bit b of the chunk number, and bit 7 needs 20 480 soft bits: an
allocation of about 74 resource blocks.  So: the generator's rate matching against a loop-form statement of 36.212 5.1.4.1 written
here, the host twin's de-rate-matching and decoder against numpy at all 127 sizes with and without fillers, the block size tables
over their whole domain, the whole record on grids of 100, 75 and 50 resource blocks, forced grants at the sizes the crafted
grids do not reach (the plan tests/test_gpu_pdsch_sizes.py runs on the device), and the stand-alone sanitizer program on them."""
import collections
import math
import subprocess

import numpy as np
import pytest

import pcfich_cases as PC
import pcfich_ref as PR
import pdcch_cases as DC
import pdsch_cases as SC
import pdsch_ref as SR
import test_pdsch_host as TH
from conftest import load_pkg


@pytest.fixture(scope="module")
def H():
    return SC.load_twin(load_pkg().capi)


def all_k():
    return load_pkg().synth.TURBO_K


# ---------------------------------------------------------------- 36.212 5.1.4.1.1 - 2 in loops
NULL = -1
# table 5.1.4-1: the inter-column permutation of the turbo code's sub-block interleaver
COLUMNS = [0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30, 1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31]


def circular_buffer(K, F):
    """w of one code block whose value k of stream i is the number i (K + 4) + k; <NULL> for the dummies and for the F fillers of
    d(0) and d(1) -> (w, R)"""
    D = K + 4
    R = 1
    while 32 * R < D:
        R += 1
    K_pi = 32 * R
    v = []
    for i in range(3):
        y = [NULL] * (K_pi - D)                                  # the N_D dummy bits come first
        for k in range(D):
            y.append(NULL if i < 2 and k < F else i * D + k)
        if i < 2:                                                # written row by row, columns permuted, read column by column
            out = []
            for col in range(32):
                for row in range(R):
                    out.append(y[32 * row + COLUMNS[col]])
        else:                                                    # v(2)_k = y_pi(k), pi(k) = (P(floor(k / R)) + 32 (k mod R) + 1) mod K_pi
            out = []
            for k in range(K_pi):
                out.append(y[(COLUMNS[k // R] + 32 * (k % R) + 1) % K_pi])
        v.append(out)
    w = list(v[0])
    for k in range(K_pi):
        w.append(v[1][k])
        w.append(v[2][k])
    return w, R


def select(w, R, rv, E):
    """bit selection without a soft-buffer limit (N_cb = K_w): E values from k0, past the nulls, around the buffer"""
    n_cb = len(w)
    k0 = R * (2 * int(math.ceil(n_cb / (8.0 * R))) * rv + 2)
    e, j = [], 0
    while len(e) < E:
        x = w[(k0 + j) % n_cb]
        if x != NULL:
            e.append(x)
        j += 1
    return e


def test_generators_rate_matching_equals_the_standard_s_loops():
    """synth.turbo_ratematch is what tests/pdsch_ref.py's de-rate-matching and every planted block lean on: on indices it equals the
    loop form above at every size, every rv, without fillers and with the most a size can have, across the buffer's wrap"""
    synth = load_pkg().synth
    n = 0
    for K in all_k():
        D = K + 4
        idx = np.arange(3 * D, dtype=np.int64).reshape(3, D)
        for F in (0, SC.filler_step(K) - 1):
            w, R = circular_buffer(K, F)
            N = 3 * D - 2 * F
            assert sum(x != NULL for x in w) == N and len(w) == 96 * R
            for rv in range(4):
                assert synth.turbo_ratematch(idx, N + 5, rv, F).tolist() == select(w, R, rv, N + 5), (K, F, rv)
                n += 1
    assert n == 127 * 8


# ---------------------------------------------------------------- the tables over their whole domain
def test_block_size_index_over_its_whole_domain(H):
    K_all = all_k()
    assert len(K_all) == 127 and [H.pdsch_host_k_at(i) for i in range(127)] == K_all
    for B in range(1, 2241):
        want = next(i for i, K in enumerate(K_all) if K >= B)
        assert H.pdsch_host_k_ceil_index(B) == want, B
        assert H.pdsch_host_k_index(B) == (want if K_all[want] == B else -1), B
    assert H.pdsch_host_k_ceil_index(2241) == -1 and H.pdsch_host_k_index(2241) == -1
    for K in K_all:                        # SC.filler_step: the distance to the size below (the smallest size has none below it)
        assert SR.block_size(K - 24 - (SC.filler_step(K) - 1)) == (K, SC.filler_step(K) - 1)
        assert K == 40 or SR.block_size(K - 24 - SC.filler_step(K)) == (K - SC.filler_step(K), 0)


def prime_factors(n):
    out, p = set(), 2
    while p * p <= n:
        while n % p == 0:
            out.add(p)
            n //= p
        p += 1
    return out | ({n} if n > 1 else set())


def test_qpp_every_size(H):
    """the interleaver of every size is a permutation and the generator's; f1 is coprime to K and every prime factor of K divides f2
    (what makes a quadratic polynomial a permutation for these K), which catches slips that still give a permutation by luck"""
    synth = load_pkg().synth
    f = np.zeros(2, np.int32)
    for i, K in enumerate(all_k()):
        perm = np.zeros(K, np.int32)
        H.pdsch_host_perm(K, SC._ip(perm))
        assert np.array_equal(np.sort(perm), np.arange(K)) and np.array_equal(perm, synth.turbo_interleaver(K)), K
        H.pdsch_host_qpp(i, SC._ip(f))
        f1, f2 = int(f[0]), int(f[1])
        assert (f1, f2) == synth.TURBO_QPP[K] and math.gcd(f1, K) == 1 and all(f2 % p == 0 for p in prime_factors(K)), (K, f1, f2)


# ---------------------------------------------------------------- de-rate-matching
def test_derm_against_numpy_every_size(H):
    """the rank tables (pds_rank_build, pds_k0) and pds_derm_value: a third of the buffer, just past one turn, past two"""
    rng = np.random.default_rng(77)
    n = 0
    for K in all_k():
        for F in (0, SC.filler_step(K) - 1):
            N = 3 * (K + 4) - 2 * F
            d = np.zeros((3, K + 4))
            for rv in range(4):
                for G in (N // 3, N + 7, 2 * N + 10):
                    llr = rng.standard_normal(G)
                    H.pdsch_host_derm(SC._dp(llr), G, K, F, rv, SC._dp(d))
                    assert np.array_equal(d, SR.derm(llr, K, F, rv)), (K, F, rv, G)
                    n += 1
    assert n == 127 * 24


# ---------------------------------------------------------------- the decoder
def test_decoder_against_numpy_every_size(H):
    """every number of windows and every length of the last one, with and without fillers: decisions, iterations and status equal
    numpy's, whose posteriors stay clear of zero; every block of the two noise levels decodes to what was encoded"""
    blocks, twin = SC.size_blocks(), SC.size_blocks_twin()
    hist, seen = collections.Counter(), set()
    for b, (bits, n_iter, st) in zip(blocks, twin):
        ref = SR.turbo_decode(b["d"], b["K"], b["F"], b["max_iter"])
        assert ref["margin"] > 1e-9
        assert (st, n_iter) == (ref["status"], ref["n_iter"]) and np.array_equal(bits, ref["bits"]), (b["K"], b["F"], b["sigma"], st, n_iter, ref["status"], ref["n_iter"])
        if b["sigma"] == 3.0:
            assert (st, n_iter) == (SR.STATUS["crc"], b["max_iter"]), (b["K"], n_iter)
        else:
            assert st == SR.STATUS["ok"] and np.array_equal(bits, b["c"]), (b["K"], b["F"])
        if b["sigma"] in (0.85, 0.95):
            hist[n_iter] += 1
            seen.add((b["K"], b["F"] > 0))
    assert seen == {(K, f) for K in all_k() for f in (False, True)}
    assert len(blocks) == 254 + 14 + 3 and sum(hist.values()) == 254 and max(hist) >= 3, sorted(hist.items())
    slow = {b["K"] for b, t in zip(blocks, twin) if t[2] == 1 and t[1] >= 3}
    assert {K % 32 for K in slow} == {0, 8, 16, 24} and slow >= {2112, 2176, 2240}      # (what the GPU test wants to see)


# ---------------------------------------------------------------- 100, 75 and 50 resource blocks
@pytest.mark.parametrize("case", SC.WIDE_CASES, ids=SC.case_id)
def test_record_against_numpy_on_wide_grids(H, case):
    """tests/test_pdsch_host.py's test_record_against_numpy on the wide grids: soft bits and de-rate-matched values to 1e-12, every
    field equal, nothing excused.  At 100 resource blocks two blocks need the jump of bit 7 of the chunk number"""
    TH.test_record_against_numpy(H, case)
    _, blocks = SC.reference(case)
    chunks = sorted(-(-len(b["llr"]) // 160) for b in blocks if "llr" in b)
    assert (chunks[-2] > 128) == (case[3] == 100) and sum(b["status"] == 1 for b in blocks) >= 8, chunks


# ---------------------------------------------------------------- forced grants at the large sizes
@pytest.mark.parametrize("call", (0, 1))
def test_forced_grants_at_the_large_sizes(H, call):
    """the plan of tests/test_gpu_pdsch_sizes.py, settled here: the twin's record equals numpy's, every planted block comes back"""
    capi = load_pkg().capi
    case, tfg, calls, planted = SC.large_forced()
    blocks = SC.large_forced_reference(call)
    pdc = SC.pdcch_twin_record(capi, case, tfg, SC.crafted(case)[1])
    rec = SC.twin_record(H, capi, case, tfg, pdc, cfg=SC.make_cfg(capi, forced=calls[call]))
    assert SC.assert_blocks_against_numpy(rec, blocks, "call %d" % call) == (4, 0)
    by = {(g[0], g[2]): bits for g, bits in zip(calls[call], planted[call])}
    for b in rec.blocks():
        assert b["crc_ok"] and b["bytes"] == np.packbits(by[(b["subframe"], b["rb_start"])]).tobytes(), (b["subframe"], b["K"], b["F"])
    want = {p[4:7] for p in SC.LARGE_PLAN if p[0] == call}
    assert {(b["K"], b["F"], b["rv"]) for b in rec.blocks()} == want
    if call == 0:
        assert max(b["n_iter"] for b in rec.blocks()) >= 2
    N = lambda b: 3 * (b["K"] + 4) - 2 * b["F"]
    assert any(2 * b["n_re"] < N(b) for b in rec.blocks()) and any(2 * b["n_re"] > N(b) for b in rec.blocks())


def test_the_plan_of_forced_grants_has_what_it_is_for():
    pairs = {p[4:6] for p in SC.LARGE_PLAN}
    assert {(2240, 63), (2240, 0), (2112, 55), (2048, 0), (1056, 31), (528, 15)} <= pairs and any(K == 2176 for K, _ in pairs)
    assert any(K % 32 == 24 and F == 7 for K, F in pairs) and {p[6] for p in SC.LARGE_PLAN} == {0, 1, 2, 3}


# ---------------------------------------------------------------- the stand-alone program under the sanitizers
def test_stand_alone_program_under_the_sanitizers_at_the_large_sizes(H, tmp_path):
    """tests/test_pdsch_host.py's program (its own main, -fsanitize=address,undefined): a clean exit and the library's results on the
    100 resource block grid and on direct decodes at the last size with 63 fillers, at the end of the first wave and at K = 56"""
    capi = load_pkg().capi
    if SC.stale(SC.SAN):
        subprocess.check_call(PC.HIPCC + ["-O1", "-g", "-DPDSCH_HOST_MAIN", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                                          "-fno-sanitize-recover=undefined", "-o", SC.SAN, SC.TWIN_SRC])
    direct = [b for b in SC.size_blocks() if (b["K"], b["F"], b["sigma"]) in ((2240, 63, 0.95), (2048, 0, 0.85), (56, 0, 0.85), (2240, 0, 3.0)) and b["max_iter"] != 1]
    assert len(direct) == 4
    case = SC.WIDE_CASES[0]
    tfg, cfi, _ = SC.crafted(case)
    pdc = SC.pdcch_twin_record(capi, case, tfg, cfi)
    n_id, cp, ports, n_rb = case[:4]
    cfg = SC.make_cfg(capi)
    path = tmp_path / "grid.bin"
    with open(path, "wb") as f:
        f.write(np.array([tfg.shape[0], PR.n_symb_of(cp), n_rb, n_id, cp, ports, DC.dl_mask_of(SC.pdcch_case(case)), 1, 0, len(direct)], np.int32).tobytes() +
                SC.jump_tables(n_rb).tobytes() + bytes(cfg) + bytes(pdc) + np.ascontiguousarray(tfg, np.complex128).tobytes())
        for b in direct:
            f.write(np.array([b["K"], b["F"], b["max_iter"], 0], np.int32).tobytes() + np.ascontiguousarray(b["d"]).tobytes())
    r = subprocess.run([SC.SAN, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-2000:]
    lines = [[int(x) for x in l.split()] for l in r.stdout.splitlines()]
    o = SC.twin_record(H, capi, case, tfg, pdc, cfg=cfg)
    assert lines[0] == [o.n_sf, o.n_blocks, o.n_ok, o.n_si, o.n_paging, o.n_ra, o.n_overflow] and o.n_ok >= 8
    want = [[b.subframe, b.slot, b.status, b.n_iter, b.n_re, b.K, int(np.ctypeslib.as_array(b.payload).sum())] for b in (o.block[i] for i in range(o.n_blocks))]
    assert lines[1:1 + o.n_blocks] == want
    for b, got in zip(direct, lines[1 + o.n_blocks:]):
        bits, n_iter, st = SC.twin_turbo(H, b["d"], b["K"], b["F"], b["max_iter"])
        assert got == [st, n_iter, H.pdsch_host_crc24a(SC._bp(bits), b["K"])]
    assert len(lines) == 1 + o.n_blocks + len(direct)
