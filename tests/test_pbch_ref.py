"""The numpy statement of the PBCH soft path (tests/pbch_ref.py) against the oracle's orc_pbch_soft on every case of
tests/pbch_cases.py and all twelve candidates, and what the case set itself promises -- asserted from the reference alone, no GPU:
every regime of the demodulator holds at least 200 LLRs, the elements left out as edges stay within the cap, the crafted grids
decode to what was put into them, and the oracle's decode_mib is the first passing candidate of orc_pbch_soft.

Bar: pbch_ref's per-element allowance (its docstring), the same one the device is held to.  numpy's exp / log and the C library's
differ by rounding only: the observed |difference| / allowance is of the order 1e-6."""
import numpy as np
import pytest

import oracle as O
import pbch_cases as PC
import pbch_ref as PB


@pytest.mark.parametrize("name", [n for n in PC.NAMES if n not in PC.INTEGERS_ONLY])
def test_reference_against_oracle(name):
    ref = PC.reference(name)
    e, d, _, _, _ = PC.oracle_soft(name)
    assert np.isfinite(e).all() and np.isfinite(d).all(), name
    worst = {}
    for k in range(12):
        w = PC.compare(ref[k]["e_est"], ref[k]["d_est"], name, k)
        for a, b in w["worst"].items():
            worst[a] = max(worst.get(a, 0.0), b)
    print(name, {a: f"{b:.2g}" for a, b in worst.items()})


def test_every_regime_is_populated_and_edges_stay_within_the_cap():
    count, n_all, n_edge = np.zeros(5, int), 0, 0
    for name in PC.NAMES:
        if name in PC.INTEGERS_ONLY:
            continue
        for k, r in enumerate(PC.reference(name)):
            count += np.bincount(r["regime"], minlength=5)
            n_all += r["regime"].size
            n_edge += int(r["edge"].sum())
            assert r["edge"].sum() <= 2 and r["d_edge"].sum() <= 2, (name, PB.CANDIDATES[k])
            # exactly one regime per LLR, and the ZERO ones are exactly 0 in the reference and in the oracle
            assert ((r["regime"] >= 0) & (r["regime"] <= 4)).all()
            z = r["regime"] == PB.ZERO
            assert (r["e_est"][z] == 0.0).all() and (PC.oracle_soft(name)[0][k][z] == 0.0).all(), (name, k)
    print(dict(zip(PB.REGIMES, count.tolist())), "edges", n_edge, "of", n_all)
    assert (count >= 200).all(), dict(zip(PB.REGIMES, count.tolist()))
    assert n_edge <= 1e-4 * n_all, (n_edge, n_all)


def test_the_case_set_covers_what_it_says():
    crafted = [c for n, c in PC.CASES.items() if n.startswith("id")]
    assert {(c["n_id"] % 3, c["cp"], c["n_tx"]) for c in crafted} == {(v, cp, p) for v in range(3) for cp in (1, 2) for p in (1, 2, 4)}
    assert {c["g"] for c in crafted} == {0, 1, 2, 3}
    for cp in (1, 2):
        for n_id in (300, 7, 503):
            fe = PB.frame_elements(n_id, cp)
            assert fe.shape[0] == PB.m_bit_of(cp) // 8
            with_rs = (0, 1) if cp == 1 else (0, 1, 3)
            for l in range(4):
                cols = fe[fe[:, 0] == l, 1]
                assert cols.size == (48 if l in with_rs else 72) and (np.diff(cols) > 0).all()
                assert not (l in with_rs and (cols % 3 == n_id % 3).any())
            rows, cols = PB.elements(n_id, cp, 3)
            assert rows.max() < PB.n_ofdm_of(cp) and rows.size == PB.m_bit_of(cp) // 2


@pytest.mark.parametrize("name", PC.NAMES)
def test_oracle_decodes_what_the_grid_carries(name):
    c = PC.CASES[name]
    cell, tfg = PC.grid(name)
    _, _, c_est, ok, rec = PC.oracle_soft(name)
    # decode_mib is the first passing candidate of the forced ones, in order
    first = int(np.flatnonzero(ok)[0]) if ok.any() else None
    if first is None:
        assert PC.cell_fields(rec) == PC.cell_fields(cell)
    else:
        g, p = PB.CANDIDATES[first]
        b = c_est[first].astype(int)
        bw = b[0] * 4 + b[1] * 2 + b[2]
        sfn8 = int("".join(map(str, b[6:14])), 2)
        sfn8 -= 256 if sfn8 >= 128 else 0                      # the reference's signed char
        want = (p, (6, 15, 25, 50, 75, 100)[bw] if bw < 6 else cell.n_rb_dl, 2 if b[3] else 1, 1 + 2 * b[4] + b[5], (sfn8 * 4 - g) % 1024)
        assert PC.cell_fields(rec)[:5] == want, (name, rec)
    if name == "noise-free":               # all four likelihoods of every LLR underflow for the one-port candidates: the all-zero word
        assert ok.sum() > 1 and first == 0 and (rec.n_ports, rec.n_rb_dl, rec.sfn) == (1, 6, 0)
        assert (PC.oracle_soft(name)[0][0] == 0.0).all()
    elif name == "pbch-rows-zero":
        assert ok.sum() > 1 and first == 0 and (rec.n_ports, rec.n_rb_dl, rec.sfn) == (1, 6, 0)
    elif c["kind"] == "crafted":           # the true candidate, and no other, passes with the bits that were sent
        k = PB.CANDIDATES.index((c["g"], c["n_tx"]))
        assert ok.tolist() == [i == k for i in range(12)], (name, ok)
        assert np.array_equal(c_est[k][:24], c["mib"])
        if name.startswith("reserved"):
            assert rec.n_rb_dl == c["n_rb_dl"] and rec.n_ports == c["n_tx"] and rec.phich_duration == (2 if c["mib"][3] else 1)
    else:
        g = c["cell"]
        assert (rec.n_ports, rec.n_rb_dl) == (g["n_ports"], g["n_rb_dl"]) and ok.sum() == 1


def test_single_candidate_export_is_the_batched_one():
    name = "series-cp1-tx2-24.0dB"
    cell, tfg = PC.grid(name)
    e, d, c, ok, _ = PC.oracle_soft(name)
    for k in (0, 4, 11):
        e1, d1, c1, ok1 = O.pbch_soft(cell, tfg, *PB.CANDIDATES[k])
        assert np.array_equal(e1, e[k]) and np.array_equal(d1, d[k]) and np.array_equal(c1, c[k]) and ok1 == ok[k]
    with pytest.raises(RuntimeError):
        O.pbch_soft(cell, tfg, 4, 1)
    with pytest.raises(RuntimeError):
        O.pbch_soft(cell, tfg, 0, 3)
    with pytest.raises(RuntimeError):
        O.pbch_soft(cell, tfg[:-1], 0, 1)
