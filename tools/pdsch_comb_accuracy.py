#!/usr/bin/env python3
"""What combining redundancy versions gains (include/lcs.h: lcs_pdsch_comb_info), measured with the numpy statement of the rule
(tests/pdsch_comb_ref.py on tests/pdsch_ref.py) on crafted grids (tests/pdsch_comb_cases.py's) in white noise at -6 .. +8 dB per
resource element ON EVERY ELEMENT, the reference elements included, so the channel estimate is as noisy as the data.  The device and
its host twin compute the rule's decisions (tests/test_gpu_pdsch_comb.py, tests/test_pdsch_comb_host.py), so no GPU is needed.

Per grid one SI transport block is sent four times, in grid subframes 5, 15, 25, 35 with rv 0, 2, 3, 1 (SIB1's order), as forced
grants with the planted CFI, so that neither the PCFICH nor the PDCCH decides what is counted.  Four geometries: 256 bits on 3 RB of
15 (two ports), 144 bits on 2 RB of 6 (one port), 440 bits on 4 RB of 15 (four ports, extended CP), 600 bits on 5 RB of 25 (two ports,
TDD); every single transmission holds at least 1.4 K coded bits.  Counted per noise level: block errors (a payload that is not the
planted one, whatever the CRC says) of a single transmission (all four, and rv 0 alone) and of the sum of the first 2, 3 and 4; and
the CRC-passing wrong payloads among them.  Writes profiles/pdsch_comb/pdsch_comb_accuracy.json and prints the table."""
import argparse
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

GEOM = [((141, 1, 2, 15, 1, None), 0, 3, 8), ((0, 1, 1, 6, 1, None), 2, 2, 5), ((256, 2, 4, 15, 4, None), 9, 4, 12),
        ((142, 1, 2, 25, 3, (0, 1, None, None, 1, 0, 1, None, None, 1)), 1, 5, 15)]      # (case, rb_start, n_prb, mcs of TBS column 2)
SNRS = (-6.0, -4.0, -2.0, 0.0, 2.0, 4.0, 6.0, 8.0)      # (beyond +4 dB only so that the single transmission's threshold is inside the range)
RVS = (0, 2, 3, 1)


def one(job):
    import numpy as np
    import pdsch_comb_cases as CC
    import pdsch_comb_ref as CR
    import pdsch_ref as SR
    gi, snr, seed = job
    case, rb, n_prb, mcs = GEOM[gi]
    sc = CC.S("accuracy-%d-%g-%d" % (gi, snr, seed), case, 36, [CC.G(5 + 10 * i, rb, n_prb, mcs, 0, rv, "a") for i, rv in enumerate(RVS)], forced=True, snr_all=snr, seed=1 + seed + 100 * gi + 1000 * SNRS.index(snr))
    tfg, cfi, planted = CC.crafted(sc)
    n_id, cp, ports, n_rb = case[:4]
    blocks = SR.receive(tfg, n_id, cp, ports, n_rb, dict(cfi=cfi, dec={}), 0, case[5] is not None, CC.mask_of(sc), 1, forced=CC.forced_list(sc))
    want = SR.payload_bytes(planted[0]["bits"], 0, planted[0]["tbs"])
    out = dict(single=[], sums={})
    for b in blocks:
        out["single"].append((b["rv"], int(b["status"] == 1), int(np.array_equal(b["payload"], want)), b["n_iter"]))
    K, F, tbs = blocks[0]["K"], blocks[0]["F"], blocks[0]["tbs"]
    for n in (2, 3, 4):
        with np.errstate(all="ignore"):
            res = SR.turbo_decode(CR.summed(blocks, list(range(n))), K, F, 8)
        pay = SR.payload_bytes(res["bits"], F, tbs)
        out["sums"][n] = (int(res["status"] == 1), int(np.array_equal(pay, want)), res["n_iter"])
    return snr, out


def crossing(levels, key, at=0.5):
    """the noise level at which the block error rate crosses `at`, linear between the two levels around it; None outside"""
    pts = [(r["snr_db"], r[key] / max(r[key.replace("errors", "blocks")], 1)) for r in levels]
    for (s0, e0), (s1, e1) in zip(pts, pts[1:]):
        if e0 >= at > e1:
            return round(s0 + (e0 - at) / (e0 - e1) * (s1 - s0), 2)
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pdsch_comb", "pdsch_comb_accuracy.json"))
    ap.add_argument("--seeds", type=int, default=10)
    ap.add_argument("--workers", type=int, default=8)
    a = ap.parse_args()
    jobs = [(gi, snr, seed) for snr in SNRS for gi in range(len(GEOM)) for seed in range(a.seeds)]
    with ProcessPoolExecutor(a.workers) as ex:
        results = list(ex.map(one, jobs, chunksize=2))
    levels = []
    for snr in SNRS:
        row = dict(snr_db=snr, single_blocks=0, single_errors=0, single_false_ok=0, rv0_blocks=0, rv0_errors=0, single_iterations=0.0)
        for n in (2, 3, 4):
            row.update({"sum%d_blocks" % n: 0, "sum%d_errors" % n: 0, "sum%d_false_ok" % n: 0, "sum%d_iterations" % n: 0.0})
        for s, out in results:
            if s != snr:
                continue
            for rv, ok, right, it in out["single"]:
                row["single_blocks"] += 1
                row["single_errors"] += not right
                row["single_false_ok"] += ok and not right
                row["single_iterations"] += it
                if rv == 0:
                    row["rv0_blocks"] += 1
                    row["rv0_errors"] += not right
            for n, (ok, right, it) in out["sums"].items():
                row["sum%d_blocks" % n] += 1
                row["sum%d_errors" % n] += not right
                row["sum%d_false_ok" % n] += ok and not right
                row["sum%d_iterations" % n] += it
        row["single_iterations"] = round(row["single_iterations"] / max(row["single_blocks"], 1), 3)
        for n in (2, 3, 4):
            row["sum%d_iterations" % n] = round(row["sum%d_iterations" % n] / max(row["sum%d_blocks" % n], 1), 3)
        levels.append({k: (int(v) if isinstance(v, bool) or (isinstance(v, int)) else v) for k, v in row.items()})
        print(levels[-1], flush=True)
    half = {k: crossing(levels, k + "_errors") for k in ("single", "rv0", "sum2", "sum3", "sum4")}
    doc = dict(geometries=[dict(case=list(g[0][:5]), tdd=g[0][5] is not None, rb_start=g[1], n_prb=g[2], mcs=g[3]) for g in GEOM], rvs=list(RVS), seeds=a.seeds,
               max_iter=8, levels=levels, snr_db_at_half_block_errors=half)
    print(half)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
