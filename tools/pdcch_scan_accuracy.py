#!/usr/bin/env python3
"""Which min_quality the blind search of every CCE (include/lcs.h: lcs_pdcch_scan_info) needs, measured with the numpy statement of
its rule (tests/pdcch_scan_ref.py) on the crafted grids of tests/pdcch_scan_cases.py in white noise at 0 / 5 / 10 / 20 dB per
resource element, with the unused CCEs of every subframe filled with random bits with probability 0.5 and 1, three seeds each.  The
device and its host twin compute the same integers (tests/test_gpu_pdcch_scan.py, tests/test_pdcch_scan_host.py): no GPU is needed.

Every grid is decoded once; the acceptance (in space, quality >= q, min_repeat = 2; common accepts as they are) is then applied for
q = 0.50, 0.55, .. 1.00.  A false accept is an accepted entry that is neither planted nor a re-reading of a planted DCI (the same
subframe, RNTI, size and bits on overlapping CCEs).  THE CAP: at most 0.5 % of the decodes examined, per grid.  min_quality governs
the UE accepts alone -- a common accept (SI, paging, RA at L = 4 / 8 below CCE 16) has no quality condition, as in the PDCCH stage, and
one of them in a 6 RB grid of 120 decodes is already 0.8 % whatever q is -- so the default of min_quality is the smallest q from
which on every grid of every noise level keeps its false UE accepts inside the cap; the false common accepts are counted beside
them.  Per q and noise level: the false UE accepts and the worst grid's share of them, the false common accepts, and the share of
the planted recurring DCIs (kinds a, b and common) that are accepted with their bits.
Writes profiles/pdcch_scan/accuracy.json and prints the table."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
CAP = 0.005


def accept(ref, q, min_repeat=2):
    """the rule's acceptance at threshold q on receive()'s decodes -> set of accepted keys"""
    hit = {k for k, d in ref["dec"].items() if d["flags"] & 4 and d["quality"] >= q}
    seen = {}
    for k in hit:
        seen.setdefault(ref["dec"][k]["rnti_x"], set()).add(k[0])
    return {k for k in hit if len(seen[ref["dec"][k]["rnti_x"]]) >= min_repeat} | {k for k, d in ref["dec"].items() if d["flags"] & 16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pdcch_scan", "accuracy.json"))
    ap.add_argument("--seeds", type=int, default=3)
    a = ap.parse_args()
    import pdcch_scan_cases as SC
    import pdcch_scan_ref as SR
    qs = [round(0.5 + 0.05 * i, 2) for i in range(11)]
    snrs, fills = (0.0, 5.0, 10.0, 20.0), (0.5, 1.0)
    doc = {"cap": CAP, "fills": list(fills), "seeds": a.seeds, "cases": [SC.case_id(c) for c in SC.CASES], "thresholds": qs, "levels": []}
    worst = {q: 0.0 for q in qs}
    for snr in snrs:
        row = dict(snr_db=snr, grids=0, decodes=0, planted=0, false_common=0, worst_false_share={q: 0.0 for q in qs}, false_accepts={q: 0 for q in qs}, found={q: 0 for q in qs})
        for case in SC.CASES:
            for fill in fills:
                for seed in range(1, a.seeds + 1):
                    tfg, cfi, planted = SC.crafted(case, snr, fill, seed)
                    n_id, cp, ports, n_rb, dur, res = case[:6]
                    ref = SR.receive(tfg, n_id, cp, ports, n_rb, cfi, dur, res, SC.sizes_of(case), 0.0, 1, SC.dl_mask_of(case), 7, SC.mi_of(case))
                    n = sum(1 for d in ref["dec"].values() if d["flags"] & 1)
                    want = [p for p in planted if p["kind"] in ("a", "b", "common")]
                    row["grids"] += 1
                    row["decodes"] += n
                    row["planted"] += len(want)
                    cand = {g: SR.candidates(s["n_cce"]) for g, s in enumerate(ref["sf"])}
                    is_false = lambda k, d: not SC.rereading(dict(subframe=k[0], L=d["L"], cce=d["cce"], size_index=k[2], bits=d["bits"], rnti=d["rnti_x"]), planted)
                    row["false_common"] += sum(1 for k, d in ref["dec"].items() if d["flags"] & 16 and is_false(k, d))
                    for q in qs:
                        acc = accept(ref, q)
                        fa = 0
                        for k in acc:
                            d = ref["dec"][k]
                            if d["flags"] & 16:
                                continue
                            fa += not SC.rereading(dict(subframe=k[0], L=d["L"], cce=d["cce"], size_index=k[2], bits=d["bits"], rnti=d["rnti_x"]), planted)
                        row["false_accepts"][q] += fa
                        row["worst_false_share"][q] = max(row["worst_false_share"][q], fa / n)
                        for p in want:
                            k = (p["g"], cand[p["g"]].index((p["L"], p["cce"])), p["i"])
                            row["found"][q] += k in acc and ref["dec"][k]["bits"] == p["bits"] and ref["dec"][k]["rnti_x"] == p["rnti"]
                    SC.crafted.cache_clear()
        for q in qs:
            worst[q] = max(worst[q], row["worst_false_share"][q])
        row["found_share"] = {str(q): round(row["found"][q] / max(row["planted"], 1), 4) for q in qs}
        row["worst_false_share"] = {str(q): round(v, 5) for q, v in row["worst_false_share"].items()}
        row["false_accepts"] = {str(q): v for q, v in row["false_accepts"].items()}
        del row["found"]
        doc["levels"].append(row)
        print("snr %4.1f dB: %d grids, %d decodes, %d planted, false common accepts %d" % (snr, row["grids"], row["decodes"], row["planted"], row["false_common"]))
        for q in qs:
            print("   q %.2f  false UE accepts %4d  worst grid %.4f  found %.4f" % (q, row["false_accepts"][str(q)], row["worst_false_share"][str(q)], row["found_share"][str(q)]))
    inside = [q for q in qs if all(worst[p] <= CAP for p in qs if p >= q)]
    doc["min_quality"] = inside[0] if inside else None
    print("smallest threshold inside the cap at every noise level:", doc["min_quality"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
