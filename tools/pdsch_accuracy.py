#!/usr/bin/env python3
"""What the 32-step windows of the PDSCH rule (include/lcs.h: lcs_pdsch_info) cost against a plain full-block max-log-MAP decoder,
measured with the numpy statement of the rule (tests/pdsch_ref.py) on the crafted grids of tests/pdsch_cases.py in white noise at
-2 / 0 / 2 / 4 / 6 dB per resource element.  The device and its host twin compute the windowed rule's decisions (tests/
test_gpu_pdsch.py, tests/test_pdsch_host.py), so no GPU is needed.  The grants are read with the PDCCH as it decodes at that
noise; the de-rate-matched values of every followed grant go through both decoders (8 iterations at the most).

Per noise level: blocks followed whose rate leaves room (3 (K + 4) <= 2 G, so that a failure is the noise's), block errors and
mean iterations of either decoder.  Writes profiles/pdsch/pdsch_accuracy.json and prints the table."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pdsch", "pdsch_accuracy.json"))
    ap.add_argument("--seeds", type=int, default=2)
    a = ap.parse_args()
    import pdcch_cases as DC
    import pdcch_ref as DR
    import pdsch_cases as SC
    import pdsch_ref as SR
    doc = {"cases": [SC.case_id(c) for c in SC.CASES], "seeds": a.seeds, "window": SR.WIN, "max_iter": 8, "levels": []}
    for snr in (-2.0, 0.0, 2.0, 4.0, 6.0):
        row = dict(snr_db=snr, blocks=0, windowed_errors=0, full_errors=0, windowed_iterations=0, full_iterations=0)
        for case in SC.CASES:
            for seed in range(1, a.seeds + 1):
                tfg, cfi, planted = SC.crafted(case, snr, seed)
                n_id, cp, ports, n_rb, res, mi = case
                pc = SC.pdcch_case(case)
                pdc = DR.receive(tfg, n_id, cp, ports, n_rb, cfi, 1, res, DC.sizes_of(pc), DC.dl_mask_of(pc), 7, DC.mi_of(pc))
                sent = {(p["g"], p["rnti"], p["rb_start"], p["n_prb"]) for p in planted if p["bits"] is not None and not p["silent"]}
                for b in SR.receive(tfg, n_id, cp, ports, n_rb, pdc, 0, mi is not None, DC.dl_mask_of(pc), 1):
                    if "d" not in b or (b["subframe"], b["rnti"], b["rb_start"], b["n_prb"]) not in sent or 3 * (b["K"] + 4) > 4 * b["n_re"]:
                        continue
                    full = SR.turbo_decode(b["d"], b["K"], b["F"], 8, win=b["K"])
                    row["blocks"] += 1
                    row["windowed_errors"] += b["status"] != 1
                    row["full_errors"] += full["status"] != 1
                    row["windowed_iterations"] += b["n_iter"]
                    row["full_iterations"] += full["n_iter"]
        n = max(row["blocks"], 1)
        row["windowed_iterations"] = round(row["windowed_iterations"] / n, 3)
        row["full_iterations"] = round(row["full_iterations"] / n, 3)
        doc["levels"].append(row)
        print(row, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
