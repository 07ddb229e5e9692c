#!/usr/bin/env python3
"""How often the PDCCH common-search-space rule (include/lcs.h: lcs_pdcch_info) finds what was sent, and how often it accepts what
was not, measured with its numpy statement (tests/pdcch_ref.py) on the crafted grids of tests/pdcch_cases.py -- per-port channels
with a slope across the band, a CFI that changes by subframe and is taken as known -- in white noise at 0 / 5 / 10 dB per resource
element, with half of the unused CCEs filled with random QPSK (pdcch_fill = 0.5).  The device and its host twin compute the same
decisions (tests/test_gpu_pdcch.py, tests/test_pdcch_host.py), so no GPU is needed.

Per noise level: planted DCIs inside the RNTI set and how many were accepted with their bits and RNTI; decodes of candidates that
carry no planted DCI and how many of those were accepted -- split into `nested` (the candidate of the other level from the same
first CCE as a planted DCI, decoded to that DCI's payload and RNTI: an L = 4 reading of the head of an L = 8 DCI, or an L = 8
reading of an L = 4 DCI and whatever follows it; PdcchInfo.messages() lists such a pair once) and `false` (everything else: fill,
noise, a planted DCI read at the wrong size).  A false accept needs a 16-bit CRC to land in a set of 62 values: about 1e-3 per
decode.  Writes profiles/pdcch/pdcch_accuracy.json and prints the table."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pdcch", "pdcch_accuracy.json"))
    ap.add_argument("--seeds", type=int, default=3)
    a = ap.parse_args()
    import pdcch_cases as DC
    import pdcch_ref as DR
    doc = {"fill": 0.5, "cases": [DC.case_id(c) for c in DC.CASES], "seeds": a.seeds, "levels": []}
    for snr in (0.0, 5.0, 10.0):
        row = dict(snr_db=snr, planted=0, found=0, other_decodes=0, nested_accepted=0, false_accepted=0)
        for case in DC.CASES:
            for seed in range(1, a.seeds + 1):
                tfg, cfi, planted = DC.crafted(case, snr, 0.5, seed)
                n_id, cp, ports, n_rb, dur, res, _ = case
                ref = DR.receive(tfg, n_id, cp, ports, n_rb, cfi, dur, res, DC.sizes_of(case), DC.dl_mask_of(case), 7, DC.mi_of(case))
                keys = {(p["g"], p["slot"], p["i"]): p for p in planted}
                for p in planted:
                    if p["rnti"] == 0x1234:
                        continue
                    d = ref["dec"][(p["g"], p["slot"], p["i"])]
                    row["planted"] += 1
                    row["found"] += (d["bits"], d["rnti_x"], d["flags"]) == (p["bits"], p["rnti"], 3)
                for (g, s, i), d in ref["dec"].items():
                    if (g, s, i) in keys or not d["flags"] & 1:
                        continue
                    row["other_decodes"] += 1
                    if d["flags"] & 2:
                        L, cce = DR.SLOT_CAND[s]
                        nested = any(p["g"] == g and p["L"] != L and p["cce"] == cce and p["i"] == i and p["bits"] == d["bits"] and p["rnti"] == d["rnti_x"] for p in planted)
                        row["nested_accepted" if nested else "false_accepted"] += 1
        doc["levels"].append(row)
        print(row, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
