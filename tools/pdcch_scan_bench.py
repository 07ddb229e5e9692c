#!/usr/bin/env python3
"""Blind search of every CCE: milliseconds per cell beside the PDCCH stage, on one GPU in one process.

Searcher.pdcch_scan_wide (cfi_force = 3, four payload sizes: formats 0/1A, 1, 2A and 1C of the bandwidth) and Searcher.pdcch_wide
(cfi_force = 3, its 240 decodes) on the SAME resident samples, interleaved call by call, at (R, n_rb) = (4, 25) and (16, 100), 20
subframes (280 rows) of a two-port cell: host wall time of each call and the GPU time between two events on the context's stream.
Medians of 20 timings after 3 warm-ups.  The data is noise, which costs a decode what a DCI costs it.  decodes: the entries the
stage formed (flags & 1), counted from lcs_pdcch_scan_decodes.  THE BAR: the scan's GPU time per decode is at most 1/8 of the PDCCH
stage's in the same session (3 integer trellis passes against 65 in fp64).  Both calls include the transform of the control
symbols, the upload of the row list and the copy of the record.  Writes one JSON document (--out) and prints it.

    python tools/pdcch_scan_bench.py --out profiles/pdcch_scan/bench.json
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pcfich_bench import FC, FS, load_pkg, timed_pair     # noqa: E402
from pdcch_bench import once                               # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    pkg = load_pkg()
    rng = np.random.default_rng(0)
    n_ofdm = 280
    doc = {"n_ofdm": n_ofdm, "subframes": 20, "bar_ratio": 0.125, "stage": []}
    for R, n_rb in ((4, 25), (16, 100)):
        n = int(0.025 * FS * R)
        d = torch.from_numpy((0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)).cuda()
        ue = pkg.capi.dci_ue_sizes(n_rb, 2)
        sizes = (ue["0/1A"], ue["1"], ue["2A"], pkg.capi.dci_common_sizes(n_rb)[1])
        with pkg.Searcher(0) as s:
            stream = torch.cuda.ExternalStream(s._lib.lcs_stream(s._h))
            cell = pkg.new_cell(n_id_1=52, n_id_2=1, cp_type=1, n_ports=2, frame_start=100.5 * R, freq_fine=1234.0)
            cell.phich_duration, cell.phich_resource = 1, 3
            args = (cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm, 0x3FF)
            scan_cfg = pkg.capi.PdcchScanCfg.make(sizes, cfi_force=3)
            old_cfg = pkg.capi.PdcchCfg.make(pkg.capi.dci_common_sizes(n_rb), cfi_force=3)
            s.pcfich_wide(*args)
            first = once(lambda: s.pdcch_scan_wide(*args, scan_cfg))
            (sh, sg), (oh, og) = timed_pair([lambda: s.pdcch_scan_wide(*args, scan_cfg), lambda: s.pdcch_wide(*args, old_cfg)], stream)
            rec = s.pdcch_scan_wide(*args, scan_cfg)
            n_dec = sum(1 for g in range(rec.n_sf) for e in s.pdcch_scan_decodes(g) if e.flags & 1)
            n_old = len(list(s.pdcch_wide(*args, old_cfg).entries()))
            per_new, per_old = 1e3 * sg / n_dec, 1e3 * og / n_old
            doc["stage"].append(dict(R=R, n_rb=n_rb, n_ports=2, sizes=list(sizes), n_cce=int(rec.n_cce[0]), candidates=int(rec.sf[0].n_cand),
                                     scan_decodes=n_dec, scan_first_call_ms=round(first, 4), scan_host_ms_per_cell=round(sh, 4), scan_gpu_ms_per_cell=round(sg, 4),
                                     pdcch_decodes=n_old, pdcch_host_ms_per_cell=round(oh, 4), pdcch_gpu_ms_per_cell=round(og, 4),
                                     scan_us_per_decode=round(per_new, 5), pdcch_us_per_decode=round(per_old, 5), ratio=round(per_new / per_old, 5),
                                     bar_met=bool(per_new <= 0.125 * per_old)))
        del d
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
