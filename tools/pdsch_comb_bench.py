#!/usr/bin/env python3
"""Combined redundancy versions: what lcs_pdsch_comb_wide costs beside lcs_pdsch_wide, on one GPU in one process.

Searcher.pdsch_comb_wide and Searcher.pdsch_wide on the SAME resident samples, interleaved call by call (tools/pdsch_bench.py's
method: host wall time of each call and the GPU time between two events on the context's stream, medians of 20 after 3 warm-ups),
at (R, n_rb) = (1, 6) and (2, 15), 26 subframes of a two-port cell with a SIB1 schedule (synth.sib1_schedule), subframe 5 only.
Two cases: `members_decode` -- the message on six resource blocks, every transmission decodes alone, so the grouping and the record
run and no combined decode does; `members_fail` -- 296 bits (K = 320) on one resource block with rv 1 and 0, fewer coded bits than
information bits in each, so one combined decode sits at the tail of the call.  Beside them lcs_turbo_decode at that K on noise (eight
iterations, one workgroup).  Writes one JSON document (--out) and prints it.

    python tools/pdsch_comb_bench.py --out profiles/pdsch_comb/pdsch_comb_bench.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pcfich_bench import FC, FS, load_pkg, timed_pair     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    pkg = load_pkg()
    doc = {"subframes": 26, "dl_mask": 1 << 5, "case": []}
    for R, n_rb in ((1, 6), (2, 15)):
        n_ofdm = 26 * 14
        for name, sfn0, n_bits, n_prb in (("members_decode", 7, 176, 6), ("members_fail", 13, 296, 1)):
            msg = np.random.default_rng(5).integers(0, 2, n_bits).astype(np.uint8)
            pdcch, pdsch, what = pkg.synth.sib1_schedule(msg, n_rb, sfn0, n_prb=n_prb)
            cellcfg = dict(n_id_1=52, n_id_2=1, cp_normal=True, n_ports=2, f_off=0.0, t0=100.0, sfn0=sfn0, n_rb_dl=n_rb, cfi=3, pdcch=pdcch, pdsch=pdsch)
            x, _, _ = pkg.synth.make_wideband_cell(7, FC, R, [(FC, R, n_rb, cellcfg)], snr_db=20.0, n_in=4 * 19200 * R)
            d = torch.from_numpy(x).cuda()
            with pkg.Searcher(0) as s:
                stream = torch.cuda.ExternalStream(s._lib.lcs_stream(s._h))
                cell = pkg.new_cell(n_id_1=52, n_id_2=1, cp_type=1, n_ports=2, frame_start=(19200.0 - 100.0) * R, freq_fine=0.0)
                cell.n_rb_dl, cell.phich_duration, cell.phich_resource = n_rb, 1, 3
                args = (cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm, 1 << 5)
                cfg = pkg.capi.PdcchCfg.make(pkg.capi.dci_common_sizes(n_rb))
                s.pdsch_comb_wide(*args, cfg)
                (ch, cg), (ph, pg) = timed_pair([lambda: s.pdsch_comb_wide(*args, cfg), lambda: s.pdsch_wide(*args, cfg)], stream)
                rec, comb = s.pdsch_comb_wide(*args, cfg)
                K = what["tbs"] + 24
                noise = np.random.default_rng(3).standard_normal((3, K + 4))
                (th, tg), = timed_pair([lambda: s.turbo_decode(noise, K)], stream)
                doc["case"].append(dict(case=name, R=R, n_rb=n_rb, tbs=what["tbs"], blocks=[(b["subframe"], b["rv"], b["status"], b["n_iter"]) for b in rec.blocks()],
                                        groups=[(g["members"], g["status"], g["n_iter"]) for g in comb.groups()],
                                        comb_host_ms=round(ch, 4), comb_gpu_ms=round(cg, 4), pdsch_host_ms=round(ph, 4), pdsch_gpu_ms=round(pg, 4),
                                        extra_host_ms=round(ch - ph, 4), extra_gpu_ms=round(cg - pg, 4),
                                        turbo_K=K, turbo_8_iterations_host_ms=round(th, 4), turbo_8_iterations_gpu_ms=round(tg, 4)))
            del d
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
