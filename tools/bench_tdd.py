#!/usr/bin/env python3
"""For information: what the full chain costs on TDD buffers next to FDD buffers of the same occupancy.

The same harness for both modes, so the two lines compare with each other (not with bench.py's pipelined figure): one context,
128 raw u8 buffers resident in HBM -- synth.make_batch_u8 as bench.py's default line draws it (every 4th carrier holds 1-2 cells),
once with FDD cells on the 5 kHz grid, once with the same draws as TDD cells on a 2.5 kHz grid of the same 31 hypotheses with the
context set to DUPLEX_TDD -- and `steps` timed search_batch calls after `warmup`.  The SSS windows move and their number does not:
the two are expected to cost the same.  Writes one JSON file and prints it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_outputs", "bench_tdd.json"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    n_buf, fs = 128, 1.92e6
    out = {}
    for mode, fc0, step, f_off_max in (("fdd", 739e6, 5e3, 60e3), ("tdd", 1.9e9, 2.5e3, 37.5e3)):
        fcs = fc0 + 100e3 * np.arange(n_buf)
        f = np.arange(-15, 16) * step
        host = pkg.synth.make_batch_u8(n_buf, 1234, fcs, tdd=(mode == "tdd"), f_off_max=f_off_max)
        d = torch.from_numpy(host).cuda()
        with pkg.Searcher(0) as S:
            S.set_duplex(pkg.DUPLEX_TDD if mode == "tdd" else pkg.DUPLEX_FDD)
            for _ in range(a.warmup):
                cells = S.search_batch(d.data_ptr(), pkg.FMT_IQ_U8, n_buf, 153600, f, fcs, fcs, fs, pkg.STAGE_FULL)
            ms = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                cells = S.search_batch(d.data_ptr(), pkg.FMT_IQ_U8, n_buf, 153600, f, fcs, fcs, fs, pkg.STAGE_FULL)
                ms.append(1e3 * (time.perf_counter() - t0))
            stats = S.last_batch_stats()
        out[mode] = dict(n_buf=n_buf, n_f=int(f.size), grid_step_hz=step, ms_per_batch_median=float(np.median(ms)), ms_per_batch_min=float(min(ms)),
                         ms_per_batch_all=[round(x, 3) for x in ms], cells_decoded=int(sum(len(c) for c in cells)),
                         peaks_past_sss=int(stats["cells_past_sss"]), occupied_buffers=int(sum(1 for c in cells if c)))
    out["tdd_over_fdd_median"] = out["tdd"]["ms_per_batch_median"] / out["fdd"]["ms_per_batch_median"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
