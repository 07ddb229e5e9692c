#!/usr/bin/env python3
"""What the unwrapped frequency estimate (lcs_set_foe_unwrap) buys a TDD band search: the same +- 75 kHz of coverage on the
reference's 5 kHz grid (31 hypotheses) instead of the 2.5 kHz grid (61) the native estimate needs.

One process, one context per line, 128 raw u8 buffers resident in HBM (synth.make_batch_u8(128, 1234, fcs, tdd=True,
f_off_max=60e3) at 1.9 GHz), every context set to DUPLEX_TDD.  Lines:
  a    native estimate, 2.5 kHz grid, 61 hypotheses: today's way to cover the band
  b    unwrap on, 5 kHz grid, 31 hypotheses: the same coverage
  c    native estimate, 5 kHz grid, 31 hypotheses -- timing only (the native estimate aliases there)
  c2   the same as c on a context of its own: c against c2 is the A/A spread of the run
  d, e an equal-work pair: native and unwrap on, both on the 2.5 kHz grid with 31 hypotheses over a second batch drawn within
       +- 37.5 kHz (tools/bench_tdd.py's TDD line).  Nothing aliases there, so n = 0 everywhere and both decode the same cells:
       e against d is what the mode's own kernel costs, where b against c also carries the cells c loses to aliasing
`warmup` calls per line, then `steps` timed search_batch calls per line, interleaved call by call; median and spread per line.
Also: the cells (a) and (b) decode, and how many of (a)'s (b) finds -- the same buffer and identity, frequencies within 100 Hz.
Writes one JSON file and prints it."""
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tdd", "bench_tdd_grid.json"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    n_buf, fs = 128, 1.92e6
    fcs = 1.9e9 + 100e3 * np.arange(n_buf)
    d = torch.from_numpy(pkg.synth.make_batch_u8(n_buf, 1234, fcs, tdd=True, f_off_max=60e3)).cuda()
    d2 = torch.from_numpy(pkg.synth.make_batch_u8(n_buf, 1234, fcs, tdd=True, f_off_max=37.5e3)).cuda()
    lines = [("a", False, np.arange(-30, 31) * 2.5e3), ("b", True, np.arange(-15, 16) * 5e3), ("c", False, np.arange(-15, 16) * 5e3),
             ("c2", False, np.arange(-15, 16) * 5e3), ("d", False, np.arange(-15, 16) * 2.5e3), ("e", True, np.arange(-15, 16) * 2.5e3)]
    ctx, ms, cells = {}, {k: [] for k, _, _ in lines}, {}
    for k, unwrap, f in lines:
        ctx[k] = pkg.Searcher(0)
        ctx[k].set_duplex(pkg.DUPLEX_TDD)
        ctx[k].set_foe_unwrap(unwrap)
    run = lambda k, f: ctx[k].search_batch((d2 if k in "de" else d).data_ptr(), pkg.FMT_IQ_U8, n_buf, 153600, f, fcs, fcs, fs, pkg.STAGE_FULL)
    for _ in range(a.warmup):
        for k, _, f in lines:
            run(k, f)
    for _ in range(a.steps):
        for k, _, f in lines:
            t0 = time.perf_counter()
            cells[k] = run(k, f)
            ms[k].append(1e3 * (time.perf_counter() - t0))
    out = dict(n_buf=n_buf, steps=a.steps, warmup=a.warmup)
    for k, unwrap, f in lines:
        v = np.array(ms[k])
        out[k] = dict(foe_unwrap=bool(unwrap), n_f=int(f.size), grid_step_hz=float(f[1] - f[0]), ms_median=float(np.median(v)), ms_min=float(v.min()),
                      ms_max=float(v.max()), ms_p25=float(np.percentile(v, 25)), ms_p75=float(np.percentile(v, 75)), ms_all=[round(x, 3) for x in v],
                      cells_decoded=int(sum(len(c) for c in cells[k])), peaks_past_sss=int(ctx[k].last_batch_stats()["cells_past_sss"]))
        ctx[k].close()
    found = 0
    for b in range(n_buf):
        for ca in cells["a"][b]:
            found += any(cb.n_id_cell() == ca.n_id_cell() and abs(cb.freq_superfine - ca.freq_superfine) < 100.0 for cb in cells["b"][b])
    out["cells_of_a_found_by_b"] = int(found)
    out["a_over_b_median"] = out["a"]["ms_median"] / out["b"]["ms_median"]
    out["b_over_c_median"] = out["b"]["ms_median"] / out["c"]["ms_median"]
    out["c_over_c2_median"] = out["c"]["ms_median"] / out["c2"]["ms_median"]
    out["e_over_d_median"] = out["e"]["ms_median"] / out["d"]["ms_median"]
    out["e_equals_d_records"] = bool([[bytes(c) for c in x] for x in cells["e"]] == [[bytes(c) for c in x] for x in cells["d"]])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
