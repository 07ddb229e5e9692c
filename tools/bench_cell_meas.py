#!/usr/bin/env python3
"""What the cell measurement (lcs_set_cell_meas) costs a band search, against the PARENT commit's library on the same box, in one
process.

    mkdir ../parent && git archive HEAD~ | tar -x -C ../parent && (cd ../parent && python __graft_entry__.py)      # the parent's library
    python tools/bench_cell_meas.py --parent-lib ../parent/lte-cell-scanner_amd/liblcs_amd.so

Two workloads of 128 raw u8 buffers resident in HBM, bench.py's own (synth.make_batch_u8 at 739 MHz): the band scan (every 4th
carrier holds 1-2 cells) and the dense band (2-3 cells in every buffer); 31 hypotheses on the 5 kHz grid, one context per line:
  p    the parent's library
  p2   the parent's library on a context of its own: p against p2 is the parent's spread against itself in this run
  pon  the parent's library with lcs_set_cell_meas(1), where the parent has the mode: what `on` is held against
  off  this tree, mode off
  on   this tree, lcs_set_cell_meas(1): k_cell_meas once per per-cell round
`warmup` calls per line, then `steps` timed search_batch calls per line, interleaved call by call; the medians decide.  Also: the
records of all lines are byte-identical, and what the measurement says about the cells.  Writes one JSON file and prints it.

    rocprofv3 --kernel-trace --stats -d DIR -o meas -- python tools/bench_cell_meas.py --trace-run && python tools/kernel_times.py DIR/.../meas_results.db k_cell_meas k_tdd_config k_chan_est

--trace-run: nothing is timed here -- ten dense-band batches with the mode on in FDD, then ten TDD batches (tools/bench_tdd_config.py's) with
lcs_set_tdd_config on as well, so that the trace holds k_cell_meas under both masks and k_tdd_config beside it."""
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
    ap.add_argument("--parent-lib", default=None, help="liblcs_amd.so built from the parent commit")
    ap.add_argument("--trace-run", action="store_true", help="the run to put under rocprofv3 --kernel-trace (see above)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meas", "bench_cell_meas.json"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    if a.trace_run:
        n_buf, fs = 128, 1.92e6
        for tdd in (False, True):
            fcs = (1.9e9 if tdd else 739e6) + 100e3 * np.arange(n_buf)
            f = np.arange(-15, 16) * (2.5e3 if tdd else 5e3)
            kw = dict(tdd=True, f_off_max=37.5e3) if tdd else dict(occupied_every=1, n_distinct=8, cells_cycle=(2, 3))
            d = torch.from_numpy(pkg.synth.make_batch_u8(n_buf, 1234 if tdd else 4321, fcs, **kw)).cuda()
            with pkg.Searcher(0) as s:
                s.set_duplex(pkg.DUPLEX_TDD if tdd else pkg.DUPLEX_FDD)
                s.set_tdd_config(tdd)
                s.set_cell_meas(True)
                for _ in range(10):
                    cells = s.search_batch(d.data_ptr(), pkg.FMT_IQ_U8, n_buf, 153600, f, fcs, fcs, fs, pkg.STAGE_FULL)
                print("tdd" if tdd else "fdd dense", "cells per batch", sum(len(c) for c in cells))
            del d
        return
    if not a.parent_lib:
        ap.error("--parent-lib is required (unless --trace-run)")
    parent = pkg.capi.load_other(a.parent_lib)
    parent_has_mode = hasattr(parent, "lcs_set_cell_meas")
    n_buf, fs = 128, 1.92e6
    fcs = 739e6 + 100e3 * np.arange(n_buf)
    f = np.arange(-15, 16) * 5e3
    lines = [("p", parent, None), ("p2", parent, None)] + ([("pon", parent, True)] if parent_has_mode else []) + [("off", None, False), ("on", None, True)]
    out = dict(n_buf=n_buf, n_f=int(f.size), steps=a.steps, warmup=a.warmup)
    for name, kw in (("band_scan", dict(seed=1234)), ("dense_band", dict(seed=4321, occupied_every=1, n_distinct=8, cells_cycle=(2, 3)))):
        seed = kw.pop("seed")
        d = torch.from_numpy(pkg.synth.make_batch_u8(n_buf, seed, fcs, **kw)).cuda()
        ctx, ms, cells = {}, {k: [] for k, _, _ in lines}, {}
        for k, lib, mode in lines:
            ctx[k] = pkg.Searcher(0, lib=lib)
            if mode is not None:
                ctx[k].set_cell_meas(mode)
        run = lambda k: ctx[k].search_batch(d.data_ptr(), pkg.FMT_IQ_U8, n_buf, 153600, f, fcs, fcs, fs, pkg.STAGE_FULL)
        for _ in range(a.warmup):
            for k, _, _ in lines:
                run(k)
        for _ in range(a.steps):
            for k, _, _ in lines:
                t0 = time.perf_counter()
                cells[k] = run(k)
                ms[k].append(1e3 * (time.perf_counter() - t0))
        w = {}
        for k, _, mode in lines:
            v = np.array(ms[k])
            w[k] = dict(cell_meas=mode, ms_median=float(np.median(v)), ms_min=float(v.min()), ms_max=float(v.max()), ms_p25=float(np.percentile(v, 25)),
                        ms_p75=float(np.percentile(v, 75)), ms_all=[round(x, 3) for x in v], cells_decoded=int(sum(len(c) for c in cells[k])))
        info = ctx["on"].last_cell_meas(n_buf, 16)
        m = [info[b][i] for b in range(n_buf) for i in range(min(len(cells["on"][b]), 16))]
        sinr = np.array([t.sinr_db[0] for t in m if t.status == 0])
        w["measurements"] = dict(cells=len(m), measured=int(sum(t.status == 0 for t in m)), no_number=int(sum(t.status == -1 for t in m)),
                                 not_measured=int(sum(t.status == pkg.MEAS_NOT_MEASURED for t in m)),
                                 sinr_db_min_median_max=[float(sinr.min()), float(np.median(sinr)), float(sinr.max())] if sinr.size else None,
                                 rsrq_db_median=float(np.median([t.rsrq_db for t in m if t.status == 0])) if sinr.size else None)
        rec = {k: [[bytes(c) for c in x] for x in cells[k]] for k, _, _ in lines}
        w["records_identical"] = all(rec[k] == rec["p"] for k, _, _ in lines)
        w["parent_spread"] = abs(w["p"]["ms_median"] / w["p2"]["ms_median"] - 1.0)
        w["on_over_parent"] = w["on"]["ms_median"] / w["p"]["ms_median"]
        w["off_over_parent"] = w["off"]["ms_median"] / w["p"]["ms_median"]
        w["on_over_off"] = w["on"]["ms_median"] / w["off"]["ms_median"]
        if parent_has_mode:
            w["on_over_parent_on"] = w["on"]["ms_median"] / w["pon"]["ms_median"]
            pm = ctx["pon"].last_cell_meas(n_buf, 16)
            w["measurements_identical_to_parent"] = all(bytes(x) == bytes(y) for a_, b_ in zip(info, pm) for x, y in zip(a_, b_))
        out[name] = w
        for k in ctx:
            ctx[k].close()
        del d
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
