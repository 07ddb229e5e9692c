#!/usr/bin/env python3
"""What the uplink-downlink configuration estimate (lcs_set_tdd_config) costs a TDD band search, against the PARENT commit's library
on the same box, in one process.

    mkdir ../parent && git archive HEAD~ | tar -x -C ../parent && (cd ../parent && python __graft_entry__.py)      # the parent's library
    python tools/bench_tdd_config.py --parent-lib ../parent/lte-cell-scanner_amd/liblcs_amd.so

128 raw u8 buffers resident in HBM (synth.make_batch_u8(128, 1234, fcs, tdd=True, f_off_max=37.5e3) at 1.9 GHz: tools/bench_tdd.py's
TDD line, configurations 0..6 in turn), the 2.5 kHz grid with 31 hypotheses, one context per line, every context in DUPLEX_TDD:
  p    the parent's library
  p2   the parent's library on a context of its own: p against p2 is the parent's spread against itself in this run
  off  this tree, mode off
  on   this tree, lcs_set_tdd_config(1): k_tdd_config once per per-cell round
`warmup` calls per line, then `steps` timed search_batch calls per line, interleaved call by call; the medians decide.
Conditions: on / p <= 1 + spread + 1 %, off / p <= 1 + spread, with spread = |p / p2 - 1|.  Also: the records of all four lines
are byte-identical, and what the estimate says about the cells.  Writes one JSON file and prints it."""
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
    ap.add_argument("--parent-lib", required=True, help="liblcs_amd.so built from the parent commit")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tdd", "bench_tdd_config.json"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    parent = pkg.capi.load_other(a.parent_lib)
    assert not hasattr(parent, "lcs_set_tdd_config"), "--parent-lib already has the mode: not the parent commit's library"
    n_buf, fs = 128, 1.92e6
    fcs = 1.9e9 + 100e3 * np.arange(n_buf)
    f = np.arange(-15, 16) * 2.5e3
    d = torch.from_numpy(pkg.synth.make_batch_u8(n_buf, 1234, fcs, tdd=True, f_off_max=37.5e3)).cuda()
    lines = [("p", parent, None), ("p2", parent, None), ("off", None, False), ("on", None, True)]
    ctx, ms, cells = {}, {k: [] for k, _, _ in lines}, {}
    for k, lib, mode in lines:
        ctx[k] = pkg.Searcher(0, lib=lib)
        ctx[k].set_duplex(pkg.DUPLEX_TDD)
        if mode is not None:
            ctx[k].set_tdd_config(mode)
    run = lambda k: ctx[k].search_batch(d.data_ptr(), pkg.FMT_IQ_U8, n_buf, 153600, f, fcs, fcs, fs, pkg.STAGE_FULL)
    for _ in range(a.warmup):
        for k, _, _ in lines:
            run(k)
    for _ in range(a.steps):
        for k, _, _ in lines:
            t0 = time.perf_counter()
            cells[k] = run(k)
            ms[k].append(1e3 * (time.perf_counter() - t0))
    out = dict(n_buf=n_buf, n_f=int(f.size), steps=a.steps, warmup=a.warmup)
    for k, _, mode in lines:
        v = np.array(ms[k])
        out[k] = dict(tdd_config=mode, ms_median=float(np.median(v)), ms_min=float(v.min()), ms_max=float(v.max()), ms_p25=float(np.percentile(v, 25)),
                      ms_p75=float(np.percentile(v, 75)), ms_all=[round(x, 3) for x in v], cells_decoded=int(sum(len(c) for c in cells[k])))
    info = ctx["on"].last_tdd_info(n_buf, 16)
    est = [info[b][i] for b in range(n_buf) for i in range(len(cells["on"][b]))]
    out["estimates"] = dict(cells=len(est), with_configuration=int(sum(t.ul_dl_config >= 0 for t in est)), without=int(sum(t.ul_dl_config == -1 for t in est)),
                            not_estimated=int(sum(t.ul_dl_config == pkg.TDD_NOT_ESTIMATED for t in est)),
                            by_configuration=[int(sum(t.ul_dl_config == c for t in est)) for c in range(7)],
                            smallest_margin=float(min([t.margin for t in est if t.ul_dl_config >= 0] or [0.0])))
    rec = {k: [[bytes(c) for c in x] for x in cells[k]] for k, _, _ in lines}
    out["records_identical"] = bool(rec["p"] == rec["p2"] == rec["off"] == rec["on"])
    spread = abs(out["p"]["ms_median"] / out["p2"]["ms_median"] - 1.0)
    out["parent_spread"] = spread
    out["on_over_parent"] = out["on"]["ms_median"] / out["p"]["ms_median"]
    out["off_over_parent"] = out["off"]["ms_median"] / out["p"]["ms_median"]
    out["condition_on"] = bool(out["on_over_parent"] <= 1.0 + spread + 0.01)
    out["condition_off"] = bool(out["off_over_parent"] <= 1.0 + spread)
    for k in ctx:
        ctx[k].close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
