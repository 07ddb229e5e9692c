#!/usr/bin/env python3
"""What the cancellation costs -> profiles/sic/bench.json.

A batch of `--n-buf` device-resident 8-bit captures (the S + W pair of tests/sic_cases.py, one seed per buffer) through
  plain    Searcher.search_batch (the full chain; this stage adds no kernel to it and changes none of it)
  sic      Searcher.search_batch_sic, 2 rounds (round 0 = plain, one cancellation, one search of the residuals as complex64)
  cancel   Searcher.sic_cancel alone, of the cells the plain search found
each timed as wall time around the synchronous call, `--reps` times after `--warmup` runs; the file keeps median, min and max.
--parent-lib PATH: a liblcs_amd.so built from the parent commit (capi.load_other); its plain search_batch is timed in the same process
on the same buffers as `plain_parent`.  Without it the file says that no parent figure was taken.

    python tools/sic_bench.py [--n-buf 16] [--reps 20] [--warmup 3] [--out profiles/sic/bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - a) * 1e3)
    return dict(median_ms=float(np.median(t)), min_ms=float(np.min(t)), max_ms=float(np.max(t)), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-buf", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sic", "bench.json"))
    a = ap.parse_args()
    import torch
    import sic_cases as K
    from conftest import load_pkg
    pkg = load_pkg()
    iq = np.stack([K.capture([K.S, K.W], seed=K.SEED + b, quantise=True)[1] for b in range(a.n_buf)])
    d = torch.from_numpy(iq).to("cuda:0")
    n_cap = iq.shape[1] // 2
    res = torch.empty((a.n_buf, n_cap), dtype=torch.complex64, device="cuda:0")
    out = dict(n_buf=a.n_buf, n_cap=n_cap, n_f=int(K.F_SET.size), fmt="u8", device=torch.cuda.get_device_name(0))
    with pkg.Searcher(0) as s:
        args = (d.data_ptr(), pkg.FMT_IQ_U8, a.n_buf, n_cap, K.F_SET, K.FC, K.FC, K.FS)
        found = s.search_batch(*args, pkg.STAGE_FULL)
        cells, rounds, _ = s.search_batch_sic(*args)
        out["cells_plain"] = sum(len(c) for c in found)
        out["cells_sic"] = sum(len(c) for c in cells)
        out["plain"] = timed(lambda: s.search_batch(*args, pkg.STAGE_FULL), a.reps, a.warmup)
        out["sic_2_rounds"] = timed(lambda: s.search_batch_sic(*args), a.reps, a.warmup)
        out["cancel_alone"] = timed(lambda: s.sic_cancel(d.data_ptr(), pkg.FMT_IQ_U8, a.n_buf, n_cap, found, K.FC, K.FC, K.FS, res.data_ptr()), a.reps, a.warmup)
        out["plain_again"] = timed(lambda: s.search_batch(*args, pkg.STAGE_FULL), a.reps, a.warmup)
    keys = ["plain", "sic_2_rounds", "cancel_alone", "plain_again"]
    out["parent_lib"] = bool(a.parent_lib)
    if a.parent_lib:
        with pkg.Searcher(0, lib=pkg.capi.load_other(a.parent_lib)) as sp:
            same = sp.search_batch(*args, pkg.STAGE_FULL)
            out["parent_records_equal"] = [[bytes(c) for c in cs] for cs in same] == [[bytes(c) for c in cs] for cs in found]
            out["plain_parent"] = timed(lambda: sp.search_batch(*args, pkg.STAGE_FULL), a.reps, a.warmup)
        keys.append("plain_parent")
    for k in keys:
        out[k]["per_buffer_ms"] = out[k]["median_ms"] / a.n_buf
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
