#!/usr/bin/env python3
"""PCFICH stage: milliseconds per cell beside the full-bandwidth measurement, on one GPU in one process.

Searcher.pcfich_wide and Searcher.cell_meas_wide on the SAME resident samples, interleaved call by call, at (R, n_rb) = (4, 25) and
(16, 100), 122 slots of a two-port and of a four-port cell: host wall time of each call -- it uploads the row list, launches
k_tfg_wide and the stage's two kernels, copies the record back and waits for the stream -- and the GPU time of the same call between
two events on the context's stream.  Medians of 20 timings after 3 warm-ups; the data is noise (no timing depends on it).  The
measurement transforms 244 rows, the PCFICH 61 (two ports) or 122 (four).  Writes one JSON document (--out) and prints it.

    python tools/pcfich_bench.py --out profiles/pcfich/pcfich_bench.json
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FS = 1.92e6
FC = 1.8425e9


def load_pkg():
    spec = importlib.util.spec_from_file_location("lte_cell_scanner_amd", os.path.join(ROOT, "lte-cell-scanner_amd", "__init__.py"),
                                                  submodule_search_locations=[os.path.join(ROOT, "lte-cell-scanner_amd")])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["lte_cell_scanner_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def timed_pair(fns, stream, n=20, warm=3):
    """the calls of fns in turn, n + warm rounds -> per call (median host ms, median GPU ms between two events on `stream`)"""
    import torch
    host, gpu = [[] for _ in fns], [[] for _ in fns]
    for i in range(warm + n):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(stream)
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            e1.record(stream)
            e1.synchronize()
            if i >= warm:
                host[k].append((t1 - t0) * 1e3)
                gpu[k].append(e0.elapsed_time(e1))
    return [(float(np.median(h)), float(np.median(g))) for h, g in zip(host, gpu)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    pkg = load_pkg()
    rng = np.random.default_rng(0)
    doc = {"n_ofdm": 854, "stage": []}
    with pkg.Searcher(0) as s:
        stream = torch.cuda.ExternalStream(s._lib.lcs_stream(s._h))      # the context's stream: the events bracket its work
        for R, n_rb in ((4, 25), (16, 100)):
            n = int(0.065 * FS * R)
            d = torch.from_numpy((0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)).cuda()
            for n_ports in (2, 4):
                cell = pkg.new_cell(n_id_1=52, n_id_2=1, cp_type=1, n_ports=n_ports, frame_start=100.5 * R, freq_fine=1234.0)
                args = (cell, d, FC, FC, FS * R, 128 * R, n_rb, 854)
                (ph, pg), (mh, mg) = timed_pair([lambda: s.pcfich_wide(*args), lambda: s.cell_meas_wide(*args)], stream)
                doc["stage"].append(dict(R=R, n_rb=n_rb, n_ports=n_ports, pcfich_rows=61 * (2 if n_ports == 4 else 1), meas_rows=244,
                                         pcfich_host_ms_per_cell=round(ph, 4), pcfich_gpu_ms_per_cell=round(pg, 4),
                                         meas_host_ms_per_cell=round(mh, 4), meas_gpu_ms_per_cell=round(mg, 4)))
            del d
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
