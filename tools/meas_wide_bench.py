#!/usr/bin/env python3
"""Full-bandwidth cell measurement: milliseconds per cell, on one GPU in one process.

(a) Searcher.cell_meas_wide with the samples resident in HBM, at (R, n_rb) = (16, 100) and (4, 25), two frames and 122 slots of
    rows: host wall time of the call -- it uploads the row list, launches k_tfg_wide, k_cell_meas_wide and k_cell_meas_wide_fin,
    copies the record back and waits for the stream -- and the GPU time of the same call between two events on the context's stream.
(b) sweep.measure_wideband for one 25 RB cell and one 100 RB cell of a 30.72 Msps complex64 capture of 80 ms: the channelizer at
    decim 4 (25 RB; 100 RB is measured in place) plus (a).
Medians of 20 timings after 3 warm-ups; the data is noise (no timing depends on it).  Writes one JSON document (--out) and prints it.

    python tools/meas_wide_bench.py --out profiles/meas_wide/meas_wide_bench.json
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


def timed(fn, stream, n=20, warm=3):
    """-> (median host ms, median GPU ms between two events on `stream`)"""
    import torch
    host, gpu = [], []
    for i in range(warm + n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        e1.record(stream)
        e1.synchronize()
        if i >= warm:
            host.append((t1 - t0) * 1e3)
            gpu.append(e0.elapsed_time(e1))
    return float(np.median(host)), float(np.median(gpu))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    pkg = load_pkg()
    rng = np.random.default_rng(0)
    doc = {"stage": [], "measure_wideband": []}
    with pkg.Searcher(0) as s:
        stream = torch.cuda.ExternalStream(s._lib.lcs_stream(s._h))      # the context's stream: the events bracket its work
        for R, n_rb in ((16, 100), (4, 25)):
            n = int(0.065 * FS * R)
            d = torch.from_numpy((0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)).cuda()
            cell = pkg.new_cell(n_id_1=52, n_id_2=1, cp_type=1, n_ports=2, frame_start=100.5 * R, freq_fine=1234.0)
            for n_ofdm in (280, 854):
                host, gpu = timed(lambda: s.cell_meas_wide(cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm), stream)
                doc["stage"].append(dict(R=R, n_rb=n_rb, n_ofdm=n_ofdm, rows=2 * (n_ofdm // 7), sample_bytes_read=2 * (n_ofdm // 7) * 128 * R * 8,
                                         host_ms_per_cell=round(host, 4), gpu_ms_per_cell=round(gpu, 4)))
            del d
        K = 16
        n_in = 153600 * K
        d = torch.from_numpy((0.1 * (rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in))).astype(np.complex64)).cuda()
        for n_rb in (25, 100):
            cell = pkg.new_cell(n_id_1=52, n_id_2=1, cp_type=1, n_ports=2, n_rb_dl=n_rb, frame_start=4321.25, freq_fine=1234.0)
            host, gpu = timed(lambda: pkg.sweep.measure_wideband(s, d.data_ptr(), pkg.FMT_C64, n_in, FS * K, FC, K, [[cell]], [FC]), stream)
            doc["measure_wideband"].append(dict(K=K, n_rb=n_rb, decim_meas=K // pkg.sweep.meas_rate(n_rb), n_in=n_in, host_ms_per_cell=round(host, 4),
                                                gpu_ms_per_cell=round(gpu, 4)))
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
