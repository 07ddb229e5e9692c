#!/usr/bin/env python3
"""PHICH stage: milliseconds per cell beside the PCFICH stage, on one GPU in one process.

Searcher.phich_wide and Searcher.pcfich_wide on the SAME resident samples, in alternating calls, at (R, n_rb) = (4, 25) and (16, 100),
20 subframes of a two-port cell at Ng = 1: host wall time of each call -- it uploads the row list, launches k_tfg_wide and the stage's
two kernels, copies the record back and waits for the stream -- and the GPU time of the same call between two events on the context's
stream.  At the normal PHICH duration both transform symbol 0 of the 20 subframes; the extended duration (three rows per subframe)
and a four-port cell (two) are timed in alternations of their own, with no bar: the stage keeps the unit tables of one key (n_rb, ports,
CP, id, duration, Ng), so every alternation holds the key still and times the steady state.  What a change of key costs -- the tables
rebuilt on the host and uploaded -- is timed apart, with the two durations in turn.  30 alternations after 3 warm-ups; per call the
median and the spread (5th and 95th percentile), and the ratio of the medians; the data is noise (no timing depends on it).  Writes
one JSON document (--out) and prints it.  The kernels' own durations come from the same tool under a kernel trace, in a run of its own,
and --summarise-trace turns the trace's database into medians per kernel and bandwidth (profiles/phich/kernel_trace.json):
    rocprofv3 --kernel-trace -d DIR -o phich -- python tools/phich_bench.py
    python tools/phich_bench.py --summarise-trace DIR/phich_results.db --out profiles/phich/kernel_trace.json

    python tools/phich_bench.py --out profiles/phich/bench.json
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
N_SF = 20


def load_pkg():
    spec = importlib.util.spec_from_file_location("lte_cell_scanner_amd", os.path.join(ROOT, "lte-cell-scanner_amd", "__init__.py"),
                                                  submodule_search_locations=[os.path.join(ROOT, "lte-cell-scanner_amd")])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["lte_cell_scanner_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def alternate(fns, stream, n=30, warm=3):
    """the calls of fns in turn, n + warm rounds -> per call dict(host / gpu: median, p05, p95 in ms)"""
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
    st = lambda v: dict(median=round(float(np.median(v)), 4), p05=round(float(np.percentile(v, 5)), 4), p95=round(float(np.percentile(v, 95)), 4))
    return [dict(host_ms=st(h), gpu_ms=st(g)) for h, g in zip(host, gpu)]


def summarise_trace(db):
    """medians in microseconds of the stages' kernels in a rocprofv3 kernel trace of this tool: the dispatches of a kernel in time order,
    the first half at 25 resource blocks and the second at 100 (the tool runs the two bandwidths one after the other with the same calls)"""
    import sqlite3
    con = sqlite3.connect(db)
    out = {"command": "rocprofv3 --kernel-trace -d DIR -o phich -- python tools/phich_bench.py; python tools/phich_bench.py --summarise-trace DIR/phich_results.db",
           "note": "medians of the kernels' durations under the profiler, which inflates short kernels; microseconds at 25 / 100 resource blocks", "kernels": {}}
    for name in ("k_phich(", "k_phich_fin(", "k_pcfich(", "k_pcfich_fin(", "k_tfg_wide<"):
        r = [x[0] for x in con.execute("select end - start from kernels where name like ? order by start", ("%" + name + "%",))]
        h = len(r) // 2
        if h:
            out["kernels"][name.rstrip("(<")] = dict(dispatches=len(r), us_25_rb=round(float(np.median(r[:h])) / 1e3, 2), us_100_rb=round(float(np.median(r[h:])) / 1e3, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--summarise-trace", default=None, metavar="DB", help="no GPU: medians per kernel from a rocprofv3 kernel trace of this tool")
    a = ap.parse_args()
    if a.summarise_trace:
        text = json.dumps(summarise_trace(a.summarise_trace), indent=1)
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return
    import torch
    pkg = load_pkg()
    capi = pkg.capi
    rng = np.random.default_rng(0)
    doc = {"n_subframes": N_SF, "alternations": 30, "stage": []}
    with pkg.Searcher(0) as s:
        stream = torch.cuda.ExternalStream(s._lib.lcs_stream(s._h))      # the context's stream: the events bracket its work
        for R, n_rb in ((4, 25), (16, 100)):
            n = int(0.025 * FS * R)
            d = torch.from_numpy((0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)).cuda()
            cells = {}
            for n_ports in (2, 4):
                cells[n_ports] = pkg.new_cell(n_id_1=52, n_id_2=1, cp_type=1, n_ports=n_ports, frame_start=100.5 * R, freq_fine=1234.0)
                cells[n_ports].phich_duration, cells[n_ports].phich_resource = 1, 3
            args = lambda p: (cells[p], d, FC, FC, FS * R, 128 * R, n_rb, N_SF * 14)
            ext = capi.PhichCfg.make(phich_duration=2)
            # one alternation per PHICH key (ports, duration): the stage keeps the tables of ONE key, so a pair never makes it rebuild them
            pairs = {"normal_2_ports": (lambda: s.phich_wide(*args(2)), lambda: s.pcfich_wide(*args(2)), N_SF),
                     "extended_duration_2_ports": (lambda: s.phich_wide(*args(2), cfg=ext), lambda: s.pcfich_wide(*args(2)), 3 * N_SF),
                     "normal_4_ports": (lambda: s.phich_wide(*args(4)), lambda: s.pcfich_wide(*args(4)), 2 * N_SF)}
            row = dict(R=R, n_rb=n_rb, units_per_subframe=capi.phich_n_group(n_rb, 3, True))
            for name, (f_phich, f_pcfich, rows) in pairs.items():
                ph, pc = alternate([f_phich, f_pcfich], stream)
                e = dict(phich_rows_transformed=rows, pcfich_rows_transformed=N_SF * (2 if "4_ports" in name else 1), phich_wide=ph, pcfich_wide=pc)
                for kind in ("host_ms", "gpu_ms"):
                    e["ratio_phich_over_pcfich_" + kind] = round(ph[kind]["median"] / pc[kind]["median"], 4)
                    e["pcfich_spread_" + kind] = round(pc[kind]["p95"] - pc[kind]["p05"], 4)
                    e["phich_minus_pcfich_" + kind] = round(ph[kind]["median"] - pc[kind]["median"], 4)
                row[name] = e
            # what a change of key costs: the two durations in turn, so that every call rebuilds the three unit tables on the host and
            # uploads them (the case of a sweep, which calls the stage once per cell)
            a_, b_ = alternate([lambda: s.phich_wide(*args(2)), lambda: s.phich_wide(*args(2), cfg=ext)], stream)
            row["key_change_every_call"] = dict(phich_wide_normal=a_, phich_wide_extended=b_,
                                                rebuild_host_ms=round(a_["host_ms"]["median"] - row["normal_2_ports"]["phich_wide"]["host_ms"]["median"], 4))
            doc["stage"].append(row)
            del d
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
