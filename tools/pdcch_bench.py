#!/usr/bin/env python3
"""PDCCH stage: milliseconds per cell beside the PCFICH and the full-bandwidth measurement, on one GPU in one process.

Searcher.pdcch_wide, Searcher.pcfich_wide and Searcher.cell_meas_wide on the SAME resident samples, interleaved call by call, at
(R, n_rb) = (4, 25) and (16, 100), 20 subframes (280 rows) of a two-port and of a four-port cell: host wall time of each call -- it
uploads the row list, launches k_tfg_wide and the stage's kernels, copies the record back and waits for the stream -- and the GPU
time of the same call between two events on the context's stream.  Medians of 20 timings after 3 warm-ups.  The data is noise, so
the PCFICH's decision is arbitrary: the PDCCH is timed with cfi_force = 3 (every candidate of every subframe decoded: 20 x 6 x 2
trellis decodes, the most a call can do) and once more with the PCFICH's decision.  first_call_ms is the very first call of a
context at that shape -- it builds the REG maps and the de-rate-matching lists on the host and allocates the stage's buffers --,
rekey_ms a call after the payload sizes changed (tables rebuilt, nothing allocated).  The PDCCH transforms 60 rows (three control
symbols of 20 subframes), the PCFICH 20 (two ports) or 40 (four), the measurement 80.  Writes one JSON document (--out) and prints it.

    python tools/pdcch_bench.py --out profiles/pdcch/pdcch_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pcfich_bench import FC, FS, load_pkg, timed_pair     # noqa: E402


def once(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    pkg = load_pkg()
    rng = np.random.default_rng(0)
    n_ofdm = 280
    doc = {"n_ofdm": n_ofdm, "subframes": 20, "stage": []}
    for R, n_rb in ((4, 25), (16, 100)):
        n = int(0.025 * FS * R)
        d = torch.from_numpy((0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)).cuda()
        sizes = pkg.capi.dci_common_sizes(n_rb)
        for n_ports in (2, 4):
            with pkg.Searcher(0) as s:                                   # a fresh context: the first call is a first call
                stream = torch.cuda.ExternalStream(s._lib.lcs_stream(s._h))
                cell = pkg.new_cell(n_id_1=52, n_id_2=1, cp_type=1, n_ports=n_ports, frame_start=100.5 * R, freq_fine=1234.0)
                cell.phich_duration, cell.phich_resource = 1, 3
                args = (cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm)
                force = pkg.capi.PdcchCfg.make(sizes, cfi_force=3)
                free = pkg.capi.PdcchCfg.make(sizes)
                other = pkg.capi.PdcchCfg.make((sizes[0] + 1, sizes[1]), cfi_force=3)
                s.pcfich_wide(*args)                                     # (the transform's twiddles and the grid are the PCFICH's to allocate)
                first = once(lambda: s.pdcch_wide(*args, 0x3FF, force))
                second = once(lambda: s.pdcch_wide(*args, 0x3FF, force))
                rekey = once(lambda: s.pdcch_wide(*args, 0x3FF, other))
                (fh, fg), (uh, ug), (ph, pg), (mh, mg) = timed_pair([lambda: s.pdcch_wide(*args, 0x3FF, force), lambda: s.pdcch_wide(*args, 0x3FF, free),
                                                                     lambda: s.pcfich_wide(*args), lambda: s.cell_meas_wide(*args)], stream)
                rec = s.pdcch_wide(*args, 0x3FF, force)
                doc["stage"].append(dict(R=R, n_rb=n_rb, n_ports=n_ports, n_cce=int(rec.n_cce[0]), decodes=len(list(rec.entries())),
                                         pdcch_first_call_ms=round(first, 4), pdcch_second_call_ms=round(second, 4), pdcch_rekey_ms=round(rekey, 4),
                                         pdcch_host_ms_per_cell=round(fh, 4), pdcch_gpu_ms_per_cell=round(fg, 4),
                                         pdcch_pcfich_cfi_host_ms_per_cell=round(uh, 4), pdcch_pcfich_cfi_gpu_ms_per_cell=round(ug, 4),
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
