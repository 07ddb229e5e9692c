#!/usr/bin/env python3
"""PDSCH stage: milliseconds per cell beside the PDCCH, the PCFICH and the full-bandwidth measurement, on one GPU in one process.

Searcher.pdsch_wide, Searcher.pdcch_wide, Searcher.pcfich_wide and Searcher.cell_meas_wide on the SAME resident samples, interleaved
call by call, at (R, n_rb) = (4, 25) and (16, 100), 20 subframes (280 rows) of a two-port and of a four-port cell: host wall time of
each call -- it uploads the row list, launches k_tfg_wide and the stage's kernels, copies the record back and waits for the stream
-- and the GPU time of the same call between two events on the context's stream.  Medians of 20 timings after 3 warm-ups.  The
samples are a generated cell (synth.make_wideband_cell, noise 20 dB below a resource element) with one format 1A grant in every
subframe: the largest transport block (mcs 26 of the N_PRB = 3 column: 2216 bits, K = 2240, seventy windows) on every resource
block of a 25-RB cell and on the first 25 of a 100-RB one, so every followed grant is the decoder's largest job; it decodes in the
iterations the record says.  worst_case: the same call with the blocks' CRC never zero is not reachable from samples, so the
decoder's cost per iteration is read from lcs_turbo_decode at K = 2240 on noise (8 iterations, one workgroup).  first_call_ms is the
very first call of a context at that shape -- it builds the PDCCH's maps, the rank tables and allocates the stage's buffers.  The
PDSCH transforms all 280 rows, the PDCCH 60, the PCFICH 20 (two ports) or 40 (four), the measurement 80.
Writes one JSON document (--out) and prints it.

    python tools/pdsch_bench.py --out profiles/pdsch/pdsch_bench.json

--alloc localized | distributed | 1c: the same workload on 24 resource blocks (N_VRB of 25) with every grant localized, a distributed
format 1A grant (Searcher.set_pdsch_alloc on), or a format 1C grant (its largest transport block: 1736 bits, K = 1760): what the
set-based enumeration of k_pdsch_llr costs against the closed form of the same build.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pcfich_bench import FC, FS, load_pkg, timed_pair     # noqa: E402
from pdcch_bench import once                              # noqa: E402


def pack_1a(n_rb, start, length, mcs, rv, tpc, size):
    riv = n_rb * (length - 1) + start if length - 1 <= n_rb // 2 else n_rb * (n_rb - length + 1) + (n_rb - 1 - start)
    out = []
    for v, n in ((1, 1), (0, 1), (riv, (n_rb * (n_rb + 1) // 2 - 1).bit_length()), (mcs, 5), (0, 3), (0, 1), (rv, 2), (tpc, 2)):
        out += [(v >> (n - 1 - i)) & 1 for i in range(n)]
    return out + [0] * (size - len(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="A/B runs: load this build of liblcs_amd.so instead of the in-tree one")
    ap.add_argument("--quick", action="store_true", help="the (4, 25) shapes only")
    ap.add_argument("--alloc", default=None, choices=["localized", "distributed", "1c"], help="24 resource blocks per grant, allocated this way (25 RB shapes only)")
    a = ap.parse_args()
    import torch
    pkg = load_pkg()
    if a.lib:
        pkg.capi.LIB_PATH = os.path.abspath(a.lib)
    n_ofdm = 280
    doc = {"n_ofdm": n_ofdm, "subframes": 20, "alloc": a.alloc, "stage": []}
    for R, n_rb in (((4, 25),) if a.quick or a.alloc else ((4, 25), (16, 100))):
        sizes = pkg.capi.dci_common_sizes(n_rb)
        for n_ports in (2, 4):
            tbs = pkg.capi.tbs_1a(26, 1)
            bits = lambda fr, sf: np.random.default_rng(100 * fr + sf).integers(0, 2, tbs).astype(np.uint8)
            cellcfg = dict(n_id_1=52, n_id_2=1, cp_normal=True, n_ports=n_ports, f_off=0.0, t0=100.0, sfn0=8, n_rb_dl=n_rb, cfi=2,
                           pdcch=lambda fr, sf: [dict(rnti=0xFFFF, bits=pack_1a(n_rb, 0, 25, 26, sf % 4, 1, sizes[0]), L=4, cce=0)],
                           pdsch=lambda fr, sf: [dict(rnti=0xFFFF, rb_start=0, n_prb=25, rv=sf % 4, bits=bits(fr, sf))])
            if a.alloc == "1c":
                tbs = pkg.capi.tbs_1c(31)
                g1c = dict(rnti=0xFFFF, rb_start=0, n_prb=24, i_tbs=31, format="1c", rv=0)
                cellcfg.update(pdcch=lambda fr, sf: [dict(rnti=0xFFFF, bits=pkg.synth.dci_1c_payload(g1c, n_rb), L=4, cce=0)],
                               pdsch=lambda fr, sf: [dict(g1c, bits=bits(fr, sf))])
            elif a.alloc:
                g1a = lambda sf: dict(rnti=0xFFFF, rb_start=0, n_prb=24, mcs=26, tpc=1, rv=sf % 4, distributed=int(a.alloc == "distributed"))
                cellcfg.update(pdcch=lambda fr, sf: [dict(rnti=0xFFFF, bits=pkg.synth.dci_1a_payload(g1a(sf), n_rb), L=4, cce=0)],
                               pdsch=lambda fr, sf: [dict(g1a(sf), bits=bits(fr, sf))])
            x, _, _ = pkg.synth.make_wideband_cell(7, FC, R, [(FC, R, n_rb, cellcfg)], snr_db=20.0, n_in=int(3.05 * 19200 * R))
            d = torch.from_numpy(x).cuda()
            with pkg.Searcher(0) as s:                                   # a fresh context: the first call is a first call
                stream = torch.cuda.ExternalStream(s._lib.lcs_stream(s._h))
                cell = pkg.new_cell(n_id_1=52, n_id_2=1, cp_type=1, n_ports=n_ports, frame_start=(19200.0 - 100.0) * R, freq_fine=0.0)
                cell.n_rb_dl, cell.phich_duration, cell.phich_resource = n_rb, 1, 3
                args = (cell, d, FC, FC, FS * R, 128 * R, n_rb, n_ofdm)
                cfg = pkg.capi.PdcchCfg.make(sizes)
                if a.alloc in ("distributed", "1c"):
                    s.set_pdsch_alloc(pkg.capi.PdschAllocCfg.make(distributed=True, format_1c=True))
                s.pcfich_wide(*args)                                     # (the transform's twiddles and the grid are the PCFICH's to allocate)
                first = once(lambda: s.pdsch_wide(*args, 0x3FF, cfg))
                second = once(lambda: s.pdsch_wide(*args, 0x3FF, cfg))
                (sh, sg), (dh, dg), (ph, pg), (mh, mg) = timed_pair([lambda: s.pdsch_wide(*args, 0x3FF, cfg), lambda: s.pdcch_wide(*args, 0x3FF, cfg),
                                                                     lambda: s.pcfich_wide(*args), lambda: s.cell_meas_wide(*args)], stream)
                rec = s.pdsch_wide(*args, 0x3FF, cfg)
                noise = np.random.default_rng(3).standard_normal((3, 2244))
                (th, tg), = timed_pair([lambda: s.turbo_decode(noise, 2240)], stream)
                doc["stage"].append(dict(R=R, n_rb=n_rb, n_ports=n_ports, blocks=int(rec.n_blocks), ok=int(rec.n_ok), iterations=sorted({b["n_iter"] for b in rec.blocks()}),
                                         K=sorted({b["K"] for b in rec.blocks()}), n_re=sorted({b["n_re"] for b in rec.blocks()}),
                                         pdsch_first_call_ms=round(first, 4), pdsch_second_call_ms=round(second, 4),
                                         pdsch_host_ms_per_cell=round(sh, 4), pdsch_gpu_ms_per_cell=round(sg, 4),
                                         pdcch_host_ms_per_cell=round(dh, 4), pdcch_gpu_ms_per_cell=round(dg, 4),
                                         pcfich_host_ms_per_cell=round(ph, 4), pcfich_gpu_ms_per_cell=round(pg, 4),
                                         meas_host_ms_per_cell=round(mh, 4), meas_gpu_ms_per_cell=round(mg, 4),
                                         turbo_2240_8_iterations_host_ms=round(th, 4), turbo_2240_8_iterations_gpu_ms=round(tg, 4)))
            del d
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
