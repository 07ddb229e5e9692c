#!/usr/bin/env python3
"""Wideband channelizer against the stage it feeds, on one GPU in one process.

(a) lcs_last_channelize_ms of one call: decim 16, s16 capture of 80 ms at 30.72 Msps, 256 carriers on the 100 kHz raster,
    n_out = 153584.
(b) GPU time of search_batch on those 256 LCS_FMT_C64 buffers at n_f = 31, full chain, as two batches of 128 (the batch
    size bench.py and sweep.search_wideband use): HIP events on the context's stream around enqueue .. collect.
Both are medians of 20 timings after 3 warm-ups.  The wideband pipeline keeps 1 / (1 + a / b) of the float path's buffer
rate; the target is a <= 0.25 b.  Writes one JSON document (--out) and prints it.

--rate up/down measures lcs_channelize_rational instead: (a) one call on an s16 capture of 80 ms at 1.92 Msps * down / up
(12/125: 20 Msps) with the carriers of the 100 kHz raster within 0.45 fs_in of the centre (12/125: 181, +-9 MHz), (b) search_batch
on those buffers as batches of at most 128.  Its record goes under the key "rational" of the same document; the integer
record at the top level stays as it is (and a plain run keeps the "rational" record).

--u8 compares the two pipelines of a band search on the integer record's carriers (256 carriers, decim 16, s16, n_f = 31), both
in this one process on one box, medians as above: (a) lcs_channelize_u8, then search_batch on the bytes (LCS_FMT_IQ_U8: the int8
correlation kernel); (b) lcs_channelize, then search_batch on the floats.  Each pipeline is timed by HIP events from in front of
the channelizer to behind the second batch's collect.  Its record -- both times, their ratio, the channelizer's share of (a)
against the search behind it, the new kernels' resources -- goes under the key "u8"; everything else in the document stays.

--stream compares the continuous form (lcs_chan_stream_push) with the one-shot call on the same samples, in this one process, HIP
events on the context's stream around each, medians as above: (a) the one-shot call (lcs_channelize on the integer record's
workload; with --rate 12/125 lcs_channelize_rational on the rational record's); (b) the same capture as 8 equal pushes of a stream
opened before the clock starts; (c) as 64 pushes; (z) one push that hands out nothing (one sample into a fresh stream: the history
append alone).  The condition is relative: b <= 1.10 a + 7 z -- seven more launches than one call, and 10 % (twice the +-4 % box
spread of README, and the recomputed columns).  (c) has no bar.  The record goes under "stream" / "<up>/<down>"; the rest stays.

--stream --u8 compares the two pipelines of a LIVE band search, one capture of n_cap = 153600 outputs per carrier arriving as 8 equal
pushes (the integer record's carriers at 30.72 Msps; with --rate 12/125 the rational record's 181), both in this one process, streams
opened before the clock starts, HIP events on the context's stream, medians as above: (a) the float stream's pushes
(lcs_chan_stream_push), then search_batch on the floats; (b) lcs_chan_stream_push_u8, then search_batch on the bytes (the int8
correlation kernel); (p) the pushes of (b) alone and (s) the search of (b) alone, from an event between the two.  The conditions are
relative: p <= 0.25 s (the channelizer stage's standing condition) and b <= 0.90 a.  The record goes under "stream_u8" / "<up>/<down>".

    python tools/chan_bench.py --out profiles/channelizer/chan_bench.json
    python tools/chan_bench.py --rate 12/125 --out profiles/channelizer/chan_bench.json
    python tools/chan_bench.py --u8 --out profiles/channelizer/chan_bench.json
    python tools/chan_bench.py --stream --out profiles/channelizer/chan_bench.json
    python tools/chan_bench.py --stream --rate 12/125 --out profiles/channelizer/chan_bench.json
    python tools/chan_bench.py --stream --u8 --out profiles/channelizer/chan_bench.json
    python tools/chan_bench.py --stream --u8 --rate 12/125 --out profiles/channelizer/chan_bench.json
"""
import argparse
import importlib.util
import json
import os
import subprocess
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


STREAM_N_CAP = 153600      # --stream --u8: outputs per capture


def sclk_sampler(device, samples, stop):
    while not stop.is_set():
        try:
            p = subprocess.run(["rocm-smi", "-d", str(device), "--showclocks", "--json"], capture_output=True, text=True, timeout=5)
            card = next(iter(json.loads(p.stdout).values()))
            v = next((v for k, v in card.items() if "sclk" in k.lower() and "mhz" in str(v).lower()), None)
            if v is not None:
                samples.append(float("".join(ch for ch in str(v) if ch.isdigit() or ch == ".")))
        except Exception:
            return
        stop.wait(0.2)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "channelizer", "chan_bench.json"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cells", type=int, default=8, help="cells planted across the band (every 32nd carrier)")
    ap.add_argument("--rate", default=None, metavar="UP/DOWN", help="measure lcs_channelize_rational at this rate change, e.g. 12/125")
    ap.add_argument("--u8", action="store_true", help="time lcs_channelize_u8 + search on bytes against lcs_channelize + search on floats")
    ap.add_argument("--stream", action="store_true", help="time the continuous form (8 and 64 pushes) against the one-shot call on the same samples")
    args = ap.parse_args()
    if args.u8 and args.rate and not args.stream:
        ap.error("--u8 runs on the integer record's carriers: it takes no --rate")
    rate = tuple(int(v) for v in args.rate.split("/")) if args.rate else None
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    D, N_CH, N_OUT, FC0 = 16, 256, 153584, 740.0e6
    fs_in, n_in = D * 1.92e6, 153600 * D
    if rate:
        up, down = rate
        fs_in, n_in = 1.92e6 * down / up, -(-153600 // up) * down
        N_CH = 2 * int(0.45 * fs_in / 100e3) + 1
    if args.u8 and args.stream:      # one capture of STREAM_N_CAP outputs and not a sample more
        u, d = rate or (1, D)
        n_in = -(-((STREAM_N_CAP - 1) * d + 16 * d) // u)
    carriers = FC0 + 100e3 * (np.arange(N_CH) - N_CH // 2)
    args.cells = min(args.cells, (N_CH - 17) // 32 + 1)
    rng = np.random.default_rng(5)
    placed = [(float(carriers[16 + 32 * i]), [dict(n_id_1=int(rng.integers(0, 168)), n_id_2=int(rng.integers(0, 3)), cp_normal=bool(i % 4 != 3),
                                                   n_ports=int((1, 2, 2, 4)[i % 4]), n_rb_dl=int((6, 15, 25, 50, 75, 100)[i % 6]),
                                                   f_off=float(rng.uniform(-60e3, 60e3)), gain_db=float(rng.uniform(0, 6)))]) for i in range(args.cells)]
    if rate:
        iq, _ = pkg.synth.make_wideband_rate(77, FC0, up, down, placed, 10.0, pkg.FMT_IQ_S16, n_in=n_in)
    else:
        iq, _ = pkg.synth.make_wideband(77, FC0, D, placed, 10.0, pkg.FMT_IQ_S16, n_in=n_in)
    dev = torch.device("cuda", args.device)
    d_wide = torch.from_numpy(iq).to(dev)
    d_out = torch.empty((N_CH, N_OUT), dtype=torch.complex64, device=dev)
    f = pkg.f_search_set_for(739e6, 100)
    torch.cuda.synchronize(dev)
    samples, stop = [], threading.Event()
    th = threading.Thread(target=sclk_sampler, args=(args.device, samples, stop), daemon=True)
    if args.u8 and args.stream:
        return bench_stream_u8(args, pkg, torch, dev, d_wide, carriers - FC0, carriers, f, n_in, fs_in, rate or (1, D), samples, stop, th)
    if args.u8:
        return bench_u8(args, pkg, torch, dev, d_wide, d_out, carriers - FC0, carriers, f, n_in, fs_in, D, N_CH, N_OUT, samples, stop, th)
    if args.stream:
        return bench_stream(args, pkg, torch, dev, d_wide, carriers - FC0, n_in, fs_in, rate or (1, D), samples, stop, th)
    with pkg.Searcher(args.device) as s:
        stream = torch.cuda.ExternalStream(pkg.capi.load().lcs_stream(s._h), device=dev)
        th.start()
        a_ms = []
        for i in range(args.warmup + args.reps):
            if rate:
                s.channelize_rational(d_wide.data_ptr(), pkg.FMT_IQ_S16, n_in, fs_in, up, down, carriers - FC0, d_out.data_ptr(), N_OUT)
            else:
                s.channelize(d_wide.data_ptr(), pkg.FMT_IQ_S16, n_in, fs_in, D, carriers - FC0, d_out.data_ptr(), N_OUT)
            a_ms.append(s.last_channelize_ms())
        s.sync()
        b_ms, n_cells = [], 0
        for i in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            n_cells = 0
            for h in range(-(-N_CH // 128)):
                sl = slice(128 * h, min(128 * h + 128, N_CH))
                cells = s.search_batch(d_out[128 * h].data_ptr(), pkg.FMT_C64, sl.stop - sl.start, N_OUT, f, carriers[sl], carriers[sl], 1.92e6, pkg.STAGE_FULL)
                n_cells += sum(len(c) for c in cells)
            e1.record(stream)
            e1.synchronize()
            b_ms.append(e0.elapsed_time(e1))
        stop.set()
        th.join(timeout=10)
    a, b = float(np.median(a_ms[args.warmup:])), float(np.median(b_ms[args.warmup:]))
    spec = importlib.util.spec_from_file_location("code_objects", os.path.join(ROOT, "tools", "code_objects.py"))
    co = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(co)
    mine = ("k_channelize_rate", "k_chan_rate_tables") if rate else ("k_channelizeI", "k_chan_tables")
    ks = {k: v for k, v in co.kernels_of(os.path.join(ROOT, "lte-cell-scanner_amd", "liblcs_amd.so")).items() if any(m in k for m in mine)}
    batches = " + ".join(str(min(128, N_CH - 128 * h)) for h in range(-(-N_CH // 128))) if rate else "2 x 128"
    taps_per_output = 16.0 * down / up if rate else 16.0 * D
    res = {"a_channelize_ms": a, ("b_search_%d_ms" % N_CH): b, "ratio_a_over_b": a / b, "target_ratio": 0.25, "meets_target": bool(a <= 0.25 * b),
           "buffer_rate_kept": 1.0 / (1.0 + a / b),
           "config": {**({"up": up, "down": down, "fs_in": fs_in} if rate else {"decim": D}), "fmt": "s16", "n_ch": N_CH, "n_in": n_in, "n_out": N_OUT,
                      "raster_hz": 100e3, "n_f": int(f.size), "batches": batches,
                      "stage": "full", "reps": args.reps, "warmup": args.warmup, "cells_planted": args.cells, ("cells_decoded_per_%d" % N_CH): n_cells},
           "a_ms_min_max": [float(min(a_ms[args.warmup:])), float(max(a_ms[args.warmup:]))],
           "b_ms_min_max": [float(min(b_ms[args.warmup:])), float(max(b_ms[args.warmup:]))],
           "channelizer_tflops_fp32": 8.0 * N_CH * taps_per_output * N_OUT / (a * 1e-3) / 1e12,
           "sclk_mhz_median": (sorted(samples)[len(samples) // 2] if samples else None), "sclk_samples": len(samples),
           "device": torch.cuda.get_device_name(dev), "kernels": ks}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    try:
        with open(args.out) as fh:
            old = json.load(fh)
    except (OSError, ValueError):
        old = {}
    if rate:
        doc = dict(old, rational=res)
    else:
        doc = dict(res, **({"rational": old["rational"]} if "rational" in old else {}))
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


def bench_stream(args, pkg, torch, dev, d_wide, shifts, n_in, fs_in, rate, samples, stop, th):
    up, down = rate
    n_ch = len(shifts)
    n_out = (n_in * up - 16 * down) // down + 1          # M(n_in): all the capture gives
    d_out = torch.empty((n_ch, n_out), dtype=torch.complex64, device=dev)
    torch.cuda.synchronize(dev)
    t = {"a": [], "b": [], "c": [], "z": []}
    emitted = {}
    with pkg.Searcher(args.device) as s:
        stream = torch.cuda.ExternalStream(pkg.capi.load().lcs_stream(s._h), device=dev)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        def pushes(n_push):
            edges = [n_in * k // n_push for k in range(n_push + 1)]
            filled = 0
            for a, b in zip(edges[:-1], edges[1:]):
                n_emit, _ = s.chan_stream_push(d_wide.data_ptr() + 4 * a, b - a, d_out.data_ptr() + 8 * filled, n_out, n_out - filled)
                filled += n_emit
            emitted[n_push] = filled

        th.start()
        for i in range(args.warmup + args.reps):      # interleaved: every form sees the same clocks
            t["a"].append(timed(lambda: s.channelize_rational(d_wide.data_ptr(), pkg.FMT_IQ_S16, n_in, fs_in, up, down, shifts, d_out.data_ptr(), n_out)))
            for key, n_push in (("b", 8), ("c", 64)):
                s.chan_stream_open(pkg.FMT_IQ_S16, fs_in, up, down, shifts)
                t[key].append(timed(lambda: pushes(n_push)))
                s.chan_stream_close()
            s.chan_stream_open(pkg.FMT_IQ_S16, fs_in, up, down, shifts)
            t["z"].append(timed(lambda: s.chan_stream_push(d_wide.data_ptr(), 1, d_out.data_ptr(), n_out, n_out)))
            s.chan_stream_close()
        stop.set()
        th.join(timeout=10)
    assert emitted == {8: n_out, 64: n_out}, emitted
    med = lambda v: float(np.median(v[args.warmup:]))
    a, b, c, z = med(t["a"]), med(t["b"]), med(t["c"]), med(t["z"])
    spec = importlib.util.spec_from_file_location("code_objects", os.path.join(ROOT, "tools", "code_objects.py"))
    co = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(co)
    ks = {k: v for k, v in co.kernels_of(os.path.join(ROOT, "lte-cell-scanner_amd", "liblcs_amd.so")).items()
          if "k_chan_keep" in k or ("k_channelize" in k and "Lb0ELb1E" in k)}
    res = {"a_one_shot_ms": a, "b_8_pushes_ms": b, "c_64_pushes_ms": c, "z_push_without_output_ms": z, "bound_ms": 1.10 * a + 7.0 * z,
           "meets_condition": bool(b <= 1.10 * a + 7.0 * z), "ratio_b_over_a": b / a, "ratio_c_over_a": c / a,
           "config": {"up": up, "down": down, "fs_in": fs_in, "fmt": "s16", "n_ch": n_ch, "n_in": n_in, "n_out": n_out, "reps": args.reps, "warmup": args.warmup},
           "ms_min_max": {k: [float(min(v[args.warmup:])), float(max(v[args.warmup:]))] for k, v in t.items()},
           "sclk_mhz_median": (sorted(samples)[len(samples) // 2] if samples else None), "sclk_samples": len(samples),
           "device": torch.cuda.get_device_name(dev), "kernels": ks}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    try:
        with open(args.out) as fh:
            old = json.load(fh)
    except (OSError, ValueError):
        old = {}
    with open(args.out, "w") as fh:
        json.dump(dict(old, stream=dict(old.get("stream", {}), **{"%d/%d" % (up, down): res})), fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


def bench_stream_u8(args, pkg, torch, dev, d_wide, shifts, carriers, f, n_in, fs_in, rate, samples, stop, th):
    up, down = rate
    n_ch, n_cap, n_push = len(shifts), STREAM_N_CAP, 8
    assert (n_in * up - 16 * down) // down + 1 == n_cap
    d_c64 = torch.empty((n_ch, n_cap), dtype=torch.complex64, device=dev)
    d_u8 = torch.empty((n_ch, n_cap, 2), dtype=torch.uint8, device=dev)
    d_gain = torch.empty(n_ch, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    edges = [n_in * k // n_push for k in range(n_push + 1)]
    t = {"a": [], "b": [], "p": [], "s": []}
    cells, kernel = {}, {}
    with pkg.Searcher(args.device) as s:
        stream = torch.cuda.ExternalStream(pkg.capi.load().lcs_stream(s._h), device=dev)

        def search(buf, fmt):
            n = 0
            for h in range(-(-n_ch // 128)):
                sl = slice(128 * h, min(128 * h + 128, n_ch))
                n += sum(len(c) for c in s.search_batch(buf[128 * h].data_ptr(), fmt, sl.stop - sl.start, n_cap, f, carriers[sl], carriers[sl], 1.92e6, pkg.STAGE_FULL))
            return n

        def events(k):
            return [torch.cuda.Event(enable_timing=True) for _ in range(k)]

        th.start()
        for i in range(args.warmup + args.reps):      # interleaved: both pipelines see the same clocks
            s.chan_stream_open(pkg.FMT_IQ_S16, fs_in, up, down, shifts)
            e = events(2)
            e[0].record(stream)
            filled = 0
            for a, b in zip(edges[:-1], edges[1:]):
                n_emit, _ = s.chan_stream_push(d_wide.data_ptr() + 4 * a, b - a, d_c64.data_ptr() + 8 * filled, n_cap, n_cap - filled)
                filled += n_emit
            cells["c64"] = search(d_c64, pkg.FMT_C64)
            e[1].record(stream)
            e[1].synchronize()
            t["a"].append(e[0].elapsed_time(e[1]))
            kernel["c64"] = s.last_xcorr_info()[0]
            s.chan_stream_close()
            assert filled == n_cap
            s.chan_stream_open_u8(pkg.FMT_IQ_S16, fs_in, up, down, shifts, n_cap)
            e = events(3)
            e[0].record(stream)
            done = 0
            for a, b in zip(edges[:-1], edges[1:]):
                done += s.chan_stream_push_u8(d_wide.data_ptr() + 4 * a, b - a, d_u8.data_ptr(), d_gain.data_ptr(), 1)[0]
            e[1].record(stream)
            cells["u8"] = search(d_u8, pkg.FMT_IQ_U8)
            e[2].record(stream)
            e[2].synchronize()
            t["b"].append(e[0].elapsed_time(e[2]))
            t["p"].append(e[0].elapsed_time(e[1]))
            t["s"].append(e[1].elapsed_time(e[2]))
            kernel["u8"] = s.last_xcorr_info()[0]
            s.chan_stream_close()
            assert done == 1
        stop.set()
        th.join(timeout=10)
    med = lambda v: float(np.median(v[args.warmup:]))
    a, b, p, sr = med(t["a"]), med(t["b"]), med(t["p"]), med(t["s"])
    spec = importlib.util.spec_from_file_location("code_objects", os.path.join(ROOT, "tools", "code_objects.py"))
    co = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(co)
    ks = {k: v for k, v in co.kernels_of(os.path.join(ROOT, "lte-cell-scanner_amd", "liblcs_amd.so")).items()
          if "k_chan_cap_power" in k or "k_chan_quant_u8" in k or "k_chan_keep" in k}
    res = {"a_float_stream_and_search_ms": a, "b_u8_stream_and_search_ms": b, "p_u8_pushes_ms": p, "s_u8_search_ms": sr,
           "ratio_p_over_s": p / sr, "target_p_over_s": 0.25, "meets_p_target": bool(p <= 0.25 * sr),
           "ratio_b_over_a": b / a, "target_b_over_a": 0.90, "meets_b_target": bool(b <= 0.90 * a),
           "config": {"up": up, "down": down, "fs_in": fs_in, "fmt": "s16", "n_ch": n_ch, "n_in": n_in, "n_cap": n_cap, "pushes": n_push, "n_f": int(f.size),
                      "batches": " + ".join(str(min(128, n_ch - 128 * h)) for h in range(-(-n_ch // 128))), "stage": "full", "reps": args.reps,
                      "warmup": args.warmup, "cells_planted": args.cells, "cells_decoded_u8": cells["u8"], "cells_decoded_c64": cells["c64"],
                      "xcorr_kernel_u8": kernel["u8"], "xcorr_kernel_c64": kernel["c64"]},
           "ms_min_max": {k: [float(min(v[args.warmup:])), float(max(v[args.warmup:]))] for k, v in t.items()},
           "sclk_mhz_median": (sorted(samples)[len(samples) // 2] if samples else None), "sclk_samples": len(samples),
           "device": torch.cuda.get_device_name(dev), "kernels": ks}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    try:
        with open(args.out) as fh:
            old = json.load(fh)
    except (OSError, ValueError):
        old = {}
    with open(args.out, "w") as fh:
        json.dump(dict(old, stream_u8=dict(old.get("stream_u8", {}), **{"%d/%d" % (up, down): res})), fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


def bench_u8(args, pkg, torch, dev, d_wide, d_c64, shifts, carriers, f, n_in, fs_in, D, N_CH, N_OUT, samples, stop, th):
    d_u8 = torch.empty((N_CH, N_OUT, 2), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    t = {"u8": dict(total=[], chan=[]), "c64": dict(total=[], chan=[])}
    cells = {}
    with pkg.Searcher(args.device) as s:
        stream = torch.cuda.ExternalStream(pkg.capi.load().lcs_stream(s._h), device=dev)
        th.start()
        for i in range(args.warmup + args.reps):
            for mode in ("u8", "c64"):      # interleaved: both pipelines see the same clocks
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                if mode == "u8":
                    s.channelize_u8(d_wide.data_ptr(), pkg.FMT_IQ_S16, n_in, fs_in, 1, D, shifts, d_u8.data_ptr(), N_OUT)
                    buf, fmt = d_u8, pkg.FMT_IQ_U8
                else:
                    s.channelize(d_wide.data_ptr(), pkg.FMT_IQ_S16, n_in, fs_in, D, shifts, d_c64.data_ptr(), N_OUT)
                    buf, fmt = d_c64, pkg.FMT_C64
                n = 0
                for h in range(N_CH // 128):
                    sl = slice(128 * h, 128 * h + 128)
                    n += sum(len(c) for c in s.search_batch(buf[128 * h].data_ptr(), fmt, 128, N_OUT, f, carriers[sl], carriers[sl], 1.92e6, pkg.STAGE_FULL))
                e1.record(stream)
                e1.synchronize()
                t[mode]["total"].append(e0.elapsed_time(e1))
                t[mode]["chan"].append(s.last_channelize_ms())
                cells[mode] = n
        stop.set()
        th.join(timeout=10)
    med = lambda v: float(np.median(v[args.warmup:]))
    a, b, a_chan, b_chan = med(t["u8"]["total"]), med(t["c64"]["total"]), med(t["u8"]["chan"]), med(t["c64"]["chan"])
    spec = importlib.util.spec_from_file_location("code_objects", os.path.join(ROOT, "tools", "code_objects.py"))
    co = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(co)
    ks = {k: v for k, v in co.kernels_of(os.path.join(ROOT, "lte-cell-scanner_amd", "liblcs_amd.so")).items()
          if "k_chan_quant_u8" in k or ("k_channelize" in k and "Lb1ELb0E" in k)}
    res = {"a_u8_pipeline_ms": a, "b_c64_pipeline_ms": b, "ratio_a_over_b": a / b, "u8_is_faster": bool(a < b),
           "a_channelize_u8_ms": a_chan, "a_search_ms": a - a_chan, "a_channelizer_share_of_search": a_chan / (a - a_chan), "target_share": 0.25,
           "meets_target": bool(a_chan <= 0.25 * (a - a_chan)), "b_channelize_ms": b_chan, "b_search_ms": b - b_chan,
           "config": {"decim": D, "fmt": "s16", "n_ch": N_CH, "n_in": n_in, "n_out": N_OUT, "raster_hz": 100e3, "n_f": int(f.size), "batches": "2 x 128",
                      "stage": "full", "reps": args.reps, "warmup": args.warmup, "cells_planted": args.cells, "cells_decoded_u8": cells["u8"],
                      "cells_decoded_c64": cells["c64"]},
           "a_ms_min_max": [float(min(t["u8"]["total"][args.warmup:])), float(max(t["u8"]["total"][args.warmup:]))],
           "b_ms_min_max": [float(min(t["c64"]["total"][args.warmup:])), float(max(t["c64"]["total"][args.warmup:]))],
           "sclk_mhz_median": (sorted(samples)[len(samples) // 2] if samples else None), "sclk_samples": len(samples),
           "device": torch.cuda.get_device_name(dev), "kernels": ks}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    try:
        with open(args.out) as fh:
            old = json.load(fh)
    except (OSError, ValueError):
        old = {}
    with open(args.out, "w") as fh:
        json.dump(dict(old, u8=res), fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
