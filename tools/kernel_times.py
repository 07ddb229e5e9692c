#!/usr/bin/env python3
"""Per-kernel times out of the database a `rocprofv3 --kernel-trace --stats` run leaves: calls, mean and median duration in
microseconds of every kernel whose name contains one of the given words (default: the per-peak tail of sss_foe.hip).
tools/kernel_times.py RESULTS.db [word ...]"""
import sqlite3
import sys

import numpy as np


def main():
    words = sys.argv[2:] or ["k_sss_win", "k_sss_ml", "k_foe_win", "k_foe_fin"]
    c = sqlite3.connect(sys.argv[1])
    rows = {}
    for name, dur, gx, wx in c.execute("select name, duration, grid_x, workgroup_x from kernels"):
        if any(w in name for w in words):
            rows.setdefault((name.split("(")[0], gx, wx), []).append(dur)
    for (name, gx, wx), d in sorted(rows.items()):
        d = np.array(d) / 1e3
        print(f"{name[:60]:60s} grid {gx:8d} wg {wx:4d} calls {d.size:5d} mean {d.mean():8.2f} us median {np.median(d):8.2f} us")


if __name__ == "__main__":
    main()
