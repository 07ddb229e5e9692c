#!/usr/bin/env python3
"""How often the PHICH rule (include/lcs.h: lcs_phich_info) is right, measured with its numpy statement (tests/phich_ref.py) on crafted
grids (tests/phich_cases.py: crafted) -- no GPU, no test asserts these numbers.  It is where LCS_PHICH_MIN_SIGMA comes from.

Population: 50 resource blocks, normal CP, normal PHICH duration; 1, 2 and 4 ports; Ng = 1/6, 1/2, 1, 2 (2, 4, 7, 13 groups); a
smooth channel that is not flat (ripple), so that the interpolated channel and the orthogonality of the sequences are as imperfect
as they are on air; white noise at 0, 5 and 10 dB per resource element (unit-power elements), also on the reference signals the
channel is estimated from.  In every subframe half of the (group, seq) pairs carry an indicator of amplitude 1 with a random sign,
the rest are silent.

Per point and per candidate min_sigma (multiples of 0.25, min_amp = LCS_PHICH_MIN_AMP): the share of silent entries that read
present, the share of planted ones that are missed, the share of planted ones read with the wrong sign, and the variance of value /
sigma over the silent entries.  The default is the smallest candidate at which the silent entries read present in at most 1 of
1000 at EVERY SNR (pooled over ports and Ng, at least 20 000 silent entries each).  Writes profiles/phich/accuracy.json and prints
the table."""
import argparse
import concurrent.futures as cf
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

SNRS = (0.0, 5.0, 10.0)
PORTS = (1, 2, 4)
RESOURCES = (1, 2, 3, 4)
NG = {1: "1/6", 2: "1/2", 3: "1", 4: "2"}
N_RB = 50
CANDIDATES = [0.25 * k for k in range(8, 33)]               # 2.0 .. 8.0
N_SUB = 60


def trial(job):
    """one grid -> (snr, ports, resource, |value| / sigma and |value| of the silent entries, the same and the sign error of the planted)"""
    import phich_cases as HC
    import phich_ref as HR
    snr, ports, res, seed = job
    name = "acc_%d_%d" % (ports, res)
    HC.CORNERS[name] = dict(n_rb=N_RB, n_ports=ports, cp=1, duration=1, resource=res, mi=None, n_id=(97 * seed + 13 * res + ports) % 504)
    tfg, planted = HC.crafted.__wrapped__(name, "half", snr, N_SUB, 0, seed, True)
    c = HC.CORNERS[name]
    ref = HR.decode(tfg, c["n_id"], 1, ports, N_RB, 0x3FF, 1, res, None, 0.0, 0.0)
    sil, pla = [], []
    for g, pat in enumerate(planted):
        v, s = ref["values"][g], ref["sigma"][g]
        ratio = np.abs(v) / np.where(s > 0, s, np.inf)
        m = pat == 0
        sil.append(np.stack([ratio[m], np.abs(v[m]), (v / np.where(s > 0, s, np.inf))[m]], 1))
        pla.append(np.stack([ratio[~m], np.abs(v[~m]), (np.sign(v[~m]) != pat[~m]).astype(float)], 1))
    return snr, ports, res, np.concatenate(sil), np.concatenate(pla)


def rates(sil, pla, min_amp, min_sigma):
    present = lambda a: (a[:, 1] >= min_amp) & (a[:, 0] >= min_sigma)
    ps, pp = present(sil), present(pla)
    return float(ps.mean()), float((~pp).mean()), float((pp & (pla[:, 2] > 0)).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=8, help="grids of %d subframes per (SNR, ports, Ng)" % N_SUB)
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phich", "accuracy.json"))
    a = ap.parse_args()
    from conftest import load_pkg
    min_amp = load_pkg().capi.PHICH_MIN_AMP
    jobs = [(snr, p, r, k) for snr in SNRS for p in PORTS for r in RESOURCES for k in range(a.seeds)]
    with cf.ProcessPoolExecutor(max_workers=a.jobs) as ex:
        res = list(ex.map(trial, jobs, chunksize=1))
    pick = lambda f: (np.concatenate([r[3] for r in res if f(r)]), np.concatenate([r[4] for r in res if f(r)]))
    by_snr = []
    for snr in SNRS:
        sil, pla = pick(lambda r: r[0] == snr)
        by_snr.append(dict(snr_db=snr, silent=int(sil.shape[0]), planted=int(pla.shape[0]),
                           false_present={"%.2f" % m: rates(sil, pla, min_amp, m)[0] for m in CANDIDATES}))
    default = next((m for m in CANDIDATES if all(b["false_present"]["%.2f" % m] <= 1e-3 for b in by_snr)), None)
    assert all(b["silent"] >= 20000 for b in by_snr), "fewer than 20 000 silent entries per SNR: raise --seeds"
    points = []
    for snr in SNRS:
        for p in PORTS:
            for r in RESOURCES:
                sil, pla = pick(lambda x: x[:3] == (snr, p, r))
                fp, miss, wrong = rates(sil, pla, min_amp, default if default is not None else CANDIDATES[-1])
                points.append(dict(snr_db=snr, ports=p, ng=NG[r], silent=int(sil.shape[0]), planted=int(pla.shape[0]), false_present=round(fp, 5),
                                   missed=round(miss, 5), wrong_sign=round(wrong, 5), var_value_over_sigma=round(float(np.var(sil[:, 2])), 4)))
    doc = dict(n_rb=N_RB, subframes_per_grid=N_SUB, seeds=a.seeds, snr_is="per resource element", min_amp=min_amp, candidates=CANDIDATES,
               false_present_by_snr=by_snr, min_sigma_default=default, points_at_default=points)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    for b in by_snr:
        print(json.dumps(b))
    for p in points:
        print(json.dumps(p))
    print("min_sigma default:", default)


if __name__ == "__main__":
    main()
