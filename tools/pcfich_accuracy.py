#!/usr/bin/env python3
"""How often the PCFICH rule (include/lcs.h: lcs_pcfich_info) is right, measured with its numpy statement (tests/pcfich_ref.py) on
planted cells -- no GPU, no test asserts these numbers.

Population: two-port cells at (R, n_rb) = (4, 25) and (1, 6), normal CP, three frames each with the pattern cfi = 1 + (3 frame +
subframe) mod 3 (synth.cell_waveform_wide(cfi=...), per-port waveforms); {no channel, EPA 5 Hz, EVA 70 Hz, ETU 300 Hz}, every port
through its own synth.fading_channel at the wide rate; SNR 10 / 5 / 0 / -3 / -6 dB per resource element (unit-power elements, white
noise of power 1 / snr per sample; the same faded signal under every SNR).  The grid is tests/meas_wide_ref.grid with the true
timing, the DFT window two 1.92 Msps samples inside the cyclic prefix, and no frequency offset: what is measured is the rule, not
the search in front of it.

Per point: decisions, wrong ones, the median margin, and the median margin of the wrong ones.  Pooled over all points: the share
of wrong decisions among those with a margin of at least m, for m = 0, 0.05, ..: the margin below which a decision should not be
trusted is read off that list.  Writes profiles/pcfich/pcfich_accuracy.json and prints the table."""
import argparse
import concurrent.futures as cf
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FS, FC = 1.92e6, 739e6
SNRS = (10.0, 5.0, 0.0, -3.0, -6.0)
CHANNELS = (("none", None, 0.0), ("EPA5", "EPA", 5.0), ("EVA70", "EVA", 70.0), ("ETU300", "ETU", 300.0))
SHAPES = ((4, 25), (1, 6))
N_FRAMES = 3
LEAD = 100                                                   # 1.92 Msps samples of silence in front of the first frame


def planted(frame, subframe):
    return 1 + (3 * frame + subframe) % 3


def trial(job):
    """one cell through one channel realisation, under every SNR -> [(snr, planted [30], cfi [30], margin [30])]"""
    import meas_wide_ref as WR
    import pcfich_ref as PR
    from conftest import load_pkg
    synth = load_pkg().synth
    (R, n_rb), (cname, prof, dop), k = job
    seed = 31000 + 1000 * SHAPES.index((R, n_rb)) + 100 * [c[0] for c in CHANNELS].index(cname) + k
    rng = np.random.default_rng(seed)
    n_id_1, n_id_2 = (37 * k + 11) % 168, k % 3
    w = synth.cell_waveform_wide(N_FRAMES, n_id_1, n_id_2, R, n_rb, True, n_ports=2, rng=rng, per_port=True, cfi=planted)
    if prof is None:
        g = np.exp(2j * np.pi * rng.random(2))
        sig = g[0] * w[0] + g[1] * w[1]
    else:
        sig = synth.fading_channel(rng, w[0], prof, dop, fs=FS * R) + synth.fading_channel(rng, w[1], prof, dop, fs=FS * R)
    sig = np.concatenate([np.zeros(LEAD * R, np.complex128), sig, np.zeros(256 * R, np.complex128)])
    n_ofdm = 20 * N_FRAMES * 7
    rows = [14 * g for g in range(10 * N_FRAMES)]
    want = np.array([planted(g // 10, g % 10) for g in range(10 * N_FRAMES)])
    out = []
    for snr in SNRS:
        sigma = np.sqrt(0.5 / 10 ** (snr / 10))
        cap = sig + sigma * (rng.standard_normal(sig.size) + 1j * rng.standard_normal(sig.size))
        tfg, _ = WR.grid(cap, (LEAD - 2) * R, 0.0, 1, FC, FC, FS * R, 128 * R, n_rb, n_ofdm, rows)
        r = PR.decode(tfg, n_id_2 + 3 * n_id_1, 1, 2, n_rb)
        out.append((snr, want.tolist(), r["cfi"].tolist(), r["margin"].tolist()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=8, help="cells per (shape, channel): 30 decisions each under every SNR")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcfich", "pcfich_accuracy.json"))
    a = ap.parse_args()
    jobs = [(s, c, k) for s in SHAPES for c in CHANNELS for k in range(a.trials)]
    with cf.ProcessPoolExecutor(max_workers=a.jobs) as ex:
        res = list(ex.map(trial, jobs, chunksize=1))
    points, pooled = [], []
    for s in SHAPES:
        for c in CHANNELS:
            for snr in SNRS:
                ok, mar = [], []
                for job, r in zip(jobs, res):
                    if job[0] != s or job[1] != c:
                        continue
                    for q, want, cfi, margin in r:
                        if q == snr:
                            ok += [x == y for x, y in zip(want, cfi)]
                            mar += margin
                ok, mar = np.array(ok), np.array(mar)
                pooled += list(zip(ok, mar))
                points.append(dict(R=s[0], n_rb=s[1], channel=c[0], snr_db=snr, decisions=int(ok.size), wrong=int((~ok).sum()),
                                   median_margin=round(float(np.median(mar)), 4),
                                   median_margin_of_wrong=round(float(np.median(mar[~ok])), 4) if (~ok).any() else None))
    ok, mar = np.array([p[0] for p in pooled]), np.array([p[1] for p in pooled])
    trust = []
    for m in np.arange(0.0, 1.0001, 0.05):
        sel = mar >= m
        trust.append(dict(margin_at_least=round(float(m), 2), decisions=int(sel.sum()), wrong=int((~ok[sel]).sum()),
                          wrong_share=round(float((~ok[sel]).mean()), 5) if sel.any() else None))
    doc = dict(ports=2, frames=N_FRAMES, trials=a.trials, snr_is="per resource element", points=points, wrong_share_by_margin=trust)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    for p in points:
        print(json.dumps(p))
    for t in trust:
        print(json.dumps(t))


if __name__ == "__main__":
    main()
