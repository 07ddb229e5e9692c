#!/usr/bin/env python3
"""Detection rate of a cell hidden under a stronger one, with and without cancellation rounds -> profiles/sic/accuracy.json.

Every point is `--seeds` captures (default 20) of a strong cell S (n_id_cell 31, 2 ports, 0 dB) and a weaker cell W `gain_db` below
it, `dt` samples later, with the same or another n_id_2; AWGN 15 dB below S's sync symbols, 8-bit quantisation (the dongle's bytes,
the int8 route).  Reported per point: how often W is listed by Searcher.search_batch and by Searcher.search_batch_sic (2 rounds), how
often S is, false identities, and the mean PSS suppression of S the stage reports.  The captures are synthesised by CPU worker
processes (they never touch the GPU); the searches run in this process.

    python tools/sic_accuracy.py [--seeds 20] [--workers 12] [--out profiles/sic/accuracy.json]"""
import argparse
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import sic_cases as K      # the cells, carrier and noise level of the tests: one definition  # noqa: E402

FC, FS, SNR_DB, F_SET = K.FC, K.FS, K.SNR_DB, K.F_SET
S, PORT_GAINS = K.S, K.PORT_GAINS
W = {k: v for k, v in K.W.items() if k not in ("t0", "gain_db")}


def points():
    pts = []
    for same in (True, False):
        for gain in (-3.0, -6.0, -9.0, -12.0):
            for dt in (0, 3, 100, 400):
                pts.append(dict(name="fdd normal 2-port flat", gain_db=gain, dt=dt, same_n_id_2=same))
    base = dict(gain_db=-6.0, dt=3, same_n_id_2=True)
    pts += [dict(base, name="extended CP", cp_normal=False), dict(base, name="tdd (2, 9)", tdd=(2, 9)), dict(base, name="1-port S", s_ports=1),
            dict(base, name="4-port S", s_ports=4), dict(base, name="EPA", channel="EPA"), dict(base, name="EVA", channel="EVA")]
    return pts


def cells_of(p):
    s = dict(S)
    w = dict(W, t0=S["t0"] + p["dt"], gain_db=p["gain_db"], n_id_2=1 if p["same_n_id_2"] else 2)
    if "s_ports" in p:
        s.update(n_ports=p["s_ports"], port_gains=PORT_GAINS[p["s_ports"]])
    for key in ("cp_normal", "tdd", "channel"):
        if key in p:
            s[key] = w[key] = p[key]
    if "channel" in p:      # the channel draws the ports' gains
        s.pop("port_gains"); w.pop("port_gains")
    return [s, w]


def synthesise(job):
    import __graft_entry__ as G
    synth = G.load_package().synth
    pi, seed, p = job
    iq, _ = synth.make_capbuf(1000 * pi + seed, FC, cells_of(p), snr_db=SNR_DB)
    return pi, seed, iq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=20)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sic", "accuracy.json"))
    a = ap.parse_args()
    pts = points()
    jobs = [(pi, s, p) for pi, p in enumerate(pts) for s in range(a.seeds)]
    t0 = time.time()
    caps = {}
    with mp.get_context("spawn").Pool(a.workers) as pool:      # before this process opens the GPU
        for k, (pi, seed, iq) in enumerate(pool.imap_unordered(synthesise, jobs, chunksize=4)):
            caps[(pi, seed)] = iq
            if k % 100 == 0:
                print("synthesised %d / %d captures, %.0f s" % (k, len(jobs), time.time() - t0), flush=True)
    import torch
    import __graft_entry__ as G
    pkg = G.load_package()
    out = dict(fc=FC, snr_db=SNR_DB, seeds=a.seeds, rounds=2, format="u8", points=[])
    # the device residual against the numpy rule (tests/sic_ref.py) on the tests' S + W capture, measured here
    import sic_ref as R
    x = K.pair().astype(np.complex64)
    d, res = torch.from_numpy(x).to("cuda:0"), torch.empty(x.size, dtype=torch.complex64, device="cuda:0")
    with pkg.Searcher(0) as s:
        found = s.search_capbuf(x.astype(np.complex128), F_SET, FC, FC, FS)[0]
        s.sic_cancel(d.data_ptr(), pkg.FMT_C64, 1, x.size, [found], FC, FC, FS, res.data_ptr())
    want, _ = R.cancel(x.astype(np.complex128), found, FC, FC, FS)
    out["residual_max_abs_over_rms_vs_sic_ref"] = float(np.abs(res.cpu().numpy().astype(np.complex128) - want).max() / np.sqrt(np.mean(np.abs(x) ** 2)))
    print("residual: max |device - sic_ref| / rms = %.3e" % out["residual_max_abs_over_rms_vs_sic_ref"], flush=True)
    searchers = {}
    for pi, p in enumerate(pts):
        tdd = "tdd" in p
        if tdd not in searchers:
            searchers[tdd] = pkg.Searcher(0)
            if tdd:
                searchers[tdd].set_duplex(pkg.DUPLEX_TDD)
        s = searchers[tdd]
        d = torch.from_numpy(np.stack([caps[(pi, seed)] for seed in range(a.seeds)])).to("cuda:0")
        n_cap = d.shape[1] // 2
        plain = s.search_batch(d.data_ptr(), pkg.FMT_IQ_U8, a.seeds, n_cap, F_SET, FC, FC, FS, pkg.STAGE_FULL)
        cells, rounds, info = s.search_batch_sic(d.data_ptr(), pkg.FMT_IQ_U8, a.seeds, n_cap, F_SET, FC, FC, FS, max_rounds=2)
        id_s, id_w = 31, 231 + (1 if p["same_n_id_2"] else 2)
        sup = [i.suppression_db for cs, inf in zip(cells, info) for c, i in zip(cs, inf) if c.n_id_cell() == id_s and i.cancelled]
        rec = dict(p, n=a.seeds,
                   w_plain=sum(id_w in [c.n_id_cell() for c in cs] for cs in plain), w_sic=sum(id_w in [c.n_id_cell() for c in cs] for cs in cells),
                   s_plain=sum(id_s in [c.n_id_cell() for c in cs] for cs in plain), s_sic=sum(id_s in [c.n_id_cell() for c in cs] for cs in cells),
                   false_plain=sum(c.n_id_cell() not in (id_s, id_w) for cs in plain for c in cs),
                   false_sic=sum(c.n_id_cell() not in (id_s, id_w) for cs in cells for c in cs),
                   s_suppression_db_mean=float(np.mean(sup)) if sup else None, s_suppression_db_min=float(np.min(sup)) if sup else None)
        if "tdd" in rec:
            rec["tdd"] = list(rec["tdd"])
        out["points"].append(rec)
        print(json.dumps(rec), flush=True)
    for s in searchers.values():
        s.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out, "%.0f s" % (time.time() - t0))


if __name__ == "__main__":
    main()
