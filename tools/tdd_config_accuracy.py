#!/usr/bin/env python3
"""How often the uplink-downlink configuration rule (include/lcs.h: lcs_set_tdd_config) is right, over a seeded population of
planted TDD cells.

Population: 7 configurations x both CP types x SNR 10 / 5 / 0 / -3 dB x {no channel, EPA 5 Hz, EVA 70 Hz, ETU 300 Hz}; the DwPTS
length walks through 3, 5, 6, 8, 9, 10, 11, 12 symbols and the ports through 1 / 2 / 4 from cell to cell.  One 80 ms buffer of
dongle bytes per cell (synth.make_capbuf), uplink subframes silent.  The CPU half: the oracle's xcorr_pss / peak_search, sss_detect
and pss_sss_foe from the numpy restatement in TDD mode (tests/sss_duplex_ref.py), the oracle's extract_tfg / tfoec / decode_mib, and
the numpy rule (tests/tdd_config_ref.py) on the oracle's UNCORRECTED grid of every planted cell that decodes.  --library adds the
library's own fused chain on a GPU (Searcher in DUPLEX_TDD with set_tdd_config) on the same buffers.

Per SNR and channel: cells planted, decoded, wrong configurations (a number other than the planted one), cells without a number
(-1), wrong DwPTS classes among the cells with the right configuration, and the smallest margin of a right decision.
Writes profiles/tdd/tdd_config_accuracy.json and prints the table."""
import argparse
import concurrent.futures as cf
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FS, FC = 1.92e6, 1.9e9
GRID = np.arange(-5e3, 5e3 + 1, 2.5e3)
SNRS = (10.0, 5.0, 0.0, -3.0)
CHANNELS = (("none", None, 0.0), ("EPA5", "EPA", 5.0), ("EVA70", "EVA", 70.0), ("ETU300", "ETU", 300.0))
DWPTS = (3, 5, 6, 8, 9, 10, 11, 12)


def population():
    out, i = [], 0
    for si, snr in enumerate(SNRS):
        for ci, (cname, chan, dop) in enumerate(CHANNELS):
            for cp_normal in (True, False):
                for cfg in range(7):
                    cell = dict(n_id_1=(37 * i + 11) % 168, n_id_2=i % 3, cp_normal=cp_normal, n_ports=(1, 2, 4)[i % 3], n_rb_dl=(6, 15, 25, 50, 75, 100)[i % 6],
                                sfn0=(53 * i) % 1024, f_off=float((i * 397) % 3001 - 1500), t0=float((i * 2711) % 19200) + 0.25 * (i % 4),
                                tdd=(cfg, DWPTS[(i + si + ci) % len(DWPTS)]))
                    if chan is not None:
                        cell.update(channel=chan, doppler_hz=dop)
                    out.append(dict(index=i, seed=7000 + i, snr=snr, channel=cname, cell=cell))
                    i += 1
    return out


def _buffer(case):
    import __graft_entry__ as ge
    return ge.load_package().synth.make_capbuf(case["seed"], FC, [case["cell"]], snr_db=case["snr"], n_cap=153600)[0]


def cpu_case(case):
    """-> dict(decoded, config, rows, margin) of the planted cell through the CPU chain"""
    import oracle as O
    import sss_duplex_ref as R
    import tdd_config_ref as TR
    O.set_legacy(False)
    O.set_threads(1)
    iq = _buffer(case).astype(np.float64)
    cap = ((iq[0::2] - 127.0) / 128.0) + 1j * ((iq[1::2] - 127.0) / 128.0)
    cell = case["cell"]
    n_id = cell["n_id_2"] + 3 * cell["n_id_1"]
    for pk in R.oracle_peaks(cap, GRID, FC, FC, FS):
        if pk.n_id_2 != cell["n_id_2"]:
            continue
        c = R.per_peak(pk, cap, FC, FC, FS, R.GEO["tdd"])
        if c is None or c.n_id_2 + 3 * c.n_id_1 != n_id:
            continue
        tfg, _ = O.extract_tfg(c, cap, FC, FC, FS)
        e = TR.estimate(n_id, c.cp_type, tfg)
        return dict(decoded=True, config=int(e["ul_dl_config"]), rows=int(e["dwpts_rs_rows"]), margin=float(e["margin"]))
    return dict(decoded=False)


def library_cases(cases, buffers):
    import __graft_entry__ as ge
    pkg = ge.load_package()
    out = []
    with pkg.Searcher(0) as s:
        s.set_duplex(pkg.DUPLEX_TDD)
        s.set_tdd_config(True)
        for case, buf in zip(cases, buffers):
            iq = buf.astype(np.float64)
            cap = ((iq[0::2] - 127.0) / 128.0) + 1j * ((iq[1::2] - 127.0) / 128.0)
            cells, _ = s.search_capbuf(cap, GRID, FC, FC, FS)
            info = s.last_tdd_info(1, 16)[0]
            n_id = case["cell"]["n_id_2"] + 3 * case["cell"]["n_id_1"]
            r = dict(decoded=False)
            for k, c in enumerate(cells[:16]):
                if c.n_id_cell() == n_id:
                    r = dict(decoded=True, config=int(info[k].ul_dl_config), rows=int(info[k].dwpts_rs_rows), margin=float(info[k].margin))
                    break
            out.append(r)
    return out


def table(cases, results):
    import tdd_config_ref as TR
    rows = []
    for snr in SNRS:
        for cname, _, _ in CHANNELS:
            sel = [(c, r) for c, r in zip(cases, results) if c["snr"] == snr and c["channel"] == cname]
            dec = [(c, r) for c, r in sel if r["decoded"]]
            right = [(c, r) for c, r in dec if r["config"] == c["cell"]["tdd"][0]]
            wrong_dw = [c["index"] for c, r in right if r["rows"] != TR.dwpts_rows(c["cell"]["tdd"][1], 1 if c["cell"]["cp_normal"] else 2)]
            rows.append(dict(snr_db=snr, channel=cname, planted=len(sel), decoded=len(dec),
                             wrong_configuration=int(sum(r["config"] >= 0 and r["config"] != c["cell"]["tdd"][0] for c, r in dec)),
                             no_configuration=int(sum(r["config"] < 0 for c, r in dec)), wrong_dwpts_class=len(wrong_dw),
                             smallest_margin=float(min([r["margin"] for _, r in right] or [0.0]))))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--library", action="store_true", help="also run the library's fused chain on GPU 0")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--limit", type=int, default=0, help="developer runs: the first N cells of every (SNR, channel) group only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tdd", "tdd_config_accuracy.json"))
    a = ap.parse_args()
    cases = population()
    if a.limit:
        cases = [c for c in cases if c["index"] % 14 < a.limit]
    with cf.ProcessPoolExecutor(max_workers=a.jobs) as ex:
        cpu = list(ex.map(cpu_case, cases, chunksize=1))
        buffers = list(ex.map(_buffer, cases, chunksize=1)) if a.library else None      # (generated by the pool: a second apiece, 34 MB in all)
    out = dict(fc=FC, grid_hz=[float(x) for x in GRID], cells=len(cases), cpu=table(cases, cpu),
               per_cell=[dict(index=c["index"], snr_db=c["snr"], channel=c["channel"], planted=list(c["cell"]["tdd"]), cp_normal=c["cell"]["cp_normal"],
                              n_ports=c["cell"]["n_ports"], cpu=r) for c, r in zip(cases, cpu)])
    if a.library:
        lib = library_cases(cases, buffers)
        out["library"] = table(cases, lib)
        out["library_disagrees_with_cpu"] = [c["index"] for c, r, q in zip(cases, cpu, lib)
                                             if r["decoded"] and q["decoded"] and (r["config"], r["rows"]) != (q["config"], q["rows"])]
        for row, q in zip(out["per_cell"], lib):
            row["library"] = q
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    for key in ("cpu", "library"):
        for row in out.get(key, []):
            print(key, json.dumps(row))


if __name__ == "__main__":
    main()
