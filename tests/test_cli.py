"""The C++ CellSearch front end (host/CellSearch.cpp): option handling on CPU, end-to-end on GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden, iq_u8_to_capbuf, load_pkg

EXE = os.path.join(ROOT, "host", "CellSearch")
SHIM = os.path.join(ROOT, "host", "test_shim")


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])


def _run(args, **kw):
    return subprocess.run([EXE] + args, capture_output=True, text=True, timeout=600, **kw)


def test_help_lists_reference_options():
    assert _run(["--help"]).stdout == _run(["-h"]).stdout
    out = _run(["-h"]).stdout
    for opt in ("-s --freq-start", "-e --freq-end", "-p --ppm", "-c --correction", "-r --record", "-l --load",
                "-d --data-dir", "-i --device-index", "-v --verbose", "-b --brief"):
        assert opt in out


def test_argument_errors_match_reference_messages():
    assert "must specify a start frequency" in _run([]).stderr
    assert "cannot read and write captured data at the same time" in _run(["-s", "739e6", "-r", "-l"]).stderr
    assert "end frequency must be >= start frequency" in _run(["-s", "739e6", "-e", "700e6", "-l"]).stderr
    r = _run(["-s", "739049999", "-l", "-d", "/nonexistent"])
    assert "start frequency has been rounded to the nearest multiple of 100kHz" in r.stdout
    assert "use --load" in _run(["-s", "739e6"]).stderr


def test_option_forms():
    """Short/long/attached/= forms of one option all parse; malformed values and stray arguments are refused."""
    for form in (["-s", "739e6"], ["-s739e6"], ["--freq-start", "739e6"], ["--freq-start=739e6"]):
        r = _run(form + ["-b"])
        assert "use --load" in r.stderr, (form, r.stderr)
    assert "could not parse ppm value" in _run(["-s", "739e6", "-p", "12x"]).stderr
    assert "unknown/extra arguments" in _run(["-s", "739e6", "stray"]).stderr


def test_shim_links_against_the_reference_signatures_and_del_oob():
    """host/searcher_shim.cpp defines the reference's eight free functions (include/searcher.h:22-124) with their exact
    signatures; host/test_shim.cpp calls them like src/CellSearch.cpp:484-558 does.  del_oob is host-only."""
    r = subprocess.run([SHIM, "--del-oob"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "del_oob ok" in r.stdout
    syms = subprocess.run(["nm", "-C", os.path.join(ROOT, "host", "searcher_shim.o")], capture_output=True, text=True).stdout
    for fn in ("xcorr_pss(", "peak_search(", "sss_detect(", "pss_sss_foe(", "extract_tfg(", "tfoec(", "decode_mib(", "del_oob(", "lcs_shim_want_xc(bool)"):
        assert re.search(r" T " + re.escape(fn), syms), fn
    assert re.search(r" T tfoec\(Cell const&, .*RS_DL const&", syms) and re.search(r" T decode_mib\(Cell const&, .*RS_DL const&\)", syms)


def test_no_gpu_is_a_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = _run(["-s", "739e6", "-l", "-d", "/nonexistent"])
    assert r.returncode != 0 and "MI355X is required" in r.stderr


@pytest.mark.gpu
def test_fulltest_known_answer(tmp_path):
    """The reference's (disabled) FullTest: `CellSearch -s 739000000 -l -d test` must match cell.ID..271."""
    pkg = load_pkg()
    g = golden("capbuf_0000")
    pkg_it = __import__("importlib").import_module("lte_cell_scanner_amd.itfile")
    pkg_it.write_it(str(tmp_path / "capbuf_0000.it"), {"capbuf": iq_u8_to_capbuf(g["iq_u8"]), "fc": g["fc"].astype(np.int32)})
    r = _run(["-s", "739000000", "-l", "-d", str(tmp_path)])
    assert r.returncode == 0, r.stderr
    assert re.search(r"cell.ID..271", r.stdout) and re.search(r"cell.ID..277", r.stdout)
    assert "Examining center frequency 739 MHz ..." in r.stdout
    assert "CID A      fc   foff RXPWR C nRB P  PR CrystalCorrectionFactor" in r.stdout
    rows = [l for l in r.stdout.splitlines() if re.match(r"^(277|271) 2    739M  35\.2k", l)]
    assert len(rows) == 2, r.stdout
    for l in rows:
        assert re.search(r" N  50 N one 1\.0000476", l), l
    # no cells on an empty carrier
    noise = np.random.default_rng(1).normal(0, 0.1, 153600) + 1j * np.random.default_rng(2).normal(0, 0.1, 153600)
    pkg_it.write_it(str(tmp_path / "capbuf_0000.it"), {"capbuf": noise, "fc": np.array([800000000], np.int32)})
    r = _run(["-s", "800000000", "-l", "-d", str(tmp_path), "-b"])
    assert r.returncode == 0 and "No LTE cells were found..." in r.stdout


@pytest.mark.gpu
def test_shim_runs_the_reference_call_sequence(tmp_path):
    """The reference's seven functions, called in the reference's order through the shim, decode the golden buffer."""
    pkg = load_pkg()
    g = golden("capbuf_0000")
    pkg_it = __import__("importlib").import_module("lte_cell_scanner_amd.itfile")
    pkg_it.write_it(str(tmp_path / "capbuf_0000.it"), {"capbuf": iq_u8_to_capbuf(g["iq_u8"]), "fc": g["fc"].astype(np.int32)})
    r = subprocess.run([SHIM, str(tmp_path / "capbuf_0000.it")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "n_comb_xc 15 n_comb_sp 15 peaks 4" in r.stdout
    rows = [l.split() for l in r.stdout.splitlines() if l.startswith("cell ")]
    got = {int(x[1]): dict(zip(x[2::2], x[3::2])) for x in rows}
    assert sorted(got) == [271, 277]
    assert got[277]["sfn"] == "74" and got[271]["sfn"] == "22" and all(v["ports"] == "2" and v["n_rb_dl"] == "50" and v["tfg_rows"] == "854" for v in got.values())
    assert abs(float(got[277]["freq_superfine"]) - 35228.46) < 0.5 and abs(float(got[271]["freq_superfine"]) - 35231.34) < 0.5


@pytest.mark.gpu
def test_shim_replays_the_reference_xcorr_pss_test(tmp_path):
    """test/test_xcorr_pss.cpp:94-124 through the reference-shaped xcorr_pss of host/searcher_shim.cpp: `xc` (searcher.h:35)
    comes back empty by default and filled after lcs_shim_want_xc(true); every output, flattened as the reference's test
    flattens it, against the oracle with that test's tolerances where it states absolute ones our arithmetic meets (xc 1e-6,
    the frequency indices equal) and this repository's bars elsewhere (1e-5 relative on the powers, 1e-11 on the power
    estimates) -- the reference's own expected vectors (test_xcorr_pss.it) are not shipped."""
    import oracle as O
    g = golden("capbuf_0000")
    cap = iq_u8_to_capbuf(g["iq_u8"])
    pkg = load_pkg()
    pkg_it = __import__("importlib").import_module("lte_cell_scanner_amd.itfile")
    pkg_it.write_it(str(tmp_path / "capbuf_0000.it"), {"capbuf": cap, "fc": g["fc"].astype(np.int32)})
    f = [30e3, 35e3, 40e3]
    out = tmp_path / "xc.bin"
    r = subprocess.run([SHIM, "--xc", str(tmp_path / "capbuf_0000.it"), str(out)] + [repr(x) for x in f], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    hdr = np.frombuffer(raw, np.int64, 8)
    d1, d2, d3, n_sp, n_spi, ncx, ncs, empty_default = [int(x) for x in hdr]
    assert (d1, d2, d3) == (3, 153600 - 136, 3) and (ncx, ncs) == (15, 15) and empty_default == 1
    o = 64
    def take(n, dt):
        nonlocal o
        a = np.frombuffer(raw, dt, n, o)
        o += a.nbytes
        return a
    xc = take(d1 * d2 * d3, np.complex128).reshape(d3, d2, d1).transpose(2, 1, 0)     # first index fastest -> [t][k][foi]
    sp, spi = take(n_sp, np.float64), take(n_spi, np.float64)
    single = take(3 * 9600 * 3, np.float64).reshape(3, 9600, 3).transpose(2, 1, 0)
    incoh = take(3 * 9600 * 3, np.float64).reshape(3, 9600, 3).transpose(2, 1, 0)
    pw = take(3 * 9600, np.float64).reshape(9600, 3).T                                 # cvectorize: column-major
    fq = take(3 * 9600, np.int64).reshape(9600, 3).T
    assert o == len(raw)
    O.set_threads(8)
    fc = float(g["fc"][0])
    ro = O.xcorr_pss(cap, np.array(f), 2, fc, fc, 1.92e6, want_xc=True, want_sp=True)
    assert np.abs(xc - ro["xc"]).max() < 1e-6                                          # test_xcorr_pss.cpp:105
    assert (np.abs(sp - ro["sp"]) / ro["sp"]).max() < 1e-11 and (np.abs(spi - ro["sp_incoherent"]) / ro["sp_incoherent"]).max() < 1e-11
    assert (np.abs(single - ro["single"]) / ro["single"]).max() < 1e-5 and (np.abs(incoh - ro["incoherent"]) / ro["incoherent"]).max() < 1e-5
    assert (np.abs(pw - ro["pow"]) / ro["pow"]).max() < 1e-5
    assert np.array_equal(fq, ro["frq"])                                               # an integer output: equal (near-ties are repaired, k_frq_repair)


@pytest.mark.gpu
def test_sweep_mixes_byte_exact_and_arbitrary_captures(tmp_path):
    """Three carriers: two recorded (byte-exact -> one int8 batch), one arbitrary complex buffer in between (-> single
    fp32 search).  Output order, duplicate merging across carriers and the table must follow the reference's rules."""
    pkg = load_pkg()
    g = golden("capbuf_0000")
    it = __import__("importlib").import_module("lte_cell_scanner_amd.itfile")
    cap = iq_u8_to_capbuf(g["iq_u8"])
    rng = np.random.default_rng(5)
    arb = 0.05 * (rng.normal(size=153600) + 1j * rng.normal(size=153600))
    it.write_it(str(tmp_path / "capbuf_0000.it"), {"capbuf": cap, "fc": np.array([738900000], np.int32)})
    it.write_it(str(tmp_path / "capbuf_0001.it"), {"capbuf": arb, "fc": np.array([739000000], np.int32)})
    it.write_it(str(tmp_path / "capbuf_0002.it"), {"capbuf": 0.5 * cap, "fc": np.array([739100000], np.int32)})   # not byte-exact any more... half-codes
    r = _run(["-s", "738.9e6", "-e", "739.1e6", "-l", "-d", str(tmp_path)])
    assert r.returncode == 0, r.stderr
    ex = [l for l in r.stdout.splitlines() if l.startswith("Examining")]
    assert ex == ["Examining center frequency 738.9 MHz ...", "Examining center frequency 739 MHz ...", "Examining center frequency 739.1 MHz ..."]
    # the same two cells are seen on carriers 0 and 2 (200 kHz apart: within the 1 MHz merge window); the stronger copy (carrier 0) stays
    table = r.stdout.split("CrystalCorrectionFactor\n")[1].splitlines()
    assert len(table) == 2 and all(re.match(r"^(277|271) 2  738\.9M", l) for l in table), table


@pytest.mark.gpu
def test_sharded_sweep_gives_the_same_report(tmp_path):
    """`-g all` (one thread + two batches in flight per visible GPU, carriers block-cyclic in batches of -B) must print
    exactly what the single-device, single-batch run prints: five carriers, batches of two -> three batches, the
    recorded cells on carriers 0 and 3, a non-byte-exact capture in the middle, noise elsewhere."""
    pkg = load_pkg()
    g = golden("capbuf_0000")
    it = __import__("importlib").import_module("lte_cell_scanner_amd.itfile")
    cap = iq_u8_to_capbuf(g["iq_u8"])
    rng = np.random.default_rng(6)
    noise_u8 = np.clip(np.rint(rng.normal(127.0, 12.0, g["iq_u8"].size)), 0, 255).astype(np.uint8)
    bufs = [cap, iq_u8_to_capbuf(noise_u8), 0.05 * (rng.normal(size=153600) + 1j * rng.normal(size=153600)),
            np.roll(cap, 4000), iq_u8_to_capbuf(noise_u8[::-1].copy())]
    for k, b in enumerate(bufs):
        it.write_it(str(tmp_path / f"capbuf_{k:04d}.it"), {"capbuf": b, "fc": np.array([739000000 + 2000000 * k], np.int32)})
    base = ["-s", "739.0e6", "-e", "739.4e6", "-l", "-d", str(tmp_path)]
    one = _run(base)
    assert one.returncode == 0, one.stderr
    # -g 0,0 / 0,0,0: two / three device threads (two contexts each) on the one GPU -- the block-cyclic batch assignment and
    # the in-order merge of `-g all` on a multi-GPU node (src/CellSearch.cpp:471-569), byte-identical report
    for extra in (["-g", "all", "-B", "2"], ["-g", "0", "-B", "1"], ["--gpu=all", "--batch", "3"], ["-g", "0,0", "-B", "1"],
                  ["-g", "0,0", "-B", "2"], ["--gpu=0,0,0", "-B", "1"]):
        r = _run(base + extra)
        assert r.returncode == 0, r.stderr
        assert r.stdout == one.stdout, (extra, r.stdout, one.stdout)
    assert one.stdout.count("Detected a cell!") == 4 and one.stdout.count("center frequency did not match") == 4
    assert "could not parse gpu index" in _run(base + ["-g", "some"]).stderr
    assert "could not parse gpu index" in _run(base + ["-g", "0,x"]).stderr
    bad = _run(base + ["-g", "0,99"])
    assert bad.returncode == 2 and "GPU(s) are visible" in bad.stderr


@pytest.mark.gpu
def test_stream_search_consumer_loop(tmp_path):
    """host/StreamSearch.cpp: the searcher thread's consumer loop (ref src/searcher_thread.cpp:83-246) in C++ over
    lcs_stream_*: cells found in one buffer are tracked from the next PUSH on (two buffers are in flight, so the buffer
    already launched still reports them once more), noise adds nothing."""
    pkg = load_pkg()
    g = golden("capbuf_0000")
    it = __import__("importlib").import_module("lte_cell_scanner_amd.itfile")
    cap = iq_u8_to_capbuf(g["iq_u8"])
    rng = np.random.default_rng(4)
    noise = iq_u8_to_capbuf(np.clip(np.rint(rng.normal(127.0, 12.0, g["iq_u8"].size)), 0, 255).astype(np.uint8))
    it.write_it(str(tmp_path / "capbuf_0000.it"), {"capbuf": cap, "fc": g["fc"].astype(np.int32)})
    it.write_it(str(tmp_path / "capbuf_0001.it"), {"capbuf": noise, "fc": g["fc"].astype(np.int32)})
    exe = os.path.join(ROOT, "host", "StreamSearch")
    r = subprocess.run([exe, "-f", "35000", "-n", "3", str(tmp_path / "capbuf_0000.it"), str(tmp_path / "capbuf_0001.it")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("buffer ")]
    assert len(lines) == 6
    assert lines[0].startswith("buffer 0: 2 new, 0 tracked") and "[cell 277 ports 2 nRB 50" in lines[0] and "[cell 271 " in lines[0]
    assert lines[1].startswith("buffer 1: 0 new, 0 tracked")
    assert lines[2].startswith("buffer 2: 0 new, 2 tracked")          # pushed after buffer 0 was collected: both cells tracked
    assert lines[4].startswith("buffer 4: 0 new, 2 tracked") and lines[5].startswith("buffer 5: 0 new, 0 tracked")
    assert "tracked: 277 271" in r.stdout
    assert subprocess.run([exe], capture_output=True, text=True).returncode == 2


@pytest.mark.gpu
def test_track_cells_consumer_loop(tmp_path):
    """host/TrackCells.cpp: LTE-Tracker's producer thread and tracker-thread loop in C++ (symbol cutter of
    src/producer_thread.cpp:96-131, 196-246, lcs_track_stream_block, the lcs::track recurrences).  Its per-block figures
    must equal what the Python host side (tracker.cut_symbols, Searcher.track_stream_block, tracker.fold_*) computes from the
    same capture: same cells, same symbols, same measurements, same loops."""
    pkg = load_pkg()
    g = golden("capbuf_0000")
    it = __import__("importlib").import_module("lte_cell_scanner_amd.itfile")
    cap = iq_u8_to_capbuf(g["iq_u8"])
    fc = float(g["fc"][0])
    it.write_it(str(tmp_path / "capbuf_0000.it"), {"capbuf": cap, "fc": g["fc"].astype(np.int32)})
    exe = os.path.join(ROOT, "host", "TrackCells")
    block = 200
    r = subprocess.run([exe, "-b", str(block), str(tmp_path / "capbuf_0000.it")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = [l.split() for l in r.stdout.splitlines() if l.startswith("symbols ")]
    # the same in Python
    FS = 1.92e6
    n_extra = int(np.floor((fc * 120 / 1e6 + 2.5e3) / 5e3))
    f = 5e3 * np.arange(-n_extra, n_extra + 1)
    with pkg.Searcher(0) as S:
        found, _ = S.search_capbuf(cap, f, fc, fc, FS)
        cells = [c for c in found if c.n_rb_dl > 0]
        assert [c.n_id_cell() for c in cells] == [277, 271]
        feeds = []
        for c in cells:
            kf = (fc - c.freq_superfine) / fc
            feeds.append(pkg.tracker.cut_symbols(cap, c.frame_start * (30.72e6 / 16) / (FS * kf), c.cp_type, c.freq_superfine, fc, fc, FS, 10 ** 9))
        n_total = min(fd[0].shape[0] for fd in feeds)
        assert f"tracking 2 cell(s), {n_total} OFDM symbols each, {block} per block" in r.stdout
        f_off = [c.freq_superfine for c in cells]
        f_tim = [fd[2][0] for fd in feeds]
        codes = [[], []]
        want = []
        for s0 in range(0, n_total, block):
            n = min(block, n_total - s0)
            o = S.track_stream_block(cells, np.stack([fd[0][s0:s0 + n] for fd in feeds]), np.stack([fd[3][s0:s0 + n] for fd in feeds]),
                                     np.stack([fd[2][s0:s0 + n] for fd in feeds]), np.stack([fd[1][s0:s0 + n] for fd in feeds]), fc, fc, FS)
            for i in range(2):
                m = o["meas"][i, 0, :o["n_meas"][i, 0]]
                f_off[i] = pkg.tracker.fold_frequency_offset(f_off[i], m)
                f_tim[i] = pkg.tracker.fold_frame_timing(f_tim[i], m)
                codes[i] += list(o["mib_ok"][i, :o["n_mib"][i]])
                fl, sy, at, _ = pkg.tracker.mib_lock_walk(np.array(codes[i], np.int32)) if codes[i] else (0.0, False, 0, False)
                want.append((s0 + n, cells[i].n_id_cell(), f_off[i], f_tim[i], at, fl, "LOCKED" if sy else "searching"))
    assert len(lines) == len(want) and len(want) >= 8
    for l, w in zip(lines, want):
        assert int(l[1]) == w[0] and int(l[3]) == w[1]
        assert abs(float(l[5]) - w[2]) < 1e-5 and abs(float(l[7]) - w[3]) < 1e-5          # printed with 6 decimals
        assert int(l[10]) == w[4] and abs(float(l[12]) - w[5]) < 0.01 and l[13] == w[6]
    assert want[-1][6] == "LOCKED" and want[-2][6] == "LOCKED"          # 80 ms hold four full frames from some offset: both cells lock
    assert subprocess.run([exe], capture_output=True, text=True).returncode == 2
    # -D: the symbols cut ON THE DEVICE (lcs_track_cut through lcs::Searcher::track_cut: the capture uploaded once, [cell][symbol][128]
    # left in HBM, lcs_track_stream_block reading it there) -- the tool checks symbol counts and every `late` against its host cutter
    # and then tracks the whole stream as one block: the same lines as the host-cut run with one block
    one = subprocess.run([exe, "-b", "100000", str(tmp_path / "capbuf_0000.it")], capture_output=True, text=True, timeout=600)
    dev = subprocess.run([exe, "-D", str(tmp_path / "capbuf_0000.it")], capture_output=True, text=True, timeout=600)
    assert one.returncode == 0 and dev.returncode == 0, dev.stderr
    assert f"device cutter: {n_total} symbols of 2 cell(s) in HBM" in dev.stdout
    sym = lambda out: [l for l in out.splitlines() if l.startswith("symbols ")]
    assert len(sym(dev.stdout)) == 2 and sym(dev.stdout) == sym(one.stdout)


@pytest.mark.gpu
def test_track_bench_cxx_driver(tmp_path):
    """host/TrackBench.cpp (the timed loop of `bench.py --stage track`): a small block file through two host threads; every block
    must come back (no failed call) with the MIB locks the Python call finds on the same block."""
    import json
    import struct
    pkg = load_pkg()
    g = golden("capbuf_0000")
    cap = iq_u8_to_capbuf(g["iq_u8"])
    fc, FS = float(g["fc"][0]), 1.92e6
    with pkg.Searcher(0) as S:
        found, _ = S.search_capbuf(cap, np.array([30e3, 35e3, 40e3]), fc, fc, FS)
        per = []
        for c in found:
            kf = (fc - c.freq_superfine) / fc
            per.append(pkg.tracker.cut_symbols(cap, c.frame_start * (30.72e6 / 16) / (FS * kf), c.cp_type, c.freq_superfine, fc, fc, FS, 980))
        cells = [found[i % 2] for i in range(4)]
        td = np.stack([per[i % 2][0] for i in range(4)]); late = np.stack([per[i % 2][1] for i in range(4)])
        ftv = np.stack([per[i % 2][2] for i in range(4)]); fov = np.stack([per[i % 2][3] for i in range(4)])
        want = int(np.count_nonzero(S.track_block(cells, td, fov, ftv, late, fc, fc, FS, want_syms=False, want_ce=False)["mib_ok"] == 3))
    tc = (pkg.capi.LcsTrackCell * 4)()
    for i, c in enumerate(cells):
        for fld in ("n_id_1", "n_id_2", "cp_type", "n_ports", "n_rb_dl", "phich_duration", "phich_resource"):
            setattr(tc[i], fld, int(getattr(c, fld)))
    blk = tmp_path / "block.trkblock"
    with open(blk, "wb") as fh:
        fh.write(struct.pack("<ii3d", 4, 980, fc, fc, FS))
        fh.write(bytes(tc))
        for a in (fov, ftv, late):
            fh.write(np.ascontiguousarray(a, np.float64).tobytes())
        fh.write(np.ascontiguousarray(td, np.complex128).tobytes())
    r = subprocess.run([os.path.join(ROOT, "host", "TrackBench"), str(blk), "2", "6", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j["blocks"] == 6 and j["failed"] == 0 and j["contexts"] == 2 and j["mib_locks_per_block"] == want and want >= 4
    assert j["symbols_per_s"] > 0 and j["gpu_ms_per_block_alone"] > 0 and j["from_bytes"] is False
    # every block STARTING FROM THE DONGLE'S BYTES: lcs_track_cut on the capture in HBM, then the block on the symbols it left there --
    # the same locks, and the cutter's `late` equal to the block file's (the host cutter's) bit for bit
    capf = tmp_path / "capture.u8"
    capf.write_bytes(np.ascontiguousarray(g["iq_u8"]).tobytes())
    r = subprocess.run([os.path.join(ROOT, "host", "TrackBench"), str(blk), "2", "6", "2", "0", str(capf)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j["blocks"] == 6 and j["failed"] == 0 and j["from_bytes"] is True and j["late_identical_to_host_cut"] is True
    assert j["mib_locks_per_block"] == want
    assert subprocess.run([os.path.join(ROOT, "host", "TrackBench")], capture_output=True, text=True).returncode == 2
