"""World size 8 before the hardware sees it: every multi-rank driver run with EIGHT ranks on the one GPU a test box has
(gloo for the collectives, `--share-gpu0`): rank arithmetic of the carrier shard (rank 7's carriers), the shape of the
per-step record all-gather (8 x (1 + 5 MAXREC)), the per-rank identity check, eight per-rank rates; the sweep tool's table at
world 8 equal to world 1; host/CellSearch with eight device threads byte-identical to one.  No scaling curve comes from
this -- the eight ranks share one GPU -- it is the logic that an 8-GPU node then only has to run faster."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden, iq_u8_to_capbuf, load_pkg

pytestmark = pytest.mark.gpu

ENV = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
ENV.update(MASTER_ADDR="127.0.0.1", GPU_MAX_HW_QUEUES="8", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")


def _json_line(stdout):
    return json.loads([l for l in stdout.splitlines() if l.startswith("{")][-1])


def test_bench_world_8_on_one_gpu():
    """`python bench.py --gpus 8` starts eight ranks itself; every rank owns its carriers FC + 100 kHz * (r B + b), keeps two
    batches in flight, packs its step's records, and the asynchronous all-gather brings 8 x (1 + 5 MAXREC) doubles to everyone."""
    B, K, steps = 8, 2, 2
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--share-gpu0", "--dist-backend", "gloo", "--steps", str(steps),
                        "--warmup", "1", "--batch", str(B), "--batches-per-step", str(K), "--full", "--no-cpu-baseline", "--no-dense", "--no-power-probe"],
                       env=dict(ENV, MASTER_PORT="29571"), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                            # rank 0 alone prints
    j = json.loads(lines[0])
    c = j["config"]
    assert j["n_gpus"] == 8 and j["verified"] is True and j["scaling"] == "weak"
    assert len(c["per_rank_buffers_per_s"]) == 8 and len(c["devices"]) == 8
    assert c["buffers_timed"] == 8 * B * K * steps
    assert j["value"] <= sum(c["per_rank_buffers_per_s"]) * 1.001    # whole job / the slowest rank's time
    coll = c["collectives"]
    assert coll["world"] == 8 and coll["backend"] == "gloo" and len(coll["gathered_records_last_step"]) == 8
    maxrec = max(64, B) * K
    assert coll["gather_out_shape"] == [8, 1 + 5 * maxrec]
    # every rank found its planted cells (buffer 0 of every batch of 8 is occupied) and names only its own carriers
    FC = 739e6
    for rank, (n, rng) in enumerate(zip(coll["gathered_records_last_step"], coll["gathered_fc_min_max_per_rank"])):
        assert n >= K, (rank, n)
        lo, hi = FC + 100e3 * rank * B, FC + 100e3 * (rank * B + B - 1)
        assert lo <= rng[0] <= rng[1] <= hi, (rank, rng, lo, hi)
    assert coll["gathered_fc_min_max_per_rank"][7][0] >= FC + 100e3 * 56


def test_sweep_tool_world_8_equals_world_1():
    """tools/sweep_cellsearch.py over 24 carriers: eight ranks of three carriers each (block-cyclic), one all-gather of the
    raw records, the merged table equal to the single-rank table."""
    tool = os.path.join(ROOT, "tools", "sweep_cellsearch.py")
    args = ["-s", "738e6", "-e", "740.3e6", "--occupied-every", "5", "--json"]
    a = subprocess.run([sys.executable, tool] + args, env=ENV, capture_output=True, text=True, timeout=900)
    assert a.returncode == 0, a.stderr[-2000:]
    b = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=8", "--master-addr", "127.0.0.1",
                        "--master-port", "29573", tool] + args + ["--share-gpu0", "--dist-backend", "gloo"], env=ENV,
                       capture_output=True, text=True, timeout=1500)
    assert b.returncode == 0, b.stderr[-2000:]
    ja, jb = _json_line(a.stdout), _json_line(b.stdout)
    assert ja["cells"] == jb["cells"] and ja["carriers"] == jb["carriers"] == 24 and len(ja["cells"]) >= 3
    assert jb["n_gpus"] == 8 and ja["n_gpus"] == 1


def test_cellsearch_cli_eight_device_threads(tmp_path):
    """host/CellSearch -g 0,0,0,0,0,0,0,0: eight device threads (two contexts each) share the one GPU; batches go to them
    block-cyclically and the report must be byte-identical to -g 0."""
    pkg = load_pkg()
    it = __import__("importlib").import_module("lte_cell_scanner_amd.itfile")
    g = golden("capbuf_0000")
    cap = iq_u8_to_capbuf(g["iq_u8"])
    rng = np.random.default_rng(8)
    fc0 = int(g["fc"][0])
    n = 18
    for k in range(n):                     # carriers 2, 9, 16 hold the recorded capture, the rest noise: more batches (-B 1) than threads
        if k % 7 == 2:
            buf = cap
        else:
            buf = iq_u8_to_capbuf(np.clip(np.rint(rng.normal(127.0, 12.0, g["iq_u8"].size)), 0, 255).astype(np.uint8))
        it.write_it(str(tmp_path / f"capbuf_{k:04d}.it"), {"capbuf": buf, "fc": np.array([fc0 + 100000 * (k - 2)], np.int32)})
    exe = os.path.join(ROOT, "host", "CellSearch")
    base = [exe, "-s", str(fc0 - 200000), "-e", str(fc0 + 100000 * (n - 3)), "-l", "-d", str(tmp_path)]
    one = subprocess.run(base + ["-g", "0", "-B", "1"], capture_output=True, text=True, timeout=900)
    assert one.returncode == 0, one.stderr[-2000:]
    eight = subprocess.run(base + ["-g", "0,0,0,0,0,0,0,0", "-B", "1"], capture_output=True, text=True, timeout=1500)
    assert eight.returncode == 0, eight.stderr[-2000:]
    assert one.stdout == eight.stdout and "277" in one.stdout and "271" in one.stdout


def test_contexts_give_their_memory_back():
    """Twelve contexts created, driven through differently shaped calls (single buffers, batches as bytes and floats with the probe on, a wide
    grid, the streaming graph, tracker block + cutter) and destroyed: the device's free memory returns to where it was -- every buffer a
    context grows (per-cell stages, operand tables, tracker / cutter workspaces, the float-batch bytes, graphs) goes with it."""
    import numpy as np
    import torch
    from conftest import golden, iq_u8_to_capbuf, f_search_set_for, load_pkg
    pkg = load_pkg()
    iq = golden("capbuf_0000")["iq_u8"]
    cap = iq_u8_to_capbuf(iq)
    FC, FS = 739e6, 1.92e6
    d8 = torch.from_numpy(np.ascontiguousarray(np.stack([iq] * 6))).cuda()
    d32 = torch.from_numpy(np.stack([cap.astype(np.complex64)] * 6)).cuda()
    td = torch.empty((2, 300, 128), dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()

    def one(k):
        with pkg.Searcher(0) as S:
            f = f_search_set_for(FC, 100) if k % 3 else f_search_set_for(2.6e9, 120)
            fcs = np.full(6, FC)
            if k % 2:
                S.set_float_batch_probe(True)
            S.search_batch(d8.data_ptr(), pkg.FMT_IQ_U8, 6, 153600, f, fcs, fcs, FS, pkg.STAGE_FULL)
            S.search_batch(d32.data_ptr(), pkg.FMT_C64, 3 + k % 3, 153600, f, fcs[:3 + k % 3], fcs[:3 + k % 3], FS, pkg.STAGE_FULL)
            cells, _ = S.search_capbuf(cap[:153600 - 1000 * k], np.array([30e3, 35e3, 40e3]), FC, FC, FS)
            S.stream_open(pkg.FMT_IQ_U8, 153600, FC, FC, FS)
            S.stream_push(iq, 35e3)
            S.stream_collect()
            S.stream_close()
            tr = [c for c in cells if c.n_rb_dl > 0][:2]
            if len(tr) == 2:
                late, n_cut = S.track_cut(d8.data_ptr(), pkg.FMT_IQ_U8, 153600, [c.cp_type for c in tr], [100.0, 7000.5], [c.freq_superfine for c in tr], FC, FC, FS,
                                          300, td.data_ptr())
                S.track_block(tr, None, np.zeros((2, 300)) + 35e3, np.zeros((2, 300)), late, FC, FC, FS, td_device_ptr=td.data_ptr(), n_sym=300, want_ce=False)

    one(0)                                  # first use pays for one-off allocations of the runtime itself
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for k in range(1, 13):
        one(k)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert abs(free1 - free0) < 64 << 20, (free0, free1)


def context_lifetime_cycles(n_cycles=8):
    """One warm-up cycle (the runtime's own lazy allocations), then n_cycles more, each a context's whole life: create; a u8 batch; a larger
    complex<float> batch (the workspace, the fp16 set and the result block grow); one host buffer through lcs_search_capbuf; lcs_stream_open /
    push / collect / lcs_stream_close; one channelizer call; one small tracker block; destroy.  Returns every reading of the device's free
    memory taken on the way (one after each entry point of each cycle) and the readings before and after the n_cycles."""
    import torch
    from conftest import f_search_set_for
    pkg = load_pkg()
    iq = golden("capbuf_0000")["iq_u8"]
    cap = iq_u8_to_capbuf(iq)
    FC, FS = 739e6, 1.92e6
    f = f_search_set_for(FC, 100)
    d8 = torch.from_numpy(np.ascontiguousarray(np.stack([iq] * 4))).cuda()
    d32 = torch.from_numpy(np.stack([cap.astype(np.complex64)] * 8)).cuda()
    n_out, D, n_ch = 256, 8, 40
    d_wide = torch.zeros((n_out - 1) * D + 16 * D, dtype=torch.complex64, device="cuda")
    d_nb = torch.zeros((n_ch, n_out), dtype=torch.complex64, device="cuda")
    rng = np.random.default_rng(5)
    n_sym = 280
    td = 0.1 * (rng.standard_normal((1, n_sym, 128)) + 1j * rng.standard_normal((1, n_sym, 128)))
    tracked = pkg.new_cell(n_id_1=92, n_id_2=1, cp_type=1, n_ports=2, n_rb_dl=6, phich_duration=1, phich_resource=1)
    torch.cuda.synchronize()
    readings = []

    def free():
        torch.cuda.synchronize()
        readings.append(torch.cuda.mem_get_info()[0])
        return readings[-1]

    def one():
        with pkg.Searcher(0) as S:
            S.search_batch(d8.data_ptr(), pkg.FMT_IQ_U8, 4, 153600, f[:9], np.full(4, FC), np.full(4, FC), FS, pkg.STAGE_FULL)
            free()
            S.search_batch(d32.data_ptr(), pkg.FMT_C64, 8, 153600, f, np.full(8, FC), np.full(8, FC), FS, pkg.STAGE_FULL)
            free()
            S.search_capbuf(cap, np.array([30e3, 35e3, 40e3]), FC, FC, FS)
            free()
            S.stream_open(pkg.FMT_IQ_U8, 153600, FC, FC, FS)
            S.stream_push(iq, 35e3)
            S.stream_collect()
            S.stream_close()
            free()
            S.channelize(d_wide.data_ptr(), pkg.FMT_C64, d_wide.numel(), D * FS, D, np.linspace(-0.4, 0.4, n_ch) * D * FS, d_nb.data_ptr(), n_out)
            free()
            S.track_block([tracked], td, np.full((1, n_sym), 35e3), np.zeros((1, n_sym)), np.zeros((1, n_sym)), FC, FC, FS, want_ce=False)
            free()
        free()

    one()
    free0 = free()
    for _ in range(n_cycles):
        one()
    return readings, free0, free()


# What context_lifetime_cycles measured at the commit before the context's memory got its owning type (hand-written free lists in
# lcs_destroy, lcs_stream_close, the channelizer's map): free memory lost over the 8 cycles, and the allocation granule -- the smallest
# non-zero step between two consecutive readings of that run (free memory stood at 308352647168 bytes before and after the 8 cycles).
LIFETIME_DRIFT_BEFORE = 0
LIFETIME_GRANULE = 2 << 20


def test_context_lifetime_leaves_no_memory_behind():
    """Eight whole context lifetimes (context_lifetime_cycles) lose no more of the device's free memory than they did when every buffer
    was freed by hand, plus one allocation granule: a buffer that a context fails to give back shows up eight times over."""
    readings, free0, free1 = context_lifetime_cycles(8)
    drift = free0 - free1
    steps = sorted({abs(b - a) for a, b in zip(readings, readings[1:])} - {0})
    print(f"lifetime: drift over 8 cycles {drift} bytes; smallest step of free memory {steps[0] if steps else None}; free0 {free0} free1 {free1}")
    assert drift <= LIFETIME_DRIFT_BEFORE + LIFETIME_GRANULE, (drift, free0, free1)


def test_results_do_not_depend_on_what_a_context_ran_before():
    """History independence.  The records of search_capbuf on the golden capture, of a streamed push of the same buffer and of a small
    u8 batch, each taken on a fresh context, equal -- field for field, bit for bit -- the records of the same three calls made on ONE
    context that has first run a dense batch three times (576 cells past SSS: the first collect launches the late per-cell rounds, the
    second enqueue doubles the cells per round and widens the per-cell grids), a complex<float> batch and extract_tfg.  Whatever a
    launch depends on is an argument of that launch; what a context keeps from earlier calls (capacities, hints) changes no result."""
    import torch
    from conftest import f_search_set_for
    pkg = load_pkg()
    iq = golden("capbuf_0000")["iq_u8"]
    cap = iq_u8_to_capbuf(iq)
    FC, FS = 739e6, 1.92e6
    f = f_search_set_for(FC, 100)
    n_dense = 288
    small = np.ascontiguousarray(np.stack([iq, np.roll(iq, 2 * 4321), iq]))
    d_small = torch.from_numpy(small).cuda()
    d_dense = torch.from_numpy(np.ascontiguousarray(np.stack([iq] * n_dense))).cuda()
    d32 = torch.from_numpy(np.stack([cap.astype(np.complex64)] * 8)).cuda()
    torch.cuda.synchronize()
    raw = lambda cells: [bytes(c) for c in cells]

    def capbuf_records(S):
        cells, peaks = S.search_capbuf(cap, f, FC, FC, FS)
        return raw(cells), raw(peaks)

    def stream_records(S):
        S.stream_open(pkg.FMT_IQ_U8, 153600, FC, FC, FS)
        S.stream_push(iq, 35e3)
        cells, again, _ms = S.stream_collect()
        S.stream_close()
        return raw(cells), again

    def batch_records(S):
        return [raw(b) for b in S.search_batch(d_small.data_ptr(), pkg.FMT_IQ_U8, 3, 153600, f, np.full(3, FC), np.full(3, FC), FS, pkg.STAGE_FULL)]

    takes = (capbuf_records, stream_records, batch_records)
    fresh = []
    for take in takes:
        with pkg.Searcher(0) as S:
            fresh.append(take(S))
    first = pkg.LcsCell.from_buffer_copy(fresh[0][0][0])
    with pkg.Searcher(0) as S:
        for _ in range(3):
            dense = S.search_batch(d_dense.data_ptr(), pkg.FMT_IQ_U8, n_dense, 153600, f, np.full(n_dense, FC), np.full(n_dense, FC), FS, pkg.STAGE_FULL)
            assert S.last_batch_stats()["cells_past_sss"] > 512, S.last_batch_stats()      # more than a round of a fresh context holds
        S.search_batch(d32.data_ptr(), pkg.FMT_C64, 8, 153600, f, np.full(8, FC), np.full(8, FC), FS, pkg.STAGE_FULL)
        S.extract_tfg(first, cap, FC, FC, FS)
        used = [take(S) for take in takes]
    assert all([c.n_id_cell() for c in b] == [277, 271] for b in dense)
    assert len(fresh[0][0]) == 2 and len(fresh[1][0]) == 2 and len(fresh[2][0]) == len(fresh[2][2]) == 2
    for name, a, b in zip(("search_capbuf", "stream", "batch"), fresh, used):
        assert a == b, name


def test_saved_launches_outlive_the_stream_and_not_the_workspace():
    """What a later call continues is a saved copy of the launch.  (a) lcs_foe_partial and (b) a batch whose per-cell rounds are
    finished by lcs_batch_collect, both begun while a stream is open and ended after lcs_stream_close -- which frees the tracked
    list the open stream lent them: the records equal those of the same calls on a context that never had a stream.  (c) A call that
    replaces the workspace ends the last batch: lcs_batch_collect and lcs_batch_readback refuse instead of reading the new buffers."""
    import torch
    from conftest import f_search_set_for
    pkg = load_pkg()
    iq = golden("capbuf_0000")["iq_u8"]
    cap = iq_u8_to_capbuf(iq)
    FC, FS = 739e6, 1.92e6
    f = f_search_set_for(FC, 100)
    d3 = torch.from_numpy(np.ascontiguousarray(np.stack([iq] * 3))).cuda()
    words = torch.empty(3 * 9600, dtype=torch.int64, device="cuda")
    meta = torch.empty(9601, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    raw = lambda cells: [bytes(c) for c in cells]

    def run(S, with_stream):
        # an open stream's graph holds the workspace's addresses: size it first for everything that follows (no cell count is learnt
        # from a PSS-only batch, so the full batch below enqueues one round per buffer)
        S.search_batch(d3.data_ptr(), pkg.FMT_IQ_U8, 3, 153600, f, FC, FC, FS, pkg.STAGE_PSS)
        S.search_capbuf(cap, f, FC, FC, FS)
        if with_stream:
            S.stream_open(pkg.FMT_IQ_U8, 153600, FC, FC, FS)
        S.foe_partial(cap, f, 0, f.size, FC, FC, FS, words.data_ptr(), meta.data_ptr())
        if with_stream:
            S.stream_close()
        cells, order, peaks = S.foe_finish(words.data_ptr(), meta.data_ptr(), f)
        S.set_max_cells_in_flight(1)      # 3 rounds enqueued for 6 cells past SSS: the collect launches the rest
        if with_stream:
            S.stream_open(pkg.FMT_IQ_U8, 153600, FC, FC, FS)
        S.batch_enqueue(d3.data_ptr(), pkg.FMT_IQ_U8, 3, 153600, f, FC, FC, FS, pkg.STAGE_FULL)
        if with_stream:
            S.stream_close()
        batch = S.batch_collect(3)
        assert S.last_batch_stats()["cells_past_sss"] > 3
        return raw(cells), order.tolist(), raw(peaks), [raw(b) for b in batch]

    with pkg.Searcher(0) as S:
        want = run(S, False)
    with pkg.Searcher(0) as S:
        got = run(S, True)
        assert got == want
        assert len(want[0]) == 2 and all(len(b) == 2 for b in want[3])
        # (c) a longer grid replaces the workspace under the collected batch
        S.batch_enqueue(d3.data_ptr(), pkg.FMT_IQ_U8, 3, 153600, f, FC, FC, FS, pkg.STAGE_FULL)
        S.search_capbuf(cap, f_search_set_for(2.6e9, 120), FC, FC, FS)
        with pytest.raises(pkg.SearcherError):
            S.batch_collect(3)
        with pytest.raises(pkg.SearcherError):
            S.batch_readback(0, f.size)


def test_searcher_and_tracker_contexts_side_by_side_from_two_threads():
    """A searcher context (full-chain batches) and a tracker context (cutter + block) driven from two host threads at once -- the shape of
    LTE-Tracker's searcher and tracker threads on one GPU: every result identical to the same calls made alone."""
    import threading
    import numpy as np
    import torch
    from conftest import golden, iq_u8_to_capbuf, f_search_set_for, load_pkg
    pkg = load_pkg()
    iq = golden("capbuf_0000")["iq_u8"]
    cap = iq_u8_to_capbuf(iq)
    FC, FS = 739e6, 1.92e6
    f = f_search_set_for(FC, 100)
    fcs = np.full(8, FC)
    d8 = torch.from_numpy(np.ascontiguousarray(np.stack([np.roll(iq, 2 * 1000 * k) for k in range(8)]))).cuda()
    td = torch.empty((2, 600, 128), dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()
    with pkg.Searcher(0) as A, pkg.Searcher(0) as B:
        cells, _ = A.search_capbuf(cap, np.array([30e3, 35e3, 40e3]), FC, FC, FS)
        tr = [c for c in cells if c.n_rb_dl > 0]
        assert len(tr) == 2
        fts = [c.frame_start * (30.72e6 / 16) / (FS * ((FC - c.freq_superfine) / FC)) for c in tr]
        fos = [c.freq_superfine for c in tr]

        def search():
            r = A.search_batch(d8.data_ptr(), pkg.FMT_IQ_U8, 8, 153600, f, fcs, fcs, FS, pkg.STAGE_FULL)
            return [[bytes(c) for c in b] for b in r]

        def track():
            late, n_cut = B.track_cut(d8.data_ptr(), pkg.FMT_IQ_U8, 153600, [c.cp_type for c in tr], fts, fos, FC, FC, FS, 600, td.data_ptr())
            o = B.track_block(tr, None, np.repeat(np.array(fos)[:, None], 600, 1), np.repeat(np.array(fts)[:, None], 600, 1), late, FC, FC, FS,
                              td_device_ptr=td.data_ptr(), n_sym=600, want_ce=False)
            return late.tobytes(), o["syms"].tobytes(), o["mib_ok"].tobytes(), o["meas"][:, :2, :100].tobytes()

        want_s, want_t = search(), track()
        got = {"s": [], "t": []}
        ts = [threading.Thread(target=lambda: got["s"].extend(search() for _ in range(20))), threading.Thread(target=lambda: got["t"].extend(track() for _ in range(40)))]
        for t in ts: t.start()
        for t in ts: t.join()
        assert len(got["s"]) == 20 and all(x == want_s for x in got["s"])
        assert len(got["t"]) == 40 and all(x == want_t for x in got["t"])
        assert sum(len(b) for b in want_s) >= 8
