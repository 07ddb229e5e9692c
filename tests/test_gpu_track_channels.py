"""The tracker block on cells that went through a RADIO CHANNEL.

tests/test_tracker.py runs lcs_track_block on the two cells of the reference's recorded capture (both normal CP, two ports, a
static channel) and tests/test_gpu_configs.py on one synthetic pair behind flat gains.  The stages of src/tracker_thread.cpp
that a frequency-selective, time-varying channel stresses -- filter_ce's 12-tap rows and its power / FOE / TOE measurements
(:176-288), interp2d between reference symbols that differ (:318-371), the SFBC combining of pbch_extract_rt on four ports --
see such a channel here: per (cell, antenna port) an independent Rayleigh tapped delay line (EPA / EVA / ETU of 36.101 B.2)
with Jakes Doppler 5 / 70 / 300 Hz, plus the zero-IF front end's DC spike and I/Q imbalance (lte-cell-scanner_amd/synth.py),
1 / 2 / 4 ports, both CP types, dongle parameters on two of the captures.  Every output array of the block against the oracle
(oracle/lcs_oracle.c: trk_get_fd / trk_chan_est / trk_mib)."""
import os

import numpy as np
import pytest

import oracle as O
from conftest import golden, iq_u8_to_capbuf, load_pkg

pytestmark = pytest.mark.gpu
FS, FC = 1.92e6, 739e6

#        n_id_1 n_id_2 cp_normal ports n_rb  channel doppler f_off    front end                                   dongle
SCENES = [(17, 0, True, 1, 6, "EPA", 5.0, 12.3e3, None, False),
          (101, 1, True, 2, 50, "EVA", 70.0, -31.0e3, dict(dc=0.2 - 0.1j), False),
          (160, 2, True, 4, 100, "ETU", 300.0, 4.4e3, dict(iq_gain_db=0.5, iq_phase_deg=3.0), True),
          (54, 1, False, 2, 25, "ETU", 70.0, -18.7e3, None, False),
          (7, 2, False, 4, 15, "EVA", 300.0, 27.1e3, dict(dc=-0.1 + 0.3j, iq_gain_db=-0.4, iq_phase_deg=-2.0), True),
          (88, 0, False, 1, 75, "EPA", 300.0, -2.0e3, None, False)]


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def blocks(pkg):
    """Per scene: (searcher record of the planted cell, its symbols as the producer cuts them, the capture's parameters)."""
    O.set_legacy(False)
    O.set_threads(min(16, os.cpu_count() or 1))
    out = []
    for k, (n1, n2, cpn, ports, nrb, chan, dop, f_off, fe, dongle) in enumerate(SCENES):
        fcp = FC * (1 + 13e-6) if dongle else FC
        fsp = FS * (1 - 21e-6) if dongle else FS
        cell = dict(n_id_1=n1, n_id_2=n2, cp_normal=cpn, n_ports=ports, n_rb_dl=nrb, f_off=f_off, t0=900.0 + 777.7 * k, channel=chan, doppler_hz=dop)
        iq, _ = pkg.synth.make_capbuf(9100 + k, FC, [cell], 12.0, fc_programmed=fcp, fs_programmed=fsp, front_end=fe)
        cap = iq_u8_to_capbuf(iq)
        f = 5e3 * np.round(f_off / 5e3) + 5e3 * np.arange(-1, 2)
        found = [c for c in O.search_capbuf(cap, f, FC, fcp, fsp)[0] if c.n_id_cell() == 3 * n1 + n2]
        assert len(found) == 1 and found[0].n_ports == ports and found[0].cp_type == (1 if cpn else 2), (k, chan, dop)
        c = found[0]
        k_factor = (FC - c.freq_superfine) / fcp
        ft = c.frame_start * (30.72e6 / 16) / (fsp * k_factor)                       # src/searcher_thread.cpp:224
        per_frame = 140 if cpn else 120
        td, late, ftv, fov = pkg.tracker.cut_symbols(cap, ft, c.cp_type, c.freq_superfine, FC, fcp, fsp, 7 * per_frame)
        out.append(dict(c=c, td=td, late=late, ftv=ftv, fov=fov, fcp=fcp, fsp=fsp, per_frame=per_frame, tag=f"scene {k} ({chan}, {dop:.0f} Hz, {ports} ports)"))
    return out


def _oracle_block(b):
    c = b["c"]
    syms, bpo, _ = O.trk_get_fd(c, b["td"], 0, 0, b["fov"], b["late"], FC, b["fcp"], b["fsp"])
    r = O.trk_chan_est(c, syms, 0, 0, b["fov"], b["ftv"], FC, b["fcp"], b["fsp"])
    r.update(syms=syms, bpo=bpo)
    per_frame, nsd = b["per_frame"], b["per_frame"] // 20
    upto = int(min(r["ce_upto"][:c.n_ports]))
    mib = []
    for o in range(b["td"].shape[0] // per_frame - 3):
        ii = [(o + fr) * per_frame + nsd + s for fr in range(4) for s in range(4)]
        mib.append(None if ii[-1] >= upto else O.trk_mib(c, syms[ii], r["ce"][:c.n_ports][:, ii], r["ce_pw"][:c.n_ports][:, ii, 3]))
    r["mib"] = mib
    return r


def test_track_block_on_fading_channels_matches_oracle(pkg, blocks):
    locks = 0
    with pkg.Searcher(0) as S:
        for b in blocks:
            c, tag = b["c"], b["tag"]
            g = S.track_block([c], b["td"], b["fov"], b["ftv"], b["late"], FC, b["fcp"], b["fsp"])
            r = _oracle_block(b)
            assert np.abs(g["syms"][0] - r["syms"]).max() < 1e-11 * np.abs(r["syms"]).max(), tag
            assert abs(g["bpo"][0] - r["bpo"]) < 1e-9, tag
            assert np.array_equal(g["n_meas"][0], r["n_meas"]) and np.array_equal(g["ce_upto"][0], r["ce_upto"]), tag
            for p in range(c.n_ports):
                n = r["n_meas"][p]
                gm, om = g["meas"][0, p, :n], r["meas"][p, :n]
                assert np.array_equal(gm[:, 0], om[:, 0]), (tag, p)
                assert np.abs(gm[:, 1:5] - om[:, 1:5]).max() < 1e-11 * om[:, 2].max(), (tag, p)
                assert np.abs(gm[:, 5] - om[:, 5]).max() < 1e-6 and np.abs(gm[:, 7] - om[:, 7]).max() < 1e-8, (tag, p)       # Hz, samples
                u = r["ce_upto"][p]
                assert np.abs(g["ce"][0, p, :u] - r["ce"][p, :u]).max() < 1e-11 * np.abs(r["ce"][p, :u]).max(), (tag, p)
                assert np.abs(g["ce_pw"][0, p, :u] - r["ce_pw"][p, :u]).max() < 1e-11 * np.abs(r["ce_pw"][p, :u]).max(), (tag, p)
            for o, m in enumerate(r["mib"]):
                if m is None:
                    assert g["mib_ok"][0, o] == -1, (tag, o)
                    continue
                assert g["mib_ok"][0, o] == (1 if m[1] else 0) | (2 if m[2] else 0), (tag, o)
                assert [(int(g["mib_bits"][0, o]) >> k) & 1 for k in range(40)] == list(m[0]), (tag, o)
                locks += int(g["mib_ok"][0, o] == 3)
    # the channel really varied: the fast scenes lose some decodes, the slow ones must lock
    assert locks >= 3


def test_track_block_of_all_scenes_in_one_call_equals_the_single_calls(pkg, blocks):
    """Two normal-CP scenes in ONE call (a 1-port and a 2-port cell side by side), then two extended-CP ones: the rows of each
    cell are those of its own call, bit for bit -- no cell's channel leaks into another's chunk of k_trk_ce."""
    with pkg.Searcher(0) as S:
        for per_frame in (140, 120):
            grp = [b for b in blocks if b["per_frame"] == per_frame and b["fcp"] == FC]
            assert len(grp) == 2
            both = S.track_block([b["c"] for b in grp], np.stack([b["td"] for b in grp]), np.stack([b["fov"] for b in grp]),
                                 np.stack([b["ftv"] for b in grp]), np.stack([b["late"] for b in grp]), FC, FC, FS)
            for i, b in enumerate(grp):
                one = S.track_block([b["c"]], b["td"], b["fov"], b["ftv"], b["late"], FC, FC, FS)
                tag = b["tag"]
                assert np.array_equal(both["syms"][i], one["syms"][0]) and both["bpo"][i] == one["bpo"][0], tag
                assert np.array_equal(both["n_meas"][i], one["n_meas"][0]) and np.array_equal(both["ce_upto"][i], one["ce_upto"][0]), tag
                assert np.array_equal(both["mib_ok"][i], one["mib_ok"][0]), tag
                ok = one["mib_ok"][0] >= 0
                assert np.array_equal(both["mib_bits"][i][ok], one["mib_bits"][0][ok]), tag
                for p in range(b["c"].n_ports):
                    n, u = one["n_meas"][0][p], one["ce_upto"][0][p]
                    assert np.array_equal(both["meas"][i, p, :n], one["meas"][0, p, :n]), (tag, p)
                    assert np.array_equal(both["ce"][i, p, :u], one["ce"][0, p, :u]), (tag, p)
                    assert np.array_equal(both["ce_pw"][i, p, :u], one["ce_pw"][0, p, :u]), (tag, p)


@pytest.mark.parametrize("n_sym", [1, 6, 7, 121, 139, 140, 141, 500, 839])
def test_track_block_of_any_length_with_both_cp_types_in_one_call(pkg, blocks, n_sym):
    """Blocks that are not a whole number of frames -- one symbol, one slot less a symbol, a frame plus one -- and a normal-CP and an
    extended-CP cell (140 / 120 symbols per frame: different reference-symbol lists, different numbers of PBCH offsets) in ONE call:
    every array of each cell against the oracle on its own truncated block."""
    grp = [blocks[1], blocks[3]]                       # EVA 70 Hz 2 ports normal CP; ETU 70 Hz 2 ports extended CP (both nominal parameters)
    assert grp[0]["per_frame"] == 140 and grp[1]["per_frame"] == 120 and grp[0]["fcp"] == FC and grp[1]["fcp"] == FC
    cut = [dict(b, td=b["td"][:n_sym], late=b["late"][:n_sym], ftv=b["ftv"][:n_sym], fov=b["fov"][:n_sym]) for b in grp]
    with pkg.Searcher(0) as S:
        g = S.track_block([b["c"] for b in cut], np.stack([b["td"] for b in cut]), np.stack([b["fov"] for b in cut]), np.stack([b["ftv"] for b in cut]),
                          np.stack([b["late"] for b in cut]), FC, FC, FS)
    for i, b in enumerate(cut):
        r = _oracle_block(b)
        tag = (n_sym, b["tag"])
        assert np.abs(g["syms"][i] - r["syms"]).max() < 1e-11 * np.abs(r["syms"]).max(), tag
        assert abs(g["bpo"][i] - r["bpo"]) < 1e-9, tag
        assert np.array_equal(g["n_meas"][i], r["n_meas"]) and np.array_equal(g["ce_upto"][i], r["ce_upto"]), (tag, g["n_meas"][i], r["n_meas"], g["ce_upto"][i], r["ce_upto"])
        for p in range(b["c"].n_ports):
            n, u = r["n_meas"][p], r["ce_upto"][p]
            if n:
                gm, om = g["meas"][i, p, :n], r["meas"][p, :n]
                assert np.array_equal(gm[:, 0], om[:, 0]) and np.abs(gm[:, 1:5] - om[:, 1:5]).max() < 1e-11 * om[:, 2].max(), (tag, p)
                assert np.abs(gm[:, 5] - om[:, 5]).max() < 1e-6 and np.abs(gm[:, 7] - om[:, 7]).max() < 1e-8, (tag, p)
            if u:
                assert np.abs(g["ce"][i, p, :u] - r["ce"][p, :u]).max() < 1e-11 * np.abs(r["ce"][p, :u]).max(), (tag, p)
        # a frame offset is attempted as soon as the block holds the PBCH symbols of its four frames and their channel estimates --
        # the fourth frame need not be complete (the reference decodes when the fourth frame's PBCH symbols have arrived,
        # src/tracker_thread.cpp:552-745)
        per_frame, nsd = b["per_frame"], b["per_frame"] // 20
        upto = int(min(r["ce_upto"][:b["c"].n_ports]))
        for o in range(g["mib_ok"].shape[1]):
            ii = [(o + fr) * per_frame + nsd + s for fr in range(4) for s in range(4)]
            if ii[-1] >= upto:
                assert g["mib_ok"][i, o] == -1, (tag, o)
                continue
            m = O.trk_mib(b["c"], r["syms"][ii], r["ce"][:b["c"].n_ports][:, ii], r["ce_pw"][:b["c"].n_ports][:, ii, 3])
            assert g["mib_ok"][i, o] == (1 if m[1] else 0) | (2 if m[2] else 0), (tag, o)
            assert [(int(g["mib_bits"][i, o]) >> k) & 1 for k in range(40)] == list(m[0]), (tag, o)


def _same(a, b):
    """bit for bit, NaNs included"""
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _assert_block_and_stats_equal(got, want, gst, wst, cells, tag):
    """every array lcs_track_block and lcs_track_stats define for the block, over the rows they define"""
    for key in ("syms", "bpo", "n_meas", "ce_upto", "mib_ok", "n_hf"):
        a, b = (gst, wst) if key == "n_hf" else (got, want)
        assert _same(a[key], b[key]), (tag, key)
    ok = want["mib_ok"] >= 0
    assert _same(got["mib_bits"][ok], want["mib_bits"][ok]), tag
    for i, c in enumerate(cells):
        h = wst["n_hf"][i]
        assert _same(gst["sync"][i, :h], wst["sync"][i, :h]) and _same(gst["sync_ce"][i, :h], wst["sync_ce"][i, :h]), (tag, i)
        for p in range(4):
            n, u = want["n_meas"][i, p], want["ce_upto"][i, p]
            assert (n == 0 and u == 0) or p < c.n_ports
            for key, rows in (("meas", n), ("ce", u), ("ce_pw", u)):
                assert _same(got[key][i, p, :rows], want[key][i, p, :rows]), (tag, key, i, p)
            for key in ("ac_fd", "ac_td"):
                assert _same(gst[key][i, p, :n], wst[key][i, p, :n]), (tag, key, i, p)


def test_one_context_serves_blocks_that_grow_shrink_and_grow_again(pkg, blocks):
    """Every tracker test above opens a context per block shape.  Here ONE context runs lcs_track_block + lcs_track_stats on
    cells x symbols (2, 500), (1, 7), (2, 839), (1, 141), (3, 280) in that order -- its workspace grows, serves smaller blocks
    placed by their own shape, and grows again; normal- and extended-CP scenes mixed -- and every array of every call equals, bit
    for bit, the same call on a fresh context.  Likewise lcs_track_cut on (2, 300), (1, 40), (3, 300), the middle call with a cell
    whose sample rate sends it through the walk (the per-cell flags behind the hits are set and cleared): what it returns -- symbols,
    `late`, counts, next positions -- is what a fresh context returns."""
    import torch
    nominal = [b for b in blocks if b["fcp"] == FC]
    n0, n1 = [b for b in nominal if b["per_frame"] == 140]
    e0, e1 = [b for b in nominal if b["per_frame"] == 120]
    plan = [((n1, e0), 500), ((e0,), 7), ((n0, e1), 839), ((n1,), 141), ((n0, e0, n1), 280)]

    def run(S, grp, n_sym):
        args = ([b["c"] for b in grp], np.stack([b["td"][:n_sym] for b in grp]), np.stack([b["fov"][:n_sym] for b in grp]),
                np.stack([b["ftv"][:n_sym] for b in grp]), np.stack([b["late"][:n_sym] for b in grp]), FC, FC, FS)
        return S.track_block(*args), S.track_stats(len(grp), n_sym)

    with pkg.Searcher(0) as S:
        for grp, n_sym in plan:
            got, gst = run(S, grp, n_sym)
            with pkg.Searcher(0) as fresh:
                want, wst = run(fresh, grp, n_sym)
            _assert_block_and_stats_equal(got, want, gst, wst, [b["c"] for b in grp], (len(grp), n_sym))

    cap = iq_u8_to_capbuf(golden("capbuf_0000")["iq_u8"])[:60000]
    d = torch.from_numpy(cap).cuda()
    cps, fts, fos = [1, 2, 1], [100.25, 9000.5, 19100.0], [1e3, -2e3, 0.0]

    def cut(S, n_cells, n_sym, fsp):
        td = torch.full((n_cells, n_sym, 128), float("nan"), dtype=torch.complex128, device="cuda")
        late, n_cut, pos_next = S.track_cut(d.data_ptr(), pkg.FMT_C128, cap.size, cps[:n_cells], fts[:n_cells], fos[:n_cells], FC, FC, fsp, n_sym, td.data_ptr(),
                                            want_state=True)
        return td.cpu().numpy(), late, n_cut, pos_next

    with pkg.Searcher(0) as S:
        for n_cells, n_sym, fsp in ((2, 300, FS), (1, 40, FS * 0.93), (3, 300, FS)):
            got = cut(S, n_cells, n_sym, fsp)
            with pkg.Searcher(0) as fresh:
                want = cut(fresh, n_cells, n_sym, fsp)
            assert all(_same(a, b) for a, b in zip(got, want)), (n_cells, n_sym)
            assert want[2].min() >= 3 and not np.isnan(want[0].real).any()


def test_track_stream_of_mixed_cp_types_equals_one_block(pkg, blocks):
    """lcs_track_stream_block on three cells ordered normal, extended, normal CP: the normal-CP group's cells are not consecutive in
    the caller's arrays, so their samples go up cell by cell, beside a group of one.  839 symbols delivered from host memory in the
    cuts (300, 301, 238) give, row for row and bit for bit, what one lcs_track_block call over the 839 symbols gives (compared as
    tests/test_tracker.py::test_gpu_track_stream_blocks_equal_one_block compares)."""
    nominal = [b for b in blocks if b["fcp"] == FC]
    n0, n1 = [b for b in nominal if b["per_frame"] == 140]
    e0 = [b for b in nominal if b["per_frame"] == 120][0]
    grp, n_all, cuts = (n0, e0, n1), 839, (300, 301, 238)
    recs = [b["c"] for b in grp]
    td, fov, ftv, late = (np.stack([b[k][:n_all] for b in grp]) for k in ("td", "fov", "ftv", "late"))
    with pkg.Searcher(0) as S:
        one = S.track_block(recs, td, fov, ftv, late, FC, FC, FS)
        st = S.track_stats(3, n_all)
        parts, a = [], 0
        for n in cuts:
            parts.append(S.track_stream_block(recs, td[:, a:a + n], fov[:, a:a + n], ftv[:, a:a + n], late[:, a:a + n], FC, FC, FS, want_stats=True))
            a += n
    assert a == n_all and np.array_equal(np.concatenate([p["syms"] for p in parts], axis=1), one["syms"])
    assert np.array_equal(parts[-1]["bpo"], one["bpo"])
    for i, c in enumerate(recs):
        for p in range(4):
            rows = np.concatenate([q["meas"][i, p, :q["n_meas"][i, p]] for q in parts])
            n = one["n_meas"][i, p]
            assert rows.shape[0] == n and np.array_equal(rows, one["meas"][i, p, :n]), (i, p)
            assert (n > 0) == (p < c.n_ports)
            if n:
                fd = np.concatenate([q["ac_fd"][i, p, :q["n_meas"][i, p]] for q in parts])
                tdc = np.concatenate([q["ac_td"][i, p, :q["n_meas"][i, p]] for q in parts])
                assert np.array_equal(fd, st["ac_fd"][i, p, :n])
                assert np.array_equal(tdc[71:], st["ac_td"][i, p, 71:n]) and np.isnan(tdc[:71].real).all()
            # channel estimates: every symbol below ce_upto exactly once, in order
            pos = 0
            for q in parts:
                assert q["ce_from"][i, p] == pos
                k = q["ce_n"][i, p]
                assert np.array_equal(q["ce"][i, p, :k], one["ce"][i, p, pos:pos + k]) and np.array_equal(q["ce_pw"][i, p, :k], one["ce_pw"][i, p, pos:pos + k])
                pos += k
            assert pos == one["ce_upto"][i, p]
        ok = np.concatenate([q["mib_ok"][i, :q["n_mib"][i]] for q in parts])
        bits = np.concatenate([q["mib_bits"][i, :q["n_mib"][i]] for q in parts])
        tried = one["mib_ok"][i] != -1
        assert tried.any() and np.array_equal(ok, one["mib_ok"][i][tried]) and np.array_equal(bits, one["mib_bits"][i][tried])
        assert [q["mib_from"][i] for q in parts] == list(np.cumsum([0] + [q["n_mib"][i] for q in parts[:-1]]))
