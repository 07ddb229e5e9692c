"""The table of tests/sic_edge_cases.py on the CPU: its premises, the reference's walk over every case, and that the table can see the
faults it is for.  No GPU code runs here and nothing is planted in a kernel: the faults are patched into sic_ref (numpy) alone."""
import types

import numpy as np
import pytest

import sic_edge_cases as E
import sic_ref as R
from test_gpu_sic import RESIDUAL_TOL

IDS = [c["name"] for c in E.CASES]


def test_table_covers_what_it_claims():
    sweep = [c for c in E.CASES if c["group"] == "identity"]
    seen = {(c["bufs"][0]["cells"][0]["id"] % 6, c["bufs"][0]["cells"][0]["ports"], c["bufs"][0]["cells"][0]["cp"], c["duplex"]) for c in sweep}
    assert len(sweep) == 72 and seen == {(r, p, cp, d) for r in range(6) for p in (1, 2, 4) for cp in (1, 2) for d in (R.FDD, R.TDD)}
    assert 503 in E.SWEEP_IDS and all(c["bufs"][0]["cells"][0]["frame_start"] % 1 != 0 for c in sweep)
    assert len({c["bufs"][0]["cells"][0]["frame_start"] for c in sweep}) == 72
    assert {c["mask"] for c in E.CASES if c["group"] == "masks"} == {1, 2, 4, 8, 5, 10}
    assert E.N_CAP % 256 != 0 and all(9600 <= c["n_cap"] <= 268800 for c in E.CASES)
    assert [len(b["cells"]) for b in E.BY_NAME["batch_2_0_1"]["bufs"]] == [2, 0, 1] and len({b["fc"] for b in E.BY_NAME["batch_2_0_1"]["bufs"]}) == 3


@pytest.mark.parametrize("name", [c["name"] for c in E.CASES if c["premise"]])
def test_premise(name):
    E.check_premise(E.BY_NAME[name])


@pytest.mark.parametrize("name", IDS)
def test_condition_and_walk(name):
    """the condition the residual bound rests on (compute_reference asserts it), what the reference says of masked-out components,
    and for every record: owner tiles the covered stretch, in symbol order, its offset continuing the window periodically"""
    c = E.BY_NAME[name]
    ref = E.reference(c)
    n = np.arange(c["n_cap"])
    for b, buf in enumerate(c["bufs"]):
        assert ref[b]["res"].size == c["n_cap"] and ref[b]["peak"] <= E.PEAK_CAP
        for i, spec in enumerate(buf["cells"]):
            info = ref[b]["info"][i]
            if spec["refused"]:
                assert info is None
                continue
            for comp in range(4):
                assert (info["power"][comp] == 0) or (c["mask"] >> comp) & 1
            geo = E.case_geo(c, b, i)
            assert info["n_sym"] == geo["n_sym"]
            sym, off = R.owner(geo, n)
            t = np.arange(geo["t_lo"], geo["t_hi"] + 1)
            a = geo["a"](np.append(t, geo["t_hi"] + 1))
            a[-1] = geo["w"](geo["t_hi"]) + 128
            walk = np.full(c["n_cap"], geo["t_lo"] - 1)
            for k, tt in enumerate(t):
                walk[a[k]:a[k + 1]] = tt
            assert np.array_equal(sym, walk)
            assert np.all(np.diff(a) > 128) and a[0] >= 0 and a[-1] <= c["n_cap"]
            assert geo["a"](geo["t_lo"] - 1) < 0 and geo["w"](geo["t_hi"] + 1) + 128 > c["n_cap"]      # the outermost whole symbols
            inside = sym >= geo["t_lo"]
            assert np.array_equal(off[inside], (n[inside] - geo["w"](sym[inside])) % 128)
    if c["group"] == "identity":      # the inputs are worth comparing: every component is there, the rebuilt signal is of the capture's size
        assert all(p > 0 for p in ref[0]["info"][0]["power"]) and 0.3 < ref[0]["peak"]


def test_reference_covers_a_long_capture():
    """268800 samples, normal CP, frame_start 100: the search over a fixed 12 frames stopped at t_hi = 1679 (window end 230500)"""
    geo = E.geo_of(E.rec(155, 2, 1, 100.0), 268800)
    assert geo["w"](geo["t_hi"]) + 128 > 268800 - 138 and geo["t_hi"] > 1679 and (geo["f_lo"], geo["n_frames"]) == (0, 14)
    # ... and the domain of sic_geometry: the shortest and longest capture, the extreme steps and frame_starts
    for n_cap in (9600, 268800):
        for fs in (0.51 * E.FS, 1.99 * E.FS):
            for fs0 in (-999999.5, 0.0, 999999.5):
                for cp in (1, 2):
                    g = E.geo_of(E.rec(155, 2, cp, fs0), n_cap, fs=fs)
                    assert g["a"](g["t_lo"]) >= 0 > g["a"](g["t_lo"] - 1) and g["w"](g["t_hi"]) + 128 <= n_cap < g["w"](g["t_hi"] + 1) + 128


def test_exact_zeros_of_the_reference():
    for tag in ("norm", "ext"):
        info = E.reference(E.BY_NAME["short_%s_no_sss" % tag])[0]["info"][0]
        assert info["gain"] == 0 and info["power"][0] == 0 and info["power"][1] == 0 and info["n_pss"] == 1 and info["power"][2] > 0
    ref = E.reference(E.BY_NAME["batch_2_0_1"])
    assert np.array_equal(ref[1]["res"], E.seen(E.BY_NAME["batch_2_0_1"], 1))


# ------------------------------------------------------------------ the table can see the faults it is for
def _clamped_sfn(cell, geo, frame):
    # an unwrapped counter: the MIB's 8-bit field would hide 1024 itself, so the fault is the counter stopping at its ends
    return min(max(cell.sfn + frame, 0), 1023)


FAULTS = {
    "third CRS row at n_symb - 2 on extended CP": ([(R, "crs_third_symbol", lambda n_symb: n_symb - 2 if n_symb == 6 else n_symb - 3)], ["id300_p2_ext_fdd", "id503_p1_ext_tdd"]),
    "ports 2 / 3 shift without the slot parity": ([(R, "crs_v23", lambda s: 0)], ["id169_p4_norm_fdd", "id2_p4_ext_tdd"]),
    "PBCH holes of symbol 3 on extended CP dropped": ([(R, "pbch_skip", lambda sym, normal: sym in (0, 1))], ["id423_p2_ext_fdd", "mask8_ext4"]),
    "PBCH partner i ^ 1 replaced by i": ([(R, "pbch_mate", lambda s: s)], ["mask8_norm2", "mask8_ext4"]),
    "frame number without the mod-1024 wrap": ([(R, "frame_sfn", _clamped_sfn)], ["origin_sfn_wrap", "long_ext_15_frames"]),
    "frame number without f_lo": ([(R, "frame_sfn", lambda cell, geo, frame: (cell.sfn + frame - geo["f_lo"]) % 1024)], ["origin_norm_below", "origin_ext_below"]),
    "owner without its +-1 correction": ([(R, "owner_corrected", lambda geo, n, t: t)], ["rate_norm_plus", "rate_ext_minus"]),
    "offset before the window as abs(n - w) % 128": ([(R, "window_offset", lambda n, w: np.abs(n - w) % 128)], ["start_norm_exact", "rate_ext_plus"]),
    "averaging over +-3 slots": ([(R, "AVG_SLOTS", 3)], ["id94_p2_norm_fdd", "end_ext_exact"]),
    "the special subframes' symbol 0 unused under a configuration": ([(R, "dl_mask_for", lambda duplex, cfg=None, _f=R.dl_mask_for: (_f(duplex, cfg)[0], False))], ["tdd_config_2_ext4", "tdd_configs_0_5"]),
    "buffer 0's carrier pair used for every buffer": ([(E, "carriers", lambda c, b: c["bufs"][0]["fc"])], ["batch_2_0_1"]),
    "late with the opposite sign in the synthesis": ([(R, "synthesis_phase", lambda geo, t, _f=R.synthesis_phase: np.conj(_f(geo, t)))], ["rate_norm_minus", "id503_p4_ext_fdd"]),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_table_sees_fault(monkeypatch, fault):
    patches, names = FAULTS[fault]
    good = {name: E.reference(E.BY_NAME[name]) for name in names}
    for obj, attr, value in patches:
        monkeypatch.setattr(obj, attr, value)
    for name in names:
        bad = E.compute_reference(E.BY_NAME[name])
        moved = max(np.abs(p["res"] - q["res"]).max() / q["rms"] for p, q in zip(bad, good[name]))
        assert moved > 100 * RESIDUAL_TOL, "case %s does not see the fault '%s': the residual moves by %.3e rms" % (name, fault, moved)
