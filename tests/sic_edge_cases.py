"""The cancellation stage at its geometric edges: a table of hand-made records on seeded noise captures (test infrastructure).

No case runs a search.  A record is new_cell(...) with every field set by hand, the capture is complex Gaussian noise: the least-squares
channel of noise is as good an H as any for comparing arithmetic, the rebuilt signal is of the capture's own size, and a misplaced
element, sign, frame number or owning symbol moves the residual by order 1.  tests/test_sic_edges_ref.py checks the premises of the
table on the CPU (and that the table sees the faults it is for), tests/test_gpu_sic_edges.py runs every case on the device against
reference(case), which is sic_ref.cancel per buffer on the values the device gets.

CASES: [dict(name, group, duplex, n_cap, fs, mask, u8, seed, premise, bufs: [dict(cells: [record spec], fc: (requested, programmed),
configs: None | [uplink-downlink configuration or None per record])])]."""
import types
import zlib

import numpy as np

import sic_ref as R
from conftest import load_pkg

FC = 739e6
FS = 1.92e6
RMS = 0.15
N_CAP = 19731                  # a frame and a bit; odd, so the subtraction's last block is a partial one
PEAK_CAP = 5.0                 # the condition on every case: max |capture| and max |y_c| <= PEAK_CAP rms, at most two cancelled cells


# ------------------------------------------------------------------ records
def rec(ident, ports=2, cp=1, frame_start=5000.3, ff=0.0, fsf=None, sfn=8, n_rb=50, dur=1, res=2, refused=False):
    """a record's fields (cp: 1 normal, 2 extended; ff / fsf: freq_fine / freq_superfine; refused: the launcher must skip it)"""
    return dict(id=ident, ports=ports, cp=cp, frame_start=float(frame_start), ff=float(ff), fsf=float(ff + 123.4 if fsf is None else fsf),
                sfn=sfn, n_rb=n_rb, dur=dur, res=res, refused=refused)


def cell_of(spec):
    return load_pkg().new_cell(n_id_1=spec["id"] // 3, n_id_2=spec["id"] % 3, cp_type=spec["cp"], n_ports=spec["ports"],
                               frame_start=spec["frame_start"], freq_fine=spec["ff"], freq_superfine=spec["fsf"], n_rb_dl=spec["n_rb"],
                               phich_duration=spec["dur"], phich_resource=spec["res"], sfn=spec["sfn"])


def geo_of(spec, n_cap=N_CAP, fc=(FC, FC), fs=FS):
    """sic_ref.geometry of a record spec (no library needed: geometry reads four fields)"""
    cell = types.SimpleNamespace(cp_type=spec["cp"], frame_start=spec["frame_start"], freq_fine=spec["ff"], freq_superfine=spec["fsf"])
    return R.geometry(cell, n_cap, fc[0], fc[1], fs)


def case_geo(c, b=0, i=0):
    return geo_of(c["bufs"][b]["cells"][i], c["n_cap"], c["bufs"][b]["fc"], c["fs"])


# ------------------------------------------------------------------ the table
CASES = []


def add(name, group, bufs, n_cap=N_CAP, duplex=R.FDD, mask=R.ALL, fs=FS, u8=False, seed=None, premise=None):
    bufs = [dict(cells=list(b["cells"]), fc=b.get("fc", (FC, FC)), configs=b.get("configs")) for b in bufs]
    CASES.append(dict(name=name, group=group, bufs=bufs, n_cap=int(n_cap), duplex=duplex, mask=mask, fs=float(fs), u8=u8,
                      seed=zlib.crc32(name.encode()) if seed is None else seed, premise=premise))


def one(spec, **kw):
    return [dict(cells=[spec], **kw)]


# identity sweep: every id mod 6, every port count, both CP types, both duplex modes; frame_start moves with the case
SWEEP_IDS = (300, 169, 2, 423, 94, 503)
N_RB = (6, 15, 25, 50, 75, 100)
i = 0
for duplex in (R.FDD, R.TDD):
    for cp in (1, 2):
        for ports in (1, 2, 4):
            for ident in SWEEP_IDS:
                spec = rec(ident, ports, cp, frame_start=(1234.567 * (i + 1)) % 19200.0, ff=(-1) ** i * (100.0 + 13.0 * i), sfn=(37 * i + 5) % 1024,
                           n_rb=N_RB[i % 6], dur=1 + i % 2, res=1 + (i // 2) % 4)
                add("id%d_p%d_%s_%s" % (ident, ports, "norm" if cp == 1 else "ext", "fdd" if duplex == R.FDD else "tdd"), "identity", one(spec), duplex=duplex)
                i += 1

# frame origin: both sides of d0 - .01 fs k > -0.5 (frame_start + cp0 - 19200 = -0.7 | -0.3), a negative frame_start, the sfn wrap
add("origin_norm_below", "origin", one(rec(155, 2, 1, 19189.3, sfn=0)), premise="origin_below")
add("origin_norm_above", "origin", one(rec(155, 2, 1, 19189.7, sfn=0)), premise="origin_above")
add("origin_ext_below", "origin", one(rec(302, 2, 2, 19167.3, sfn=0)), premise="origin_below")
add("origin_ext_above", "origin", one(rec(302, 2, 2, 19167.7, sfn=0)), premise="origin_above")
add("origin_negative", "origin", one(rec(155, 2, 1, -2.5, sfn=77)), premise="origin_negative")
add("origin_sfn_wrap", "origin", one(rec(155, 2, 1, 1000.4, sfn=1022)), n_cap=4 * 19200 + 77, premise="sfn_wrap")

# rates: step away from 1 by +-3e-4 (and 5e-5 more from the carriers), so rounding stretches or shrinks symbols
FC_OFF = (FC, FC - 40e3)
for cp, tag in ((1, "norm"), (2, "ext")):
    for sign, stag in ((1, "plus"), (-1, "minus")):
        add("rate_%s_%s" % (tag, stag), "rates", one(rec(155 if cp == 1 else 302, 2, cp, 4321.6, ff=sign * 5000.0), fc=FC_OFF),
            fs=FS * (1 + sign * 3e-4), premise="stretched" if sign > 0 else "shrunk")
add("rate_norm_superfine_plus", "rates", one(rec(155, 2, 1, 4321.6, ff=5000.0, fsf=12000.0), fc=FC_OFF), fs=FS * (1 + 3e-4), premise="stretched")
add("rate_ext_superfine_minus", "rates", one(rec(302, 4, 2, 4321.6, ff=-5000.0, fsf=-12000.0), fc=FC_OFF), fs=FS * (1 - 3e-4), premise="shrunk")

# capture ends, one record per CP type: the captures are chosen from the geometry itself
for cp, tag, ident, ports in ((1, "norm", 155, 2), (2, "ext", 302, 4)):
    base = rec(ident, ports, cp, 7003.3, sfn=500)
    g = geo_of(base)
    n_exact = int(g["w"](g["t_hi"])) + 128
    add("end_%s_exact" % tag, "ends", one(base), n_cap=n_exact, premise="end_exact")
    add("end_%s_one_short" % tag, "ends", one(base), n_cap=n_exact - 1, premise="end_one_short")
    at0 = dict(base, frame_start=base["frame_start"] - float(g["a"](g["t_lo"])))
    add("start_%s_exact" % tag, "ends", one(at0), premise="start_exact")
    add("start_%s_one_early" % tag, "ends", one(dict(at0, frame_start=at0["frame_start"] - 1.0)), premise="start_one_early")
    # half a frame whose only whole sync symbol is a PSS: the SSS before it starts 3 samples before the capture
    n_symb = 7 if cp == 1 else 6
    cp0, sym_len, cp_len = (10, 137, 9) if cp == 1 else (32, 160, 32)
    fs0 = (cp_len - 2 + 3) - sym_len * (n_symb - 1) - cp0 + 0.3 + (19200.0 if cp == 2 else 0.0)      # a(PSS symbol of slot 0) == 3
    add("short_%s_no_sss" % tag, "ends", one(rec(ident, ports, cp, fs0, sfn=500)), n_cap=9600, premise="no_sss")
    add("long_%s_15_frames" % tag, "ends", one(rec(ident, ports, cp, 700.3 if cp == 1 else 9100.6, sfn=1015)), n_cap=268800, premise="long")

# masks: every single component, and the two pairs that leave the other pair out
MASK_RECORDS = (("norm2", rec(155, 2, 1, 6100.4, sfn=200)), ("ext4", rec(302, 4, 2, 6100.4, sfn=200)))
for tag, spec in MASK_RECORDS:
    for mask in (1, 2, 4, 8, 5, 10):
        add("mask%d_%s" % (mask, tag), "masks", one(spec), mask=mask)

# lists and batches
A0, A1 = rec(155, 2, 1, 3000.7, sfn=11), rec(302, 4, 2, 9555.2, ff=-350.0, sfn=640, n_rb=100, dur=2, res=4)
add("list_two_cells", "lists", [dict(cells=[A0, A1])])
add("list_refused_between", "lists", [dict(cells=[A0, dict(rec(77, 2, 1, 4000.0), n_rb=0, refused=True), A1])])
add("batch_2_0_1", "lists", [dict(cells=[A0, A1], fc=(FC, FC)), dict(cells=[], fc=(FC + 1e6, FC + 1e6 - 25e3)),
                             dict(cells=[rec(94, 1, 1, 12000.9, ff=2000.0, sfn=1023)], fc=(FC - 2e6, FC - 2e6 + 31e3))])
add("list_two_cells_u8", "lists", [dict(cells=[A0, A1])], u8=True)
add("tdd_configs_0_5", "lists", [dict(cells=[A0, rec(169, 2, 1, 11000.1, sfn=300)], configs=[0, 5])], duplex=R.TDD)
add("tdd_config_7_is_none", "lists", [dict(cells=[A0], configs=[7])], duplex=R.TDD)
add("tdd_config_2_ext4", "lists", [dict(cells=[A1], configs=[2])], duplex=R.TDD, premise="special_symbols")

BY_NAME = {c["name"]: c for c in CASES}
GROUPS = ("identity", "origin", "rates", "ends", "masks", "lists")
assert len(BY_NAME) == len(CASES) and {c["group"] for c in CASES} == set(GROUPS)


# ------------------------------------------------------------------ premises (asserted on the CPU by tests/test_sic_edges_ref.py)
def window_steps(g):
    """(w(t + 1) - w(t), the nominal length) of every symbol but the last"""
    t = np.arange(g["t_lo"], g["t_hi"])
    nominal = (np.where((t + 1) % 7 == 0, 138, 137) if g["normal"] else np.full(t.shape, 160))
    return g["w"](t + 1) - g["w"](t), nominal


def check_premise(c):
    g, p = case_geo(c), c["premise"]
    spec = c["bufs"][0]["cells"][0]
    syncs = R.sync_symbols(g, c["duplex"])
    if p == "origin_below":        # d0 keeps the frame's length: the record's frame starts at the capture's end, frame -1 fills it
        assert g["d0"] > 19000 and g["f_lo"] == -1 and g["t_lo"] < 0 and R.frame_sfn(types.SimpleNamespace(sfn=spec["sfn"]), g, g["f_lo"]) == 1023
        assert any(t // g["n_symb"] == -19 for t in range(g["t_lo"], 0))                              # slot 1 of frame -1: its PBCH
    elif p == "origin_above":
        assert -0.5 < g["d0"] < 0 and g["f_lo"] == 0 and g["t_lo"] == 1                                  # symbol 0 starts before the capture
    elif p == "origin_negative":
        assert g["d0"] == 7.5 and g["t_lo"] == 0 and g["a"](0) == 0                                      # w(0) = rint(7.5) = 8: a tie
    elif p == "sfn_wrap":
        sfns = [(spec["sfn"] + f) % 1024 for f in range(g["f_lo"], g["f_lo"] + g["n_frames"])]
        assert sfns == [1021, 1022, 1023, 0, 1]                                                          # 1023 -> 0, and two 40 ms periods besides
    elif p in ("stretched", "shrunk"):
        step, nominal = window_steps(g)
        assert abs(g["step"] - 1) > 2e-4 and set(step - nominal) == ({0, 1} if p == "stretched" else {0, -1})
    elif p == "end_exact":
        assert g["w"](g["t_hi"]) + 128 == c["n_cap"]
    elif p == "end_one_short":
        assert g["w"](g["t_hi"] + 1) + 128 == c["n_cap"] + 1
    elif p == "start_exact":
        assert g["a"](g["t_lo"]) == 0
    elif p == "start_one_early":
        assert g["a"](g["t_lo"] - 1) == -1
    elif p == "no_sss":
        assert [kind for _, kind, _ in syncs] == ["pss"] and g["a"](syncs[0][0]) == 3 and g["t_lo"] == syncs[0][0]
    elif p == "long":
        assert g["n_frames"] == 15 and g["w"](g["t_hi"]) + 128 > c["n_cap"] - (138 if g["normal"] else 160) and (spec["sfn"] + g["f_lo"] + g["n_frames"] - 1) > 1023
    elif p == "special_symbols":
        mask, special = R.dl_mask_for(R.TDD, c["bufs"][0]["configs"][0])
        assert special and any(R.usable(g, t, mask, True) and not R.usable(g, t, mask, False) for t in range(g["t_lo"], g["t_hi"] + 1))
    else:
        assert p is None, p


# ------------------------------------------------------------------ captures and the reference
_captures, _references = {}, {}


def capture(c, b):
    """what buffer b of the case holds on the device: complex64 [n_cap], or the dongle's bytes uint8 [2 n_cap]"""
    key = (c["name"], b)
    if key not in _captures:
        rng = np.random.default_rng([c["seed"], b])
        g = rng.standard_normal(c["n_cap"]) + 1j * rng.standard_normal(c["n_cap"])
        if c["u8"]:
            iq = np.empty(2 * c["n_cap"], np.uint8)
            iq[0::2] = np.clip(np.rint(127 + 20 * g.real), 0, 255)
            iq[1::2] = np.clip(np.rint(127 + 20 * g.imag), 0, 255)
            _captures[key] = iq
        else:
            _captures[key] = (RMS / np.sqrt(2.0) * g).astype(np.complex64)
        _captures[key].setflags(write=False)
    return _captures[key]


def seen(c, b):
    """the capture's values as the kernels read them, complex128"""
    x = capture(c, b)
    if c["u8"]:
        return ((x[0::2].astype(np.float64) - 127.0) / 128.0) + 1j * ((x[1::2].astype(np.float64) - 127.0) / 128.0)
    return x.astype(np.complex128)


def carriers(c, b):
    return c["bufs"][b]["fc"]


def compute_reference(c):
    """-> per buffer dict(res complex128, info: one sic_ref record per cell of the list (None: refused), rms, peak: max |y_c| / rms)"""
    out = []
    for b, buf in enumerate(c["bufs"]):
        x = seen(c, b)
        good = [i for i, s in enumerate(buf["cells"]) if not s["refused"]]
        cfg = None if buf["configs"] is None else [buf["configs"][i] for i in good]
        fr, fp = carriers(c, b)
        res, info, ys = R.cancel(x, [cell_of(buf["cells"][i]) for i in good], fr, fp, c["fs"], duplex=c["duplex"], mask=c["mask"], ul_dl_config=cfg,
                                 waveforms=True)
        rms = float(np.sqrt(np.mean(np.abs(x) ** 2)))
        peak = max([float(np.abs(y).max()) for y in ys], default=0.0) / rms
        # the condition the residual bound rests on (2^-24 (sum_c |y_c| + |res|) <= 2^-24 * 15 rms): never a measurement of the device
        assert len(good) <= 2 and np.abs(x).max() <= PEAK_CAP * rms and peak <= PEAK_CAP, (c["name"], b, len(good), np.abs(x).max() / rms, peak)
        full = [None] * len(buf["cells"])
        for i, inf in zip(good, info):
            full[i] = inf
        out.append(dict(res=res, info=full, rms=rms, peak=peak))
    return out


def reference(c):
    if c["name"] not in _references:
        _references[c["name"]] = compute_reference(c)
    return _references[c["name"]]
