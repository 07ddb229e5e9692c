"""Inputs the PHICH tests share (tests/test_phich_host.py, tests/test_gpu_phich.py, tools/phich_accuracy.py): crafted grids with planted
HARQ indicators, captures with the generator's PHICH in them, and the host twin's loader.

A crafted grid holds what the stage reads and nothing else: the reference signals of symbol 0 (ports 0, 1) and symbol 1 (ports 2, 3)
of every subframe's first slot through one complex gain per port -- flat, so that the interpolated channel is exact and a planted
indicator of amplitude 1 reads +-1 to rounding --, or with `ripple` through a smooth channel that is not; the PHICH of
synth.phich_region through the same gains; white noise on those rows when snr_db says so."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import pcfich_cases as PC
import pcfich_ref as PR
import phich_ref as HR
from conftest import load_pkg

# the corners of the rule: one small shape each
CORNERS = {
    "6rb_one_unit": dict(n_rb=6, n_ports=1, cp=1, duration=1, resource=1, mi=None, n_id=7),
    "15rb": dict(n_rb=15, n_ports=2, cp=1, duration=1, resource=3, mi=None, n_id=141),
    "25rb_4ports": dict(n_rb=25, n_ports=4, cp=1, duration=1, resource=3, mi=None, n_id=68),
    "ext_cp": dict(n_rb=15, n_ports=2, cp=2, duration=1, resource=4, mi=None, n_id=329),
    "ext_cp_4ports": dict(n_rb=25, n_ports=4, cp=2, duration=1, resource=2, mi=None, n_id=256),
    "ext_duration": dict(n_rb=25, n_ports=2, cp=1, duration=2, resource=2, mi=None, n_id=503),
    "ext_duration_4ports": dict(n_rb=15, n_ports=4, cp=1, duration=2, resource=3, mi=None, n_id=0),
    "100rb_ng2_mi2": dict(n_rb=100, n_ports=2, cp=1, duration=1, resource=4, mi=[2] * 10, n_id=68),
    # a TDD pattern: subframes with m_i 0 (U = 0: read with nothing in them), 1 and 2
    "tdd_mi_012": dict(n_rb=25, n_ports=2, cp=1, duration=1, resource=3, mi=[2, 1, 0, 0, 0, 2, 1, 0, 0, 0], n_id=141),
}
MASKS = [0x3FF, 0x021, 0x200]


def mi_of(corner):
    return [1] * 10 if corner["mi"] is None else list(corner["mi"])


def n_ofdm_of(cp, n_sub=3, ragged=2):
    """n_sub subframes and `ragged` rows of one more: the grid ends inside a subframe"""
    return 2 * n_sub * PR.n_symb_of(cp) + ragged


def pattern(seed, g, n_group, n_seq, plant):
    """what is planted in subframe g -> [n_group][n_seq] of 0 (silent), +1 (NACK), -1 (ACK)"""
    rng = np.random.default_rng(100003 * seed + g)
    sign = 1 - 2 * rng.integers(0, 2, (n_group, n_seq))
    if plant == "all":
        return sign
    if plant == "half":
        return sign * (rng.random((n_group, n_seq)) < 0.5)
    if plant == "none":
        return 0 * sign
    if plant == "one_group":                      # every sequence of group 0, its neighbours silent
        sign[1:] = 0
        return sign
    raise ValueError(plant)


@functools.lru_cache(maxsize=None)
def crafted(name, plant="all", snr_db=None, n_sub=3, ragged=2, seed=1, ripple=False, amp=1.0):
    """-> (tfg [n_ofdm][12 n_rb], planted: per grid subframe the pattern [n_group][n_seq], None where nothing could be planted)"""
    c = CORNERS[name]
    synth = load_pkg().synth
    n_rb, P, cp, n_id = c["n_rb"], c["n_ports"], c["cp"], c["n_id"]
    n, nc = PR.n_symb_of(cp), 12 * n_rb
    n_ofdm = n_ofdm_of(cp, n_sub, ragged)
    rng = np.random.default_rng(7000 + seed)
    gain = np.exp(2j * np.pi * rng.random(4)) * (0.8 + 0.4 * rng.random(4))
    k = np.arange(nc)
    tau = 0.3 * rng.random()

    def chan(p, r):
        if not ripple:
            return np.full(nc, gain[p])
        return gain[p] * np.exp(-2j * np.pi * tau * (k - nc / 2) / (128.0 * n_rb / 6)) * (1.0 + 0.2 * np.cos(2 * np.pi * k / nc + p + r / 40.0))

    tfg = np.zeros((n_ofdm, nc), np.complex128)
    planted = []
    mi, need, n_seq = mi_of(c), HR.rows_needed(P, c["duration"]), HR.n_seq_of(cp)
    for g in range(PR.n_sf_of(n_ofdm, cp)):
        r0, sf = 2 * g * n, g % 10
        planted.append(None)
        for sym in range(min(2, n_ofdm - r0)):
            rs = PR.rs_row(n_id, cp, n_rb, 2 * sf, sym)
            for p in ([0, 1] if sym == 0 else [2, 3]):
                if p < P:
                    idx = PR.shift_of(p, n_id, 2 * sf) + 6 * np.arange(2 * n_rb)
                    tfg[r0 + sym, idx] = rs * chan(p, r0 + sym)[idx]
        if r0 + need - 1 < n_ofdm and mi[sf] > 0:
            n_group = synth.phich_n_group(n_rb, c["resource"] - 1, cp == 1, mi[sf])
            pat = pattern(seed, g, n_group, n_seq, plant)
            his = [dict(group=int(a), seq=int(b), ack=int(pat[a, b] < 0), amp=amp) for a, b in zip(*np.nonzero(pat))]
            try:
                for l, cols, vals in synth.phich_region(n_id, n_rb, P, cp == 1, sf, 3, his, c["duration"] == 2, c["resource"] - 1, mi[sf]):
                    tfg[r0 + l, cols] = sum(vals[p] * chan(p, r0 + l)[cols] for p in range(P))
                planted[-1] = pat
            except ValueError:                    # a refused map: nothing is there
                pass
        if snr_db is not None:
            sigma = 10 ** (-snr_db / 20) / np.sqrt(2.0)
            rows = slice(r0, min(r0 + 3, n_ofdm))
            shape = tfg[rows].shape
            tfg[rows] += sigma * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    tfg.setflags(write=False)
    return tfg, planted


# ---------------------------------------------------------------- the host twin (tests/host/phich_host.cpp)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lte-cell-scanner_amd", "csrc")
TWIN_SRC = os.path.join(ROOT, "tests", "host", "phich_host.cpp")
TWIN_LIB = os.path.join(ROOT, "tests", "host", "libphich_host.so")
HIPCC = PC.HIPCC
_dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
_up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
_ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
MAX_ENT = 400


def stale(target, src=TWIN_SRC):
    dep = [src] + [os.path.join(CSRC, h) for h in ("phich.h", "pdcch.h", "pcfich.h", "cell_meas.h", "tdd_config.h", "lte_device.h")] + [os.path.join(ROOT, "include", "lcs.h")]
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in dep)


def load_twin(capi):
    """phich.h compiled for the host (built where it is missing or older than its sources)"""
    if stale(TWIN_LIB):
        subprocess.check_call(HIPCC + ["-O2", "-fPIC", "-shared", "-o", TWIN_LIB, TWIN_SRC])
    h = C.CDLL(TWIN_LIB)
    h.phich_host.argtypes = [C.POINTER(C.c_double)] + [C.c_int] * 9 + [C.POINTER(C.c_int32), C.c_int, C.c_double, C.c_double, C.POINTER(C.c_uint32),
                                                                       C.POINTER(capi.PhichInfo), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    h.phich_host.restype = None
    h.phich_host_map.argtypes = [C.c_int] * 7 + [C.POINTER(C.c_int32)]
    h.phich_host_map.restype = C.c_int
    h.phich_host_layout.argtypes = [C.POINTER(C.c_int32)]
    h.phich_host_layout.restype = None
    h.phich_host_default.argtypes = [C.c_int]
    h.phich_host_default.restype = C.c_double
    return h


def twin_map(H, n_rb, n_ports, cp, n_id, duration, resource, mi):
    """-> (n_unit, re [n_unit][3][4] of (l << 16 | column)); n_unit -1: refused"""
    re = np.zeros(50 * 12, np.int32)
    n = H.phich_host_map(n_rb, n_ports, cp, n_id, duration, resource, mi, _ip(re))
    return n, re[:12 * max(n, 0)].reshape(-1, 3, 4)


def twin_record(H, capi, name, tfg, mask=0x3FF, min_amp=None, min_sigma=None):
    """-> (PhichInfo, values [n_sf][400], sigma [n_sf][400]) of the twin on a grid of corner `name`"""
    c = CORNERS[name]
    tfg = np.ascontiguousarray(tfg, np.complex128)
    jump = PC.jump_tables(c["n_rb"])
    o = capi.PhichInfo()
    o.tdd = c["mi"] is not None
    n_sf = PR.n_sf_of(tfg.shape[0], c["cp"])
    values, sigma = np.zeros((n_sf, MAX_ENT)), np.zeros((n_sf, MAX_ENT))
    mi = np.array(mi_of(c), np.int32)
    H.phich_host(_dp(tfg.view(np.float64)), tfg.shape[0], PR.n_symb_of(c["cp"]), c["n_rb"], c["n_id"], c["cp"], c["n_ports"], mask, c["duration"], c["resource"],
                 _ip(mi), int(c["mi"] is not None), capi.PHICH_MIN_AMP if min_amp is None else min_amp, capi.PHICH_MIN_SIGMA if min_sigma is None else min_sigma,
                 _up(jump), C.byref(o), _dp(values), _dp(sigma))
    return o, values, sigma


def ref_record(name, tfg, mask=0x3FF, min_amp=None, min_sigma=None):
    """the numpy rule on the same grid"""
    c = CORNERS[name]
    capi = load_pkg().capi
    return HR.decode(tfg, c["n_id"], c["cp"], c["n_ports"], c["n_rb"], mask, c["duration"], c["resource"], c["mi"],
                     capi.PHICH_MIN_AMP if min_amp is None else min_amp, capi.PHICH_MIN_SIGMA if min_sigma is None else min_sigma)


def cell_of(pkg, name, **kw):
    c = CORNERS[name]
    cell = pkg.new_cell(n_id_1=c["n_id"] // 3, n_id_2=c["n_id"] % 3, cp_type=c["cp"], n_ports=c["n_ports"], **kw)
    cell.phich_duration, cell.phich_resource = c["duration"], c["resource"]
    return cell


def cfg_of(capi, name, **kw):
    """the call's configuration: None for an FDD corner with the defaults"""
    c = CORNERS[name]
    if c["mi"] is None and not kw:
        return None
    return capi.PhichCfg.make(phich_mi=c["mi"], **kw)


def assert_record_close(rec, values, sigma, ref, tol, what="", min_amp=None, min_sigma=None):
    """rec / values / sigma: a record with its tables (the twin's, or the device's values); ref: HR.decode()'s dict.  Values and sigma
    within tol of the subframe's largest |value|; the decisions equal but for entries within 1e-9 of a threshold, which are counted and
    returned with the worst difference."""
    capi = load_pkg().capi
    min_amp = capi.PHICH_MIN_AMP if min_amp is None else min_amp
    min_sigma = capi.PHICH_MIN_SIGMA if min_sigma is None else min_sigma
    head = lambda r, g: (g(r, "n_sf"), g(r, "n_read"), g(r, "dl_mask"), g(r, "n_rb"), g(r, "n_ports"))
    assert head(rec, getattr) == head(ref, lambda r, k: r[k]), (what, head(rec, getattr), head(ref, lambda r, k: r[k]))
    worst, near, total, listed = 0.0, 0, 0, 0
    mine = {(h["subframe"], h["group"], h["seq"]): h for h in rec.indicators()}
    for g in range(ref["n_sf"]):
        s, r = rec.sf[g], ref["sf"][g]
        assert (s.n_unit, s.n_group) == (r["n_unit"], r["n_group"]), (what, g, s.n_unit, s.n_group, r)
        if r["n_unit"] <= 0:
            assert (s.n_present, s.n_ack, s.n_nack, s.noise) == (0, 0, 0, 0.0), (what, g)
            continue
        n = r["n_group"] * ref["n_seq"]
        rv, rs, rf = ref["values"][g].reshape(-1), ref["sigma"][g].reshape(-1), ref["flags"][g].reshape(-1)
        scale = max(float(np.abs(rv).max()), 1e-300)
        worst = max(worst, float(np.abs(values[g][:n] - rv).max()) / scale)
        if sigma is not None:
            worst = max(worst, float(np.abs(sigma[g][:n] - rs).max()) / scale)
        assert abs(s.noise - r["noise"]) <= 10 * tol * max(r["noise"], scale * scale), (what, g, s.noise, r["noise"])
        total += n
        if rec.n_dropped:
            assert (s.n_present, s.n_ack) == (r["n_present"], r["n_ack"]), (what, g)
        for i in range(n):
            key = (g, i // ref["n_seq"], i % ref["n_seq"])
            fl = (1 | (2 if mine[key]["ack"] else 0)) if key in mine else 0
            listed += int(rf[i] != 0)
            if listed > capi.PHICH_MAX_HI:                   # beyond the cap of the list: the subframe's counts speak for these
                continue
            if fl != int(rf[i]):
                # only an entry on a threshold may differ
                on_edge = abs(abs(rv[i]) - min_amp) <= 1e-9 or abs(abs(rv[i]) - min_sigma * rs[i]) <= 1e-9 or abs(rv[i]) <= 1e-9
                assert on_edge, (what, key, fl, int(rf[i]), rv[i], rs[i])
                near += 1
    assert worst <= tol, (what, worst)
    return worst, near, total


# ---------------------------------------------------------------- captures with the generator's PHICH in them
N_FRAMES = 3


def capture_pattern(frame, subframe, n_group, n_seq):
    """what the capture plants: about a third of the entries, signs by a hash of the position -> [n_group][n_seq] of 0, +1, -1"""
    rng = np.random.default_rng(977 * frame + 31 * subframe + 5)
    sign = 1 - 2 * rng.integers(0, 2, (n_group, n_seq))
    return sign * (rng.random((n_group, n_seq)) < 0.35)


@functools.lru_cache(maxsize=None)
def phich_capture(R, n_rb, cp_type, n_ports, phich_res=2, snr_db=20.0):
    """pcfich_cases.pcfich_capture with capture_pattern's PHICH in every subframe (normal duration, the MIB's Ng code phich_res): three
    frames behind FRAME_START R samples of silence, in noise, as complex64"""
    import meas_wide_cases as WC
    pkg = load_pkg()
    rng = np.random.default_rng(9500 + 100 * R + 10 * cp_type + n_ports)
    n_group, n_seq = pkg.synth.phich_n_group(n_rb, phich_res, cp_type == 1), HR.n_seq_of(cp_type)

    def phich(frame, subframe):
        pat = capture_pattern(frame, subframe, n_group, n_seq)
        return [dict(group=int(a), seq=int(b), ack=int(pat[a, b] < 0)) for a, b in zip(*np.nonzero(pat))]

    w = pkg.synth.cell_waveform_wide(N_FRAMES, WC.CELL_ID[0], WC.CELL_ID[1], R, n_rb, cp_type == 1, n_ports=n_ports, rng=rng, cfi=PC.planted_cfi,
                                     phich_res=phich_res, phich=phich)
    cap = np.concatenate([np.zeros(int(WC.FRAME_START * R), np.complex128), w])
    sigma = np.sqrt(0.5 / 10 ** (snr_db / 10) / 2)
    return (0.2 * (cap + sigma * (rng.standard_normal(cap.size) + 1j * rng.standard_normal(cap.size)))).astype(np.complex64)


# ---------------------------------------------------------------- uplink grants and their answers
def format0_bits(n_rb, rb_start, n_prb, cyclic_shift, size):
    """a format 0 payload (36.212 5.3.3.1.1, FDD) as an int, bit t = the t-th bit sent: flag 0, hopping 0, the RIV of (rb_start,
    n_prb), mcs 9, ndi 1, tpc 1, the cyclic shift field, no CQI request, padding up to `size`"""
    assert rb_start + n_prb <= n_rb
    riv = n_rb * (n_prb - 1) + rb_start if n_prb - 1 <= n_rb // 2 else n_rb * (n_rb - n_prb + 1) + (n_rb - 1 - rb_start)
    fields = [(0, 1), (0, 1), (riv, (n_rb * (n_rb + 1) // 2 - 1).bit_length()), (9, 5), (1, 1), (1, 2), (cyclic_shift, 3), (0, 1)]
    bits = [(v >> (w - 1 - i)) & 1 for v, w in fields for i in range(w)]
    bits += [0] * (size - len(bits))
    return sum(b << t for t, b in enumerate(bits))


LINK_SHAPE = (2, 15, 1, 2)          # (R, n_rb, CP type, ports)
LINK_RNTIS = (0x4A31, 0x0107)
# (grid subframe of the grant, RNTI, rb_start, n_prb, cyclic shift, the answer eight subframes later: "ack" / "nack")
LINK_GRANTS = [(1, 0x4A31, 3, 2, 1, "ack"), (4, 0x4A31, 10, 1, 6, "nack"), (2, 0x0107, 0, 4, 0, "nack"), (6, 0x0107, 13, 2, 7, "ack"),
               (25, 0x4A31, 5, 1, 2, "ack")]          # the last one is answered beyond the grid
LINK_CFI, LINK_L = 3, 4


@functools.lru_cache(maxsize=None)
def link_capture(snr_db=20.0):
    """phich_capture's cell with LINK_GRANTS as format 0 DCIs in their RNTIs' search spaces and the PHICH of each eight subframes later
    at capi.phich_index; nothing else in the control region"""
    import meas_wide_cases as WC
    pkg = load_pkg()
    capi, synth = pkg.capi, pkg.synth
    R, n_rb, cp, ports = LINK_SHAPE
    n_id = WC.CELL_ID[1] + 3 * WC.CELL_ID[0]
    size = capi.dci_1a_size(n_rb, False)
    n_cce = synth.pdcch_layout(n_id, n_rb, ports, cp == 1, LINK_CFI)[1]
    n_group = capi.phich_n_group(n_rb, 3, cp == 1)
    dcis, his = {}, {}
    for g, rnti, rb, n_prb, cs, answer in LINK_GRANTS:
        bits = format0_bits(n_rb, rb, n_prb, cs, size)
        cce = capi.ue_search_space(rnti, g % 10, n_cce, LINK_L)[0]
        dcis.setdefault(divmod(g, 10), []).append(dict(rnti=rnti, bits=[(bits >> t) & 1 for t in range(size)], L=LINK_L, cce=cce))
        grp, seq = capi.phich_index(rb, cs, n_group, cp == 1)
        his.setdefault(divmod(g + 8, 10), []).append(dict(group=grp, seq=seq, ack=int(answer == "ack")))
    rng = np.random.default_rng(9700)
    w = synth.cell_waveform_wide(N_FRAMES, WC.CELL_ID[0], WC.CELL_ID[1], R, n_rb, cp == 1, n_ports=ports, rng=rng, cfi=LINK_CFI, phich_res=2,
                                 pdcch=lambda fr, sf: dcis.get((fr, sf), []), phich=lambda fr, sf: his.get((fr, sf), []))
    cap = np.concatenate([np.zeros(int(WC.FRAME_START * R), np.complex128), w])
    sigma = np.sqrt(0.5 / 10 ** (snr_db / 10) / 2)
    return (0.2 * (cap + sigma * (rng.standard_normal(cap.size) + 1j * rng.standard_normal(cap.size)))).astype(np.complex64)
