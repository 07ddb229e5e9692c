"""Carrier-frequency sweep and frequency-hypothesis split over the GPUs of one node (host-side drivers).

Two independent shard axes, both over torch.distributed (backend "nccl" = RCCL on ROCm,
"gloo" in the CPU tests), one process per GPU:

* ``run_sweep`` -- the outer loop of the reference's CLI (src/CellSearch.cpp:465-573): every carrier on the 100 kHz
  raster gets one capture buffer and one pass of the searcher chain, results are merged with the reference's
  duplicate rule (:285-319).  Carriers are independent: rank r of `world` takes carriers r, r+world, ... through the
  device-resident batch API; the only communication is ONE all-gather of the fixed-size cell records at the end
  (raw lcs_cell bytes -- a numpy structured view, no per-cell Python objects on the way).
* ``search_capbuf_foe_split`` -- ONE buffer spread over the ranks (latency mode): the frequency hypotheses are split
  into contiguous blocks, every rank correlates its block, and the blocks meet where the reference takes the maximum
  over the frequency axis (xc_peak_freq, src/searcher.cpp:369-382): a MAX all-reduce over 3 x 9600 packed words
  ``bits(pow_f32) << 32 | (0xFFFFFFFF - foi)`` -- non-negative floats order like their bit patterns, and the
  complemented index makes the LOWEST foi win a tie, as the reference's strict `>` does (:374).  peak_search then runs
  identically everywhere; the per-peak stages run on the rank that owns the winning hypothesis (it holds the
  xc_incoherent_single slice the refinement step reads, :457-465) and the decoded cells are all-gathered.
"""
from __future__ import annotations

from typing import Callable, List, Sequence

import numpy as np

MAXC = 104   # == capi.MAX_PEAKS: cell records kept per carrier: the longest list the reference can return (include/lcs.h LCS_MAX_PEAKS)
FIELDS = ("fc_requested", "fc_programmed", "pss_pow", "freq", "frame_start", "freq_fine", "freq_superfine",
          "ind", "n_id_2", "n_id_1", "cp_type", "n_ports", "n_rb_dl", "phich_duration", "phich_resource", "sfn")


def cell_dtype():
    from . import capi
    return capi.cell_dtype()


def fc_search_set(freq_start: float, freq_end: float) -> np.ndarray:
    """src/CellSearch.cpp:465: freq_start : 100 kHz : freq_end."""
    n = int(np.floor((freq_end - freq_start) / 100e3)) + 1
    return freq_start + 100e3 * np.arange(n)


def shard(n_carriers: int, rank: int, world: int) -> np.ndarray:
    """Block-cyclic assignment of carrier indices to ranks."""
    return np.arange(rank, n_carriers, world)


def cells_to_records(cells) -> np.ndarray:
    """Cell objects (LcsCell or anything with the FIELDS attributes) -> structured array with lcs_cell's layout."""
    rec = np.zeros(len(cells), cell_dtype())
    for i, c in enumerate(cells):
        for f in FIELDS:
            rec[i][f] = getattr(c, f)
    return rec


def record_to_dict(r) -> dict:
    d = {f: (float(r[f]) if r.dtype[f].kind == "f" else int(r[f])) for f in FIELDS}
    d["n_id_cell"] = d["n_id_2"] + 3 * d["n_id_1"] if (d["n_id_1"] >= 0 and d["n_id_2"] >= 0) else -1
    return d


def dedup(detected: Sequence[Sequence[dict]]) -> List[dict]:
    """src/CellSearch.cpp:285-319: same cell ID within 1 MHz -> keep the one with the larger pss_pow."""
    final: List[dict] = []
    for cells in detected:
        for c in cells:
            for i, f in enumerate(final):
                if c["n_id_cell"] == f["n_id_cell"] and \
                        abs((c["fc_requested"] + c["freq_superfine"]) - (f["fc_requested"] + f["freq_superfine"])) < 1e6:
                    if c["pss_pow"] > f["pss_pow"]:
                        final[i] = c
                    break
            else:
                final.append(c)
    return final


def records_with_gain(cells_per_carrier, gain) -> List[List[dict]]:
    """The per-carrier cell lists of a band search on 8-bit carriers (search_wideband(out="u8"), WidebandFeed(out="u8")) as
    record_to_dict dicts on ONE power scale: carrier k's bytes are its floats times gain[k] (Searcher.channelize_u8's gains, or
    WidebandFeed.gains), and a correlation power scales with the square of the buffer's amplitude, so pss_pow is divided by
    gain[k]**2 -- exactly, the gain being a power of two.  dedup() on the result compares carriers as it does for float buffers."""
    gain = np.asarray(gain.detach().cpu().numpy() if hasattr(gain, "detach") else gain, np.float64).reshape(-1)
    if len(cells_per_carrier) != gain.size:
        raise ValueError(f"records_with_gain: {len(cells_per_carrier)} carriers, {gain.size} gains")
    out = []
    for cells, g in zip(cells_per_carrier, gain):
        recs = [record_to_dict(r) for r in cells_to_records(cells)]
        for d in recs:
            d["pss_pow"] /= g * g
        out.append(recs)
    return out


def meas_with_gain(meas_per_carrier, gain) -> list:
    """The per-carrier measurement lists (Searcher.last_cell_meas) of a band search on 8-bit carriers on ONE power scale, as
    records_with_gain does for pss_pow: carrier k's bytes are its floats times gain[k], and rsrp, noise, rssi and the sums a_re_im are
    powers of the buffer, so they are divided by gain[k]**2 -- exactly, the gain being a power of two; rsrq and the SINR are ratios
    and stay what they are.  Returns copies (capi.CellMeas); records that hold no measurement pass unchanged."""
    gain = np.asarray(gain.detach().cpu().numpy() if hasattr(gain, "detach") else gain, np.float64).reshape(-1)
    if len(meas_per_carrier) != gain.size:
        raise ValueError(f"meas_with_gain: {len(meas_per_carrier)} carriers, {gain.size} gains")
    out = []
    for recs, g in zip(meas_per_carrier, gain):
        row = []
        for m in recs:
            m = m.copy()
            if m.status == 0:
                g2 = g * g
                for p in range(2):
                    m.rsrp[p] /= g2
                    m.noise[p] /= g2
                for i in range(4):
                    m.a_re_im[i] /= g2
                m.rssi /= g2
            row.append(m)
        out.append(row)
    return out


def search_wideband(searcher, d_wide_ptr: int, fmt: int, n_in: int, fs_in: float, decim: int, fc_centre: float, carriers, f_search_set,
                    n_out: int = None, chunk: int = 128, max_cells_per_buf: int = 16, rate=None, out: str = "c64", meas: bool = False,
                    sic_rounds: int = 0):
    """A band search from ONE wideband capture resident in HBM (n_in samples of fmt at fs_in, centred on fc_centre): the
    carriers (absolute Hz, e.g. fc_search_set(...)) are channelized `chunk` at a time (Searcher.channelize: mix, low-pass,
    decimate by decim) into a torch buffer this function owns, and every chunk goes through the full chain as a
    complex<float> batch with fc_requested = fc_programmed = the carrier and fs_programmed = fs_in / decim -- the batch
    is queued right behind the channelizer on the searcher's stream, nothing waits in between.  n_out is even (the float
    batch needs an even n_cap); 153584 = the most an 80 ms capture gives, rounded down: 15 combining windows as for a
    dongle buffer.  rate = (up, down) takes a capture at any rate with fs_in * up / down = 1.92 Msps (20 Msps: (12, 125))
    through Searcher.channelize_rational instead: decim is ignored, fs_programmed = fs_in * up / down, and n_out -- unless
    given -- is the largest even count the capture holds (without rate it is 153584).  out = "u8" channelizes into bytes
    (Searcher.channelize_u8: every carrier scaled by a power of two of its own, component rms 16..32 codes) and hands the
    chunks over as FMT_IQ_U8 batches, which take the int8 correlation kernel and a quarter of the memory; a byte batch takes
    any n_cap, so with a rate n_out is then all the capture holds, odd or even.  The search runs in the searcher's duplex mode
    (Searcher.set_duplex: one capture covers one band, and a band has one duplex; a TDD band wants f_search_set in 2.5 kHz steps,
    or Searcher.set_foe_unwrap(True) and the usual 5 kHz).
    Returns one list of cells (LcsCell)
    per carrier, in the order of `carriers`: ``dedup([[record_to_dict(r) for r in cells_to_records(c)] for c in result])`` merges them as a sweep's.
    meas=True turns Searcher.set_cell_meas on for these batches (and puts the mode back afterwards) and returns the cells as
    record_to_dict dicts instead, each with its measurement (capi.CellMeas) as cell["meas"]; with out="u8" the measurement and
    pss_pow are already on one power scale over the carriers (meas_with_gain, records_with_gain).
    sic_rounds=N (2..4; 0, the default, and 1: the search as it always was) runs every chunk through Searcher.search_batch_sic with
    max_rounds=N instead: after each round the decoded cells' PSS, SSS, CRS and PBCH are subtracted from their carrier's buffer and the
    residual is searched again; the function then returns (cells, rounds): per carrier the cells and the round each was found in
    (0: the plain search).  Not together with meas (the measurement belongs to one fused call, the rounds are several)."""
    import torch
    from . import capi
    carriers = np.ascontiguousarray(np.atleast_1d(carriers), np.float64)
    if out not in ("c64", "u8"):
        raise ValueError(f"search_wideband: out must be 'c64' or 'u8', not {out!r}")
    up, down = (int(rate[0]), int(rate[1])) if rate is not None else (1, int(decim))      # up == 1 is the integer path, bit for bit
    fs_out = float(fs_in) * up / down
    if n_out is None and rate is None:
        n_out = 153584
    elif n_out is None:      # what the capture holds: (n_out - 1) * down + 16 * down <= n_in * up
        n_out = (int(n_in) * up - 16 * down) // down + 1
        if out != "u8":
            n_out &= ~1
    chunk = max(1, min(int(chunk), carriers.size))
    dev = getattr(searcher, "device", -1)
    tdev = torch.device("cuda", dev if dev >= 0 else torch.cuda.current_device())
    if out == "u8":
        buf, batch_fmt, channelize = torch.empty((chunk, int(n_out), 2), dtype=torch.uint8, device=tdev), capi.FMT_IQ_U8, searcher.channelize_u8
    else:
        buf, batch_fmt, channelize = torch.empty((chunk, int(n_out)), dtype=torch.complex64, device=tdev), capi.FMT_C64, searcher.channelize_rational
    cells, all_rounds = [], []
    if int(sic_rounds) > 1:
        if meas:
            raise ValueError("search_wideband: sic_rounds and meas do not go together")
        for a in range(0, carriers.size, chunk):
            fc = carriers[a:a + chunk]
            channelize(d_wide_ptr, fmt, n_in, fs_in, up, down, fc - float(fc_centre), buf.data_ptr(), n_out)
            found, rounds, _ = searcher.search_batch_sic(buf.data_ptr(), batch_fmt, fc.size, int(n_out), f_search_set, fc, fc, fs_out,
                                                         max_rounds=int(sic_rounds), max_cells_per_buf=max_cells_per_buf)
            cells += found
            all_rounds += rounds
        return cells, all_rounds
    if not meas:
        for a in range(0, carriers.size, chunk):
            fc = carriers[a:a + chunk]
            channelize(d_wide_ptr, fmt, n_in, fs_in, up, down, fc - float(fc_centre), buf.data_ptr(), n_out)
            cells += searcher.search_batch(buf.data_ptr(), batch_fmt, fc.size, int(n_out), f_search_set, fc, fc, fs_out, capi.STAGE_FULL, max_cells_per_buf)
        return cells
    was_on = searcher.cell_meas_mode
    searcher.set_cell_meas(True)
    try:
        for a in range(0, carriers.size, chunk):
            fc = carriers[a:a + chunk]
            if out == "u8":
                gain = channelize(d_wide_ptr, fmt, n_in, fs_in, up, down, fc - float(fc_centre), buf.data_ptr(), n_out, want_gain=True)
            else:
                channelize(d_wide_ptr, fmt, n_in, fs_in, up, down, fc - float(fc_centre), buf.data_ptr(), n_out)
                gain = np.ones(fc.size)
            found = searcher.search_batch(buf.data_ptr(), batch_fmt, fc.size, int(n_out), f_search_set, fc, fc, fs_out, capi.STAGE_FULL, max_cells_per_buf)
            recs = records_with_gain(found, gain)
            info = meas_with_gain(searcher.last_cell_meas(fc.size, max_cells_per_buf), gain)
            for rs_, ms_ in zip(recs, info):
                for d, m in zip(rs_, ms_):
                    d["meas"] = m
            cells += recs
    finally:
        searcher.set_cell_meas(was_on)
    return cells


MEAS_MAX_RB = {1: 6, 2: 15, 4: 25, 8: 50, 16: 100}      # the resource blocks a 128 R-point grid holds (lcs_cell_meas_wide)


def meas_rate(n_rb: int) -> int:
    """R of the narrowest measurement rate 1.92e6 R whose grid holds n_rb resource blocks"""
    for R, most in MEAS_MAX_RB.items():
        if 6 <= n_rb <= most:
            return R
    raise ValueError(f"measure_wideband: no measurement rate holds n_rb = {n_rb} (6 .. 100)")


def map_frame_start(frame_start: float, decim_search: int, decim_meas: int) -> float:
    """A position in the outputs of channelize(decim_search) as a position in the outputs of channelize(decim_meas) of the same
    capture.  Output m of a decimation D is the filter centred on wide sample m D + (16 D - 1) / 2 (include/lcs.h: lcs_channelize),
    so the wide sample of the one is read back through the other; decim_meas = 1 is the capture itself (no filter, no delay)."""
    wide = frame_start * decim_search + (16 * decim_search - 1) / 2
    return (wide - ((16 * decim_meas - 1) / 2 if decim_meas > 1 else 0.0)) / decim_meas


def measure_wideband(searcher, d_wide_ptr: int, fmt: int, n_in: int, fs_in: float, fc_centre: float, decim_search: int, cells_per_carrier,
                     carriers, n_rb: int = None, dl_mask: int = None, pcfich: bool = False, pdcch=False, tdd_config: int = None, pdsch=False,
                     pdsch_comb=False, pdsch_alloc=None, pdcch_scan=None, phich=False):
    """The full-bandwidth measurement (Searcher.cell_meas_wide) of what search_wideband found in the SAME capture, still in HBM:
    cells_per_carrier is its result (lists of LcsCell, or of dicts with meas=True) for `carriers`, searched at decim_search.
    For every cell with a MIB: R = meas_rate(n_rb or the cell's n_rb_dl), the capture is channelized once more at the cell's
    carrier with decim_meas = K / R (K = fs_in / 1.92e6; the integer path only, decim_meas >= 2) into complex64 at 1.92e6 R, the
    cell's frame_start is mapped into that buffer (map_frame_start; a negative position is advanced by whole frames), and the stage
    measures as many whole slots as the buffer holds, 122 at the most.  K == R is accepted only for a complex64 capture already
    centred on the carrier, which is measured in place.  dl_mask: None takes the narrow record's where the cell carries one
    (meas=True), else 0x3FF (FDD) / 0x021 (TDD, the searcher's duplex mode).
    Returns one list per carrier, entry k belonging to cell k: a capi.CellMeasWide, or None for a cell without a MIB; a dict cell
    also gets it as cell["meas_wide"].  The wide records come from float carriers and need no gain, whatever `out` the search used.
    pcfich=True also reads the PCFICH (Searcher.pcfich_wide) of every such cell from the same re-channelized buffer, under the same
    mask and over the same slots: entry k is then the pair (CellMeasWide, PcfichInfo), and a dict cell gets cell["pcfich"] as well.
    The PCFICH spans the cell's own bandwidth: with an n_rb other than the cell's n_rb_dl its record is None.
    pdcch=True (or a capi.PdcchCfg) also decodes the PDCCH common search space (Searcher.pdcch_wide) of every such cell whose MIB
    says its PHICH configuration, from the same buffer, mask and slots: a dict cell gets cell["pdcch"] (a PdcchInfo, or None as for
    the PCFICH), and entry k is (CellMeasWide, PdcchInfo) -- (CellMeasWide, PcfichInfo, PdcchInfo) with pcfich=True.  True takes the
    sizes of capi.dci_common_sizes for the cell's bandwidth and the searcher's duplex mode; in TDD with a known uplink-downlink
    configuration (tdd_config = 0 .. 6) the m_i of capi.tdd_phich_mi are passed, else FDD's.
    pdsch=True (or a capi.PdschCfg) also follows the format 1A grants of that search space into the PDSCH (Searcher.pdsch_wide, with
    the PDCCH configuration that pdcch names or, without one, its defaults) from the same buffer, mask and slots: a dict cell gets
    cell["pdsch"] (a PdschInfo, or None as for the PDCCH), and the PdschInfo is appended to entry k's tuple.
    pdsch_comb=True (or a capi.PdschCombCfg) takes Searcher.pdsch_comb_wide for that step (it implies pdsch): the redundancy versions
    of SIB1 (and, with an si_window in the configuration, of other SI messages) are combined.  A dict cell also gets
    cell["pdsch_comb"] (a PdschCombInfo, or None) and, where the payload of a rule-1 group that passed a CRC parses,
    cell["sib1"] = capi.sib1_fields(...); the PdschCombInfo is appended to entry k's tuple after the PdschInfo.
    pdsch_alloc (a capi.PdschAllocCfg) is the searcher's setting (Searcher.set_pdsch_alloc) for the length of this call, so that
    distributed 1A grants and format 1C grants are followed too; the setting the searcher had comes back afterwards.  Its sfn0 is
    the caller's: the frame number of the first frame the stage reads, ONE value for every cell -- right only where the cells share
    their frame timing; pass -1 where they do not or it is not known.
    pdcch_scan (a capi.PdcchScanCfg) also runs the blind search of every CCE (Searcher.pdcch_scan_wide) of every such cell whose MIB
    says its PHICH configuration, from the same buffer, mask and slots: a dict cell gets cell["pdcch_scan"] (a PdcchScanInfo, or None
    as for the PDCCH), and the record is appended to entry k's tuple after every other one.
    phich=True (or a capi.PhichCfg) also reads the PHICH (Searcher.phich_wide) of every such cell whose MIB says its PHICH
    configuration, from the same buffer, mask and slots and with no channelizer call of its own: a dict cell gets cell["phich"] (a
    PhichInfo, or None as for the PDCCH), and the record is appended to entry k's tuple after every other one.  True takes the cell's
    PHICH configuration and, in TDD with a known tdd_config, the m_i of capi.tdd_phich_mi.
    Raises ValueError for a capture whose rate is no integer multiple of 1.92 Msps (rational rates), for K / R < 2 off the
    carrier or in an integer format, and for a capture too short for two slots of the cell."""
    import ctypes as C
    import torch
    from . import capi
    carriers = np.ascontiguousarray(np.atleast_1d(carriers), np.float64)
    if len(cells_per_carrier) != carriers.size:
        raise ValueError(f"measure_wideband: {len(cells_per_carrier)} cell lists, {carriers.size} carriers")
    K = float(fs_in) / 1.92e6
    if abs(K - round(K)) > 1e-9 * K or round(K) < 1:
        raise ValueError(f"measure_wideband: fs_in = {fs_in} is no integer multiple of 1.92 Msps; rational-rate captures are not measured")
    K, D_s = int(round(K)), int(decim_search)
    dev = getattr(searcher, "device", -1)
    tdev = torch.device("cuda", dev if dev >= 0 else torch.cuda.current_device())
    bufs = {}                                             # decim_meas -> (buffer, the carrier it holds)
    out = []
    set_alloc = bool(pdsch or pdsch_comb) and pdsch_alloc is not None
    before = getattr(searcher, "pdsch_alloc", None)
    if set_alloc:
        searcher.set_pdsch_alloc(pdsch_alloc)
    try:
        for fc, cells in zip(carriers, cells_per_carrier):
            row = []
            for cell in cells:
                d = cell if isinstance(cell, dict) else None
                get = (lambda k: d[k]) if d is not None else (lambda k: getattr(cell, k))
                if get("n_rb_dl") not in (6, 15, 25, 50, 75, 100) or get("cp_type") not in (1, 2):
                    row.append(None)
                    continue
                rb = int(n_rb) if n_rb is not None else int(get("n_rb_dl"))
                R = meas_rate(rb)
                if K % R or K < R:
                    raise ValueError(f"measure_wideband: {rb} resource blocks need 1.92e6 x {R} samples per second, which fs_in = {fs_in} (K = {K}) does not give by an integer decimation")
                D_m = K // R
                if D_m == 1:
                    if fmt != capi.FMT_C64 or float(fc) != float(fc_centre):
                        raise ValueError("measure_wideband: K / R < 2 -- the capture is used in place, which takes a complex64 capture centred on the cell's carrier")
                    ptr, n_cap = int(d_wide_ptr), int(n_in)
                else:
                    if not 2 <= D_m <= 16:
                        raise ValueError(f"measure_wideband: decim_meas = {D_m} is outside the channelizer's 2 .. 16")
                    n_cap = (int(n_in) - 16 * D_m) // D_m + 1
                    if D_m not in bufs:
                        bufs[D_m] = [torch.empty(max(n_cap, 1), dtype=torch.complex64, device=tdev), None]
                    if bufs[D_m][1] != float(fc):
                        searcher.channelize(d_wide_ptr, fmt, n_in, fs_in, D_m, [float(fc) - float(fc_centre)], bufs[D_m][0].data_ptr(), n_cap)
                        bufs[D_m][1] = float(fc)
                    ptr = bufs[D_m][0].data_ptr()
                fs_m = float(fs_in) / D_m
                n_symb = 7 if get("cp_type") == 1 else 6      # LCS_CP_NORMAL / LCS_CP_EXTENDED
                k_factor = (float(fc) - get("freq_fine")) / float(fc)
                frame = 0.01 * fs_m * k_factor
                start = map_frame_start(get("frame_start"), D_s, D_m)
                while start < 0:
                    start += frame
                # whole slots between the first DFT the stage takes (it moves 10 ms back where it can) and the buffer's end
                first = start + (10 if n_symb == 7 else 32) * R * k_factor
                if first - frame > -0.5:
                    first -= frame
                n_slots = int((n_cap - 128 * R - first) / (frame / 20)) - 1
                if n_slots < 2:
                    raise ValueError("measure_wideband: the capture holds less than two slots of the cell at the measurement rate")
                if d is None:
                    mc = capi.LcsCell.from_buffer_copy(bytes(cell))
                else:
                    mc = capi.LcsCell()
                    searcher._lib.lcs_cell_init(C.byref(mc))
                    for f in FIELDS:
                        setattr(mc, f, d[f])
                mc.frame_start = start
                if dl_mask is not None:
                    mask = int(dl_mask)
                elif d is not None and getattr(d.get("meas"), "status", -1) == 0:
                    mask = int(d["meas"].dl_mask)
                else:
                    mask = 0x3FF if searcher.duplex == capi.DUPLEX_FDD else 0x021
                # what every stage below takes: the cell, its samples and rate, the grid's shape, the mask
                wide = (mc, ptr, float(fc), float(fc), fs_m, 128 * R, rb, min(122, n_slots) * n_symb, mask)
                # the stages that decode span the cell's own bandwidth, and all but the PCFICH need its PHICH configuration
                own_rb = lambda: rb == int(get("n_rb_dl"))
                decodable = lambda: own_rb() and get("phich_duration") in (1, 2) and get("phich_resource") in (1, 2, 3, 4)
                tdd = searcher.duplex != capi.DUPLEX_FDD
                tdd_mi = lambda: capi.tdd_phich_mi(tdd_config) if tdd and tdd_config is not None else None      # None: FDD's
                default_pdcch_cfg = lambda: capi.PdcchCfg.make(capi.dci_common_sizes(rb, tdd), phich_mi=tdd_mi())
                rec = searcher.cell_meas_wide(*wide, n_cap=n_cap)
                if d is not None:
                    d["meas_wide"] = rec
                if pcfich:
                    pc = searcher.pcfich_wide(*wide, n_cap=n_cap) if own_rb() else None
                    if d is not None:
                        d["pcfich"] = pc
                    rec = (rec, pc)
                if pdcch:
                    pd = None
                    if decodable():
                        pd = searcher.pdcch_wide(*wide, default_pdcch_cfg() if pdcch is True else pdcch, n_cap=n_cap)
                    if d is not None:
                        d["pdcch"] = pd
                    rec = (rec if isinstance(rec, tuple) else (rec,)) + (pd,)
                if pdsch or pdsch_comb:
                    ps = pc = None
                    if decodable():
                        cfg = default_pdcch_cfg() if pdcch is True or not pdcch else pdcch
                        pcfg = None if pdsch is True or not pdsch else pdsch
                        if pdsch_comb:
                            ps, pc = searcher.pdsch_comb_wide(*wide, cfg, pcfg, None if pdsch_comb is True else pdsch_comb, n_cap=n_cap)
                        else:
                            ps = searcher.pdsch_wide(*wide, cfg, pcfg, n_cap=n_cap)
                    if d is not None:
                        d["pdsch"] = ps
                    rec = (rec if isinstance(rec, tuple) else (rec,)) + (ps,)
                    if pdsch_comb:
                        if d is not None:
                            d["pdsch_comb"] = pc
                            sib = [capi.sib1_fields(g["bytes"]) for g in (pc.groups() if pc is not None else []) if g["rule"] == 1 and g["crc_ok"]]
                            sib = [x for x in sib if x is not None]
                            if sib:
                                d["sib1"] = sib[0]
                        rec = rec + (pc,)
                if pdcch_scan is not None:
                    sc = searcher.pdcch_scan_wide(*wide, pdcch_scan, n_cap=n_cap) if decodable() else None
                    if d is not None:
                        d["pdcch_scan"] = sc
                    rec = (rec if isinstance(rec, tuple) else (rec,)) + (sc,)
                if phich:
                    ph = None
                    if decodable():
                        cfg = phich
                        if phich is True:
                            cfg = capi.PhichCfg.make(phich_mi=tdd_mi()) if tdd_mi() is not None else None
                        ph = searcher.phich_wide(*wide, cfg, n_cap=n_cap)
                    if d is not None:
                        d["phich"] = ph
                    rec = (rec if isinstance(rec, tuple) else (rec,)) + (ph,)
                row.append(rec)
            out.append(row)
    finally:
        if set_alloc:
            searcher.set_pdsch_alloc(before)
    return out


class WidebandFeed:
    """A band search from a wideband STREAM: push() takes the front end's transfer buffers as they come (n_samples of fmt at fs_in,
    centred on fc_centre, resident in HBM), the searcher's channelizer stream (Searcher.chan_stream_open, rate = (up, down),
    (1, decim) for the integer form) continues every carrier over the cuts, and whenever n_cap outputs per carrier are complete
    they go through the full chain as one FMT_C64 capture per carrier -- fc_requested = fc_programmed = the carrier, fs_programmed =
    fs_in * up / down, batches of at most 128 carriers, as search_wideband does.  Two [n_ch][n_cap] complex64 buffers are filled in
    turn; a transfer buffer that straddles a capture's end is split there (chan_stream_count, bisected on the chunk length: counts
    grow by at most one per sample, so the split is exact).  The searcher's one channelizer stream is this object's until close().
    out = "u8": the stream hands out 8-bit captures (Searcher.chan_stream_open_u8), searched as FMT_IQ_U8 batches on the int8
    correlation kernel.  bufs are then two [n_ch][n_cap][2] uint8 buffers, written in turn one whole capture at a time (cur: the one
    the next capture goes to; filled stays 0, the capture in hand lives in the library), and `gains` is the float32 [n_ch] device
    tensor of the last finished capture's gains (None before the first), read without synchronising: records_with_gain(cells, feed.gains)
    puts the cells of its carriers on one power scale.
    The captures are searched in the searcher's duplex and frequency-estimate modes (Searcher.set_duplex, set_foe_unwrap), as
    search_wideband's are."""

    def __init__(self, searcher, fmt: int, fs_in: float, rate, fc_centre: float, carriers, f_search_set, n_cap: int = 153600,
                 max_cells_per_buf: int = 16, out: str = "c64"):
        import torch
        from . import capi
        if out not in ("c64", "u8"):
            raise ValueError(f"WidebandFeed: out must be 'c64' or 'u8', not {out!r}")
        self.searcher, self.fmt, self.n_cap, self.max_cells_per_buf = searcher, int(fmt), int(n_cap), int(max_cells_per_buf)
        self.carriers = np.ascontiguousarray(np.atleast_1d(carriers), np.float64)
        self.f_search_set = f_search_set
        up, down = int(rate[0]), int(rate[1])
        self.fs_out = float(fs_in) * up / down
        self._sample_bytes = {capi.FMT_C64: 8, capi.FMT_IQ_S16: 4, capi.FMT_IQ_S8: 2}.get(self.fmt, 1)
        dev = getattr(searcher, "device", -1)
        tdev = torch.device("cuda", dev if dev >= 0 else torch.cuda.current_device())
        self.cur, self.filled, self._u8 = 0, 0, out == "u8"
        if self._u8:
            self.bufs = [torch.empty((self.carriers.size, self.n_cap, 2), dtype=torch.uint8, device=tdev) for _ in range(2)]
            self._gains = [torch.empty(self.carriers.size, dtype=torch.float32, device=tdev) for _ in range(2)]
            self.gains = None
            searcher.chan_stream_open_u8(self.fmt, fs_in, up, down, self.carriers - float(fc_centre), self.n_cap)
        else:
            self.bufs = [torch.empty((self.carriers.size, self.n_cap), dtype=torch.complex64, device=tdev) for _ in range(2)]
            searcher.chan_stream_open(self.fmt, fs_in, up, down, self.carriers - float(fc_centre))
        self._open = True

    def _longest(self, n: int, room: int) -> int:
        """the longest chunk of at most n samples that hands out at most `room` outputs (out = "u8": completes at most `room` captures)"""
        count = self.searcher.chan_stream_count_u8 if self._u8 else self.searcher.chan_stream_count
        if count(n) <= room:
            return n
        lo, hi = 0, n                  # count(lo) <= room < count(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if count(mid) <= room else (lo, mid)
        return lo

    def _search(self, buf):
        from . import capi
        cells = []
        for a in range(0, self.carriers.size, 128):
            fc = self.carriers[a:a + 128]
            cells += self.searcher.search_batch(buf[a].data_ptr(), capi.FMT_IQ_U8 if self._u8 else capi.FMT_C64, fc.size, self.n_cap, self.f_search_set,
                                                fc, fc, self.fs_out, capi.STAGE_FULL, self.max_cells_per_buf)
        return cells

    def _push_u8(self, d_ptr: int, n_samples: int):
        """every library push completes at most one capture, into the buffer and the gain tensor whose turn it is"""
        done, off = [], 0
        while off < n_samples:
            n = self._longest(n_samples - off, 1)      # >= 1: one sample hands out at most one output
            buf, gain = self.bufs[self.cur], self._gains[self.cur]
            n_done, _ = self.searcher.chan_stream_push_u8(d_ptr + off * self._sample_bytes, n, buf.data_ptr(), gain.data_ptr(), 1)
            off += n
            if n_done:
                self.gains = gain
                done.append(self._search(buf))
                self.cur ^= 1
        return done

    def push(self, d_ptr: int, n_samples: int):
        """Feed n_samples at d_ptr (device; they must stay unchanged until the searcher's stream has run the work queued here).
        Returns the per-carrier cell lists of every capture this push completed: usually []."""
        done, off, n_samples = [], 0, int(n_samples)
        if self._u8:
            return self._push_u8(d_ptr, n_samples)
        while off < n_samples:
            room = self.n_cap - self.filled
            n = self._longest(n_samples - off, room)
            buf = self.bufs[self.cur]
            n_emit, _ = self.searcher.chan_stream_push(d_ptr + off * self._sample_bytes, n, buf.data_ptr() + 8 * self.filled, self.n_cap, room)
            off += n
            self.filled += n_emit
            if self.filled == self.n_cap:
                done.append(self._search(buf))
                self.cur, self.filled = self.cur ^ 1, 0
        return done

    def close(self):
        if self._open:
            self._open = False
            self.searcher.chan_stream_close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _all_gather_bytes(arr: np.ndarray, dist, device, world: int) -> List[np.ndarray]:
    """One all-gather of a fixed-size numpy array (viewed as bytes) -> the array of every rank."""
    import torch
    t = torch.from_numpy(arr.view(np.uint8).reshape(-1).copy())
    if device is not None:
        t = t.to(device)
    out = torch.empty((world, t.numel()), dtype=torch.uint8, device=t.device)
    dist.all_gather_into_tensor(out.view(-1), t)
    host = out.cpu().numpy()
    return [host[r].view(arr.dtype).reshape(arr.shape) for r in range(world)]


def run_sweep(search_fn: Callable, get_capbufs: Callable[[np.ndarray], object], fcs: np.ndarray, rank: int = 0, world: int = 1,
              dist=None, device=None, batch: int = 64):
    """search_fn(bufs, fc_of_each) -> (records [n][MAXC] structured, counts [n]) as Searcher.batch_collect_raw returns
    them, or per-buffer lists of cell objects; get_capbufs(carrier_indices) -> the capture buffers of those carriers in
    whatever form search_fn takes.  Returns (cells_final, detected_per_carrier) on every rank (the all-gather leaves
    all ranks with the full list; only rank 0 normally prints it)."""
    mine = shard(len(fcs), rank, world)
    n_max = int(np.ceil(len(fcs) / world))
    rec = np.zeros((n_max, MAXC), cell_dtype())
    cnt = np.zeros(n_max, np.int32)
    for a in range(0, len(mine), batch):
        idx = mine[a:a + batch]
        res = search_fn(get_capbufs(idx), fcs[idx])
        if isinstance(res, tuple):
            r, c = res
            rec[a:a + len(idx)] = r[:, :MAXC]
            cnt[a:a + len(idx)] = np.minimum(c, MAXC)
            if np.any(np.asarray(c) > MAXC):
                import warnings
                warnings.warn(f"run_sweep: a carrier reported more than {MAXC} cells; the list was truncated", RuntimeWarning)
        else:
            for j, cells in enumerate(res):
                cnt[a + j] = min(len(cells), MAXC)
                rec[a + j, :cnt[a + j]] = cells_to_records(cells[:MAXC])
    if dist is not None:      # the sweep's only collective: counts ride in front of the records.  Also run at world 1 when
        # a process group is live: the RCCL path of an 8-GPU node exercised on one GPU (tests/test_gpu_rccl.py)
        blob = np.concatenate([cnt.view(np.uint8), rec.view(np.uint8).reshape(-1)])
        blobs = _all_gather_bytes(blob, dist, device, world)
        parts = [(b[:cnt.nbytes].view(np.int32), b[cnt.nbytes:].view(cell_dtype()).reshape(rec.shape)) for b in blobs]
    else:
        parts = [(cnt, rec)]
    detected = [[] for _ in range(len(fcs))]
    for r in range(world):
        c_r, rec_r = parts[r]
        for j, ci in enumerate(shard(len(fcs), r, world)):
            detected[ci] = [record_to_dict(rec_r[j, k]) for k in range(int(c_r[j]))]
    return dedup(detected), detected


class SearcherStages:
    """The searcher.h functions of a GPU `Searcher` in the form search_capbuf_foe_split takes."""

    def __init__(self, searcher, z_th1_fn):
        self._s, self.z_th1 = searcher, z_th1_fn
        for name in ("peak_search", "sss_detect", "pss_sss_foe", "extract_tfg", "tfoec", "decode_mib"):
            setattr(self, name, getattr(searcher, name))

    def xcorr_pss(self, capbuf, f, ds, fc_req, fc_prog, fs):
        return self._s.xcorr_pss(capbuf, f, ds, fc_req, fc_prog, fs, want_incoherent=False)


# ---------------------------------------------------------------------------------------------- foe-axis split
def foe_blocks(n_f: int, world: int) -> List[np.ndarray]:
    """Contiguous, near-equal blocks of hypothesis indices, one per rank (some empty when world > n_f)."""
    edges = np.linspace(0, n_f, world + 1).round().astype(int)
    return [np.arange(edges[r], edges[r + 1]) for r in range(world)]


def pack_pow_frq(pow_: np.ndarray, frq_global: np.ndarray) -> np.ndarray:
    """(pow as float32-exact doubles, global foi) -> int64 words whose MAX is the reference's first-maximum rule."""
    bits = pow_.astype(np.float32).view(np.uint32).astype(np.int64)
    return (bits << 32) | (0xFFFFFFFF - frq_global.astype(np.int64))


def unpack_pow_frq(words: np.ndarray):
    pow32 = (words >> 32).astype(np.uint32).view(np.float32)
    return pow32.astype(np.float64), (0xFFFFFFFF - (words & 0xFFFFFFFF)).astype(np.int32)


def search_capbuf_foe_split(stages, capbuf, f_search_set, fc_requested, fc_programmed, fs_programmed, rank=0, world=1,
                            dist=None, device=None, ds_comb_arm=2, thresh2_n_sigma=3.0):
    """One capture buffer, hypotheses split over the ranks.  `stages` offers the searcher.h functions
    (xcorr_pss, peak_search, sss_detect, pss_sss_foe, extract_tfg, tfoec, decode_mib, z_th1): a Searcher plus the
    package's z_th1, or the oracle in the CPU tests.  Returns (cells in peak order, dict of the collapsed arrays)."""
    import torch
    f = np.asarray(f_search_set, np.float64)
    blocks = foe_blocks(f.size, world)
    own = blocks[rank]
    words = np.full((3, 9600), -1, np.int64)        # smaller than any packed word (pow >= 0 packs non-negative)
    single_full = np.zeros((3, 9600, f.size), np.float32)
    sp_inc, n_comb_xc = None, 0
    if own.size:
        r = stages.xcorr_pss(capbuf, f[own], ds_comb_arm, fc_requested, fc_programmed, fs_programmed)
        words = pack_pow_frq(r["pow"], own[0] + r["frq"])
        single_full[:, :, own] = r["single"]
        sp_inc, n_comb_xc = r["sp_incoherent"], int(r["n_comb_xc"])
    if dist is not None:
        t = torch.from_numpy(words)
        if device is not None:
            t = t.to(device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)         # where the hypotheses meet: MAX with index, 230 KB
        words = t.cpu().numpy()
        # sp_incoherent does not depend on the hypotheses: a rank with an empty block takes it from rank 0
        meta = torch.zeros(9601, dtype=torch.float64)
        if rank == 0:
            meta[:9600] = torch.from_numpy(sp_inc)
            meta[9600] = n_comb_xc
        if device is not None:
            meta = meta.to(device)
        dist.broadcast(meta, src=0)
        meta = meta.cpu().numpy()
        sp_inc, n_comb_xc = meta[:9600].copy(), int(meta[9600])
    pow_, frq = unpack_pow_frq(words)
    Z = stages.z_th1(sp_inc, n_comb_xc, ds_comb_arm)
    # the greedy loop depends on the collapsed arrays only; the refinement reads `single` at the winning hypothesis
    peaks = stages.peak_search(pow_, frq, Z, f, fc_requested, fc_programmed, single_full, ds_comb_arm)
    mine = []
    for order, pk in enumerate(peaks):
        foi = int(np.flatnonzero(f == pk.freq)[0])           # the hypothesis the peak was found at (lowest index on duplicates)
        if foi not in own:
            continue
        c = stages.sss_detect(pk, capbuf, thresh2_n_sigma, fc_requested, fc_programmed, fs_programmed)
        c = c[0] if isinstance(c, tuple) else c
        if c.n_id_1 == -1:
            continue
        c = stages.pss_sss_foe(c, capbuf, fc_requested, fc_programmed, fs_programmed)
        tfg, ts = stages.extract_tfg(c, capbuf, fc_requested, fc_programmed, fs_programmed)
        c, tfg_comp, _ = stages.tfoec(c, tfg, ts, fc_requested, fc_programmed)
        c = stages.decode_mib(c, tfg_comp)
        if c.n_rb_dl == -1:
            continue
        mine.append((order, c))
    rec = np.zeros(MAXC, cell_dtype())
    order = np.full(MAXC, -1, np.int32)
    if mine:
        rec[:len(mine)] = cells_to_records([c for _, c in mine[:MAXC]])
        order[:len(mine)] = [o for o, _ in mine[:MAXC]]
    if dist is not None:
        blobs = _all_gather_bytes(np.concatenate([order.view(np.uint8), rec.view(np.uint8)]), dist, device, world)
        allc = []
        for b in blobs:
            o, rr = b[:order.nbytes].view(np.int32), b[order.nbytes:].view(cell_dtype())
            allc += [(int(o[k]), record_to_dict(rr[k])) for k in range(MAXC) if o[k] >= 0]
    else:
        allc = [(int(order[k]), record_to_dict(rec[k])) for k in range(MAXC) if order[k] >= 0]
    allc.sort(key=lambda x: x[0])
    return [c for _, c in allc], dict(pow=pow_, frq=frq, sp_incoherent=sp_inc, n_comb_xc=n_comb_xc)


def search_capbuf_foe_split_dev(searcher, capbuf, f_search_set, fc_requested, fc_programmed, fs_programmed, rank=0, world=1,
                                dist=None, device=None):
    """The same split with everything between the correlation and the peak search staying on the GPUs: `searcher`
    (a Searcher on this rank's GPU) leaves the packed (pow, ~foi) words and the power estimate in two torch tensors on
    `device` (lcs_foe_partial), torch.distributed reduces / broadcasts them in place (RCCL: one 230 KB MAX all-reduce, one
    77 KB broadcast, and a second 230 KB MAX all-reduce of the exactly recomputed near-ties, lcs_foe_contend -- no host copy of
    any array), lcs_foe_finish takes them back.  Only the decoded cell records (a few
    hundred bytes) travel through the host, in one all-gather.  Returns (cells in peak order, peak list)."""
    import torch
    f = np.asarray(f_search_set, np.float64)
    own = foe_blocks(f.size, world)[rank]
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    words = torch.empty(3 * 9600, dtype=torch.int64, device=dev)
    meta = torch.empty(9601, dtype=torch.float64, device=dev)
    searcher.foe_partial(capbuf, f, int(own[0]) if own.size else 0, int(own.size), fc_requested, fc_programmed, fs_programmed,
                         words.data_ptr(), meta.data_ptr())
    if dist is not None:
        dist.all_reduce(words, op=dist.ReduceOp.MAX)
        dist.broadcast(meta, src=0)
        torch.cuda.synchronize(dev)
    # near-ties of the arg-max (within one rank's share or across two): every contending rank recomputes its contenders and the
    # global winner in the reference's arithmetic; a second MAX all-reduce makes the exact winner everybody's (lcs.h)
    words2 = torch.empty(3 * 9600, dtype=torch.int64, device=dev)
    searcher.foe_contend(f, words.data_ptr(), words2.data_ptr())
    if dist is not None:
        dist.all_reduce(words2, op=dist.ReduceOp.MAX)
        torch.cuda.synchronize(dev)
    searcher.foe_resolve(words.data_ptr(), words2.data_ptr())
    cells, order, peaks = searcher.foe_finish(words.data_ptr(), meta.data_ptr(), f)
    rec = np.zeros(MAXC, cell_dtype())
    ordv = np.full(MAXC, -1, np.int32)
    n = min(len(cells), MAXC)
    if n:
        rec[:n] = cells_to_records(cells[:n])
        ordv[:n] = order[:n]
    if dist is not None:
        gdev = dev if dist.get_backend() == "nccl" else None        # the record gather of a gloo test run goes through host tensors
        blobs = _all_gather_bytes(np.concatenate([ordv.view(np.uint8), rec.view(np.uint8)]), dist, gdev, world)
    else:
        blobs = [np.concatenate([ordv.view(np.uint8), rec.view(np.uint8)])]
    allc = []
    for b in blobs:
        o, rr = b[:ordv.nbytes].view(np.int32), b[ordv.nbytes:].view(cell_dtype())
        allc += [(int(o[k]), record_to_dict(rr[k])) for k in range(MAXC) if o[k] >= 0]
    allc.sort(key=lambda x: x[0])
    return [c for _, c in allc], peaks
