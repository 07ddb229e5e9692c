"""lte-cell-scanner_amd -- MI355X-native LTE cell-search hot path.

Python host-side mirror of the reference's searcher interface (include/searcher.h:22-119):
the same seven functions with the same argument meaning, each a thin call through the C ABI
of liblcs_amd.so (include/lcs.h) into hand-written HIP kernels.  numpy arrays stand in for
the IT++ containers; 2-D results are [3][9600] row-major, 3-D results [t][idx][foi].

There is deliberately no CPU implementation here: without the HIP library / a GPU every
call raises (``SearcherError``).  The CPU oracle used by the tests lives in oracle/ and is
never imported from this package.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from . import synth
from . import sweep
from . import itfile
from . import tracker
from .capi import LcsCell, LcsTrackCell, TddInfo, CellMeas, CellMeasWide, PcfichInfo, PdcchCfg, PdcchInfo, PdcchScanCfg, PdcchScanInfo, PhichCfg, PhichInfo, PdschCfg, PdschInfo, FMT_C64, FMT_IQ_U8, FMT_C128, FMT_IQ_S8, FMT_IQ_S16, STAGE_PSS, STAGE_FULL, MAX_PEAKS, DUPLEX_FDD, DUPLEX_TDD, TDD_NOT_ESTIMATED, MEAS_NOT_MEASURED
from .capi import SicInfo, SIC_PSS, SIC_SSS, SIC_CRS, SIC_PBCH, SIC_ALL, SIC_MAX_ROUNDS

FS_LTE = 30720000.0        # include/constants.h:32
DS_COMB_ARM = 2            # src/CellSearch.cpp:484
THRESH2_N_SIGMA = 3        # src/CellSearch.cpp:528


class SearcherError(RuntimeError):
    pass


def _ref(rec):
    """a ctypes record by reference; None: a null pointer"""
    return None if rec is None else C.byref(rec)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def new_cell(**kw) -> LcsCell:
    c = LcsCell()
    capi.load().lcs_cell_init(C.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def f_search_set_for(freq_start: float, ppm: float, step: float = 5e3) -> np.ndarray:
    """Frequency-offset grid of the CLI (src/CellSearch.cpp:463-464); step = 5e3 is the reference's grid exactly.
    A TDD search (Searcher.set_duplex) needs step <= 4e3: its PSS/SSS frequency estimate is by itself unambiguous within +- 2330 Hz
    (normal CP) / +- 2000 Hz (extended) of the hypothesis only (include/lcs.h: lcs_set_duplex); host/CellSearch -x tdd uses 2.5e3.
    With Searcher.set_foe_unwrap(True) the estimate is unwrapped by a PSS-only one and TDD takes step = 5e3 as well: half the
    hypotheses for the same coverage (host/CellSearch -x tdd --foe-unwrap)."""
    n_extra = int(np.floor((freq_start * ppm / 1e6 + step / 2) / step))
    return np.arange(-n_extra, n_extra + 1) * float(step)


class Searcher:
    """One context = one GPU + stream + workspace (lcs_create / lcs_destroy)."""

    def __init__(self, device: int = -1, lib=None):
        self._lib = lib if lib is not None else capi.load()      # lib: another build from capi.load_other (developer A/B runs)
        h = C.c_void_p()
        rc = self._lib.lcs_create(device, C.byref(h))
        if rc != 0:
            raise SearcherError(f"lcs_create failed: {capi.ERRORS.get(rc, rc)} (an MI355X is required; no CPU fallback)")
        self._h = h
        self.device = device
        self._phich_cp_normal = True

    def close(self):
        if getattr(self, "_h", None):
            self._lib.lcs_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc, what, allow_overflow=False):
        if rc == 0 or (allow_overflow and rc == -4):
            return rc
        raise SearcherError(f"{what}: {capi.ERRORS.get(rc, rc)}: {self._lib.lcs_last_error(self._h).decode()}")

    def set_max_cells_in_flight(self, n: int):
        self._chk(self._lib.lcs_set_max_cells_in_flight(self._h, n), "lcs_set_max_cells_in_flight")

    # ---- searcher.h:22-41 -------------------------------------------------------------
    def xcorr_pss(self, capbuf, f_search_set, ds_comb_arm, fc_requested, fc_programmed, fs_programmed,
                  want_incoherent=True, want_xc=False, want_sp=False):
        cap = np.ascontiguousarray(capbuf, np.complex128)
        f = np.ascontiguousarray(f_search_set, np.float64)
        n_cap, n_f = cap.size, f.size
        out = dict(pow=np.empty((3, 9600)), frq=np.empty((3, 9600), np.int32),
                   single=np.empty((3, 9600, n_f), np.float32),
                   incoherent=np.empty((3, 9600, n_f), np.float32) if want_incoherent else None,
                   sp_incoherent=np.empty(9600))
        xc = np.empty((3, n_cap - 136, n_f), np.complex64) if want_xc else None
        sp = np.empty(((n_cap - 136 - 137) // 9600) * 9600) if want_sp else None
        ncx, ncs = C.c_uint16(0), C.c_uint16(0)
        rc = self._lib.lcs_xcorr_pss(self._h, _dp(cap), n_cap, _dp(f), n_f, int(ds_comb_arm), fc_requested,
                                     fc_programmed, fs_programmed, _dp(out["pow"]), _ip(out["frq"]),
                                     _fp(out["single"]), _fp(out["incoherent"]), _dp(out["sp_incoherent"]),
                                     xc.ctypes.data_as(C.POINTER(C.c_float)) if want_xc else None, _dp(sp),
                                     C.byref(ncx), C.byref(ncs))
        self._chk(rc, "lcs_xcorr_pss")
        out.update(n_comb_xc=ncx.value, n_comb_sp=ncs.value, xc=xc, sp=sp)
        return out

    # ---- searcher.h:44-56 -------------------------------------------------------------
    def peak_search(self, pow_, frq, Z_th1, f_search_set, fc_requested, fc_programmed, single, ds_comb_arm,
                    max_cells=MAX_PEAKS):
        pow_ = np.ascontiguousarray(pow_, np.float64)
        frq = np.ascontiguousarray(frq, np.int32)
        Z = np.ascontiguousarray(Z_th1, np.float64)
        f = np.ascontiguousarray(f_search_set, np.float64)
        single = np.ascontiguousarray(single, np.float32)
        cells = (LcsCell * max_cells)()
        n = C.c_int(0)
        rc = self._lib.lcs_peak_search(self._h, _dp(pow_), _ip(frq), _dp(Z), _dp(f), f.size, fc_requested,
                                       fc_programmed, _fp(single), int(ds_comb_arm), cells, max_cells, C.byref(n))
        self._chk(rc, "lcs_peak_search")
        return [cells[i].copy() for i in range(n.value)]

    # ---- searcher.h:59-76 -------------------------------------------------------------
    def sss_detect(self, cell, capbuf, thresh2_n_sigma, fc_requested, fc_programmed, fs_programmed):
        cap = np.ascontiguousarray(capbuf, np.complex128)
        out = LcsCell()
        d = dict(h1_np=np.empty(62), h2_np=np.empty(62), h1_nrm=np.empty(62, np.complex128),
                 h2_nrm=np.empty(62, np.complex128), h1_ext=np.empty(62, np.complex128),
                 h2_ext=np.empty(62, np.complex128), ll_nrm=np.empty((168, 2)), ll_ext=np.empty((168, 2)))
        rc = self._lib.lcs_sss_detect(self._h, C.byref(cell), _dp(cap), cap.size, thresh2_n_sigma, fc_requested,
                                      fc_programmed, fs_programmed, C.byref(out), _dp(d["h1_np"]), _dp(d["h2_np"]),
                                      _dp(d["h1_nrm"]), _dp(d["h2_nrm"]), _dp(d["h1_ext"]), _dp(d["h2_ext"]),
                                      _dp(d["ll_nrm"]), _dp(d["ll_ext"]))
        self._chk(rc, "lcs_sss_detect")
        return out, d

    # ---- searcher.h:79-85 -------------------------------------------------------------
    def pss_sss_foe(self, cell, capbuf, fc_requested, fc_programmed, fs_programmed):
        cap = np.ascontiguousarray(capbuf, np.complex128)
        out = LcsCell()
        rc = self._lib.lcs_pss_sss_foe(self._h, C.byref(cell), _dp(cap), cap.size, fc_requested, fc_programmed,
                                       fs_programmed, C.byref(out))
        self._chk(rc, "lcs_pss_sss_foe")
        return out

    # ---- searcher.h:88-98 -------------------------------------------------------------
    def extract_tfg(self, cell, capbuf, fc_requested, fc_programmed, fs_programmed):
        cap = np.ascontiguousarray(capbuf, np.complex128)
        tfg = np.zeros((854, 72), np.complex128)
        ts = np.zeros(854)
        n = C.c_int(0)
        rc = self._lib.lcs_extract_tfg(self._h, C.byref(cell), _dp(cap), cap.size, fc_requested, fc_programmed,
                                       fs_programmed, _dp(tfg), _dp(ts), C.byref(n))
        self._chk(rc, "lcs_extract_tfg")
        return tfg[:n.value].copy(), ts[:n.value].copy()

    # ---- searcher.h:101-112 -----------------------------------------------------------
    def tfoec(self, cell, tfg, tfg_timestamp, fc_requested, fc_programmed):
        tfg = np.ascontiguousarray(tfg, np.complex128)
        ts = np.ascontiguousarray(tfg_timestamp, np.float64)
        tfgc, tsc = np.empty_like(tfg), np.empty_like(ts)
        out = LcsCell()
        rc = self._lib.lcs_tfoec(self._h, C.byref(cell), _dp(tfg), _dp(ts), tfg.shape[0], fc_requested,
                                 fc_programmed, _dp(tfgc), _dp(tsc), C.byref(out))
        self._chk(rc, "lcs_tfoec")
        return out, tfgc, tsc

    # ---- searcher.h:115-119 -----------------------------------------------------------
    def decode_mib(self, cell, tfg):
        tfg = np.ascontiguousarray(tfg, np.complex128)
        out = LcsCell()
        rc = self._lib.lcs_decode_mib(self._h, C.byref(cell), _dp(tfg), tfg.shape[0], C.byref(out))
        self._chk(rc, "lcs_decode_mib")
        return out

    # ---- one forced candidate of decode_mib's twelve, before the CRC decides (exported for direct testing) ------
    def pbch_soft(self, cell, tfg, frame_timing_guess: int, n_ports: int):
        """-> (e_est [1920 | 1728] descrambled LLRs, d_est [3][40] de-rate-matched, c_est [40] uint8 decoded bits, crc_ok)"""
        tfg = np.ascontiguousarray(tfg, np.complex128)
        e, d = np.zeros(1920), np.zeros((3, 40))
        bits, ok = C.c_uint64(0), C.c_int(0)
        rc = self._lib.lcs_pbch_soft(self._h, C.byref(cell), _dp(tfg), tfg.shape[0], int(frame_timing_guess), int(n_ports),
                                     _dp(e), _dp(d), C.byref(bits), C.byref(ok))
        self._chk(rc, "lcs_pbch_soft")
        c_est = np.array([(bits.value >> t) & 1 for t in range(40)], np.uint8)
        return e[:1920 if tfg.shape[0] == 854 else 1728].copy(), d, c_est, bool(ok.value)

    # ---- searcher.cpp:1369-1477 (internal to decode_mib; exported for direct testing) ------
    def chan_est(self, cell, tfg, port: int):
        tfg = np.ascontiguousarray(tfg, np.complex128)
        ce = np.empty_like(tfg)
        npw = C.c_double(0)
        self._chk(self._lib.lcs_chan_est(self._h, C.byref(cell), _dp(tfg), tfg.shape[0], int(port), _dp(ce), C.byref(npw)), "lcs_chan_est")
        return ce, npw.value

    # ---- CellSearch.cpp:484-558, one buffer -----------------------------------------
    def search_capbuf(self, capbuf, f_search_set, fc_requested, fc_programmed, fs_programmed, max_cells=MAX_PEAKS):
        cap = np.ascontiguousarray(capbuf, np.complex128)
        f = np.ascontiguousarray(f_search_set, np.float64)
        cells, peaks = (LcsCell * max_cells)(), (LcsCell * MAX_PEAKS)()
        n, npk = C.c_int(0), C.c_int(0)
        rc = self._lib.lcs_search_capbuf(self._h, _dp(cap), cap.size, _dp(f), f.size, fc_requested, fc_programmed,
                                         fs_programmed, cells, max_cells, C.byref(n), peaks, MAX_PEAKS, C.byref(npk))
        self._chk(rc, "lcs_search_capbuf")
        return [cells[i].copy() for i in range(min(n.value, max_cells))], [peaks[i].copy() for i in range(min(npk.value, MAX_PEAKS))]

    # ---- one buffer, hypotheses split over GPUs (lcs_foe_*; driver: sweep.search_capbuf_foe_split_dev) ----
    def foe_partial(self, capbuf, f_search_set, f_first: int, f_count: int, fc_requested, fc_programmed, fs_programmed,
                    d_words_ptr: int, d_meta_ptr: int):
        cap = np.ascontiguousarray(capbuf, np.complex128)
        f = np.ascontiguousarray(f_search_set, np.float64)
        self._chk(self._lib.lcs_foe_partial(self._h, _dp(cap), cap.size, _dp(f), f.size, int(f_first), int(f_count), fc_requested,
                                            fc_programmed, fs_programmed, C.c_void_p(d_words_ptr), C.c_void_p(d_meta_ptr)), "lcs_foe_partial")

    def foe_contend(self, f_search_set, d_words_ptr: int, d_words2_ptr: int):
        """After the MAX all-reduce of the words: this rank's exact packed maxima at the positions it contends for (-1 elsewhere)
        into d_words2, which the caller MAX-all-reduces in turn (lcs_foe_contend)."""
        f = np.ascontiguousarray(f_search_set, np.float64)
        self._chk(self._lib.lcs_foe_contend(self._h, _dp(f), f.size, C.c_void_p(d_words_ptr), C.c_void_p(d_words2_ptr)), "lcs_foe_contend")

    def foe_resolve(self, d_words_ptr: int, d_words2_ptr: int):
        """The reduced exact words take the place of the approximate ones (lcs_foe_resolve); then foe_finish."""
        self._chk(self._lib.lcs_foe_resolve(self._h, C.c_void_p(d_words_ptr), C.c_void_p(d_words2_ptr)), "lcs_foe_resolve")

    def foe_finish(self, d_words_ptr: int, d_meta_ptr: int, f_search_set, max_cells: int = MAX_PEAKS):
        """-> (cells this rank decoded, their positions in the peak list, the whole peak list)"""
        f = np.ascontiguousarray(f_search_set, np.float64)
        cells, peaks = (LcsCell * max_cells)(), (LcsCell * MAX_PEAKS)()
        order = np.zeros(max_cells, np.int32)
        n, npk = C.c_int(0), C.c_int(0)
        rc = self._lib.lcs_foe_finish(self._h, C.c_void_p(d_words_ptr), C.c_void_p(d_meta_ptr), _dp(f), f.size, cells, _ip(order), max_cells,
                                      C.byref(n), peaks, MAX_PEAKS, C.byref(npk))
        self._chk(rc, "lcs_foe_finish")
        return [cells[i].copy() for i in range(n.value)], order[:n.value].copy(), [peaks[i].copy() for i in range(min(npk.value, MAX_PEAKS))]

    # ---- batched, device-resident ---------------------------------------------------
    def batch_enqueue(self, d_ptr: int, fmt: int, n_buf: int, n_cap: int, f_search_set, fc_requested, fc_programmed,
                      fs_programmed: float, stage_mask: int = STAGE_FULL):
        f = np.ascontiguousarray(f_search_set, np.float64)
        fr = np.ascontiguousarray(np.broadcast_to(np.asarray(fc_requested, np.float64), (n_buf,)))
        fp_ = np.ascontiguousarray(np.broadcast_to(np.asarray(fc_programmed, np.float64), (n_buf,)))
        rc = self._lib.lcs_batch_enqueue(self._h, C.c_void_p(d_ptr), fmt, n_buf, n_cap, _dp(f), f.size, _dp(fr),
                                         _dp(fp_), fs_programmed, stage_mask)
        self._chk(rc, "lcs_batch_enqueue")

    def batch_collect(self, n_buf: int, max_cells_per_buf: int = 16):
        """-> per-buffer cell lists.  LCS_ERR_OVERFLOW (more peaks / cells than the library's or the caller's
        arrays hold: results truncated) is surfaced as a warning and kept in ``self.last_overflow``."""
        cells = (LcsCell * (n_buf * max_cells_per_buf))()
        cnt = (C.c_int * n_buf)()
        rc = self._lib.lcs_batch_collect(self._h, cells, max_cells_per_buf, cnt)
        self._note_overflow(self._chk(rc, "lcs_batch_collect", allow_overflow=True), "lcs_batch_collect")
        return [[cells[b * max_cells_per_buf + i].copy() for i in range(min(cnt[b], max_cells_per_buf))]
                for b in range(n_buf)]

    def _note_overflow(self, rc, what, stacklevel=3):
        self.last_overflow = rc == -4
        if self.last_overflow:
            import warnings
            warnings.warn(f"{what}: LCS_ERR_OVERFLOW: {self._lib.lcs_last_error(self._h).decode()} (results truncated)",
                          RuntimeWarning, stacklevel=stacklevel)

    def batch_readback(self, buf: int, n_f: int):
        """xcorr_pss outputs of buffer `buf` of the last batch in the reference's layouts (debug)."""
        out = dict(single=np.empty((3, 9600, n_f), np.float32), pow=np.empty((3, 9600)), frq=np.empty((3, 9600), np.int32),
                   sp_incoherent=np.empty(9600), z_th1=np.empty(9600))
        self._chk(self._lib.lcs_batch_readback(self._h, buf, _fp(out["single"]), _dp(out["pow"]), _ip(out["frq"]),
                                               _dp(out["sp_incoherent"]), _dp(out["z_th1"])), "lcs_batch_readback")
        return out

    def search_batch_host(self, h_capbufs, fmt: int, n_buf: int, n_cap: int, f_search_set, fc_requested, fc_programmed,
                          fs_programmed: float, stage_mask: int = STAGE_FULL, max_cells_per_buf: int = 16):
        a = np.ascontiguousarray(h_capbufs, dtype=np.uint8 if fmt == FMT_IQ_U8 else np.complex64)
        assert a.size == n_buf * n_cap * (2 if fmt == FMT_IQ_U8 else 1)
        f = np.ascontiguousarray(f_search_set, np.float64)
        fr = np.ascontiguousarray(np.broadcast_to(np.asarray(fc_requested, np.float64), (n_buf,)))
        fp_ = np.ascontiguousarray(np.broadcast_to(np.asarray(fc_programmed, np.float64), (n_buf,)))
        cells = (LcsCell * (n_buf * max_cells_per_buf))()
        cnt = (C.c_int * n_buf)()
        rc = self._lib.lcs_search_batch_host(self._h, a.ctypes.data_as(C.c_void_p), fmt, n_buf, n_cap, _dp(f), f.size, _dp(fr),
                                             _dp(fp_), fs_programmed, stage_mask, cells, max_cells_per_buf, cnt)
        self._note_overflow(self._chk(rc, "lcs_search_batch_host", allow_overflow=True), "lcs_search_batch_host")
        return [[cells[b * max_cells_per_buf + i].copy() for i in range(min(cnt[b], max_cells_per_buf))]
                for b in range(n_buf)]

    def host_alloc(self, n_bytes: int) -> np.ndarray:
        """Page-locked host memory as a uint8 array (lcs_host_alloc): batch_enqueue_host DMAs from it without staging.
        Keep the Searcher alive while the array is in use; host_free() releases it."""
        p = C.c_void_p()
        self._chk(self._lib.lcs_host_alloc(self._h, n_bytes, C.byref(p)), "lcs_host_alloc")
        a = np.ctypeslib.as_array((C.c_uint8 * n_bytes).from_address(p.value))
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[a.ctypes.data] = p
        return a

    def host_free(self, a: np.ndarray):
        p = self._pinned.pop(a.ctypes.data)
        self._chk(self._lib.lcs_host_free(self._h, p), "lcs_host_free")

    def batch_enqueue_host(self, h_capbufs, fmt: int, n_buf: int, n_cap: int, f_search_set, fc_requested, fc_programmed,
                           fs_programmed: float, stage_mask: int = STAGE_FULL):
        """Asynchronous host-fed batch (lcs_batch_enqueue_host): returns once the copy and the kernels are queued;
        results come from batch_collect / batch_collect_raw.  The array must stay untouched until then."""
        # (the same lifetime rule holds for batch_enqueue's DEVICE buffers: complex<float> batches are read in place by
        # every stage until batch_collect returns -- include/lcs.h)
        a = h_capbufs if (isinstance(h_capbufs, np.ndarray) and h_capbufs.flags.c_contiguous) else np.ascontiguousarray(h_capbufs)
        assert a.nbytes == n_buf * n_cap * (2 if fmt == FMT_IQ_U8 else 8)
        f = np.ascontiguousarray(f_search_set, np.float64)
        fr = np.ascontiguousarray(np.broadcast_to(np.asarray(fc_requested, np.float64), (n_buf,)))
        fp_ = np.ascontiguousarray(np.broadcast_to(np.asarray(fc_programmed, np.float64), (n_buf,)))
        self._keep = a
        rc = self._lib.lcs_batch_enqueue_host(self._h, a.ctypes.data_as(C.c_void_p), fmt, n_buf, n_cap, _dp(f), f.size, _dp(fr),
                                              _dp(fp_), fs_programmed, stage_mask)
        self._chk(rc, "lcs_batch_enqueue_host")

    def search_batch(self, d_ptr: int, fmt: int, n_buf: int, n_cap: int, f_search_set, fc_requested, fc_programmed,
                     fs_programmed: float, stage_mask: int = STAGE_FULL, max_cells_per_buf: int = 16):
        self.batch_enqueue(d_ptr, fmt, n_buf, n_cap, f_search_set, fc_requested, fc_programmed, fs_programmed, stage_mask)
        return self.batch_collect(n_buf, max_cells_per_buf)

    # ---- successive cancellation (include/lcs.h: lcs_sic_cancel_dev, lcs_search_*_sic; the rule: csrc/sic.h) ----
    def sic_cancel(self, d_ptr: int, fmt: int, n_buf: int, n_cap: int, cells, fc_requested, fc_programmed, fs_programmed: float,
                   d_residual_ptr: int, mask: int = SIC_ALL, ul_dl_config=None):
        """Rebuild the known signals (PSS, SSS, CRS, PBCH: `mask`) of cells[b] -- the decoded records of buffer b -- and subtract them
        from the n_buf device-resident captures at d_ptr (FMT_IQ_U8 or FMT_C64) into the complex64 buffer [n_buf][n_cap] at
        d_residual_ptr.  ul_dl_config (TDD): per buffer a list with each record's uplink-downlink configuration (0..6 as last_tdd_info
        reports it, anything else: none) -- CRS and PBCH then go in that configuration's downlink subframes and in symbol 0 of
        subframes 1 and 6 too, not in subframes 0 and 5 alone.  -> [n_buf] lists of SicInfo, one per record."""
        per = max(1, max((len(c) for c in cells), default=1))
        arr = (LcsCell * (n_buf * per))()
        for b in range(n_buf):
            for i, c in enumerate(cells[b]):
                arr[b * per + i] = c
        cnt = np.array([len(cells[b]) for b in range(n_buf)], np.int32)
        fr = np.ascontiguousarray(np.broadcast_to(np.asarray(fc_requested, np.float64), (n_buf,)))
        fp_ = np.ascontiguousarray(np.broadcast_to(np.asarray(fc_programmed, np.float64), (n_buf,)))
        info = (SicInfo * (n_buf * per))()
        cfg = None
        if ul_dl_config is not None:
            cfg = np.full(n_buf * per, capi.TDD_NOT_ESTIMATED, np.int32)
            for b in range(n_buf):
                for i, v in enumerate(ul_dl_config[b]):
                    cfg[b * per + i] = int(v)
        rc = self._lib.lcs_sic_cancel_cfg_dev(self._h, C.c_void_p(d_ptr), fmt, n_buf, n_cap, arr, _ip(cnt), per, _ip(cfg), _dp(fr), _dp(fp_),
                                              fs_programmed, int(mask), C.c_void_p(d_residual_ptr), info)
        self._chk(rc, "lcs_sic_cancel_cfg_dev")
        return [[info[b * per + i].copy() for i in range(cnt[b])] for b in range(n_buf)]

    def search_capbuf_sic(self, capbuf, f_search_set, fc_requested, fc_programmed, fs_programmed, max_rounds: int = 2, mask: int = SIC_ALL,
                          max_cells=MAX_PEAKS):
        """search_capbuf, then up to max_rounds - 1 rounds that cancel every cell found so far from the capture and search the
        residual.  -> (cells, rounds, info): the round each cell was found in (0: the plain search, whose records these are) and the
        SicInfo of the last cancellation it took part in."""
        cap = np.ascontiguousarray(capbuf, np.complex128)
        f = np.ascontiguousarray(f_search_set, np.float64)
        cells, peaks = (LcsCell * max_cells)(), (LcsCell * MAX_PEAKS)()
        n, npk = C.c_int(0), C.c_int(0)
        rounds, info = np.zeros(max_cells, np.int32), (SicInfo * max_cells)()
        rc = self._lib.lcs_search_capbuf_sic(self._h, _dp(cap), cap.size, _dp(f), f.size, fc_requested, fc_programmed, fs_programmed, cells,
                                             max_cells, C.byref(n), peaks, MAX_PEAKS, C.byref(npk), int(max_rounds), int(mask), _ip(rounds), info)
        self._chk(rc, "lcs_search_capbuf_sic")
        k = min(n.value, max_cells)
        return [cells[i].copy() for i in range(k)], [int(r) for r in rounds[:k]], [info[i].copy() for i in range(k)]

    def search_batch_sic(self, d_ptr: int, fmt: int, n_buf: int, n_cap: int, f_search_set, fc_requested, fc_programmed, fs_programmed: float,
                         max_rounds: int = 2, mask: int = SIC_ALL, max_cells_per_buf: int = 16):
        """search_batch (the full chain) with cancellation rounds, per buffer as search_capbuf_sic -> (cells, rounds, info), each [n_buf] lists"""
        f = np.ascontiguousarray(f_search_set, np.float64)
        fr = np.ascontiguousarray(np.broadcast_to(np.asarray(fc_requested, np.float64), (n_buf,)))
        fp_ = np.ascontiguousarray(np.broadcast_to(np.asarray(fc_programmed, np.float64), (n_buf,)))
        m = max_cells_per_buf
        cells, info = (LcsCell * (n_buf * m))(), (SicInfo * (n_buf * m))()
        n, rounds = np.zeros(n_buf, np.int32), np.zeros(n_buf * m, np.int32)
        rc = self._lib.lcs_search_batch_sic_dev(self._h, C.c_void_p(d_ptr), fmt, n_buf, n_cap, _dp(f), f.size, _dp(fr), _dp(fp_), fs_programmed, cells, m,
                                                n.ctypes.data_as(C.POINTER(C.c_int)), int(max_rounds), int(mask), _ip(rounds), info)
        self._chk(rc, "lcs_search_batch_sic_dev")
        k = [min(int(x), m) for x in n]
        return ([[cells[b * m + i].copy() for i in range(k[b])] for b in range(n_buf)], [[int(rounds[b * m + i]) for i in range(k[b])] for b in range(n_buf)],
                [[info[b * m + i].copy() for i in range(k[b])] for b in range(n_buf)])

    def last_sic_tdd_info(self, n_buf: int = 1, max_cells_per_buf: int = MAX_PEAKS):
        """The TddInfo of every cell the last search_*_sic call returned, laid out like its cells (a cell of round r: what round r's chain
        estimated); max_cells_per_buf is that call's (search_capbuf_sic: max_cells).  last_tdd_info() itself describes the last ROUND."""
        return self._last_records("lcs_last_sic_tdd_info", capi.TddInfo, n_buf, max_cells_per_buf)

    def last_sic_cell_meas(self, n_buf: int = 1, max_cells_per_buf: int = MAX_PEAKS):
        """likewise the CellMeas records (a cell found in round r >= 1 is measured on the residual it was found in)"""
        return self._last_records("lcs_last_sic_cell_meas", capi.CellMeas, n_buf, max_cells_per_buf)

    def last_sic_stats(self) -> dict:
        """the last search_*_sic call: rounds run (1: the plain search alone), cancellation launches, cells added, duplicates dropped"""
        st = (C.c_int * 4)()
        self._chk(self._lib.lcs_last_sic_stats(self._h, C.byref(st)), "lcs_last_sic_stats")
        return dict(rounds=st[0], cancellations=st[1], added=st[2], dropped=st[3])

    # ---- LTE-Tracker's per-symbol pipeline on a block of symbols (src/tracker_thread.cpp:823-1068) ----
    def track_block(self, cells, td, freq_off, frame_timing, late, fc_requested, fc_programmed, fs_programmed,
                    want_syms=True, want_ce=True, td_device_ptr=None, n_sym=None, out=None):
        """cells: list of searcher records (LcsCell with n_id_1/2, cp_type, n_ports, n_rb_dl, PHICH fields) or LcsTrackCell;
        td [n_cells][n_sym][128] complex128 (or a device pointer via td_device_ptr + n_sym); the metadata arrays are
        [n_cells][n_sym].  Returns a dict (see lcs_track_block in include/lcs.h); 'bpo' = bulk phase after the block."""
        n_cells = len(cells)
        tc = (capi.LcsTrackCell * n_cells)()
        for i, c in enumerate(cells):
            for f in ("n_id_1", "n_id_2", "cp_type", "n_ports", "n_rb_dl", "phich_duration", "phich_resource"):
                setattr(tc[i], f, int(getattr(c, f)))
            tc[i].bulk_phase_offset = float(getattr(c, "bulk_phase_offset", 0.0))
        fo = np.ascontiguousarray(freq_off, np.float64).reshape(n_cells, -1)
        n_sym = fo.shape[1] if n_sym is None else n_sym
        ft = np.ascontiguousarray(frame_timing, np.float64).reshape(n_cells, n_sym)
        lt = np.ascontiguousarray(late, np.float64).reshape(n_cells, n_sym)
        if td_device_ptr is None:
            tdh = np.ascontiguousarray(td, np.complex128).reshape(n_cells, n_sym, 128)
            tdp, on_dev = tdh.ctypes.data_as(C.c_void_p), 0
        else:
            tdp, on_dev = C.c_void_p(td_device_ptr), 1
        max_rs, max_off = n_sym // 3 + 4, max(1, n_sym // 120 - 3)
        if out is not None:      # a dict this method returned for the same block shape: its arrays are reused (rows beyond n_meas keep old values)
            assert out["meas"].shape == (n_cells, 4, max_rs, 9) and out["mib_ok"].shape == (n_cells, max_off)
            assert (out["syms"] is not None) == bool(want_syms) and (out["ce"] is not None) == bool(want_ce)
        else:
            out = dict(syms=np.empty((n_cells, n_sym, 72), np.complex128) if want_syms else None,
                       ce=np.full((n_cells, 4, n_sym, 72), np.nan + 0j, np.complex128) if want_ce else None,
                       ce_pw=np.full((n_cells, 4, n_sym, 4), np.nan) if want_ce else None,
                       ce_upto=np.zeros((n_cells, 4), np.int32), meas=np.full((n_cells, 4, max_rs, 9), np.nan),
                       n_meas=np.zeros((n_cells, 4), np.int32), mib_ok=np.full((n_cells, max_off), -1, np.int32),
                       mib_bits=np.zeros((n_cells, max_off), np.uint64))
        ms = C.c_float(0)
        rc = self._lib.lcs_track_block(self._h, tc, n_cells, n_sym, tdp, on_dev, _dp(fo), _dp(ft), _dp(lt), fc_requested, fc_programmed,
                                       fs_programmed, _dp(out["syms"]), _dp(out["ce"]), _dp(out["ce_pw"]), _ip(out["ce_upto"]),
                                       _dp(out["meas"]), max_rs, _ip(out["n_meas"]), _ip(out["mib_ok"]),
                                       out["mib_bits"].ctypes.data_as(C.POINTER(C.c_uint64)), max_off, C.byref(ms))
        self._chk(rc, "lcs_track_block")
        out["bpo"] = np.array([tc[i].bulk_phase_offset for i in range(n_cells)])
        out["gpu_ms"] = ms.value
        return out

    def _mode(self, getter: str) -> int:
        """a context setting through its lcs_get_* function"""
        d = C.c_int(-1)
        self._chk(getattr(self._lib, getter)(self._h, C.byref(d)), getter)
        return d.value

    def _last_records(self, what: str, rec, n_buf: int, max_cells_per_buf: int):
        """a side table of the last fused call (lcs_last_tdd_info, lcs_last_cell_meas) -> [n_buf][max_cells_per_buf] records"""
        info = (rec * (n_buf * max_cells_per_buf))()
        rc = getattr(self._lib, what)(self._h, info, max_cells_per_buf)
        self._note_overflow(self._chk(rc, what, allow_overflow=True), what, stacklevel=4)      # the warning names the public method's caller
        return [[info[b * max_cells_per_buf + i].copy() for i in range(max_cells_per_buf)] for b in range(n_buf)]

    def set_duplex(self, duplex: int):
        """DUPLEX_FDD (default) or DUPLEX_TDD: where sss_detect and pss_sss_foe look for the SSS relative to the PSS, for every call
        on this searcher (lcs_set_duplex, include/lcs.h).  Refused for any other value and while a stream is open."""
        self._chk(self._lib.lcs_set_duplex(self._h, int(duplex)), "lcs_set_duplex")

    @property
    def duplex(self) -> int:
        return self._mode("lcs_get_duplex")

    def set_foe_unwrap(self, on: bool):
        """pss_sss_foe unwrapped by a PSS-only coarse estimate, for every call on this searcher (lcs_set_foe_unwrap, include/lcs.h):
        the native estimate aliases by whole periods fs / pss_sss_dist -- 4660 / 4000 Hz in TDD --, and the phase between the two
        halves of the PSS picks the period.  With it a TDD band is searched on the reference's 5 kHz grid.  Off by default (every
        record is then what it was, bit for bit); refused while a stream is open."""
        self._chk(self._lib.lcs_set_foe_unwrap(self._h, 1 if on else 0), "lcs_set_foe_unwrap")

    @property
    def foe_unwrap(self) -> bool:
        return self._mode("lcs_get_foe_unwrap") != 0

    def pss_foe_coarse(self, cell, capbuf, fc_requested, fc_programmed, fs_programmed):
        """The coarse estimate as a stage of its own (lcs_pss_foe_coarse), in the searcher's duplex mode and whatever the unwrap
        setting -> (f_coarse in Hz relative to cell.freq, C, occurrences summed)"""
        cap = np.ascontiguousarray(capbuf, np.complex128)
        f, c2, n = C.c_double(0.0), (C.c_double * 2)(), C.c_int(0)
        rc = self._lib.lcs_pss_foe_coarse(self._h, C.byref(cell), _dp(cap), cap.size, fc_requested, fc_programmed, fs_programmed,
                                          C.byref(f), c2, C.byref(n))
        self._chk(rc, "lcs_pss_foe_coarse")
        return f.value, complex(c2[0], c2[1]), n.value

    def set_tdd_config(self, on: bool):
        """Estimate the uplink-downlink configuration (36.211 table 4.2-2) and the DwPTS class of every cell a fused call decodes,
        from its reference signals on the device (lcs_set_tdd_config, include/lcs.h); last_tdd_info() reads the records.  It takes
        effect in DUPLEX_TDD only.  Off by default (every record is then what it was, bit for bit); refused while a stream is open,
        and stream_open is refused while it is on."""
        self._chk(self._lib.lcs_set_tdd_config(self._h, 1 if on else 0), "lcs_set_tdd_config")

    @property
    def tdd_config_mode(self) -> bool:
        return self._mode("lcs_get_tdd_config") != 0

    def tdd_config(self, cell, tfg):
        """The estimate as a stage of its own (lcs_tdd_config): a cell with identity and CP type and its grid from extract_tfg, raw
        or compensated, two frames to 854 rows -> TddInfo"""
        tfg = np.ascontiguousarray(tfg, np.complex128)
        out = capi.TddInfo()
        self._chk(self._lib.lcs_tdd_config(self._h, C.byref(cell), _dp(tfg), tfg.shape[0], C.byref(out)), "lcs_tdd_config")
        return out

    def last_tdd_info(self, n_buf: int = 1, max_cells_per_buf: int = 16):
        """The records of the last search_capbuf (n_buf = 1) or batch: per buffer a list of max_cells_per_buf TddInfo, entry k
        belonging to cell k of that buffer; the entries behind a buffer's cells, and all of them without the mode, read
        TDD_NOT_ESTIMATED (lcs_last_tdd_info)."""
        return self._last_records("lcs_last_tdd_info", capi.TddInfo, n_buf, max_cells_per_buf)

    def set_cell_meas(self, on: bool):
        """Measure RSRP, RSSI, RSRQ and the noise power of every cell a fused call decodes, from its reference signals on the device
        (lcs_set_cell_meas, include/lcs.h); last_cell_meas() reads the records.  Off by default (every record is then what it was,
        bit for bit, and no kernel is added); refused while a stream is open, and stream_open is refused while it is on."""
        self._chk(self._lib.lcs_set_cell_meas(self._h, 1 if on else 0), "lcs_set_cell_meas")

    @property
    def cell_meas_mode(self) -> bool:
        return self._mode("lcs_get_cell_meas") != 0

    def cell_meas(self, cell, tfg, dl_mask: int = 0x3FF):
        """The measurement as a stage of its own (lcs_cell_meas): a cell with identity and CP type (n_ports 0 / unknown: port 0 alone)
        and its grid from extract_tfg, raw or compensated, two frames to 854 rows; dl_mask: bit s set = subframe s is measured
        (tdd_dl_mask(configuration) for a TDD cell) -> CellMeas"""
        tfg = np.ascontiguousarray(tfg, np.complex128)
        out = capi.CellMeas()
        self._chk(self._lib.lcs_cell_meas(self._h, C.byref(cell), _dp(tfg), tfg.shape[0], int(dl_mask), C.byref(out)), "lcs_cell_meas")
        return out

    def last_cell_meas(self, n_buf: int = 1, max_cells_per_buf: int = 16):
        """The records of the last search_capbuf (n_buf = 1) or batch: per buffer a list of max_cells_per_buf CellMeas, entry k
        belonging to cell k of that buffer; the entries behind a buffer's cells, and all of them without the mode, read
        MEAS_NOT_MEASURED (lcs_last_cell_meas)."""
        return self._last_records("lcs_last_cell_meas", capi.CellMeas, n_buf, max_cells_per_buf)

    # ---- the full-bandwidth grid and measurement (lcs_extract_tfg_wide, lcs_cell_meas_wide) ---
    @staticmethod
    def _wide_samples(d_capbuf, n_cap):
        """a device pointer with its sample count, or a torch tensor of complex64 on the device (its whole length unless n_cap says less)"""
        if hasattr(d_capbuf, "data_ptr"):
            t = d_capbuf
            if str(t.dtype) != "torch.complex64" or not t.is_cuda or not t.is_contiguous():
                raise ValueError("the wide samples are a contiguous complex64 tensor on the device, or a device pointer and n_cap")
            return int(t.data_ptr()), int(t.numel() if n_cap is None else n_cap)
        if n_cap is None:
            raise ValueError("a device pointer needs n_cap")
        return int(d_capbuf), int(n_cap)

    def _wide_args(self, cell, d_capbuf, n_cap, fc_requested, fc_programmed, fs_programmed, n_fft, n_rb, n_ofdm):
        """the arguments every entry point on device samples starts with: the context, the cell, the samples, the frequencies, the
        grid's shape"""
        ptr, n_cap = self._wide_samples(d_capbuf, n_cap)
        return (self._h, C.byref(cell), C.c_void_p(ptr), n_cap, float(fc_requested), float(fc_programmed), float(fs_programmed), int(n_fft), int(n_rb),
                int(n_ofdm))

    def _grid_args(self, cell, tfg_wide, n_rb):
        """the same for the entry points on a grid from the host, tfg_wide [n_ofdm][12 n_rb] complex"""
        tfg = np.ascontiguousarray(tfg_wide, np.complex128)
        if tfg.ndim != 2 or tfg.shape[1] != 12 * int(n_rb):
            raise ValueError("tfg_wide is [n_ofdm][12 n_rb]")
        return (self._h, C.byref(cell), _dp(tfg), int(tfg.shape[0]), int(n_rb))

    def extract_tfg_wide(self, cell, d_capbuf, fc_requested, fc_programmed, fs_programmed, n_fft: int, n_rb: int, n_ofdm: int, n_cap=None):
        """The grid of a cell over n_rb resource blocks from complex64 samples at fs_programmed = 15 kHz x n_fft that are on the
        device, centred on the cell (a channel of channelize at decim = K / R): n_fft = 128 R, R in 1, 2, 4, 8, 16; cell.frame_start
        counts in those samples.  -> (tfg [n_ofdm][12 n_rb] complex128, the rows' ideal locations [n_ofdm])."""
        tfg = np.empty((max(int(n_ofdm), 0), 12 * max(int(n_rb), 0)), np.complex128)
        ts = np.empty(max(int(n_ofdm), 0))
        args = self._wide_args(cell, d_capbuf, n_cap, fc_requested, fc_programmed, fs_programmed, n_fft, n_rb, n_ofdm)
        self._chk(self._lib.lcs_extract_tfg_wide(*args, _dp(tfg), _dp(ts)), "lcs_extract_tfg_wide")
        return tfg, ts

    def cell_meas_wide(self, cell, d_capbuf, fc_requested, fc_programmed, fs_programmed, n_fft: int, n_rb: int, n_ofdm: int, dl_mask: int = 0x3FF,
                       n_cap=None):
        """RSRP, RSSI, RSRQ and the noise power over n_rb resource blocks, with the per-RB profile, from the same samples
        (lcs_cell_meas_wide: only port 0's reference rows are transformed) -> CellMeasWide"""
        out = capi.CellMeasWide()
        args = self._wide_args(cell, d_capbuf, n_cap, fc_requested, fc_programmed, fs_programmed, n_fft, n_rb, n_ofdm)
        self._chk(self._lib.lcs_cell_meas_wide(*args, int(dl_mask), C.byref(out)), "lcs_cell_meas_wide")
        return out

    def pcfich_wide(self, cell, d_capbuf, fc_requested, fc_programmed, fs_programmed, n_fft: int, n_rb: int, n_ofdm: int, dl_mask: int = 0x3FF,
                    n_cap=None):
        """The control format indicator of every downlink subframe from the same samples (lcs_pcfich_wide: only symbol 0 of every
        subframe of the mask is transformed, and symbol 1 for a 4-port cell); n_rb is the cell's bandwidth -> PcfichInfo"""
        out = capi.PcfichInfo()
        args = self._wide_args(cell, d_capbuf, n_cap, fc_requested, fc_programmed, fs_programmed, n_fft, n_rb, n_ofdm)
        self._chk(self._lib.lcs_pcfich_wide(*args, int(dl_mask), C.byref(out)), "lcs_pcfich_wide")
        return out

    def pcfich(self, cell, tfg_wide, n_rb: int, dl_mask: int = 0x3FF):
        """The same stage on a grid from the host, tfg_wide [n_ofdm][12 n_rb] complex whose row 0 is symbol 0 of slot 0 of a frame
        (extract_tfg_wide's) (lcs_pcfich) -> PcfichInfo"""
        out = capi.PcfichInfo()
        self._chk(self._lib.lcs_pcfich(*self._grid_args(cell, tfg_wide, n_rb), int(dl_mask), C.byref(out)), "lcs_pcfich")
        return out

    @staticmethod
    def _pdcch_cfg(cfg, n_rb):
        """a PdcchCfg as it is, or None: FDD, the cell's PHICH configuration, the two sizes of the common search space"""
        return cfg if cfg is not None else capi.PdcchCfg.make(capi.dci_common_sizes(int(n_rb), False))

    def pdcch_wide(self, cell, d_capbuf, fc_requested, fc_programmed, fs_programmed, n_fft: int, n_rb: int, n_ofdm: int, dl_mask: int = 0x3FF,
                   cfg=None, n_cap=None):
        """The DCIs of the PDCCH common search space (SI, paging, random-access responses) of every downlink subframe from the same
        samples (lcs_pdcch_wide: symbols 0 .. 2 of every subframe of the mask are transformed, 0 .. 3 up to 10 resource blocks; the
        CFI is the PCFICH's, decided on the device).  cfg: a capi.PdcchCfg; None = FDD defaults -> PdcchInfo"""
        args = self._wide_args(cell, d_capbuf, n_cap, fc_requested, fc_programmed, fs_programmed, n_fft, n_rb, n_ofdm)
        cfg = self._pdcch_cfg(cfg, n_rb)
        out = capi.PdcchInfo()
        self._chk(self._lib.lcs_pdcch_wide(*args, int(dl_mask), C.byref(cfg), C.byref(out)), "lcs_pdcch_wide")
        out.sizes = tuple(cfg.size[:cfg.n_sizes])
        return out

    def pdcch(self, cell, tfg_wide, n_rb: int, dl_mask: int = 0x3FF, cfg=None):
        """The same stage on a grid from the host, tfg_wide [n_ofdm][12 n_rb] complex whose row 0 is symbol 0 of slot 0 of a frame
        (extract_tfg_wide's) (lcs_pdcch) -> PdcchInfo"""
        args = self._grid_args(cell, tfg_wide, n_rb)
        cfg = self._pdcch_cfg(cfg, n_rb)
        out = capi.PdcchInfo()
        self._chk(self._lib.lcs_pdcch(*args, int(dl_mask), C.byref(cfg), C.byref(out)), "lcs_pdcch")
        out.sizes = tuple(cfg.size[:cfg.n_sizes])
        return out

    def pdcch_scan_wide(self, cell, d_capbuf, fc_requested, fc_programmed, fs_programmed, n_fft: int, n_rb: int, n_ofdm: int, dl_mask: int = 0x3FF,
                        cfg=None, n_cap=None):
        """The blind search of every CCE of every downlink subframe from the same samples (lcs_pdcch_scan_wide): the grants the cell
        gives to its users, their RNTIs and the CCEs they cover.  cfg: a capi.PdcchScanCfg (its sizes have no default: capi.dci_ue_sizes
        names the formats' for a cell) -> PdcchScanInfo"""
        args = self._wide_args(cell, d_capbuf, n_cap, fc_requested, fc_programmed, fs_programmed, n_fft, n_rb, n_ofdm)
        if cfg is None:
            raise ValueError("pdcch_scan_wide needs a capi.PdcchScanCfg")
        out = capi.PdcchScanInfo()
        self._chk(self._lib.lcs_pdcch_scan_wide(*args, int(dl_mask), C.byref(cfg), C.byref(out)), "lcs_pdcch_scan_wide")
        out.sizes = tuple(cfg.size[:cfg.n_sizes])
        return out

    def pdcch_scan(self, cell, tfg_wide, n_rb: int, dl_mask: int = 0x3FF, cfg=None):
        """The same stage on a grid from the host, tfg_wide [n_ofdm][12 n_rb] complex (lcs_pdcch_scan) -> PdcchScanInfo"""
        args = self._grid_args(cell, tfg_wide, n_rb)
        if cfg is None:
            raise ValueError("pdcch_scan needs a capi.PdcchScanCfg")
        out = capi.PdcchScanInfo()
        self._chk(self._lib.lcs_pdcch_scan(*args, int(dl_mask), C.byref(cfg), C.byref(out)), "lcs_pdcch_scan")
        out.sizes = tuple(cfg.size[:cfg.n_sizes])
        return out

    def pdcch_scan_decodes(self, g: int) -> list:
        """Every decode of grid subframe g of this context's last scan (lcs_pdcch_scan_decodes): a list of capi.PdcchScanDec, n_cand x
        n_sizes of them in candidate (capi.scan_candidates) and size order"""
        cap = capi.PDCCH_SCAN_MAX_CAND * capi.PDCCH_SCAN_MAX_SIZES
        buf = (capi.PdcchScanDec * cap)()
        n = self._lib.lcs_pdcch_scan_decodes(self._h, int(g), buf, cap)
        if n < 0:
            self._chk(n, "lcs_pdcch_scan_decodes")
        return [buf[i] for i in range(n)]

    def phich_wide(self, cell, d_capbuf, fc_requested, fc_programmed, fs_programmed, n_fft: int, n_rb: int, n_ofdm: int, dl_mask: int = 0x3FF,
                   cfg=None, n_cap=None):
        """The HARQ indicators (ACK / NACK of uplink transport blocks) of every downlink subframe from the same samples
        (lcs_phich_wide: symbol 0 of every subframe read is transformed, symbol 1 too with 4 ports, symbols 0 .. 2 at the extended
        PHICH duration; no CFI is needed).  cfg: a capi.PhichCfg; None = the cell's PHICH configuration, FDD, the default thresholds
        -> PhichInfo"""
        args = self._wide_args(cell, d_capbuf, n_cap, fc_requested, fc_programmed, fs_programmed, n_fft, n_rb, n_ofdm)
        out = capi.PhichInfo()
        self._chk(self._lib.lcs_phich_wide(*args, int(dl_mask), None if cfg is None else C.byref(cfg), C.byref(out)), "lcs_phich_wide")
        out.tdd = cfg is not None and cfg.tdd
        self._phich_cp_normal = int(cell.cp_type) == 1      # the shape of phich_values' table
        return out

    def phich(self, cell, tfg_wide, n_rb: int, dl_mask: int = 0x3FF, cfg=None):
        """The same stage on a grid from the host, tfg_wide [n_ofdm][12 n_rb] complex whose row 0 is symbol 0 of slot 0 of a frame
        (extract_tfg_wide's) (lcs_phich) -> PhichInfo"""
        args = self._grid_args(cell, tfg_wide, n_rb)
        out = capi.PhichInfo()
        self._chk(self._lib.lcs_phich(*args, int(dl_mask), None if cfg is None else C.byref(cfg), C.byref(out)), "lcs_phich")
        out.tdd = cfg is not None and cfg.tdd
        self._phich_cp_normal = int(cell.cp_type) == 1      # the shape of phich_values' table
        return out

    def phich_values(self, g: int):
        """The full table of grid subframe g of this context's last PHICH call (lcs_phich_values): values [n_group][n_seq], n_seq = 8
        with the normal CP and 4 with the extended (an empty array for a subframe that was not read or holds no unit)"""
        buf = np.zeros(capi.PHICH_MAX_ENTRIES)
        n = self._lib.lcs_phich_values(self._h, int(g), _dp(buf), buf.size)
        if n < 0:
            self._chk(n, "lcs_phich_values")
        n_seq = 8 if self._phich_cp_normal else 4
        return buf[:n].reshape(-1, n_seq).copy()

    def pdsch_wide(self, cell, d_capbuf, fc_requested, fc_programmed, fs_programmed, n_fft: int, n_rb: int, n_ofdm: int, dl_mask: int = 0x3FF,
                   cfg=None, pdsch_cfg=None, n_cap=None, want_pdcch: bool = False):
        """The transport blocks behind the format 1A grants of the common search space (SI, paging, random-access responses) of every
        downlink subframe from the same samples (lcs_pdsch_wide: every row of the subframes of the mask is transformed; PCFICH,
        PDCCH, the grants' soft bits and the turbo decoder run on the device).  cfg: a capi.PdcchCfg as pdcch_wide's; pdsch_cfg: a
        capi.PdschCfg or None -> PdschInfo, or (PdschInfo, PdcchInfo) with want_pdcch"""
        args = self._wide_args(cell, d_capbuf, n_cap, fc_requested, fc_programmed, fs_programmed, n_fft, n_rb, n_ofdm)
        cfg = self._pdcch_cfg(cfg, n_rb)
        out, pd = capi.PdschInfo(), capi.PdcchInfo()
        self._chk(self._lib.lcs_pdsch_wide(*args, int(dl_mask), *self._pdsch_own(cfg, pdsch_cfg, out, pd, want_pdcch)), "lcs_pdsch_wide")
        return (out, pd) if want_pdcch else out

    def pdsch(self, cell, tfg_wide, n_rb: int, dl_mask: int = 0x3FF, cfg=None, pdsch_cfg=None, want_pdcch: bool = False):
        """The same stage on a grid from the host, tfg_wide [n_ofdm][12 n_rb] complex whose row 0 is symbol 0 of slot 0 of a frame
        (extract_tfg_wide's) (lcs_pdsch) -> PdschInfo, or (PdschInfo, PdcchInfo) with want_pdcch"""
        args = self._grid_args(cell, tfg_wide, n_rb)
        cfg = self._pdcch_cfg(cfg, n_rb)
        out, pd = capi.PdschInfo(), capi.PdcchInfo()
        self._chk(self._lib.lcs_pdsch(*args, int(dl_mask), *self._pdsch_own(cfg, pdsch_cfg, out, pd, want_pdcch)), "lcs_pdsch")
        return (out, pd) if want_pdcch else out

    def pdsch_comb_wide(self, cell, d_capbuf, fc_requested, fc_programmed, fs_programmed, n_fft: int, n_rb: int, n_ofdm: int, dl_mask: int = 0x3FF,
                        cfg=None, pdsch_cfg=None, comb_cfg=None, n_cap=None, want_pdcch: bool = False):
        """pdsch_wide, then the SI blocks that repeat one transport block are grouped and every group none of whose members decoded
        is decoded from the sum of its members' soft bits, on the device (lcs_pdsch_comb_wide; the rule: include/lcs.h,
        lcs_pdsch_comb_info).  comb_cfg: a capi.PdschCombCfg or None (SIB1 rule on, SI windows off)
        -> (PdschInfo, PdschCombInfo), or (PdschInfo, PdschCombInfo, PdcchInfo) with want_pdcch"""
        args = self._wide_args(cell, d_capbuf, n_cap, fc_requested, fc_programmed, fs_programmed, n_fft, n_rb, n_ofdm)
        cfg = self._pdcch_cfg(cfg, n_rb)
        out, pd, comb = capi.PdschInfo(), capi.PdcchInfo(), capi.PdschCombInfo()
        own = self._pdsch_own(cfg, pdsch_cfg, out, pd, want_pdcch)
        self._chk(self._lib.lcs_pdsch_comb_wide(*args, int(dl_mask), *own, _ref(comb_cfg), C.byref(comb)), "lcs_pdsch_comb_wide")
        return (out, comb, pd) if want_pdcch else (out, comb)

    def pdsch_comb(self, cell, tfg_wide, n_rb: int, dl_mask: int = 0x3FF, cfg=None, pdsch_cfg=None, comb_cfg=None, want_pdcch: bool = False):
        """The same on a grid from the host as pdsch takes it (lcs_pdsch_comb)
        -> (PdschInfo, PdschCombInfo), or (PdschInfo, PdschCombInfo, PdcchInfo) with want_pdcch"""
        args = self._grid_args(cell, tfg_wide, n_rb)
        cfg = self._pdcch_cfg(cfg, n_rb)
        out, pd, comb = capi.PdschInfo(), capi.PdcchInfo(), capi.PdschCombInfo()
        own = self._pdsch_own(cfg, pdsch_cfg, out, pd, want_pdcch)
        self._chk(self._lib.lcs_pdsch_comb(*args, int(dl_mask), *own, _ref(comb_cfg), C.byref(comb)), "lcs_pdsch_comb")
        return (out, comb, pd) if want_pdcch else (out, comb)

    @staticmethod
    def _pdsch_own(cfg, pdsch_cfg, out, pd, want_pdcch):
        """what the four PDSCH entries take behind the mask: the two configurations and the two records (the PDCCH's only on demand)"""
        pd.sizes = tuple(cfg.size[:cfg.n_sizes])
        return C.byref(cfg), _ref(pdsch_cfg), C.byref(out), C.byref(pd) if want_pdcch else None

    def pdsch_last_soft(self, subframe: int, which: int, n: int):
        """the first n soft bits of the which-th grant the last pdsch / pdsch_wide call followed in grid subframe `subframe`
        (lcs_pdsch_last_soft)"""
        out = np.zeros(max(int(n), 1))
        self._chk(self._lib.lcs_pdsch_last_soft(self._h, int(subframe), int(which), _dp(out), int(n)), "lcs_pdsch_last_soft")
        return out[:int(n)]

    def set_pdsch_alloc(self, cfg=None):
        """which grants beyond localized format 1A the pdsch calls of this searcher follow (lcs_set_pdsch_alloc): cfg a
        capi.PdschAllocCfg, or None for the stage without distributed allocations and format 1C"""
        self._chk(self._lib.lcs_set_pdsch_alloc(self._h, C.byref(cfg) if cfg is not None else None), "lcs_set_pdsch_alloc")
        self._pdsch_alloc = cfg

    @property
    def pdsch_alloc(self):
        """the setting last given to set_pdsch_alloc (None: the stage without distributed allocations and format 1C)"""
        return getattr(self, "_pdsch_alloc", None)

    def pdsch_last_alloc(self, block_index: int) -> dict:
        """how block `block_index` of the last pdsch call's record was allocated (lcs_pdsch_last_alloc): format "1a" / "1c",
        distributed, gap, n_gap, n_vrb, n_step, n_prb and prb [2][n_prb], the PRBs of its VRBs in the subframe's two slots"""
        out = capi.PdschAlloc()
        self._chk(self._lib.lcs_pdsch_last_alloc(self._h, int(block_index), C.byref(out)), "lcs_pdsch_last_alloc")
        return out.as_dict()

    def turbo_decode(self, d, K: int, F: int = 0, max_iter: int = 0):
        """The stage's turbo decoder alone (lcs_turbo_decode): d [3][K + 4] de-rate-matched values, positive means 0
        -> (bits [K] uint8 with the fillers zero, iterations run, whether the CRC24A over bits F .. K - 1 is zero)"""
        d = np.ascontiguousarray(d, np.float64)
        if d.shape != (3, int(K) + 4):
            raise ValueError("d is [3][K + 4]")
        bits = np.zeros(max(int(K), 1), np.uint8)
        n_iter, ok = C.c_int(0), C.c_int(0)
        self._chk(self._lib.lcs_turbo_decode(self._h, _dp(d), int(K), int(F), int(max_iter), bits.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(n_iter), C.byref(ok)),
                  "lcs_turbo_decode")
        return bits[:int(K)], n_iter.value, bool(ok.value)

    def set_batch_screen(self, on: bool):
        """int8 batches run a two-digit screen and the exact kernel only where a detection is possible (lcs_set_batch_screen,
        include/lcs.h); on by default, the records are the same either way."""
        self._chk(self._lib.lcs_set_batch_screen(self._h, 1 if on else 0), "lcs_set_batch_screen")

    def get_batch_screen(self) -> bool:
        on = C.c_int(0)
        self._chk(self._lib.lcs_get_batch_screen(self._h, C.byref(on)), "lcs_get_batch_screen")
        return bool(on.value)

    def last_screen_stats(self):
        """(lag tiles flagged, tiles in all, work items recomputed, buffers that flagged everything) of the last collected batch
        (lcs_last_screen_stats)."""
        st = (C.c_int * 4)()
        self._chk(self._lib.lcs_last_screen_stats(self._h, st), "lcs_last_screen_stats")
        return tuple(int(x) for x in st)

    def set_float_batch_probe(self, on: bool):
        """complex<float> batches (FMT_C64) are checked for dongle data on the device and then take the u8 / int8 route
        (lcs_set_float_batch_probe, include/lcs.h); off by default."""
        self._chk(self._lib.lcs_set_float_batch_probe(self._h, 1 if on else 0), "lcs_set_float_batch_probe")

    def track_cut(self, d_capbuf_ptr, fmt, n_cap, cp_types, frame_timing, freq_off, fc_requested, fc_programmed, fs_programmed, n_sym,
                  d_td_ptr, ts_first=0.0, sym_first=None, pos_first=None, want_state=False):
        """The producer thread's symbol extraction on the device (lcs_track_cut, src/producer_thread.cpp:96-131, 196-246): the
        OFDM symbols of len(cp_types) tracked cells cut out of ONE capture buffer resident in HBM (fmt FMT_IQ_U8 / FMT_C64 /
        FMT_C128 at device pointer d_capbuf_ptr) into the device array d_td_ptr [n_cells][n_sym][128] complex128 -- what
        track_block takes as td_device_ptr.  ts_first / sym_first / pos_first continue a stream over several buffers (see
        include/lcs.h).  Returns (late [n_cells][n_sym], n_cut [n_cells]) and, with want_state, pos_next [n_cells]."""
        n_cells = len(cp_types)
        cp = np.ascontiguousarray(cp_types, np.int32)
        ft = np.ascontiguousarray(frame_timing, np.float64).reshape(n_cells)
        fo = np.ascontiguousarray(freq_off, np.float64).reshape(n_cells)
        sf = None if sym_first is None else np.ascontiguousarray(sym_first, np.int64).reshape(n_cells)
        pf = None if pos_first is None else np.ascontiguousarray(pos_first, np.int64).reshape(n_cells)
        late = np.zeros((n_cells, n_sym), np.float64)
        n_cut = np.zeros(n_cells, np.int32)
        pos_next = np.zeros(n_cells, np.int64)
        i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)) if a is not None else None
        rc = self._lib.lcs_track_cut(self._h, C.c_void_p(d_capbuf_ptr), int(fmt), int(n_cap), float(ts_first), n_cells, _ip(cp), _dp(ft), _dp(fo),
                                     i64(sf), i64(pf), float(fc_requested), float(fc_programmed), float(fs_programmed), int(n_sym),
                                     C.c_void_p(d_td_ptr), _dp(late), _ip(n_cut), i64(pos_next))
        self._chk(rc, "lcs_track_cut")
        return (late, n_cut, pos_next) if want_state else (late, n_cut)

    def track_stream_block(self, cells, td, freq_off, frame_timing, late, fc_requested, fc_programmed, fs_programmed, want_stats=False,
                           want_syms=True, want_ce=True, td_device_ptr=None):
        """Continuous tracking (lcs_track_stream_block): the next block of a symbol stream.  `cells` as in track_block; the
        objects' bulk_phase_offset attribute (if any) seeds the first call.  Returns a dict whose rows carry their index in
        the whole stream: syms [c][n_sym][72]; meas [c][4][n_meas][9] (+ ac_fd, ac_td with want_stats); ce / ce_pw lists per
        (cell, port) with ce_from; mib_ok / mib_bits lists per cell with mib_from."""
        n_cells = len(cells)
        if not hasattr(self, "_trk_stream_cells"):
            tc = (capi.LcsTrackCell * n_cells)()
            for i, c in enumerate(cells):
                for f in ("n_id_1", "n_id_2", "cp_type", "n_ports", "n_rb_dl", "phich_duration", "phich_resource"):
                    setattr(tc[i], f, int(getattr(c, f)))
                tc[i].bulk_phase_offset = float(getattr(c, "bulk_phase_offset", 0.0))
            self._trk_stream_cells = tc
        tc = self._trk_stream_cells
        fo = np.ascontiguousarray(freq_off, np.float64).reshape(n_cells, -1)
        n_sym = fo.shape[1]
        ft = np.ascontiguousarray(frame_timing, np.float64).reshape(n_cells, n_sym)
        lt = np.ascontiguousarray(late, np.float64).reshape(n_cells, n_sym)
        if td_device_ptr is None:      # host samples (a page-locked array from host_alloc is DMA'd in place); else [n_cells][n_sym][128] complex128 in HBM
            tdh = np.ascontiguousarray(td, np.complex128).reshape(n_cells, n_sym, 128)
            td_arg = tdh.ctypes.data_as(C.c_void_p)
        else:
            td_arg = C.c_void_p(td_device_ptr)
        max_rs, ce_cap, max_off = n_sym // 3 + 8, n_sym + 64, n_sym // 120 + 4
        o = dict(syms=np.empty((n_cells, n_sym, 72), np.complex128) if want_syms else None,
                 ce=np.full((n_cells, 4, ce_cap, 72), np.nan + 0j, np.complex128) if want_ce else None,
                 ce_pw=np.full((n_cells, 4, ce_cap, 4), np.nan) if want_ce else None, ce_from=np.zeros((n_cells, 4), np.int64), ce_n=np.zeros((n_cells, 4), np.int32),
                 meas=np.full((n_cells, 4, max_rs, 9), np.nan), n_meas=np.zeros((n_cells, 4), np.int32),
                 ac_fd=np.full((n_cells, 4, max_rs, 12), np.nan + 0j, np.complex128) if want_stats else None,
                 ac_td=np.full((n_cells, 4, max_rs, 72), np.nan + 0j, np.complex128) if want_stats else None,
                 mib_ok=np.full((n_cells, max_off), -1, np.int32), mib_bits=np.zeros((n_cells, max_off), np.uint64),
                 mib_from=np.zeros(n_cells, np.int64), n_mib=np.zeros(n_cells, np.int32))
        i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
        rc = self._lib.lcs_track_stream_block(self._h, tc, n_cells, n_sym, td_arg, _dp(fo), _dp(ft), _dp(lt),
                                              fc_requested, fc_programmed, fs_programmed, _dp(o["syms"]), _dp(o["ce"]), _dp(o["ce_pw"]), ce_cap,
                                              i64(o["ce_from"]), _ip(o["ce_n"]), _dp(o["meas"]), _dp(o["ac_fd"]), _dp(o["ac_td"]), max_rs,
                                              _ip(o["n_meas"]), _ip(o["mib_ok"]), o["mib_bits"].ctypes.data_as(C.POINTER(C.c_uint64)), max_off,
                                              i64(o["mib_from"]), _ip(o["n_mib"]))
        self._chk(rc, "lcs_track_stream_block")
        o["bpo"] = np.array([tc[i].bulk_phase_offset for i in range(n_cells)])
        return o

    def track_stream_reset(self):
        self._chk(self._lib.lcs_track_stream_reset(self._h), "lcs_track_stream_reset")
        if hasattr(self, "_trk_stream_cells"):
            del self._trk_stream_cells

    def track_stats(self, n_cells, n_sym, want_ac_td=True):
        """Display statistics (do_ac_fd, do_ac_td, do_pss_sss_sigpower_ce) of the block the last track_block call
        processed; see lcs_track_stats in include/lcs.h.  -> dict(ac_fd [c][4][max_rs][12], ac_td [c][4][max_rs][72],
        sync [c][max_hf][4] = (tp, sp, np, np_blank), sync_ce [c][max_hf][72], n_hf [c])."""
        max_rs, max_hf = n_sym // 3 + 4, n_sym // 60 + 2
        out = dict(ac_fd=np.full((n_cells, 4, max_rs, 12), np.nan + 0j, np.complex128),
                   ac_td=np.full((n_cells, 4, max_rs, 72), np.nan + 0j, np.complex128) if want_ac_td else None,
                   sync=np.full((n_cells, max_hf, 4), np.nan), sync_ce=np.full((n_cells, max_hf, 72), np.nan + 0j, np.complex128),
                   n_hf=np.zeros(n_cells, np.int32))
        rc = self._lib.lcs_track_stats(self._h, n_cells, n_sym, _dp(out["ac_fd"]), _dp(out["ac_td"]), max_rs, _dp(out["sync"]),
                                       _dp(out["sync_ce"]), max_hf, _ip(out["n_hf"]))
        self._chk(rc, "lcs_track_stats")
        return out

    # ---- streaming mode (LTE-Tracker's searcher thread, src/searcher_thread.cpp:83-246) ----
    def stream_open(self, fmt: int, n_cap: int, fc_requested: float, fc_programmed: float, fs_programmed: float):
        """Capture the one-buffer, single-hypothesis chain as a hipGraph (see include/lcs.h)."""
        self._chk(self._lib.lcs_stream_open(self._h, fmt, n_cap, fc_requested, fc_programmed, fs_programmed), "lcs_stream_open")
        self._stream_fmt, self._stream_n = fmt, n_cap

    def stream_push(self, samples, f_off: float, tracked=()):
        """samples: host array, uint8 I/Q (2*n_cap) or complex64 (n_cap).  Returns immediately."""
        a = np.ascontiguousarray(samples, dtype=np.uint8 if self._stream_fmt == FMT_IQ_U8 else np.complex64)
        assert a.size == (2 if self._stream_fmt == FMT_IQ_U8 else 1) * self._stream_n
        t = np.ascontiguousarray(np.asarray(list(tracked), dtype=np.int16))
        self._chk(self._lib.lcs_stream_push(self._h, a.ctypes.data_as(C.c_void_p), float(f_off),
                                            t.ctypes.data_as(C.POINTER(C.c_int16)), int(t.size)), "lcs_stream_push")

    def stream_collect(self, max_cells: int = 16):
        """-> (new cells, number of tracked cells seen again, GPU milliseconds of the pass)."""
        cells = (LcsCell * max_cells)()
        n, dup, ms = C.c_int(0), C.c_int(0), C.c_float(0)
        self._note_overflow(self._chk(self._lib.lcs_stream_collect(self._h, cells, max_cells, C.byref(n), C.byref(dup), C.byref(ms)),
                                      "lcs_stream_collect", allow_overflow=True), "lcs_stream_collect")
        return [cells[i].copy() for i in range(min(n.value, max_cells))], dup.value, ms.value

    def stream_close(self):
        self._chk(self._lib.lcs_stream_close(self._h), "lcs_stream_close")

    # ---- wideband channelizer (lcs_channelize, include/lcs.h) ---------------------------
    def channelize(self, d_wide_ptr: int, fmt: int, n_in: int, fs_in: float, decim: int, f_shift, d_out_ptr: int, n_out: int):
        """One wideband capture in HBM (n_in samples of FMT_C64 / FMT_IQ_S8 / FMT_IQ_S16 at fs_in) -> len(f_shift) narrowband
        buffers [n_ch][n_out] complex64 at fs_in / decim in HBM at d_out_ptr: mixed down by f_shift (Hz, carrier minus capture
        centre), low-passed by channelizer_taps(decim), decimated.  Queued on the context's stream; returns at once -- a
        batch_enqueue(d_out_ptr, FMT_C64, n_ch, n_out, ...) on the same Searcher is ordered behind it."""
        f = np.ascontiguousarray(np.atleast_1d(f_shift), np.float64)
        self._chk(self._lib.lcs_channelize(self._h, C.c_void_p(d_wide_ptr), int(fmt), int(n_in), float(fs_in), int(decim), _dp(f), int(f.size),
                                           C.c_void_p(d_out_ptr), int(n_out)), "lcs_channelize")

    def channelize_rational(self, d_wide_ptr: int, fmt: int, n_in: int, fs_in: float, up: int, down: int, f_shift, d_out_ptr: int, n_out: int):
        """channelize at the rational rate change fs_out = fs_in * up / down (lcs_channelize_rational: gcd(up, down) = 1,
        1 < down / up <= 16, down <= 128 -- 20 Msps -> 1.92 Msps is 12/125), low-passed by channelizer_proto(down) at the fine rate
        up * fs_in; needs n_in >= ((n_out - 1) * down + 16 * down - 1) // up + 1.  Queued and ordered like channelize."""
        f = np.ascontiguousarray(np.atleast_1d(f_shift), np.float64)
        self._chk(self._lib.lcs_channelize_rational(self._h, C.c_void_p(d_wide_ptr), int(fmt), int(n_in), float(fs_in), int(up), int(down), _dp(f),
                                                    int(f.size), C.c_void_p(d_out_ptr), int(n_out)), "lcs_channelize_rational")

    def channelize_u8(self, d_wide_ptr: int, fmt: int, n_in: int, fs_in: float, up: int, down: int, f_shift, d_out_ptr: int, n_out: int,
                      want_gain: bool = False):
        """channelize (up == 1, down in 2..16) or channelize_rational (any other rate) with 8-bit carriers (lcs_channelize_u8): the
        buffers at d_out_ptr are [n_ch][n_out][2] uint8, the FMT_IQ_U8 batch layout, each carrier scaled by a power of two 2^e
        that puts its component rms in (16, 32] codes and rounded to 127 + rint(.), clamped to 0..255.  Queued and ordered like
        channelize: a batch_enqueue(d_out_ptr, FMT_IQ_U8, n_ch, n_out, ...) behind it takes the int8 correlation kernel.
        want_gain: returns the gains 2^e as a float32 torch tensor [n_ch] on the device (written by the same stream)."""
        f = np.ascontiguousarray(np.atleast_1d(f_shift), np.float64)
        gain = None
        if want_gain:
            import torch
            gain = torch.empty(int(f.size), dtype=torch.float32, device=torch.device("cuda", self.device if self.device >= 0 else torch.cuda.current_device()))
        self._chk(self._lib.lcs_channelize_u8(self._h, C.c_void_p(d_wide_ptr), int(fmt), int(n_in), float(fs_in), int(up), int(down), _dp(f), int(f.size),
                                              C.c_void_p(d_out_ptr), int(n_out), C.c_void_p(gain.data_ptr() if gain is not None else None)),
                  "lcs_channelize_u8")
        return gain

    # ---- the channelizer's continuous form (lcs_chan_stream_open, include/lcs.h) -----------
    def chan_stream_open(self, fmt: int, fs_in: float, up: int, down: int, f_shift):
        """Open the context's channelizer stream: samples of fmt at fs_in, pushed in chunks of any size, come out as len(f_shift)
        carriers at fs_in * up / down -- after any pushes bit for bit what ONE channelize_rational call on all the samples gives
        ((1, decim): channelize).  Steps, taps and the filter bank are built here, once."""
        f = np.ascontiguousarray(np.atleast_1d(f_shift), np.float64)
        self._chk(self._lib.lcs_chan_stream_open(self._h, int(fmt), float(fs_in), int(up), int(down), _dp(f), int(f.size)), "lcs_chan_stream_open")

    def chan_stream_count(self, n_chunk: int) -> int:
        """Outputs per carrier a push of n_chunk samples would hand out now (lcs_chan_stream_count)."""
        n = C.c_uint32(0)
        self._chk(self._lib.lcs_chan_stream_count(self._h, int(n_chunk), C.byref(n)), "lcs_chan_stream_count")
        return n.value

    def chan_stream_push(self, d_chunk_ptr: int, n_chunk: int, d_out_ptr: int, row_stride: int, out_cap: int):
        """Push n_chunk samples at d_chunk_ptr (device).  Output m_first + j of carrier k goes to complex64 element k * row_stride + j
        behind d_out_ptr (device, 8-byte aligned), j < n_emit <= out_cap.  Queued on the context's stream; the chunk must stay
        unchanged until that work has run.  Returns (n_emit, m_first), known without waiting for the GPU."""
        n, m = C.c_uint32(0), C.c_uint64(0)
        self._chk(self._lib.lcs_chan_stream_push(self._h, C.c_void_p(d_chunk_ptr), int(n_chunk), C.c_void_p(d_out_ptr), int(row_stride), int(out_cap),
                                                 C.byref(n), C.byref(m)), "lcs_chan_stream_push")
        return n.value, m.value

    def chan_stream_close(self):
        self._chk(self._lib.lcs_chan_stream_close(self._h), "lcs_chan_stream_close")

    def chan_stream_open_u8(self, fmt: int, fs_in: float, up: int, down: int, f_shift, n_cap: int):
        """Open the context's channelizer stream for 8-bit captures (lcs_chan_stream_open_u8): as chan_stream_open, but the stream
        hands out whole captures of n_cap outputs per carrier as bytes, the FMT_IQ_U8 batch layout, each capture of each carrier
        scaled by channelize_u8's rule with a gain of its own -- the same bytes and gains however the samples are cut into pushes."""
        f = np.ascontiguousarray(np.atleast_1d(f_shift), np.float64)
        self._chk(self._lib.lcs_chan_stream_open_u8(self._h, int(fmt), float(fs_in), int(up), int(down), _dp(f), int(f.size), int(n_cap)),
                  "lcs_chan_stream_open_u8")

    def chan_stream_count_u8(self, n_chunk: int) -> int:
        """Captures a push_u8 of n_chunk samples would complete now (lcs_chan_stream_count_u8)."""
        n = C.c_uint32(0)
        self._chk(self._lib.lcs_chan_stream_count_u8(self._h, int(n_chunk), C.byref(n)), "lcs_chan_stream_count_u8")
        return n.value

    def chan_stream_push_u8(self, d_chunk_ptr: int, n_chunk: int, d_out_ptr: int, d_gain_ptr: int, cap_room: int):
        """Push n_chunk samples at d_chunk_ptr (device).  Capture cap_first + j goes to slot j of d_out_ptr (device, uint8
        [cap_room][n_ch][n_cap][2], 16-byte aligned) and its gains to slot j of d_gain_ptr (device, float32 [cap_room][n_ch]; 0 or
        None for no gains), j < n_done <= cap_room.  Queued on the context's stream.  Returns (n_done, cap_first), known without
        waiting for the GPU."""
        n, m = C.c_uint32(0), C.c_uint64(0)
        self._chk(self._lib.lcs_chan_stream_push_u8(self._h, C.c_void_p(d_chunk_ptr), int(n_chunk), C.c_void_p(d_out_ptr), C.c_void_p(d_gain_ptr or None),
                                                    int(cap_room), C.byref(n), C.byref(m)), "lcs_chan_stream_push_u8")
        return n.value, m.value

    def last_channelize_ms(self) -> float:
        """HIP-event time (ms) of the last channelize / channelize_rational / channelize_u8 call of this context (lcs_last_channelize_ms)."""
        ms = C.c_float(0)
        self._chk(self._lib.lcs_last_channelize_ms(self._h, C.byref(ms)), "lcs_last_channelize_ms")
        return ms.value

    def last_xcorr_ms(self):
        ms, n = C.c_float(0), C.c_int(0)
        self._chk(self._lib.lcs_last_xcorr_ms(self._h, C.byref(ms), C.byref(n)), "lcs_last_xcorr_ms")
        return ms.value, n.value

    def last_frq_repairs(self) -> int:
        """Positions of xc_incoherent_collapsed_frq the last correlation call recomputed in the reference's arithmetic
        (near-ties of the arg-max, lcs_last_frq_repairs)."""
        n = C.c_int(0)
        self._chk(self._lib.lcs_last_frq_repairs(self._h, C.byref(n)), "lcs_last_frq_repairs")
        return n.value

    def last_frq_repair_stats(self):
        """-> (positions listed as near-ties, positions left unrepaired by the work bound) of the last correlation call
        (lcs_last_frq_repair_stats; the second is 0 on any real data)."""
        a, b = C.c_int(0), C.c_int(0)
        self._chk(self._lib.lcs_last_frq_repair_stats(self._h, C.byref(a), C.byref(b)), "lcs_last_frq_repair_stats")
        return a.value, b.value

    @staticmethod
    def frq_tie_eps() -> float:
        """The library's near-tie margin (lcs_frq_tie_eps): the correlation kernels must hold half of it on xc_incoherent_single."""
        return frq_tie_eps()

    def last_batch_stats(self):
        """Counters of the last collected batch (lcs_last_batch_stats): dict with cells_past_sss and pbch_candidates_decoded among them."""
        a = (C.c_int * 8)()
        self._chk(self._lib.lcs_last_batch_stats(self._h, a), "lcs_last_batch_stats")
        return dict(records=a[0], overflow=a[1], cells_last_round=a[4], cells_past_sss=a[5], redetected=a[6], pbch_candidates_decoded=a[7])

    def last_collect_host_us(self) -> float:
        """Host microseconds the last batch_collect spent outside its wait for the GPU (lcs_last_collect_host_us)."""
        us = C.c_double(0)
        self._chk(self._lib.lcs_last_collect_host_us(self._h, C.byref(us)), "lcs_last_collect_host_us")
        return us.value

    def last_xcorr_info(self):
        """-> (kernel name, matrix-core operations executed by the last enqueue's correlation launches)."""
        ops, name = C.c_double(0), C.c_char_p()
        self._chk(self._lib.lcs_last_xcorr_info(self._h, C.byref(ops), C.byref(name)), "lcs_last_xcorr_info")
        return (name.value or b"").decode(), ops.value

    def batch_collect_raw(self, n_buf: int, max_cells_per_buf: int = 16):
        """Like batch_collect but without building Python objects: (records [n_buf][max_cells] as a numpy structured
        array with lcs_cell's layout, counts [n_buf])."""
        rec = np.zeros((n_buf, max_cells_per_buf), capi.cell_dtype())
        cnt = np.zeros(n_buf, np.int32)
        rc = self._lib.lcs_batch_collect(self._h, rec.ctypes.data_as(C.POINTER(LcsCell)), max_cells_per_buf,
                                         cnt.ctypes.data_as(C.POINTER(C.c_int)))
        self._note_overflow(self._chk(rc, "lcs_batch_collect", allow_overflow=True), "lcs_batch_collect")
        return rec, cnt

    def sync(self):
        self._chk(self._lib.lcs_sync(self._h), "lcs_sync")


def tdd_dl_mask(ul_dl_config: int) -> int:
    """The downlink subframes of uplink-downlink configuration 0..6 (36.211 table 4.2-2) as a dl_mask for Searcher.cell_meas, special
    subframes excluded; -1 for anything else (lcs_tdd_dl_mask)."""
    return int(capi.load().lcs_tdd_dl_mask(int(ul_dl_config)))


def frq_tie_eps() -> float:
    """Relative margin below which the two best hypotheses of a position are a near-tie for the repair (lcs_frq_tie_eps)."""
    return float(capi.load().lcs_frq_tie_eps())


def device_count() -> int:
    """GPUs the library can use (lcs_device_count)."""
    return capi.load().lcs_device_count()


def kalibrate(searcher: "Searcher", capbuf, fc_requested: float, fc_programmed: float, fs_programmed: float,
              ppm: float = 120.0, correction: float = 1.0):
    """LO calibration step of LTE-Tracker (src/LTE-Tracker.cpp:565-741) on one capture buffer: search
    the +-ppm grid shifted by the current correction (:586), take the strongest decoded cell (:712-722)
    and return (best cell, residual frequency offset, correction_residual of :724-731), or None when no
    cell was decoded (the reference then tries again on a fresh capture)."""
    n_extra = int(np.floor((fc_requested * ppm / 1e6 + 2.5e3) / 5e3))
    f = (fc_requested * correction - fc_requested) + np.arange(-n_extra, n_extra + 1) * 5000.0
    cells, _ = searcher.search_capbuf(capbuf, f, fc_requested, fc_programmed, fs_programmed)
    if not cells:
        return None
    best = max(cells, key=lambda c: c.pss_pow)
    crystal_freq_actual = fc_programmed - best.freq_superfine
    return best, best.freq_superfine, (fc_requested / fc_requested * fc_programmed) / crystal_freq_actual


def z_th1(sp_incoherent, n_comb_xc, ds_comb_arm=DS_COMB_ARM, thresh1_n_nines=12):
    """Detection threshold of the CLI main loop (src/CellSearch.cpp:500-503)."""
    L = capi.load()
    R_th1 = L.lcs_chi2cdf_inv(1 - pow(10.0, -thresh1_n_nines), 2.0 * n_comb_xc * (2 * ds_comb_arm + 1))
    rx_cutoff = (6 * 12 * 15e3 / 2 + 4 * 15e3) / (FS_LTE / 16 / 2)
    return R_th1 * np.asarray(sp_incoherent) / rx_cutoff / 137 / 2 / n_comb_xc / (2 * ds_comb_arm + 1)


# ---- table accessors (used by tests) ------------------------------------------------
def table_pss_td(n_id_2):
    o = np.empty(137, np.complex128)
    capi.load().lcs_table_pss_td(n_id_2, _dp(o))
    return o


def table_pss_fd(n_id_2):
    o = np.empty(62, np.complex128)
    capi.load().lcs_table_pss_fd(n_id_2, _dp(o))
    return o


def table_sss_fd(n_id_1, n_id_2, slot):
    o = np.empty(62, np.int32)
    capi.load().lcs_table_sss_fd(n_id_1, n_id_2, slot, _ip(o))
    return o


def table_lte_pn(c_init, n):
    o = np.empty(n, np.uint8)
    capi.load().lcs_table_lte_pn(c_init, n, o.ctypes.data_as(C.POINTER(C.c_uint8)))
    return o


def chi2cdf_inv(p, k):
    return capi.load().lcs_chi2cdf_inv(p, k)


def channelizer_taps(decim: int) -> np.ndarray:
    """The 16 * decim taps of the channelizer's low-pass (lcs_channelizer_taps): sinc x Kaiser(7.75), sum 1."""
    o = np.empty(16 * max(int(decim), 0))
    rc = capi.load().lcs_channelizer_taps(int(decim), _dp(o))
    if rc != 0:
        raise SearcherError(f"lcs_channelizer_taps({decim}): {capi.ERRORS.get(rc, rc)}")
    return o


def channelizer_proto(down: int) -> np.ndarray:
    """The 16 * down taps of the rational channelizer's low-pass at the fine rate (lcs_channelizer_proto): the rule of
    channelizer_taps for any down in 2..128."""
    o = np.empty(16 * max(int(down), 0))
    rc = capi.load().lcs_channelizer_proto(int(down), _dp(o))
    if rc != 0:
        raise SearcherError(f"lcs_channelizer_proto({down}): {capi.ERRORS.get(rc, rc)}")
    return o
