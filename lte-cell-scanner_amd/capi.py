"""ctypes view of the C ABI declared in include/lcs.h (liblcs_amd.so).

The shared library is the product; this module only loads it and declares prototypes.
There is no fallback: if the library is missing or no MI355X is visible, calls raise.
"""
from __future__ import annotations

import ctypes as C
import math
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblcs_amd.so")

LCS_OK = 0
FMT_C64, FMT_IQ_U8, FMT_C128 = 0, 1, 2      # FMT_C128: lcs_track_cut only
FMT_IQ_S8, FMT_IQ_S16 = 3, 4                # wideband captures of lcs_channelize: interleaved signed 8 / 16 bit
STAGE_PSS, STAGE_FULL = 1, 3
MAX_PEAKS = 104            # LCS_MAX_PEAKS: the longest list peak_search can return (include/lcs.h)
DUPLEX_FDD, DUPLEX_TDD = 0, 1      # LCS_DUPLEX_*: where the SSS lies relative to the PSS (include/lcs.h: lcs_set_duplex)
TDD_NOT_ESTIMATED = -2     # LCS_TDD_NOT_ESTIMATED: a record of lcs_last_tdd_info that belongs to no decoded cell, or to a call without the mode
MEAS_NOT_MEASURED = -2     # LCS_MEAS_NOT_MEASURED: a record of lcs_last_cell_meas that belongs to no decoded cell, or to a call without the mode
ERRORS = {-1: "LCS_ERR_NO_DEVICE", -2: "LCS_ERR_BAD_ARG", -3: "LCS_ERR_HIP", -4: "LCS_ERR_OVERFLOW", -5: "LCS_ERR_NOMEM"}


class LcsCell(C.Structure):
    """lcs_cell: POD mirror of the reference's class Cell (include/common.h.in:101-129)."""
    _fields_ = [
        ("fc_requested", C.c_double), ("fc_programmed", C.c_double), ("pss_pow", C.c_double),
        ("freq", C.c_double), ("frame_start", C.c_double), ("freq_fine", C.c_double),
        ("freq_superfine", C.c_double),
        ("ind", C.c_int32), ("n_id_2", C.c_int32), ("n_id_1", C.c_int32), ("cp_type", C.c_int32),
        ("n_ports", C.c_int32), ("n_rb_dl", C.c_int32), ("phich_duration", C.c_int32),
        ("phich_resource", C.c_int32), ("sfn", C.c_int32), ("reserved", C.c_int32),
    ]

    def n_id_cell(self) -> int:          # src/common.cpp:29-31
        return self.n_id_2 + 3 * self.n_id_1 if (self.n_id_1 >= 0 and self.n_id_2 >= 0) else -1

    def n_symb_dl(self) -> int:          # src/common.cpp:32-34
        return 7 if self.cp_type == 1 else (6 if self.cp_type == 2 else -1)

    def as_dict(self) -> dict:
        return {f: getattr(self, f) for f, _ in self._fields_ if f != "reserved"}

    def copy(self) -> "LcsCell":
        o = LcsCell()
        C.memmove(C.byref(o), C.byref(self), C.sizeof(LcsCell))
        return o

    def __repr__(self) -> str:  # pragma: no cover
        return "LcsCell(" + ", ".join(f"{k}={v}" for k, v in self.as_dict().items()) + ")"


def cell_dtype():
    """numpy structured dtype with the layout of lcs_cell (zero-copy views of result arrays)."""
    import numpy as np
    m = {C.c_double: "<f8", C.c_int32: "<i4"}
    return np.dtype([(n, m[t]) for n, t in LcsCell._fields_])


class LcsTrackCell(C.Structure):
    """lcs_track_cell: what the tracker's per-symbol pipeline reads of a tracked cell (include/lcs.h)."""
    _fields_ = [("n_id_1", C.c_int32), ("n_id_2", C.c_int32), ("cp_type", C.c_int32), ("n_ports", C.c_int32),
                ("n_rb_dl", C.c_int32), ("phich_duration", C.c_int32), ("phich_resource", C.c_int32), ("reserved", C.c_int32),
                ("bulk_phase_offset", C.c_double)]


class TddInfo(C.Structure):
    """lcs_tdd_info: the uplink-downlink configuration of a TDD cell as its reference signals show it (include/lcs.h:
    lcs_set_tdd_config).  ul_dl_config 0..6 or -1, dwpts_rs_rows 1..4 or -1 (both TDD_NOT_ESTIMATED where nothing was estimated),
    margin = the smallest distance of a deciding T from 1/2, T per subframe, R per reference row of the special subframe."""
    _fields_ = [("ul_dl_config", C.c_int32), ("dwpts_rs_rows", C.c_int32), ("margin", C.c_double), ("T", C.c_double * 10), ("R", C.c_double * 4)]

    def copy(self) -> "TddInfo":
        o = TddInfo()
        C.memmove(C.byref(o), C.byref(self), C.sizeof(TddInfo))
        return o

    def as_dict(self) -> dict:
        return dict(ul_dl_config=self.ul_dl_config, dwpts_rs_rows=self.dwpts_rs_rows, margin=self.margin, T=list(self.T), R=list(self.R))

    def __repr__(self) -> str:  # pragma: no cover
        return f"TddInfo(ul_dl_config={self.ul_dl_config}, dwpts_rs_rows={self.dwpts_rs_rows}, margin={self.margin:.3f})"


assert C.sizeof(TddInfo) == 128


SIC_PSS, SIC_SSS, SIC_CRS, SIC_PBCH, SIC_ALL = 1, 2, 4, 8, 15      # LCS_SIC_*: the components a cancellation takes out
SIC_MAX_ROUNDS = 4


class SicInfo(C.Structure):
    """lcs_sic_info: what a cancellation did to one cell (include/lcs.h: lcs_sic_cancel_dev).  power = the energy of the rebuilt PSS,
    SSS, CRS and PBCH, gain = the sync gain, pss_before / pss_after = the energy of the cell's PSS subcarriers in the capture and in the
    residual, n_sym = symbols covered (0: not cancelled), n_pss of them PSS symbols, n_dup = times a later round found the cell again,
    ul_dl_config = the TDD configuration whose downlink subframes were cancelled (TDD_NOT_ESTIMATED: subframes 0 and 5, or FDD)."""
    _fields_ = [("power", C.c_double * 4), ("gain_re", C.c_double), ("gain_im", C.c_double), ("pss_before", C.c_double), ("pss_after", C.c_double),
                ("n_sym", C.c_int32), ("n_pss", C.c_int32), ("n_dup", C.c_int32), ("ul_dl_config", C.c_int32)]

    def copy(self) -> "SicInfo":
        o = SicInfo()
        C.memmove(C.byref(o), C.byref(self), C.sizeof(SicInfo))
        return o

    @property
    def cancelled(self) -> bool:
        return self.n_sym > 0

    @property
    def gain(self) -> complex:
        return complex(self.gain_re, self.gain_im)

    @property
    def suppression_db(self) -> float:
        """10 log10(pss_before / pss_after); inf when nothing is left, nan when the cell was not cancelled"""
        if self.n_sym <= 0 or self.pss_before <= 0:
            return math.nan
        return math.inf if self.pss_after <= 0 else 10.0 * math.log10(self.pss_before / self.pss_after)


assert C.sizeof(SicInfo) == 80


class CellMeas(C.Structure):
    """lcs_meas_info: RSRP, RSSI, RSRQ and the noise power of a cell from its cell-specific reference signals (include/lcs.h:
    lcs_set_cell_meas).  status 0 measured, -1 no number, MEAS_NOT_MEASURED never written; n_rows reference rows of the subframes in
    dl_mask, n_ports ports measured (1 or 2); rsrp and noise per port and rssi in the grid's power units, rsrq = 6 rsrp[0] / rssi,
    a_re_im = the neighbour-product sums A_0, A_1.  The SINR is the caller's division: the properties below do it."""
    _fields_ = [("status", C.c_int32), ("n_rows", C.c_int32), ("n_ports", C.c_int32), ("dl_mask", C.c_int32), ("rsrp", C.c_double * 2),
                ("noise", C.c_double * 2), ("rssi", C.c_double), ("rsrq", C.c_double), ("a_re_im", C.c_double * 4), ("reserved", C.c_double * 4)]

    def copy(self) -> "CellMeas":
        o = CellMeas()
        C.memmove(C.byref(o), C.byref(self), C.sizeof(CellMeas))
        return o

    @property
    def measured(self) -> bool:
        return self.status == 0

    @property
    def sinr(self) -> tuple:
        """rsrp[p] / noise[p] of the ports measured, inf where noise <= 0"""
        return tuple((self.rsrp[p] / self.noise[p]) if self.noise[p] > 0 else math.inf for p in range(max(self.n_ports, 0)))

    @property
    def rsrp_db(self) -> tuple:
        return tuple(_db10(self.rsrp[p]) for p in range(max(self.n_ports, 0)))

    @property
    def rsrq_db(self) -> float:
        return _db10(self.rsrq)

    @property
    def sinr_db(self) -> tuple:
        return tuple(_db10(v) for v in self.sinr)

    def as_dict(self) -> dict:
        return dict(status=self.status, n_rows=self.n_rows, n_ports=self.n_ports, dl_mask=self.dl_mask, rsrp=list(self.rsrp), noise=list(self.noise),
                    rssi=self.rssi, rsrq=self.rsrq, a_re_im=list(self.a_re_im))

    def __repr__(self) -> str:  # pragma: no cover
        return f"CellMeas(status={self.status}, n_rows={self.n_rows}, dl_mask={self.dl_mask:#x}, rsrp={list(self.rsrp)}, rsrq={self.rsrq:.4f})"


def _db10(x: float) -> float:
    return math.inf if x == math.inf else (10.0 * math.log10(x) if x > 0 else -math.inf)


assert C.sizeof(CellMeas) == 128

MEAS_WIDE_MAX_RB = 100


class CellMeasWide(C.Structure):
    """lcs_meas_wide_info: the measurement of CellMeas over n_rb resource blocks of an n_fft-point grid taken from wide samples
    (include/lcs.h: lcs_cell_meas_wide), with a per-RB profile: rsrq = n_rb rsrp[0] / rssi; rsrp_rb[p][i] and rssi_rb[i] per resource
    block, lowest frequency first (numpy views of the record, cut to n_rb; the record's arrays hold 100 entries, zero beyond n_rb)."""
    _fields_ = [("status", C.c_int32), ("n_rows", C.c_int32), ("n_ports", C.c_int32), ("dl_mask", C.c_int32), ("n_rb", C.c_int32), ("n_fft", C.c_int32),
                ("reserved_i", C.c_int32 * 2), ("rsrp", C.c_double * 2), ("noise", C.c_double * 2), ("rssi", C.c_double), ("rsrq", C.c_double),
                ("a_re_im", C.c_double * 4), ("reserved", C.c_double * 2), ("_rsrp_rb", (C.c_double * MEAS_WIDE_MAX_RB) * 2), ("_rssi_rb", C.c_double * MEAS_WIDE_MAX_RB)]

    def copy(self) -> "CellMeasWide":
        o = CellMeasWide()
        C.memmove(C.byref(o), C.byref(self), C.sizeof(CellMeasWide))
        return o

    def _n(self) -> int:
        return min(max(int(self.n_rb), 0), MEAS_WIDE_MAX_RB)

    @property
    def rsrp_rb(self):
        """[2][n_rb] view: |B_p[i]| / n_rows per port and resource block"""
        import numpy as np
        return np.ctypeslib.as_array(self._rsrp_rb)[:, :self._n()]

    @property
    def rssi_rb(self):
        """[n_rb] view: the power of each resource block's 12 columns per reference row"""
        import numpy as np
        return np.ctypeslib.as_array(self._rssi_rb)[:self._n()]

    measured = CellMeas.measured
    sinr = CellMeas.sinr
    rsrp_db = CellMeas.rsrp_db
    rsrq_db = CellMeas.rsrq_db
    sinr_db = CellMeas.sinr_db

    def as_dict(self) -> dict:
        return dict(status=self.status, n_rows=self.n_rows, n_ports=self.n_ports, dl_mask=self.dl_mask, n_rb=self.n_rb, n_fft=self.n_fft, rsrp=list(self.rsrp),
                    noise=list(self.noise), rssi=self.rssi, rsrq=self.rsrq, a_re_im=list(self.a_re_im), rsrp_rb=self.rsrp_rb.tolist(), rssi_rb=self.rssi_rb.tolist())

    def __repr__(self) -> str:  # pragma: no cover
        return f"CellMeasWide(status={self.status}, n_rb={self.n_rb}, n_fft={self.n_fft}, n_rows={self.n_rows}, rsrp={list(self.rsrp)}, rsrq={self.rsrq:.4f})"


assert C.sizeof(CellMeasWide) == 2528

PCFICH_MAX_SF = (854 + 11) // 12      # LCS_PCFICH_MAX_SF


class PcfichInfo(C.Structure):
    """lcs_pcfich_info: the control format indicator of every subframe of a full-bandwidth grid (include/lcs.h: lcs_pcfich_wide,
    lcs_pcfich).  cfi[g] in 1 .. 3, or 0 for a subframe that was not decoded; corr[g][c] the normalised correlation with codeword
    c + 1, margin[g] = best - second.  cfi, corr, margin are numpy views of the record cut to its n_sf subframes; n_ctrl_sym the
    control region's OFDM symbols per subframe (cfi + 1 up to 10 resource blocks), 0 where not decoded."""
    _fields_ = [("n_sf", C.c_int32), ("n_decoded", C.c_int32), ("n_cfi", C.c_int32 * 3), ("dl_mask", C.c_int32), ("n_rb", C.c_int32), ("n_ports", C.c_int32),
                ("mean_n_ctrl_sym", C.c_double), ("min_margin", C.c_double), ("_cfi", C.c_int32 * PCFICH_MAX_SF), ("_corr", (C.c_double * 3) * PCFICH_MAX_SF),
                ("_margin", C.c_double * PCFICH_MAX_SF)]

    def copy(self) -> "PcfichInfo":
        o = PcfichInfo()
        C.memmove(C.byref(o), C.byref(self), C.sizeof(PcfichInfo))
        return o

    def _n(self) -> int:
        return min(max(int(self.n_sf), 0), PCFICH_MAX_SF)

    @property
    def cfi(self):
        import numpy as np
        return np.ctypeslib.as_array(self._cfi)[:self._n()]

    @property
    def corr(self):
        import numpy as np
        return np.ctypeslib.as_array(self._corr)[:self._n()]

    @property
    def margin(self):
        import numpy as np
        return np.ctypeslib.as_array(self._margin)[:self._n()]

    @property
    def n_ctrl_sym(self):
        import numpy as np
        c = self.cfi
        return np.where(c > 0, c + (1 if self.n_rb <= 10 else 0), 0)

    def as_dict(self) -> dict:
        return dict(n_sf=self.n_sf, n_decoded=self.n_decoded, n_cfi=list(self.n_cfi), dl_mask=self.dl_mask, n_rb=self.n_rb, n_ports=self.n_ports,
                    mean_n_ctrl_sym=self.mean_n_ctrl_sym, min_margin=self.min_margin, cfi=self.cfi.tolist(), corr=self.corr.tolist(), margin=self.margin.tolist())

    def __repr__(self) -> str:  # pragma: no cover
        return f"PcfichInfo(n_sf={self.n_sf}, n_decoded={self.n_decoded}, n_cfi={list(self.n_cfi)}, mean_n_ctrl_sym={self.mean_n_ctrl_sym:.3f}, min_margin={self.min_margin:.3f})"


assert C.sizeof(PcfichInfo) == 2640

PDCCH_SLOTS, PDCCH_MAX_SIZES = 6, 2      # LCS_PDCCH_SLOTS, LCS_PDCCH_MAX_SIZES
RNTI_SI, RNTI_PAGING, RNTI_RA = 1, 2, 4   # bits of lcs_pdcch_cfg.rnti_mask


class PdcchCfg(C.Structure):
    """lcs_pdcch_cfg (include/lcs.h).  PdcchCfg.make(sizes, ...) fills it: phich_duration / phich_resource 0 = the cell's; phich_mi
    None = FDD (every m_i 1), else ten values of 36.211 table 6.9-1 (tdd_phich_mi; None entries, the uplink subframes, count as 0)."""
    _fields_ = [("phich_duration", C.c_int32), ("phich_resource", C.c_int32), ("phich_mi", C.c_int32 * 10), ("n_sizes", C.c_int32),
                ("size", C.c_int32 * PDCCH_MAX_SIZES), ("rnti_mask", C.c_int32), ("cfi_force", C.c_int32)]

    @classmethod
    def make(cls, sizes, phich_duration=0, phich_resource=0, phich_mi=None, rnti_mask=0, cfi_force=0) -> "PdcchCfg":
        sizes = [int(a) for a in sizes]
        if not 1 <= len(sizes) <= PDCCH_MAX_SIZES:
            raise ValueError("PdcchCfg: one or two payload sizes")
        o = cls()
        o.phich_duration, o.phich_resource, o.rnti_mask, o.cfi_force, o.n_sizes = int(phich_duration), int(phich_resource), int(rnti_mask), int(cfi_force), len(sizes)
        for i, a in enumerate(sizes):
            o.size[i] = a
        for i in range(10):
            o.phich_mi[i] = -1 if phich_mi is None else (0 if phich_mi[i] is None else int(phich_mi[i]))
        return o


class PdcchDec(C.Structure):
    """lcs_pdcch_dec: bits = the payload (bit t = the t-th bit sent), rnti_x, flags (1 decoded, 2 accepted), quality"""
    _fields_ = [("bits", C.c_uint64), ("rnti_x", C.c_uint32), ("flags", C.c_int32), ("quality", C.c_double)]


class PdcchInfo(C.Structure):
    """lcs_pdcch_info: the decodes of the PDCCH common search space of every subframe of a full-bandwidth grid (include/lcs.h:
    lcs_pdcch_wide, lcs_pdcch).  cfi / n_reg / n_cce: numpy views cut to n_sf (0: subframe not read); dec[g][slot][size] the entries
    (slots 0 .. 3: L = 4 from CCE 4 slot; 4, 5: L = 8 from CCE 8 (slot - 4)).  sizes: the payload sizes of the call."""
    _fields_ = [("n_sf", C.c_int32), ("n_read", C.c_int32), ("n_accepted", C.c_int32), ("n_si", C.c_int32), ("n_paging", C.c_int32), ("n_ra", C.c_int32),
                ("dl_mask", C.c_int32), ("n_rb", C.c_int32), ("n_ports", C.c_int32), ("reserved", C.c_int32),
                ("_cfi", C.c_int32 * PCFICH_MAX_SF), ("_n_reg", C.c_int32 * PCFICH_MAX_SF), ("_n_cce", C.c_int32 * PCFICH_MAX_SF),
                ("dec", ((PdcchDec * PDCCH_MAX_SIZES) * PDCCH_SLOTS) * PCFICH_MAX_SF)]
    sizes = ()

    def copy(self) -> "PdcchInfo":
        o = PdcchInfo()
        C.memmove(C.byref(o), C.byref(self), C.sizeof(PdcchInfo))
        o.sizes = tuple(self.sizes)
        return o

    def _n(self) -> int:
        return min(max(int(self.n_sf), 0), PCFICH_MAX_SF)

    @property
    def cfi(self):
        import numpy as np
        return np.ctypeslib.as_array(self._cfi)[:self._n()]

    @property
    def n_reg(self):
        import numpy as np
        return np.ctypeslib.as_array(self._n_reg)[:self._n()]

    @property
    def n_cce(self):
        import numpy as np
        return np.ctypeslib.as_array(self._n_cce)[:self._n()]

    @staticmethod
    def slot_candidate(slot: int):
        """(L, first CCE) of candidate slot 0 .. 5"""
        return (4, 4 * slot) if slot < 4 else (8, 8 * (slot - 4))

    def entries(self):
        """(subframe, slot, size index, PdcchDec) of every decoded entry"""
        for g in range(self._n()):
            for s in range(PDCCH_SLOTS):
                for i in range(PDCCH_MAX_SIZES):
                    d = self.dec[g][s][i]
                    if d.flags & 1:
                        yield g, s, i, d

    def messages(self) -> list:
        """The accepted decodes as dicts: subframe, L, cce, kind ("si" / "paging" / "ra"), rnti, size (None when the record does not
        know its call's sizes), bits (the payload as an int, bit t = the t-th bit sent), quality.  A DCI found at L = 8 and at L = 4
        from the same first CCE with the same payload is listed once, the better quality kept."""
        best = {}
        for g, s, i, d in self.entries():
            if not d.flags & 2:
                continue
            L, cce = self.slot_candidate(s)
            kind = "si" if d.rnti_x == 0xFFFF else "paging" if d.rnti_x == 0xFFFE else "ra"
            m = dict(subframe=g, L=L, cce=cce, kind=kind, rnti=int(d.rnti_x), size=(self.sizes[i] if i < len(self.sizes) else None), bits=int(d.bits),
                     quality=float(d.quality))
            key = (g, cce, i, int(d.bits), int(d.rnti_x))
            if key not in best or m["quality"] > best[key]["quality"]:
                best[key] = m
        return sorted(best.values(), key=lambda m: (m["subframe"], m["cce"], m["L"], -1 if m["size"] is None else m["size"]))

    def __repr__(self) -> str:  # pragma: no cover
        return f"PdcchInfo(n_sf={self.n_sf}, n_read={self.n_read}, n_accepted={self.n_accepted}, n_si={self.n_si}, n_paging={self.n_paging}, n_ra={self.n_ra})"


assert C.sizeof(PdcchCfg) == 68 and C.sizeof(PdcchDec) == 24 and C.sizeof(PdcchInfo) == 21640

# Payload sizes of the two DCI formats of the common search space (36.212 5.3.3.1.3, 5.3.3.1.4).
# 1A = flag 1 + localized/distributed 1 + RIV ceil(log2(n_rb (n_rb + 1) / 2)) + MCS 5 + HARQ 3 + NDI 1 + RV 2 + TPC 2
#    = 15 + ceil(log2(n_rb (n_rb + 1) / 2)); TDD has a 4-bit HARQ number and a 2-bit DAI: + 3.  One zero is appended when the size
#    is one of the ambiguous sizes of table 5.3.3.1.2-1 (12, 14, 16, 20, 24, 26, 32, 40, 44, 56).
# 1C = gap bit (n_rb >= 50) + ceil(log2(v (v + 1) / 2)) + TBS index 5, v = floor(N_VRB,gap1 / N_step), N_step = 2 (n_rb < 50) or 4,
#    N_VRB,gap1 = 2 min(N_gap, n_rb - N_gap) with N_gap = 3, 8, 12, 27, 32, 48 (36.211 table 6.2.3.2-1): v = 3, 7, 12, 11, 16, 24.
_DCI_SIZES = {6: (21, 23, 8), 15: (22, 25, 10), 25: (25, 27, 12), 50: (27, 29, 13), 75: (27, 30, 14), 100: (28, 31, 15)}
_DCI_AMBIGUOUS = (12, 14, 16, 20, 24, 26, 32, 40, 44, 56)


def dci_1a_size(n_rb: int, tdd: bool = False) -> int:
    """the size of format 1A from its fields (what the table holds)"""
    a = 15 + (n_rb * (n_rb + 1) // 2 - 1).bit_length() + (3 if tdd else 0)
    return a + 1 if a in _DCI_AMBIGUOUS else a


def dci_common_sizes(n_rb: int, tdd: bool = False):
    """(size of DCI format 1A, size of format 1C) of the common search space of an n_rb cell"""
    fdd, td, c = _DCI_SIZES[int(n_rb)]
    return (td if tdd else fdd), c


# ---------------------------------------------------------------- the blind search of every CCE (include/lcs.h: lcs_pdcch_scan_info)
PDCCH_SCAN_MAX_SIZES, PDCCH_SCAN_MAX_CCE, PDCCH_SCAN_MAX_CAND, PDCCH_SCAN_MAX_MSG = 6, 88, 165, 1024
PDCCH_SCAN_MIN_QUALITY = 0.75             # LCS_PDCCH_SCAN_MIN_QUALITY: tools/pdcch_scan_accuracy.py measures it
SCAN_DECODED, SCAN_ACCEPTED, SCAN_IN_SPACE, SCAN_TB_OK, SCAN_COMMON = 1, 2, 4, 8, 16


class PdcchScanCfg(C.Structure):
    """lcs_pdcch_scan_cfg.  PdcchScanCfg.make(sizes, ...): up to six payload sizes A in 8 .. 64; min_quality None = the default;
    min_repeat 1 turns the recurrence rule off; the other arguments as PdcchCfg.make's."""
    _fields_ = [("phich_duration", C.c_int32), ("phich_resource", C.c_int32), ("phich_mi", C.c_int32 * 10), ("n_sizes", C.c_int32),
                ("size", C.c_int32 * PDCCH_SCAN_MAX_SIZES), ("rnti_mask", C.c_int32), ("cfi_force", C.c_int32), ("min_repeat", C.c_int32),
                ("reserved", C.c_int32 * 2), ("min_quality", C.c_double)]

    @classmethod
    def make(cls, sizes, min_quality=None, min_repeat=2, phich_duration=0, phich_resource=0, phich_mi=None, rnti_mask=0, cfi_force=0) -> "PdcchScanCfg":
        sizes = [int(a) for a in sizes]
        if not 1 <= len(sizes) <= PDCCH_SCAN_MAX_SIZES:
            raise ValueError("PdcchScanCfg: one to six payload sizes")
        o = cls()
        o.phich_duration, o.phich_resource, o.rnti_mask, o.cfi_force, o.n_sizes = int(phich_duration), int(phich_resource), int(rnti_mask), int(cfi_force), len(sizes)
        o.min_repeat, o.min_quality = int(min_repeat), PDCCH_SCAN_MIN_QUALITY if min_quality is None else float(min_quality)
        for i, a in enumerate(sizes):
            o.size[i] = a
        for i in range(10):
            o.phich_mi[i] = -1 if phich_mi is None else (0 if phich_mi[i] is None else int(phich_mi[i]))
        return o


class PdcchScanDec(C.Structure):
    """lcs_pdcch_scan_dec: flags 1 decoded, 2 accepted, 4 in space, 8 tb_ok, 16 common kind"""
    _fields_ = [("bits", C.c_uint64), ("rnti_x", C.c_uint32), ("flags", C.c_int32), ("n_err", C.c_int16), ("n_obs", C.c_int16), ("n_repeat", C.c_int32),
                ("quality", C.c_double)]


class PdcchScanMsg(C.Structure):
    _fields_ = [("g", C.c_int16), ("L", C.c_uint8), ("cce", C.c_uint8), ("size_index", C.c_uint8), ("pad", C.c_uint8 * 3), ("d", PdcchScanDec)]


class PdcchScanSf(C.Structure):
    _fields_ = [("cfi", C.c_int32), ("n_reg", C.c_int32), ("n_cce", C.c_int32), ("n_cand", C.c_int32), ("n_common", C.c_int32), ("n_ue", C.c_int32),
                ("cce_mask", C.c_uint32 * 3)]


def scan_candidates(n_cce: int) -> list:
    """[(L, first CCE)] of a subframe with n_cce CCEs in the record's order: by L ascending, then by CCE"""
    return [(L, c) for L in (1, 2, 4, 8) for c in range(0, n_cce - L + 1, L)]


def ue_search_space(rnti: int, sf: int, n_cce: int, L: int) -> list:
    """The first CCEs of the candidates of the UE-specific search space of `rnti` in subframe sf at level L (36.213 9.1.1), in the
    order m' = 0 .. M(L) - 1 (duplicates where floor(n_cce / L) < M(L); none where it is 0)"""
    y = int(rnti)
    for _ in range(int(sf) % 10 + 1):
        y = (39827 * y) % 65537
    n = int(n_cce) // int(L)
    return [int(L) * ((y + m) % n) for m in range(6 if L <= 2 else 2)] if n else []


class PdcchScanInfo(C.Structure):
    """lcs_pdcch_scan_info: what the blind search of every CCE found (include/lcs.h: lcs_pdcch_scan_wide, lcs_pdcch_scan).  sf[g]: cfi,
    n_reg, n_cce, n_cand, the accepted common and UE entries and the CCEs they cover; msg[: n_msg]: every entry in space with
    sufficient quality and every accepted common one.  sizes: the payload sizes of the call."""
    _fields_ = [("n_sf", C.c_int32), ("n_read", C.c_int32), ("n_accepted", C.c_int32), ("n_si", C.c_int32), ("n_paging", C.c_int32), ("n_ra", C.c_int32),
                ("dl_mask", C.c_int32), ("n_rb", C.c_int32), ("n_ports", C.c_int32), ("n_ue", C.c_int32), ("n_rnti", C.c_int32), ("n_msg", C.c_int32),
                ("n_dropped", C.c_int32), ("n_sizes", C.c_int32), ("reserved", C.c_int32 * 2),
                ("sf", PdcchScanSf * PCFICH_MAX_SF), ("msg", PdcchScanMsg * PDCCH_SCAN_MAX_MSG)]
    sizes = ()

    def copy(self) -> "PdcchScanInfo":
        o = PdcchScanInfo()
        C.memmove(C.byref(o), C.byref(self), C.sizeof(PdcchScanInfo))
        o.sizes = tuple(self.sizes)
        return o

    def _n(self) -> int:
        return min(max(int(self.n_sf), 0), PCFICH_MAX_SF)

    @property
    def cfi(self):
        import numpy as np
        return np.array([self.sf[g].cfi for g in range(self._n())], np.int32)

    @property
    def n_cce(self):
        import numpy as np
        return np.array([self.sf[g].n_cce for g in range(self._n())], np.int32)

    def listed(self) -> list:
        """every entry of msg[: n_msg] as a dict, in the record's order"""
        out = []
        for i in range(min(max(int(self.n_msg), 0), PDCCH_SCAN_MAX_MSG)):
            m, d = self.msg[i], self.msg[i].d
            kind = "si" if d.rnti_x == 0xFFFF else "paging" if d.rnti_x == 0xFFFE else "ra" if d.flags & SCAN_COMMON else "ue"
            out.append(dict(subframe=int(m.g), L=int(m.L), cce=int(m.cce), size_index=int(m.size_index), kind=kind, rnti=int(d.rnti_x),
                            size=(self.sizes[m.size_index] if m.size_index < len(self.sizes) else None), bits=int(d.bits), quality=float(d.quality),
                            flags=int(d.flags), n_repeat=int(d.n_repeat), n_err=int(d.n_err), n_obs=int(d.n_obs)))
        return out

    def messages(self) -> list:
        """The accepted entries.  A DCI that is read again at a lower level or at an overlapping start -- the same subframe, RNTI, size
        and bits, on CCEs that overlap -- is listed once, at the largest accepted L (the better quality among equals)."""
        acc = sorted((m for m in self.listed() if m["flags"] & SCAN_ACCEPTED), key=lambda m: (-m["L"], -m["quality"]))
        kept = []
        for m in acc:
            same = lambda k: (k["subframe"], k["rnti"], k["size_index"], k["bits"]) == (m["subframe"], m["rnti"], m["size_index"], m["bits"])
            if not any(same(k) and k["cce"] < m["cce"] + m["L"] and m["cce"] < k["cce"] + k["L"] for k in kept):
                kept.append(m)
        return sorted(kept, key=lambda m: (m["subframe"], m["cce"], m["L"], m["size_index"]))

    def rntis(self) -> dict:
        """{C-RNTI: number of its grants} over messages()"""
        out = {}
        for m in self.messages():
            if m["kind"] == "ue":
                out[m["rnti"]] = out.get(m["rnti"], 0) + 1
        return out

    def load(self, n_rb: int, tdd: bool = False) -> list:
        """Per subframe read: dict(subframe, n_cce, cce_used, dl_grants, ul_grants, dl_prb, ul_prb, rntis) from the UE grants of
        messages(): format 0 and 1A by their first bit, formats 1, 1B/1D, 2A and 2 by their size (dci_ue_sizes with the record's port
        count); a grant whose size is none of them, or whose allocation does not read, counts as a grant without PRBs."""
        ports = int(self.n_ports)
        by_size = {}
        for name, a in dci_ue_sizes(n_rb, ports, tdd).items():
            by_size.setdefault(a, name)
        out = []
        msgs = self.messages()
        for g in range(self._n()):
            s = self.sf[g]
            if not s.cfi:
                continue
            row = dict(subframe=g, n_cce=int(s.n_cce), cce_used=sum(bin(w).count("1") for w in s.cce_mask), dl_grants=0, ul_grants=0, dl_prb=0, ul_prb=0, rntis=set())
            for m in msgs:
                if m["subframe"] != g or m["kind"] != "ue":
                    continue
                row["rntis"].add(m["rnti"])
                name = by_size.get(m["size"])
                f = None
                if name == "0/1A":
                    f = dci_0_fields(m["bits"], n_rb, tdd) if not m["bits"] & 1 else dci_1a_fields(m["bits"], n_rb, tdd)
                    if f is not None and "n_rb_alloc" in f and "prbs" not in f:
                        f = dict(f, prbs=list(range(f["rb_start"], f["rb_start"] + f["n_rb_alloc"])))
                elif name == "1":
                    f = dci_1_fields(m["bits"], n_rb, tdd)
                elif name in ("2A", "2"):
                    f = dci_2x_fields(m["bits"], n_rb, ports, name, tdd)
                up = name == "0/1A" and not m["bits"] & 1
                row["ul_grants" if up else "dl_grants"] += 1
                if f is not None and f.get("prbs") is not None:
                    row["ul_prb" if up else "dl_prb"] += len(f["prbs"])
            row["rntis"] = sorted(row["rntis"])
            out.append(row)
        return out

    def __repr__(self) -> str:  # pragma: no cover
        return (f"PdcchScanInfo(n_sf={self.n_sf}, n_read={self.n_read}, n_accepted={self.n_accepted}, n_ue={self.n_ue}, n_rnti={self.n_rnti}, "
                f"n_msg={self.n_msg}, n_dropped={self.n_dropped})")


assert C.sizeof(PdcchScanCfg) == 104 and C.sizeof(PdcchScanDec) == 32 and C.sizeof(PdcchScanMsg) == 40 and C.sizeof(PdcchScanSf) == 36 and C.sizeof(PdcchScanInfo) == 43616

PHICH_MAX_HI, PHICH_MAX_GROUP, PHICH_MAX_ENTRIES = 1024, 100, 400   # LCS_PHICH_MAX_HI, LCS_PHICH_MAX_GROUP, LCS_PHICH_MAX_ENTRIES
PHICH_MIN_AMP = 0.25                      # LCS_PHICH_MIN_AMP: a design floor
PHICH_MIN_SIGMA = 3.5                     # LCS_PHICH_MIN_SIGMA: tools/phich_accuracy.py measures it
PHICH_PRESENT, PHICH_ACK = 1, 2


class PhichCfg(C.Structure):
    """lcs_phich_cfg.  PhichCfg.make(...): the PHICH configuration as PdcchCfg.make's (0 = the cell's, phich_mi None = FDD); min_amp /
    min_sigma None = the defaults."""
    _fields_ = [("phich_duration", C.c_int32), ("phich_resource", C.c_int32), ("phich_mi", C.c_int32 * 10), ("reserved", C.c_int32 * 2),
                ("min_amp", C.c_double), ("min_sigma", C.c_double)]

    @classmethod
    def make(cls, phich_duration=0, phich_resource=0, phich_mi=None, min_amp=None, min_sigma=None) -> "PhichCfg":
        o = cls()
        o.phich_duration, o.phich_resource = int(phich_duration), int(phich_resource)
        o.min_amp = PHICH_MIN_AMP if min_amp is None else float(min_amp)
        o.min_sigma = PHICH_MIN_SIGMA if min_sigma is None else float(min_sigma)
        for i in range(10):
            o.phich_mi[i] = -1 if phich_mi is None else (0 if phich_mi[i] is None else int(phich_mi[i]))
        return o

    @property
    def tdd(self) -> bool:
        return any(m >= 0 for m in self.phich_mi)


class PhichSf(C.Structure):
    """lcs_phich_sf: n_unit -1 = the subframe was not read"""
    _fields_ = [("n_unit", C.c_int32), ("n_group", C.c_int32), ("n_present", C.c_int32), ("n_ack", C.c_int32), ("n_nack", C.c_int32), ("reserved", C.c_int32),
                ("noise", C.c_double)]


class PhichHi(C.Structure):
    """lcs_phich_hi: flags 1 present, 2 ack"""
    _fields_ = [("g", C.c_int16), ("group", C.c_uint8), ("seq", C.c_uint8), ("flags", C.c_int32), ("value", C.c_double), ("sigma", C.c_double)]


class PhichInfo(C.Structure):
    """lcs_phich_info: the HARQ indicators of every subframe of a full-bandwidth grid (include/lcs.h: lcs_phich_wide, lcs_phich).
    sf[g]: the subframe's units, groups, counts and noise; hi[: n_hi]: the present entries by (g, group, seq).  tdd: whether the call
    that made the record gave any m_i."""
    _fields_ = [("n_sf", C.c_int32), ("n_read", C.c_int32), ("n_present", C.c_int32), ("n_ack", C.c_int32), ("n_nack", C.c_int32), ("n_hi", C.c_int32),
                ("n_dropped", C.c_int32), ("dl_mask", C.c_int32), ("n_rb", C.c_int32), ("n_ports", C.c_int32), ("reserved", C.c_int32 * 2),
                ("sf", PhichSf * PCFICH_MAX_SF), ("hi", PhichHi * PHICH_MAX_HI)]
    tdd = False

    def copy(self) -> "PhichInfo":
        o = PhichInfo()
        C.memmove(C.byref(o), C.byref(self), C.sizeof(PhichInfo))
        o.tdd = self.tdd
        return o

    def _n(self) -> int:
        return min(max(int(self.n_sf), 0), PCFICH_MAX_SF)

    @property
    def n_unit(self):
        import numpy as np
        return np.array([self.sf[g].n_unit for g in range(self._n())], np.int32)

    @property
    def noise(self):
        import numpy as np
        return np.array([self.sf[g].noise for g in range(self._n())])

    def indicators(self) -> list:
        """the present entries as dicts, in the record's order: subframe, group, seq, ack, value, sigma"""
        out = []
        for i in range(min(max(int(self.n_hi), 0), PHICH_MAX_HI)):
            h = self.hi[i]
            out.append(dict(subframe=int(h.g), group=int(h.group), seq=int(h.seq), ack=bool(h.flags & PHICH_ACK), value=float(h.value), sigma=float(h.sigma)))
        return out

    def ack_rate(self):
        """the ACK share of the present entries (None without one): 1 - the cell's uplink block error rate"""
        return None if self.n_present <= 0 else self.n_ack / self.n_present

    def __repr__(self) -> str:  # pragma: no cover
        return f"PhichInfo(n_sf={self.n_sf}, n_read={self.n_read}, n_present={self.n_present}, n_ack={self.n_ack}, n_nack={self.n_nack}, n_dropped={self.n_dropped})"


assert C.sizeof(PhichCfg) == 72 and C.sizeof(PhichSf) == 32 and C.sizeof(PhichHi) == 24 and C.sizeof(PhichInfo) == 26928


def phich_n_group(n_rb: int, phich_resource: int, cp_normal: bool, mi: int = 1) -> int:
    """PHICH groups of a subframe (36.211 6.9): m_i ceil(Ng n_rb / 8), twice that with the extended CP.  phich_resource as lcs_cell's:
    1 .. 4 for Ng = 1/6, 1/2, 1, 2"""
    num, den = ((1, 6), (1, 2), (1, 1), (2, 1))[int(phich_resource) - 1]
    return int(mi) * -(-(num * int(n_rb)) // (8 * den)) * (1 if cp_normal else 2)


def phich_index(rb_start: int, cyclic_shift: int, n_group: int, cp_normal: bool, i_phich: int = 0):
    """(group, seq) of the indicator that answers an uplink grant (36.213 9.1.2): n_group = (I_PRB + n_DMRS) mod N_group + I_PHICH
    N_group, n_seq = (floor(I_PRB / N_group) + n_DMRS) mod 2 N_SF, with I_PRB = the grant's lowest PRB, n_DMRS = its cyclic-shift field
    (36.213 table 9.1.2-2 maps the field 0 .. 7 onto itself) and N_group = the groups of the subframe with m_i = 1"""
    rb_start, n_dmrs, n_group = int(rb_start), int(cyclic_shift), int(n_group)
    if n_group <= 0 or rb_start < 0 or not 0 <= n_dmrs <= 7 or i_phich not in (0, 1):
        raise ValueError("phich_index: needs n_group >= 1, rb_start >= 0, a cyclic shift field 0 .. 7 and I_PHICH 0 or 1")
    return (rb_start + n_dmrs) % n_group + int(i_phich) * n_group, (rb_start // n_group + n_dmrs) % (8 if cp_normal else 4)


def phich_for_grants(scan_info, phich_info, n_rb: int) -> list:
    """For every accepted format 0 message of a scan (PdcchScanInfo.messages()) at grid subframe g: the indicator of phich_info at
    subframe g + 8 and the index phich_index derives from the grant (N_group and the CP from what phich_info read that subframe
    with).  -> [dict(subframe, rnti, rb_start, cyclic_shift, phich_subframe, group, seq, status, value)] with status "ack", "nack",
    "absent", or "outside" when g + 8 is no subframe that phich_info read.  FDD only: a record of a TDD call raises (the TDD timing
    of 36.213 table 9.1.2-1 is not implemented)."""
    if getattr(phich_info, "tdd", False):
        raise ValueError("phich_for_grants: FDD only, and the PHICH record is a TDD call's")
    n_rb = int(n_rb)
    a01 = dci_1a_size(n_rb, False)
    present = {(h["subframe"], h["group"], h["seq"]): h for h in phich_info.indicators()}
    out = []
    for m in scan_info.messages():
        if m["kind"] != "ue" or m["size"] != a01 or m["bits"] & 1:
            continue
        f = dci_0_fields(m["bits"], n_rb, False)
        if f is None or f["rb_start"] is None:
            continue
        g8 = m["subframe"] + 8
        row = dict(subframe=m["subframe"], rnti=m["rnti"], rb_start=f["rb_start"], cyclic_shift=f["cyclic_shift"], phich_subframe=g8, group=None, seq=None,
                   status="outside", value=None)
        if g8 < phich_info._n() and phich_info.sf[g8].n_unit >= 0:
            s8 = phich_info.sf[g8]
            row["status"] = "absent"
            if s8.n_group > 0:
                row["group"], row["seq"] = phich_index(f["rb_start"], f["cyclic_shift"], int(s8.n_group), s8.n_group == s8.n_unit)
                h = present.get((g8, row["group"], row["seq"]))
                if h is not None:
                    row["status"], row["value"] = ("ack" if h["ack"] else "nack"), h["value"]
        out.append(row)
    return out


# Payload sizes of the DCI formats of the UE-specific search space, Release 8/9, no carrier indicator (36.212 5.3.3.1).  THE TABLE IS
# FROM MEMORY OF THE STANDARD; dci_ue_size_derived recomputes it from the field widths, and tests/test_pdcch_scan_host.py holds the
# two together.  With RIV = ceil(log2(n_rb (n_rb + 1) / 2)), RBG size P = 1, 2, 2, 3, 4, 4 for 6 .. 100 resource blocks, the bitmap
# B = ceil(n_rb / P), the header H = 1 where n_rb > 10, and T = 3 more bits in TDD (a 4-bit HARQ number and a 2-bit DAI):
#   0      flag 1 + hopping 1 + RIV + MCS/RV 5 + NDI 1 + TPC 2 + cyclic shift 3 + CQI request 1 (+ UL index / DAI 2 in TDD), padded to 1A
#   1A     flag 1 + localized/distributed 1 + RIV + MCS 5 + HARQ 3 + NDI 1 + RV 2 + TPC 2 + T (dci_1a_size)
#   1      H + B + MCS 5 + HARQ 3 + NDI 1 + RV 2 + TPC 2 + T
#   1B/1D  localized/distributed 1 + RIV + MCS 5 + HARQ 3 + NDI 1 + RV 2 + TPC 2 + TPMI 2 (2 ports) or 4
#          (4 ports) + PMI confirmation (1B) or power offset (1D) 1 + T
#   2A     H + B + TPC 2 + HARQ 3 + swap flag 1 + 2 x (MCS 5 + NDI 1 + RV 2) + precoding 0 (2 ports) or 2 (4 ports) + T
#   2      the same with precoding 3 (2 ports) or 6 (4 ports)
# Padding: a format other than 0/1A whose size equals 0/1A's gets one zero; then zeros are appended while the size is one of the
# ambiguous sizes 12, 14, 16, 20, 24, 26, 32, 40, 44, 56 (and, for format 1, while it equals 0/1A's).
_RBG_P = {6: 1, 15: 2, 25: 2, 50: 3, 75: 4, 100: 4}
_DCI_UE_SIZES = {      # (n_rb, ports) -> sizes of formats 1, 1B/1D, 2A, 2 in FDD (0/1A: dci_1a_size)
    (6, 1): (19, None, None, None), (6, 2): (19, 22, 28, 31), (6, 4): (19, 25, 30, 34),
    (15, 1): (23, None, None, None), (15, 2): (23, 25, 31, 34), (15, 4): (23, 27, 33, 37),
    (25, 1): (27, None, None, None), (25, 2): (27, 27, 36, 39), (25, 4): (27, 28, 38, 42),
    (50, 1): (31, None, None, None), (50, 2): (31, 28, 41, 43), (50, 4): (31, 30, 42, 46),
    (75, 1): (33, None, None, None), (75, 2): (33, 29, 42, 45), (75, 4): (33, 31, 45, 48),
    (100, 1): (39, None, None, None), (100, 2): (39, 30, 48, 51), (100, 4): (39, 33, 50, 54),
}
_DCI_UE_NAMES = ("1", "1B/1D", "2A", "2")


def dci_ue_size_derived(fmt: str, n_rb: int, ports: int, tdd: bool = False):
    """the size of a format of the UE-specific search space from its field widths and the padding rules (None: the format needs
    more ports)"""
    n_rb, ports, t = int(n_rb), int(ports), 3 if tdd else 0
    riv = (n_rb * (n_rb + 1) // 2 - 1).bit_length()
    a01 = dci_1a_size(n_rb, tdd)
    if fmt == "0/1A":
        return a01
    ra = (1 if n_rb > 10 else 0) + -(-n_rb // _RBG_P[n_rb])
    if fmt == "1":
        a = ra + 13 + t
    elif ports < 2:
        return None
    elif fmt == "1B/1D":
        a = 14 + riv + (2 if ports == 2 else 4) + 1 + t
    elif fmt == "2A":
        a = ra + 22 + (0 if ports == 2 else 2) + t
    elif fmt == "2":
        a = ra + 22 + (3 if ports == 2 else 6) + t
    else:
        raise ValueError("no such format")
    if a == a01:
        a += 1
    while a in _DCI_AMBIGUOUS or (fmt == "1" and a == a01):
        a += 1
    return a


def dci_ue_sizes(n_rb: int, ports: int, tdd: bool = False) -> dict:
    """{"0/1A", "1", "1B/1D", "2A", "2"} -> payload size for an n_rb cell with 1, 2 or 4 ports (the formats that need two ports are
    left out with one).  FDD from the table; TDD from the derivation (the table holds FDD alone)."""
    ports = 4 if int(ports) == 4 else 2 if int(ports) == 2 else 1
    out = {"0/1A": dci_1a_size(int(n_rb), tdd)}
    for name, a in zip(_DCI_UE_NAMES, _DCI_UE_SIZES[(int(n_rb), ports)]):
        if a is not None:
            out[name] = dci_ue_size_derived(name, n_rb, ports, True) if tdd else a
    return out


def _dci_take(bits, size):
    if isinstance(bits, int):
        bits = [(bits >> t) & 1 for t in range(size)]
    bits = [int(b) for b in bits]
    pos = [0]

    def take(n):
        v = 0
        for _ in range(n):
            v = (v << 1) | bits[pos[0]]
            pos[0] += 1
        return v
    return take


def _riv_decode(riv, n_rb):
    """-> (rb_start, n_rb_alloc) or None for a value no allocation gives"""
    l1, s = riv // n_rb + 1, riv % n_rb
    if s + l1 > n_rb:
        l1, s = n_rb + 2 - l1, n_rb - 1 - s
    return (s, l1) if 1 <= l1 <= n_rb - s and riv < n_rb * (n_rb + 1) // 2 else None


def ra_type01_prbs(header: int, field: int, n_rb: int) -> list:
    """The PRB set of a type 0 (header 0: one bit per RBG, the first RBG on the field's MSB) or type 1 (header 1: subset, shift, one
    bit per PRB of the subset) allocation of ceil(n_rb / P) bits (36.213 7.1.6.1, 7.1.6.2)"""
    n_rb = int(n_rb)
    P = _RBG_P[n_rb]
    nb = -(-n_rb // P)
    bit = lambda i, width: (field >> (width - 1 - i)) & 1
    if not header:
        return [r for i in range(nb) if bit(i, nb) for r in range(P * i, min(P * i + P, n_rb))]
    lp = (P - 1).bit_length()
    n1 = nb - lp - 1
    p, shift = field >> (nb - lp), bit(lp, nb)
    if p >= P:
        return None
    q = (n_rb - 1) // P
    n_sub = (n_rb - 1) // (P * P) * P + (P if p < q % P else (n_rb - 1) % P + 1 if p == q % P else 0)
    delta = n_sub - n1 if shift else 0
    out = []
    for i in range(n1):
        if bit(lp + 1 + i, nb):
            v = (i + delta) // P * P * P + p * P + (i + delta) % P
            if v < n_rb:
                out.append(v)
    return out


def dci_0_fields(bits, n_rb: int, tdd: bool = False):
    """The fields of a format 0 payload (36.212 5.3.3.1.1; the first bit is 0, format 1A's is 1) -> dict with rb_start, n_rb_alloc and
    prbs (None for a RIV that no allocation gives), or None when the first bit says 1A"""
    n_rb = int(n_rb)
    take = _dci_take(bits, dci_1a_size(n_rb, tdd))
    if take(1):
        return None
    out = dict(format="0", hopping=take(1))
    riv = take((n_rb * (n_rb + 1) // 2 - 1).bit_length())
    out.update(mcs=take(5), ndi=take(1), tpc=take(2), cyclic_shift=take(3))
    if tdd:
        out["ul_index_dai"] = take(2)
    out["cqi_request"] = take(1)
    al = _riv_decode(riv, n_rb)
    out.update(riv=riv, rb_start=None if al is None else al[0], n_rb_alloc=None if al is None else al[1], prbs=None if al is None else list(range(al[0], al[0] + al[1])))
    return out


def dci_1_fields(bits, n_rb: int, tdd: bool = False) -> dict:
    """The fields of a format 1 payload (36.212 5.3.3.1.2): type 0 or type 1 resource allocation -> prbs"""
    n_rb = int(n_rb)
    take = _dci_take(bits, dci_ue_size_derived("1", n_rb, 1, tdd))
    header = take(1) if n_rb > 10 else 0
    field = take(-(-n_rb // _RBG_P[n_rb]))
    out = dict(format="1", ra_type=header, ra=field, mcs=take(5), harq=take(4 if tdd else 3), ndi=take(1), rv=take(2), tpc=take(2))
    if tdd:
        out["dai"] = take(2)
    out["prbs"] = ra_type01_prbs(header, field, n_rb)
    return out


def dci_2x_fields(bits, n_rb: int, ports: int, fmt: str = "2A", tdd: bool = False) -> dict:
    """The fields of a format 2 or 2A payload (36.212 5.3.3.1.5, 5.3.3.1.5A) with 2 or 4 ports -> prbs, two transport blocks"""
    n_rb, ports = int(n_rb), int(ports)
    take = _dci_take(bits, dci_ue_size_derived(fmt, n_rb, ports, tdd))
    header = take(1) if n_rb > 10 else 0
    field = take(-(-n_rb // _RBG_P[n_rb]))
    out = dict(format=fmt, ra_type=header, ra=field, tpc=take(2))
    if tdd:
        out["dai"] = take(2)
    out.update(harq=take(4 if tdd else 3), swap=take(1))
    out["tb"] = [dict(mcs=take(5), ndi=take(1), rv=take(2)) for _ in range(2)]
    out["precoding"] = take({("2A", 2): 0, ("2A", 4): 2, ("2", 2): 3, ("2", 4): 6}[(fmt, ports)])
    out["prbs"] = ra_type01_prbs(header, field, n_rb)
    return out


# 36.211 table 6.9-1: m_i per uplink-downlink configuration and subframe; None = an uplink subframe.  Only a default the caller may
# override (lcs_pdcch_cfg.phich_mi): a wrong entry here is a wrong default, not a wrong kernel.
_TDD_PHICH_MI = [[2, 1, None, None, None, 2, 1, None, None, None], [0, 1, None, None, 1, 0, 1, None, None, 1], [0, 0, None, 1, 0, 0, 0, None, 1, 0],
                 [1, 0, None, None, None, 0, 0, 0, 1, 1], [0, 0, None, None, 0, 0, 0, 0, 1, 1], [0, 0, None, 0, 0, 0, 0, 0, 1, 0],
                 [1, 1, None, None, None, 1, 1, None, None, 1]]


def tdd_phich_mi(config: int) -> list:
    """m_i of subframes 0 .. 9 of uplink-downlink configuration 0 .. 6 (None: uplink)"""
    return list(_TDD_PHICH_MI[int(config)])


def dci_1a_fields(bits, n_rb: int, tdd: bool = False) -> dict:
    """The fields of a format 1A payload (36.212 5.3.3.1.3) as it is used with SI-, P- and RA-RNTI.  bits: the payload as an int (bit t
    = the t-th bit sent: PdcchInfo.messages()' "bits") or a sequence of bits in the order sent."""
    size = dci_common_sizes(n_rb, tdd)[0]
    if isinstance(bits, int):
        bits = [(bits >> t) & 1 for t in range(size)]
    bits = [int(b) for b in bits]
    pos = [0]

    def take(n):
        v = 0
        for b in bits[pos[0]:pos[0] + n]:
            v = (v << 1) | b
        pos[0] += n
        return v
    out = dict(flag_1a=take(1), distributed=take(1))
    riv = take((n_rb * (n_rb + 1) // 2 - 1).bit_length())
    length, start = riv // n_rb + 1, riv % n_rb
    if length + start > n_rb:
        length, start = n_rb - length + 2, n_rb - 1 - start
    out.update(riv=riv, rb_start=start, n_rb_alloc=length, mcs=take(5), harq=take(4 if tdd else 3), ndi=take(1), rv=take(2), tpc=take(2))
    if tdd:
        out["dai"] = take(2)
    return out


# ---- the PDSCH behind the grants of the common search space (include/lcs.h: lcs_pdsch_info) ----
PDSCH_MAX_BLOCKS, PDSCH_MAX_FORCED, PDSCH_PAYLOAD, PDSCH_N_STATUS = 32, 4, 280, 10
PDSCH_OK, PDSCH_CRC, PDSCH_DISTRIBUTED, PDSCH_MCS, PDSCH_ROWS, PDSCH_SPECIAL, PDSCH_SILENT, PDSCH_BAD_ALLOC, PDSCH_NO_CFI = range(1, 10)
PDSCH_STATUS = {0: "none", 1: "ok", 2: "crc", 3: "distributed", 4: "mcs", 5: "rows", 6: "special", 7: "silent", 8: "bad_alloc", 9: "no_cfi"}
# 36.213 table 7.1.7.2.1-1, columns N_PRB = 2 and 3, I_TBS 0 .. 26: written from memory of the standard, as pdsch.h's copy (what pins
# both is said there)
_TBS_1A = [[32, 56, 72, 104, 120, 144, 176, 208, 256, 296, 328, 376, 440, 488, 552, 600, 632, 696, 776, 840, 904, 1000, 1064, 1128, 1192, 1256, 1480],
           [56, 88, 144, 176, 208, 224, 256, 328, 392, 456, 504, 584, 680, 744, 840, 904, 968, 1064, 1160, 1288, 1384, 1480, 1608, 1736, 1800, 1864, 2216]]


def tbs_1a(mcs: int, tpc: int) -> int:
    """the transport block size of a format 1A grant with SI-, P- or RA-RNTI (36.213 7.1.7.2.1): I_TBS = mcs <= 26, column N_PRB = 2
    where the low TPC bit is 0, else 3"""
    return _TBS_1A[int(tpc) & 1][int(mcs)]


class PdschGrant(C.Structure):
    _fields_ = [("subframe", C.c_int32), ("rnti", C.c_int32), ("rb_start", C.c_int32), ("n_prb", C.c_int32), ("tbs", C.c_int32), ("rv", C.c_int32)]


class PdschCfg(C.Structure):
    """lcs_pdsch_cfg.  PdschCfg.make(i_1a, max_iter, rnti_mask, forced): zeros are the defaults; forced: up to four dicts or tuples
    (subframe, rnti, rb_start, n_prb, tbs, rv) that replace the PDCCH's grants"""
    _fields_ = [("i_1a", C.c_int32), ("max_iter", C.c_int32), ("rnti_mask", C.c_int32), ("n_forced", C.c_int32), ("forced", PdschGrant * PDSCH_MAX_FORCED)]

    @classmethod
    def make(cls, i_1a=0, max_iter=0, rnti_mask=0, forced=()) -> "PdschCfg":
        forced = list(forced)
        if len(forced) > PDSCH_MAX_FORCED:
            raise ValueError("PdschCfg: at most four forced grants")
        o = cls()
        o.i_1a, o.max_iter, o.rnti_mask, o.n_forced = int(i_1a), int(max_iter), int(rnti_mask), len(forced)
        for i, g in enumerate(forced):
            v = [g[k] for k in ("subframe", "rnti", "rb_start", "n_prb", "tbs", "rv")] if isinstance(g, dict) else list(g)
            o.forced[i] = PdschGrant(*[int(x) for x in v])
        return o


class PdschBlock(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("subframe", "slot", "rnti", "kind", "rb_start", "n_prb", "mcs", "rv", "tbs", "n_re", "K", "F", "n_iter", "status")] + \
               [("payload", C.c_uint8 * PDSCH_PAYLOAD)]


class PdschInfo(C.Structure):
    """lcs_pdsch_info: the transport blocks behind the format 1A grants of every subframe of a full-bandwidth grid (include/lcs.h:
    lcs_pdsch_wide, lcs_pdsch)"""
    _fields_ = [(k, C.c_int32) for k in ("n_sf", "n_blocks", "n_ok", "n_si", "n_paging", "n_ra", "n_overflow", "dl_mask", "n_rb", "n_ports")] + \
               [("n_status", C.c_int32 * PDSCH_N_STATUS), ("block", PdschBlock * PDSCH_MAX_BLOCKS)]

    def copy(self) -> "PdschInfo":
        o = PdschInfo()
        C.memmove(C.byref(o), C.byref(self), C.sizeof(PdschInfo))
        return o

    def blocks(self) -> list:
        """the listed grants as dicts: the block's fields, kind and status as words, crc_ok, and bytes = the transport block (tbs / 8
        bytes rounded up, MSB first; empty unless the block was decoded)"""
        out = []
        for i in range(min(max(int(self.n_blocks), 0), PDSCH_MAX_BLOCKS)):
            b = self.block[i]
            d = {k: int(getattr(b, k)) for k, _ in PdschBlock._fields_[:14]}
            d["kind"] = {1: "si", 2: "paging", 4: "ra"}.get(b.kind, "other")
            d["status"] = PDSCH_STATUS.get(b.status, "?")
            d["crc_ok"] = b.status == PDSCH_OK
            d["bytes"] = bytes(b.payload[:(b.tbs + 7) // 8]) if b.status in (PDSCH_OK, PDSCH_CRC) else b""
            out.append(d)
        return out

    def __repr__(self) -> str:  # pragma: no cover
        return f"PdschInfo(n_sf={self.n_sf}, n_blocks={self.n_blocks}, n_ok={self.n_ok}, n_si={self.n_si}, n_paging={self.n_paging}, n_ra={self.n_ra})"


assert C.sizeof(PdschCfg) == 112 and C.sizeof(PdschBlock) == 336 and C.sizeof(PdschInfo) == 10832

# ---- distributed allocations and format 1C (include/lcs.h: lcs_pdsch_alloc_cfg; the rule is written from memory of the standard) ----
PDSCH_ALLOC_RB = 112
# 36.213 table 7.1.7.2.3-1: the transport block sizes of format 1C, as pdsch.h's copy
_TBS_1C = [40, 56, 72, 120, 136, 144, 176, 208, 224, 256, 280, 296, 328, 336, 392, 488, 552, 600, 632, 696, 776, 840, 904, 1000, 1064, 1128, 1224, 1288, 1384, 1480,
           1608, 1736]


def tbs_1c(i: int) -> int:
    """the transport block size of a format 1C grant with I_TBS = i (36.213 7.1.7.2.3)"""
    return _TBS_1C[int(i)]


def dvrb_gap(n_rb: int):
    """(N_gap,1, N_gap,2 or None) of an n_rb cell (36.211 table 6.2.3.2-1)"""
    n_rb = int(n_rb)
    g1 = -(-n_rb // 2) if n_rb <= 10 else 4 if n_rb == 11 else 8 if n_rb <= 19 else 12 if n_rb <= 26 else 18 if n_rb <= 44 else 27 if n_rb <= 63 else 32 if n_rb <= 79 else 48
    return g1, (None if n_rb < 50 else 9 if n_rb <= 63 else 16)


def dvrb_sizes(n_rb: int, gap: int) -> dict:
    """n_gap, n_vrb, the interleaving unit, n_row and n_null of gap index 0 (N_gap,1) or 1 (N_gap,2; n_rb >= 50)"""
    n_rb = int(n_rb)
    n_gap = dvrb_gap(n_rb)[1 if gap else 0]
    if n_gap is None:
        raise ValueError("dvrb: no second gap below 50 resource blocks")
    n_vrb = (n_rb // (2 * n_gap)) * 2 * n_gap if gap else 2 * min(n_gap, n_rb - n_gap)
    unit = 2 * n_gap if gap else n_vrb
    p = 1 if n_rb <= 10 else 2 if n_rb <= 26 else 3 if n_rb <= 63 else 4
    n_row = -(-unit // (4 * p)) * p
    return dict(n_gap=n_gap, n_vrb=n_vrb, unit=unit, n_row=n_row, n_null=4 * n_row - unit)


def dvrb_prb(n_rb: int, gap: int, vrb: int, slot: int) -> int:
    """the PRB that distributed VRB `vrb` takes in a slot of that parity (36.211 6.2.3.2)"""
    z = dvrb_sizes(n_rb, gap)
    unit, n_row, n_null = z["unit"], z["n_row"], z["n_null"]
    if not 0 <= int(vrb) < z["n_vrb"]:
        raise ValueError("dvrb_prb: the VRB is outside N_VRB")
    t, o = int(vrb) % unit, unit * (int(vrb) // unit)
    a, b = 2 * n_row * (t % 2) + t // 2, n_row * (t % 4) + t // 4
    r = b
    if n_null and t >= unit - n_null:
        r = a - n_row if t % 2 else a - n_row + n_null // 2
    elif n_null and t % 4 >= 2:
        r = b - n_null // 2
    if int(slot) & 1:
        r = (r + unit // 2) % unit
    return o + (r if r < unit // 2 else r + z["n_gap"] - unit // 2)


def dci_1c_riv_bits(n_rb: int) -> int:
    v1 = dvrb_sizes(n_rb, 0)["n_vrb"] // (2 if int(n_rb) < 50 else 4)
    return (v1 * (v1 + 1) // 2 - 1).bit_length()


def dci_1c_fields(bits, n_rb: int) -> dict:
    """The fields of a format 1C payload (36.212 5.3.3.1.4).  bits: the payload as an int (bit t = the t-th bit sent) or a sequence of
    bits in the order sent -> gap, riv, riv_ok, rb_start and n_rb_alloc (VRBs), n_step, i_tbs, tbs"""
    n_rb = int(n_rb)
    size = (1 if n_rb >= 50 else 0) + dci_1c_riv_bits(n_rb) + 5
    if isinstance(bits, int):
        bits = [(bits >> t) & 1 for t in range(size)]
    bits = [int(b) for b in bits]
    pos = [0]

    def take(n):
        v = 0
        for b in bits[pos[0]:pos[0] + n]:
            v = (v << 1) | b
        pos[0] += n
        return v
    gap = take(1) if n_rb >= 50 else 0
    step = 2 if n_rb < 50 else 4
    riv = take(dci_1c_riv_bits(n_rb))
    n = dvrb_sizes(n_rb, gap)["n_vrb"] // step
    length, start = riv // n + 1, riv % n
    if length + start > n:
        length, start = n - length + 2, n - 1 - start
    i_tbs = take(5)
    return dict(gap=gap, riv=riv, riv_ok=riv < n * (n + 1) // 2, rb_start=step * start, n_rb_alloc=step * length, n_step=step, i_tbs=i_tbs, tbs=_TBS_1C[i_tbs])


class PdschAllocCfg(C.Structure):
    """lcs_pdsch_alloc_cfg.  PdschAllocCfg.make(distributed, format_1c, sfn0, si_window): which grants beyond localized 1A the PDSCH
    calls follow; sfn0 = the frame number of grid subframe 0 (-1: unknown) and si_window in subframes (0: unknown) give a 1C SI
    grant its assumed redundancy version"""
    _fields_ = [("flags", C.c_int32), ("sfn0", C.c_int32), ("si_window", C.c_int32), ("reserved", C.c_int32)]

    @classmethod
    def make(cls, distributed=False, format_1c=False, sfn0=-1, si_window=0) -> "PdschAllocCfg":
        o = cls()
        o.flags, o.sfn0, o.si_window = (1 if distributed else 0) | (2 if format_1c else 0), int(sfn0), int(si_window)
        return o


class PdschAlloc(C.Structure):
    """lcs_pdsch_alloc: how a listed block was allocated (lcs_pdsch_last_alloc)"""
    _fields_ = [(k, C.c_int32) for k in ("format", "distributed", "gap", "n_gap", "n_vrb", "n_step", "n_prb", "reserved")] + [("prb", (C.c_uint8 * PDSCH_ALLOC_RB) * 2)]

    def as_dict(self) -> dict:
        d = {k: int(getattr(self, k)) for k in ("distributed", "gap", "n_gap", "n_vrb", "n_step", "n_prb")}
        d["format"] = "1c" if self.format else "1a"
        d["prb"] = [[int(self.prb[s][i]) for i in range(self.n_prb)] for s in range(2)]
        return d


assert C.sizeof(PdschAllocCfg) == 16 and C.sizeof(PdschAlloc) == 256

# ---- the redundancy versions of an SI transport block, combined (include/lcs.h: lcs_pdsch_comb_info) ----
PDSCH_COMB_MAX_GROUPS, PDSCH_COMB_MAX_MEMBERS, PDSCH_COMB_N_STATUS = 8, 4, 5
PDSCH_COMB_MEMBER, PDSCH_COMB_OK, PDSCH_COMB_CRC, PDSCH_COMB_SILENT = range(1, 5)
PDSCH_COMB_STATUS = {0: "none", 1: "member", 2: "ok", 3: "crc", 4: "silent"}


def sib1_rv(sfn: int) -> int:
    """the redundancy version of the SIB1 transmission in subframe 5 of (even) frame sfn: ceil(3 k / 2) mod 4 with k = (sfn / 2) mod 4
    (36.321 5.3.1), i.e. 0, 2, 3, 1"""
    k = (int(sfn) // 2) % 4
    return -(-3 * k // 2) % 4


class PdschCombCfg(C.Structure):
    """lcs_pdsch_comb_cfg.  PdschCombCfg.make(si_window, sib1): si_window 0 = rule 2 off, else 1 .. 61 subframes; sib1=False switches
    rule 1 off"""
    _fields_ = [("si_window", C.c_int32), ("no_sib1", C.c_int32), ("reserved", C.c_int32 * 2)]

    @classmethod
    def make(cls, si_window=0, sib1=True) -> "PdschCombCfg":
        o = cls()
        o.si_window, o.no_sib1 = int(si_window), 0 if sib1 else 1
        return o


class PdschCombGroup(C.Structure):
    _fields_ = [("n_members", C.c_int32), ("member", C.c_int32 * PDSCH_COMB_MAX_MEMBERS)] + \
               [(k, C.c_int32) for k in ("rule", "tbs", "K", "F", "rv_mask", "n_ok_members", "n_same", "n_iter", "status")] + \
               [("reserved", C.c_int32 * 2), ("payload", C.c_uint8 * PDSCH_PAYLOAD)]


class PdschCombInfo(C.Structure):
    """lcs_pdsch_comb_info: the groups of SI blocks that repeat one transport block and what the sum of their soft bits decodes to
    (include/lcs.h: lcs_pdsch_comb_wide, lcs_pdsch_comb)"""
    _fields_ = [(k, C.c_int32) for k in ("n_groups", "n_overflow", "n_members", "n_decoded")] + \
               [("n_status", C.c_int32 * PDSCH_COMB_N_STATUS), ("reserved", C.c_int32 * 3), ("group", PdschCombGroup * PDSCH_COMB_MAX_GROUPS)]

    def groups(self) -> list:
        """the listed groups as dicts: members (block indices of the PDSCH record), rule, tbs, K, F, rvs, n_ok_members, n_same, n_iter,
        status as a word, crc_ok (the payload passed a CRC: in a member, or combined) and bytes = the transport block (empty for a
        silent sum)"""
        out = []
        for i in range(min(max(int(self.n_groups), 0), PDSCH_COMB_MAX_GROUPS)):
            g = self.group[i]
            d = {k: int(getattr(g, k)) for k in ("rule", "tbs", "K", "F", "n_ok_members", "n_same", "n_iter")}
            d["members"] = [int(g.member[m]) for m in range(min(max(int(g.n_members), 0), PDSCH_COMB_MAX_MEMBERS))]
            d["rvs"] = [rv for rv in range(4) if (g.rv_mask >> rv) & 1]
            d["status"] = PDSCH_COMB_STATUS.get(g.status, "?")
            d["crc_ok"] = g.status in (PDSCH_COMB_MEMBER, PDSCH_COMB_OK)
            d["bytes"] = bytes(g.payload[:(g.tbs + 7) // 8]) if g.status in (PDSCH_COMB_MEMBER, PDSCH_COMB_OK, PDSCH_COMB_CRC) else b""
            out.append(d)
        return out

    def __repr__(self) -> str:  # pragma: no cover
        return f"PdschCombInfo(n_groups={self.n_groups}, n_overflow={self.n_overflow}, n_status={list(self.n_status)})"


assert C.sizeof(PdschCombCfg) == 16 and C.sizeof(PdschCombGroup) == 344 and C.sizeof(PdschCombInfo) == 2800


def sib1_fields(payload):
    """The fields of a BCCH-DL-SCH-Message that carries SystemInformationBlockType1, read in UPER up to and including tdd-Config
    (written from memory of 36.331; synth.sib1_message is the matching writer: a convenience, not part of any kernel's rule).
    payload: bytes (MSB first) or a sequence of bits.  -> dict(plmns [(mcc, mnc, reserved)], tac, cell_id, barred, intra_freq, csg,
    csg_id, q_rx_lev_min and q_rx_lev_min_offset (the fields' values: dBm and dB are twice them), p_max, band, sched [(periodicity in
    radio frames, [SIB numbers])],
    tdd (subframeAssignment, specialSubframePatterns) or None, si_window (ms), value_tag), or None for a message that is not SIB1 or
    runs out of bits."""
    bits = [(byte >> (7 - i)) & 1 for byte in payload for i in range(8)] if isinstance(payload, (bytes, bytearray)) else [int(b) & 1 for b in payload]
    pos = [0]

    def take(n):
        if pos[0] + n > len(bits):
            raise IndexError
        v = 0
        for b in bits[pos[0]:pos[0] + n]:
            v = (v << 1) | b
        pos[0] += n
        return v
    try:
        if take(1) != 0 or take(1) != 1:
            return None
        has_pmax, has_tdd, _ext = take(1), take(1), take(1)
        has_csg_id = take(1)
        plmns, mcc = [], None
        for _ in range(take(3) + 1):
            if take(1):
                mcc = "".join(str(take(4)) for _ in range(3))
            mnc = "".join(str(take(4)) for _ in range(2 + take(1)))
            plmns.append((mcc, mnc, take(1) == 0))
        if len(plmns) > 6 or plmns[0][0] is None:
            return None
        out = dict(plmns=plmns, tac=take(16), cell_id=take(28), barred=take(1) == 0, intra_freq=take(1) == 0, csg=bool(take(1)))
        out["csg_id"] = take(27) if has_csg_id else None
        has_off = take(1)
        out["q_rx_lev_min"] = take(6) - 70
        out["q_rx_lev_min_offset"] = take(3) + 1 if has_off else None
        out["p_max"] = take(6) - 30 if has_pmax else None
        out["band"] = take(6) + 1
        sched = []
        for _ in range(take(5) + 1):
            per = take(3)
            sibs = []
            for _ in range(take(5)):
                if take(1):
                    return None          # an extended SIB type: beyond this reading
                sibs.append(take(4) + 3)
            sched.append((8 << per if per < 7 else None, sibs))
        out["sched"] = sched
        out["tdd"] = (take(3), take(4)) if has_tdd else None
        w = take(3)
        out["si_window"] = (1, 2, 5, 10, 15, 20, 40)[w] if w < 7 else None
        out["value_tag"] = take(5)
        return out
    except IndexError:
        return None


EXPORTS = [
    "lcs_create", "lcs_destroy", "lcs_last_error", "lcs_version", "lcs_cell_init", "lcs_set_max_cells_in_flight", "lcs_set_float_batch_probe",
    "lcs_set_batch_screen", "lcs_get_batch_screen", "lcs_last_screen_stats", "lcs_set_duplex", "lcs_get_duplex", "lcs_set_foe_unwrap", "lcs_get_foe_unwrap", "lcs_pss_foe_coarse",
    "lcs_set_tdd_config", "lcs_get_tdd_config", "lcs_tdd_config", "lcs_last_tdd_info",
    "lcs_set_cell_meas", "lcs_get_cell_meas", "lcs_cell_meas", "lcs_last_cell_meas", "lcs_tdd_dl_mask",
    "lcs_extract_tfg_wide", "lcs_cell_meas_wide", "lcs_pcfich_wide", "lcs_pcfich", "lcs_pdcch_wide", "lcs_pdcch", "lcs_pdcch_scan_wide", "lcs_pdcch_scan", "lcs_pdcch_scan_decodes", "lcs_phich_wide", "lcs_phich", "lcs_phich_values", "lcs_pdsch_wide", "lcs_pdsch", "lcs_turbo_decode", "lcs_pdsch_last_soft", "lcs_pdsch_comb_wide", "lcs_pdsch_comb",
    "lcs_set_pdsch_alloc", "lcs_pdsch_last_alloc",
    "lcs_xcorr_pss", "lcs_peak_search", "lcs_sss_detect", "lcs_pss_sss_foe", "lcs_extract_tfg", "lcs_tfoec",
    "lcs_decode_mib", "lcs_pbch_soft", "lcs_chan_est", "lcs_search_capbuf", "lcs_search_batch_dev", "lcs_search_batch_host", "lcs_batch_enqueue",
    "lcs_batch_collect", "lcs_batch_readback", "lcs_batch_enqueue_host", "lcs_host_alloc", "lcs_host_free", "lcs_device_alloc", "lcs_device_free", "lcs_device_upload", "lcs_device_count",
    "lcs_foe_partial", "lcs_foe_finish", "lcs_foe_contend", "lcs_foe_resolve", "lcs_track_block", "lcs_track_stats", "lcs_track_stream_block", "lcs_track_stream_reset", "lcs_track_cut", "lcs_stream_open", "lcs_stream_push", "lcs_stream_collect", "lcs_stream_close",
    "lcs_last_xcorr_ms", "lcs_last_xcorr_info", "lcs_last_frq_repairs", "lcs_last_frq_repair_stats", "lcs_frq_tie_eps", "lcs_last_batch_stats", "lcs_last_collect_host_us", "lcs_stream", "lcs_sync", "lcs_table_pss_td", "lcs_table_pss_fd", "lcs_table_sss_fd",
    "lcs_table_lte_pn", "lcs_chi2cdf_inv", "lcs_channelizer_taps", "lcs_channelize", "lcs_last_channelize_ms",
    "lcs_channelizer_proto", "lcs_channelize_rational", "lcs_channelize_u8",
    "lcs_chan_stream_open", "lcs_chan_stream_count", "lcs_chan_stream_push", "lcs_chan_stream_close",
    "lcs_chan_stream_open_u8", "lcs_chan_stream_count_u8", "lcs_chan_stream_push_u8",
    "lcs_sic_cancel_dev", "lcs_search_capbuf_sic", "lcs_search_batch_sic_dev", "lcs_last_sic_stats", "lcs_table_pbch_symbols",
    "lcs_sic_cancel_cfg_dev", "lcs_last_sic_tdd_info", "lcs_last_sic_cell_meas",
]

_lib = None


def load() -> C.CDLL:
    """Load liblcs_amd.so (built by __graft_entry__.build()); raises if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950); "
                           "there is no CPU fallback for the searcher path")
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64; when torch
    # is installed it must be loaded first so that this library binds to the same runtime
    # (torch tensors' device pointers are handed to lcs_batch_enqueue).
    try:
        import torch  # noqa: F401
    except Exception:  # torch is optional plumbing, not a dependency of the C ABI
        pass
    _lib = _declare(C.CDLL(LIB_PATH))
    return _lib


def load_other(path: str) -> C.CDLL:
    """Another build of liblcs_amd.so beside the in-tree one, in the same process and with the same prototypes (developer A/B runs:
    tools/bench_tdd_config.py times the parent commit's library call by call against this tree's).  Not cached; hand it to
    Searcher(device, lib=...)."""
    load()      # torch's HIP runtime first, as for the in-tree library
    return _declare(C.CDLL(os.path.abspath(path)))


def _declare(L: C.CDLL) -> C.CDLL:
    vp, dp, ip, fp = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_float)
    cp, u16p = C.POINTER(LcsCell), C.POINTER(C.c_uint16)
    L.lcs_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.lcs_destroy.argtypes = [vp]
    L.lcs_destroy.restype = None
    L.lcs_last_error.argtypes = [vp]
    L.lcs_last_error.restype = C.c_char_p
    L.lcs_version.restype = C.c_char_p
    L.lcs_cell_init.argtypes = [cp]
    L.lcs_cell_init.restype = None
    L.lcs_set_max_cells_in_flight.argtypes = [vp, C.c_int]
    if hasattr(L, "lcs_set_duplex"):      # (absent from older developer builds loaded through bench.py --lib)
        L.lcs_set_duplex.argtypes = [vp, C.c_int]
        L.lcs_get_duplex.argtypes = [vp, C.POINTER(C.c_int)]
    if hasattr(L, "lcs_set_foe_unwrap"):      # (likewise)
        L.lcs_set_foe_unwrap.argtypes = [vp, C.c_int]
        L.lcs_get_foe_unwrap.argtypes = [vp, C.POINTER(C.c_int)]
        L.lcs_pss_foe_coarse.argtypes = [vp, C.POINTER(LcsCell), C.POINTER(C.c_double), C.c_uint32, C.c_double, C.c_double, C.c_double,
                                         C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
    if hasattr(L, "lcs_set_tdd_config"):      # (likewise)
        L.lcs_set_tdd_config.argtypes = [vp, C.c_int]
        L.lcs_get_tdd_config.argtypes = [vp, C.POINTER(C.c_int)]
        L.lcs_tdd_config.argtypes = [vp, C.POINTER(LcsCell), C.POINTER(C.c_double), C.c_int, C.POINTER(TddInfo)]
        L.lcs_last_tdd_info.argtypes = [vp, C.POINTER(TddInfo), C.c_int]
    if hasattr(L, "lcs_set_cell_meas"):      # (likewise)
        L.lcs_set_cell_meas.argtypes = [vp, C.c_int]
        L.lcs_get_cell_meas.argtypes = [vp, C.POINTER(C.c_int)]
        L.lcs_cell_meas.argtypes = [vp, C.POINTER(LcsCell), C.POINTER(C.c_double), C.c_int, C.c_int, C.POINTER(CellMeas)]
        L.lcs_last_cell_meas.argtypes = [vp, C.POINTER(CellMeas), C.c_int]
        L.lcs_tdd_dl_mask.argtypes = [C.c_int]
    if hasattr(L, "lcs_cell_meas_wide"):      # (likewise)
        L.lcs_extract_tfg_wide.argtypes = [vp, C.POINTER(LcsCell), vp, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, dp, dp]
        L.lcs_cell_meas_wide.argtypes = [vp, C.POINTER(LcsCell), vp, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.POINTER(CellMeasWide)]
    if hasattr(L, "lcs_pcfich_wide"):      # (likewise)
        L.lcs_pcfich_wide.argtypes = [vp, C.POINTER(LcsCell), vp, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.POINTER(PcfichInfo)]
        L.lcs_pcfich.argtypes = [vp, C.POINTER(LcsCell), dp, C.c_int, C.c_int, C.c_int, C.POINTER(PcfichInfo)]
    if hasattr(L, "lcs_pdcch_wide"):      # (likewise)
        L.lcs_pdcch_wide.argtypes = [vp, C.POINTER(LcsCell), vp, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.POINTER(PdcchCfg), C.POINTER(PdcchInfo)]
        L.lcs_pdcch.argtypes = [vp, C.POINTER(LcsCell), dp, C.c_int, C.c_int, C.c_int, C.POINTER(PdcchCfg), C.POINTER(PdcchInfo)]
    if hasattr(L, "lcs_pdcch_scan_wide"):      # (likewise)
        L.lcs_pdcch_scan_wide.argtypes = [vp, C.POINTER(LcsCell), vp, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.POINTER(PdcchScanCfg), C.POINTER(PdcchScanInfo)]
        L.lcs_pdcch_scan.argtypes = [vp, C.POINTER(LcsCell), dp, C.c_int, C.c_int, C.c_int, C.POINTER(PdcchScanCfg), C.POINTER(PdcchScanInfo)]
        L.lcs_pdcch_scan_decodes.argtypes = [vp, C.c_int, C.POINTER(PdcchScanDec), C.c_int]
    if hasattr(L, "lcs_phich_wide"):       # (likewise)
        L.lcs_phich_wide.argtypes = [vp, C.POINTER(LcsCell), vp, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.POINTER(PhichCfg), C.POINTER(PhichInfo)]
        L.lcs_phich.argtypes = [vp, C.POINTER(LcsCell), dp, C.c_int, C.c_int, C.c_int, C.POINTER(PhichCfg), C.POINTER(PhichInfo)]
        L.lcs_phich_values.argtypes = [vp, C.c_int, dp, C.c_int]
    if hasattr(L, "lcs_pdsch_wide"):      # (likewise)
        L.lcs_pdsch_wide.argtypes = [vp, C.POINTER(LcsCell), vp, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.POINTER(PdcchCfg), C.POINTER(PdschCfg), C.POINTER(PdschInfo), C.POINTER(PdcchInfo)]
        L.lcs_pdsch.argtypes = [vp, C.POINTER(LcsCell), dp, C.c_int, C.c_int, C.c_int, C.POINTER(PdcchCfg), C.POINTER(PdschCfg), C.POINTER(PdschInfo), C.POINTER(PdcchInfo)]
        L.lcs_pdsch_last_soft.argtypes = [vp, C.c_int, C.c_int, dp, C.c_int]
        L.lcs_turbo_decode.argtypes = [vp, dp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    if hasattr(L, "lcs_pdsch_comb_wide"):      # (likewise)
        L.lcs_pdsch_comb_wide.argtypes = L.lcs_pdsch_wide.argtypes + [C.POINTER(PdschCombCfg), C.POINTER(PdschCombInfo)]
        L.lcs_pdsch_comb.argtypes = L.lcs_pdsch.argtypes + [C.POINTER(PdschCombCfg), C.POINTER(PdschCombInfo)]
    if hasattr(L, "lcs_set_pdsch_alloc"):      # (likewise)
        L.lcs_set_pdsch_alloc.argtypes = [vp, C.POINTER(PdschAllocCfg)]
        L.lcs_pdsch_last_alloc.argtypes = [vp, C.c_int, C.POINTER(PdschAlloc)]
    L.lcs_xcorr_pss.argtypes = [vp, dp, C.c_uint32, dp, C.c_uint16, C.c_uint8, C.c_double, C.c_double, C.c_double,
                                dp, ip, fp, fp, dp, fp, dp, u16p, u16p]
    L.lcs_peak_search.argtypes = [vp, dp, ip, dp, dp, C.c_uint16, C.c_double, C.c_double, fp, C.c_uint8, cp, C.c_int,
                                  C.POINTER(C.c_int)]
    L.lcs_sss_detect.argtypes = [vp, cp, dp, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_double, cp,
                                 dp, dp, dp, dp, dp, dp, dp, dp]
    L.lcs_pss_sss_foe.argtypes = [vp, cp, dp, C.c_uint32, C.c_double, C.c_double, C.c_double, cp]
    L.lcs_extract_tfg.argtypes = [vp, cp, dp, C.c_uint32, C.c_double, C.c_double, C.c_double, dp, dp, C.POINTER(C.c_int)]
    L.lcs_tfoec.argtypes = [vp, cp, dp, dp, C.c_int, C.c_double, C.c_double, dp, dp, cp]
    L.lcs_decode_mib.argtypes = [vp, cp, dp, C.c_int, cp]
    if hasattr(L, "lcs_pbch_soft"):      # (likewise)
        L.lcs_pbch_soft.argtypes = [vp, cp, dp, C.c_int, C.c_int, C.c_int, dp, dp, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
    L.lcs_chan_est.argtypes = [vp, cp, dp, C.c_int, C.c_int, dp, dp]
    L.lcs_search_capbuf.argtypes = [vp, dp, C.c_uint32, dp, C.c_uint16, C.c_double, C.c_double, C.c_double,
                                    cp, C.c_int, C.POINTER(C.c_int), cp, C.c_int, C.POINTER(C.c_int)]
    L.lcs_search_batch_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_uint32, dp, C.c_uint16, dp, dp, C.c_double,
                                       C.c_int, cp, C.c_int, C.POINTER(C.c_int)]
    L.lcs_search_batch_host.argtypes = L.lcs_search_batch_dev.argtypes
    if hasattr(L, "lcs_sic_cancel_dev"):      # (a parent commit's library loaded by load_other has none)
        sp = C.POINTER(SicInfo)
        L.lcs_sic_cancel_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_uint32, cp, ip, C.c_int, dp, dp, C.c_double, C.c_int, vp, sp]
        L.lcs_search_capbuf_sic.argtypes = [vp, dp, C.c_uint32, dp, C.c_uint16, C.c_double, C.c_double, C.c_double, cp, C.c_int, C.POINTER(C.c_int),
                                            cp, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, ip, sp]
        L.lcs_search_batch_sic_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_uint32, dp, C.c_uint16, dp, dp, C.c_double, cp, C.c_int,
                                               C.POINTER(C.c_int), C.c_int, C.c_int, ip, sp]
        L.lcs_last_sic_stats.argtypes = [vp, C.POINTER(C.c_int * 4)]
        L.lcs_sic_cancel_cfg_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_uint32, cp, ip, C.c_int, ip, dp, dp, C.c_double, C.c_int, vp, sp]
        L.lcs_last_sic_tdd_info.argtypes = [vp, C.POINTER(TddInfo), C.c_int]
        L.lcs_last_sic_cell_meas.argtypes = [vp, C.POINTER(CellMeas), C.c_int]
        L.lcs_table_pbch_symbols.argtypes = [C.c_int] * 7 + [dp]
    L.lcs_batch_readback.argtypes = [vp, C.c_int, fp, dp, ip, dp, dp]
    L.lcs_batch_enqueue.argtypes = [vp, vp, C.c_int, C.c_int, C.c_uint32, dp, C.c_uint16, dp, dp, C.c_double, C.c_int]
    L.lcs_batch_enqueue_host.argtypes = L.lcs_batch_enqueue.argtypes
    L.lcs_host_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.lcs_host_free.argtypes = [vp, vp]
    if hasattr(L, "lcs_device_alloc"):
        L.lcs_device_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
        L.lcs_device_free.argtypes = [vp, vp]
        L.lcs_device_upload.argtypes = [vp, vp, vp, C.c_size_t]
    L.lcs_device_count.argtypes = []
    L.lcs_batch_collect.argtypes = [vp, cp, C.c_int, C.POINTER(C.c_int)]
    L.lcs_foe_partial.argtypes = [vp, dp, C.c_uint32, dp, C.c_uint16, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, vp, vp]
    L.lcs_foe_finish.argtypes = [vp, vp, vp, dp, C.c_uint16, cp, ip, C.c_int, C.POINTER(C.c_int), cp, C.c_int, C.POINTER(C.c_int)]
    if hasattr(L, "lcs_foe_contend"):
        L.lcs_foe_contend.argtypes = [vp, dp, C.c_uint16, vp, vp]
        L.lcs_foe_resolve.argtypes = [vp, vp, vp]
    L.lcs_track_block.argtypes = [vp, C.POINTER(LcsTrackCell), C.c_int, C.c_int, vp, C.c_int, dp, dp, dp, C.c_double, C.c_double, C.c_double,
                                  dp, dp, dp, ip, dp, C.c_int, ip, ip, C.POINTER(C.c_uint64), C.c_int, C.POINTER(C.c_float)]
    L.lcs_track_stats.argtypes = [vp, C.c_int, C.c_int, dp, dp, C.c_int, dp, dp, C.c_int, ip]
    i64p = C.POINTER(C.c_int64)
    L.lcs_track_stream_block.argtypes = [vp, C.POINTER(LcsTrackCell), C.c_int, C.c_int, vp, dp, dp, dp, C.c_double, C.c_double, C.c_double,
                                         dp, dp, dp, C.c_int, i64p, ip, dp, dp, dp, C.c_int, ip, ip, C.POINTER(C.c_uint64), C.c_int, i64p, ip]
    L.lcs_track_stream_reset.argtypes = [vp]
    if hasattr(L, "lcs_set_batch_screen"):
        L.lcs_set_batch_screen.argtypes = [vp, C.c_int]
        L.lcs_get_batch_screen.argtypes = [vp, C.POINTER(C.c_int)]
        L.lcs_last_screen_stats.argtypes = [vp, C.POINTER(C.c_int)]
    if hasattr(L, "lcs_set_float_batch_probe"):
        L.lcs_set_float_batch_probe.argtypes = [vp, C.c_int]
    if hasattr(L, "lcs_track_cut"):
        L.lcs_track_cut.argtypes = [vp, vp, C.c_int, C.c_uint32, C.c_double, C.c_int, ip, dp, dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                    C.c_double, C.c_double, C.c_double, C.c_int, vp, dp, ip, C.POINTER(C.c_int64)]
    L.lcs_stream_open.argtypes = [vp, C.c_int, C.c_uint32, C.c_double, C.c_double, C.c_double]
    L.lcs_stream_push.argtypes = [vp, vp, C.c_double, C.POINTER(C.c_int16), C.c_int]
    L.lcs_stream_collect.argtypes = [vp, cp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float)]
    L.lcs_stream_close.argtypes = [vp]
    L.lcs_last_xcorr_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    L.lcs_last_xcorr_info.argtypes = [vp, dp, C.POINTER(C.c_char_p)]
    if hasattr(L, "lcs_last_frq_repairs"):      # (absent from older developer builds loaded through bench.py --lib)
        L.lcs_last_frq_repairs.argtypes = [vp, C.POINTER(C.c_int)]
        L.lcs_last_collect_host_us.argtypes = [vp, dp]
    if hasattr(L, "lcs_last_batch_stats"):
        L.lcs_last_batch_stats.argtypes = [vp, C.POINTER(C.c_int)]
    if hasattr(L, "lcs_last_frq_repair_stats"):
        L.lcs_last_frq_repair_stats.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.lcs_frq_tie_eps.argtypes = []
    L.lcs_frq_tie_eps.restype = C.c_double
    L.lcs_channelizer_taps.argtypes = [C.c_int, dp]
    L.lcs_channelize.argtypes = [vp, vp, C.c_int, C.c_uint64, C.c_double, C.c_int, dp, C.c_int, vp, C.c_uint32]
    L.lcs_last_channelize_ms.argtypes = [vp, fp]
    L.lcs_channelizer_proto.argtypes = [C.c_int, dp]
    L.lcs_channelize_rational.argtypes = [vp, vp, C.c_int, C.c_uint64, C.c_double, C.c_int, C.c_int, dp, C.c_int, vp, C.c_uint32]
    L.lcs_channelize_u8.argtypes = [vp, vp, C.c_int, C.c_uint64, C.c_double, C.c_int, C.c_int, dp, C.c_int, vp, C.c_uint32, vp]
    L.lcs_chan_stream_open.argtypes = [vp, C.c_int, C.c_double, C.c_int, C.c_int, dp, C.c_int]
    L.lcs_chan_stream_count.argtypes = [vp, C.c_uint64, C.POINTER(C.c_uint32)]
    L.lcs_chan_stream_push.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.lcs_chan_stream_close.argtypes = [vp]
    L.lcs_chan_stream_open_u8.argtypes = [vp, C.c_int, C.c_double, C.c_int, C.c_int, dp, C.c_int, C.c_uint32]
    L.lcs_chan_stream_count_u8.argtypes = [vp, C.c_uint64, C.POINTER(C.c_uint32)]
    L.lcs_chan_stream_push_u8.argtypes = [vp, vp, C.c_uint64, vp, vp, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.lcs_stream.argtypes = [vp]
    L.lcs_stream.restype = vp
    L.lcs_sync.argtypes = [vp]
    L.lcs_table_pss_td.argtypes = [C.c_int, dp]
    L.lcs_table_pss_fd.argtypes = [C.c_int, dp]
    L.lcs_table_sss_fd.argtypes = [C.c_int, C.c_int, C.c_int, ip]
    L.lcs_table_lte_pn.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8)]
    L.lcs_chi2cdf_inv.argtypes = [C.c_double, C.c_double]
    L.lcs_chi2cdf_inv.restype = C.c_double
    return L
