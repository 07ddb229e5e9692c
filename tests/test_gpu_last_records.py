"""GPU test of the read-back that lcs_last_tdd_info and lcs_last_cell_meas share: the side tables of a fused call, compacted per
buffer in peak order into the caller's array.

On the two-mode TDD synthetic batch of tests/tdd_config_cases.py: refused before any fused call, entry k beside cell k when the
array holds every cell, LCS_ERR_OVERFLOW with the entries that fit when it does not, and the cleared record throughout after a
batch with the mode off."""
import ctypes as C
import struct

import numpy as np
import pytest

import tdd_config_cases as K
from conftest import load_pkg

pytestmark = pytest.mark.gpu
FS = K.FS
MAXC = 16
OK, BAD_ARG, OVERFLOW = 0, -2, -4
# the cleared records (tdd_info_clear, meas_clear with the sentinel -2): the integers -2, every double 0
CLEARED = {"lcs_last_tdd_info": struct.pack("<2i15d", -2, -2, *([0.0] * 15)), "lcs_last_cell_meas": struct.pack("<4i14d", -2, -2, -2, -2, *([0.0] * 14))}


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def _batch(pkg, s):
    import torch
    n = len(K.BUFFERS)
    d = torch.from_numpy(np.stack([K.u8(b) for b in range(n)])).cuda()
    cells = s.search_batch(d.data_ptr(), pkg.FMT_IQ_U8, n, 153600, K.GRID, K.FC, K.FC, FS, pkg.STAGE_FULL, MAXC)
    del d
    return cells


def _read(pkg, s, name, n_buf, per_buf):
    """-> (return code, the last error, [n_buf][per_buf] records as bytes)"""
    rec = pkg.capi.TddInfo if name == "lcs_last_tdd_info" else pkg.capi.CellMeas
    info = (rec * max(1, n_buf * per_buf))()
    rc = getattr(s._lib, name)(s._h, info, per_buf)
    return rc, s._lib.lcs_last_error(s._h).decode(), [[bytes(info[b * per_buf + k]) for k in range(per_buf)] for b in range(n_buf)]


@pytest.mark.parametrize("name", ["lcs_last_tdd_info", "lcs_last_cell_meas"])
def test_last_records_fit_overflow_and_mode_off(pkg, name):
    n = len(K.BUFFERS)
    with pkg.Searcher(0) as s:
        s.set_duplex(pkg.DUPLEX_TDD), s.set_tdd_config(True), s.set_cell_meas(True)
        rc, err, _ = _read(pkg, s, name, n, MAXC)
        assert rc == BAD_ARG and err == name + " needs lcs_search_capbuf or a batch on this context first"

        cells = _batch(pkg, s)
        rc, _, full = _read(pkg, s, name, n, MAXC)
        assert rc == OK
        want = s.last_tdd_info(n, MAXC) if name == "lcs_last_tdd_info" else s.last_cell_meas(n, MAXC)
        two = [b for b in range(n) if len(cells[b]) >= 2]
        assert two and all(1 <= len(cells[b]) <= MAXC for b in range(n)), [len(c) for c in cells]
        for b in range(n):
            planted = K.planted(b)
            for k, c in enumerate(cells[b]):      # entry k belongs to cell k: it is a record, and a planted cell's names its configuration
                assert full[b][k] != CLEARED[name] and full[b][k] == bytes(want[b][k])
                if c.n_id_cell() in planted:
                    cfg = planted[c.n_id_cell()][0]
                    if name == "lcs_last_tdd_info":
                        assert want[b][k].ul_dl_config == cfg, (b, k)
                    else:
                        assert want[b][k].status == 0 and want[b][k].dl_mask == pkg.tdd_dl_mask(cfg), (b, k)
            assert all(r == CLEARED[name] for r in full[b][len(cells[b]):]), b

        rc, err, one = _read(pkg, s, name, n, 1)
        assert rc == OVERFLOW and err == "more results than the output array holds"
        assert [row[0] for row in one] == [row[0] for row in full]

        s.set_tdd_config(False), s.set_cell_meas(False)
        assert [[bytes(c) for c in row] for row in _batch(pkg, s)] == [[bytes(c) for c in row] for row in cells]
        rc, _, off = _read(pkg, s, name, n, MAXC)
        assert rc == OK and all(r == CLEARED[name] for row in off for r in row)
