"""host/CellSearch --meas: RSRP, RSRQ and the SINR on the reference signals as three more columns of the report, on a recorded .it
capture of two planted cells (tests/cell_meas_cases.py, buffer 4); the columns follow UD DW with -x tdd --tdd-config
(tests/tdd_config_cases.py, buffer 2); without the flag the report is what it was."""
import os
import subprocess

import numpy as np
import pytest

import cell_meas_cases as CS
import tdd_config_cases as K
from conftest import ROOT, load_pkg

EXE = os.path.join(ROOT, "host", "CellSearch")
HEAD = "CID A      fc   foff RXPWR C nRB P  PR CrystalCorrectionFactor"
LEGEND = "RSRP: power per reference resource element of port 0, dB re full scale ; RSRQ: 6 RSRP / RSSI, dB ; SINR: RSRP / noise on port 0's reference signals, dB"
FS = 1.92e6


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])


def test_help_lists_the_option():
    h = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "-M --meas" in h and "-T --tdd-config" in h


def _rows(plain, flagged, extra_head, width):
    """the table rows of the two reports as {n_id_cell: the appended columns}, after checking that everything else is identical"""
    a, b = plain.splitlines(), flagged.splitlines()
    head = next(i for i, l in enumerate(a) if l.startswith(HEAD))
    assert b[:head] == a[:head] and b[head] == LEGEND and b[head + 1] == a[head] + extra_head
    rows_a, rows_b = a[head + 1:], b[head + 2:]
    assert len(rows_a) == len(rows_b) >= 2
    got = {}
    for ra, rb in zip(rows_a, rows_b):
        assert rb.startswith(ra) and len(rb) == len(ra) + width, (ra, rb)
        got[int(ra.split()[0])] = rb[len(ra):].split()
    return got


def _check_values(pkg, got, cells, info):
    assert set(got) == {c.n_id_cell() for c in cells}
    for c, m in zip(cells, info):
        assert m.status == 0
        want = (m.rsrp_db[0], m.rsrq_db, m.sinr_db[0])
        cols = [float(v) for v in got[c.n_id_cell()]]
        print(c.n_id_cell(), cols, want)
        # within 0.05 dB: what printing to one decimal leaves of the same record (1e-9: a decimal is no binary fraction)
        assert all(abs(x - w) <= 0.05 + 1e-9 for x, w in zip(cols, want)), (cols, want)


@pytest.mark.gpu
def test_report_gains_three_columns_and_is_unchanged_without_the_flag(tmp_path):
    pkg = load_pkg()
    pkg.itfile.write_it(str(tmp_path / "capbuf_0000.it"), {"capbuf": CS.cap(4), "fc": np.array([int(CS.FC)], np.int32)})
    base = [EXE, "-s", str(int(CS.FC)), "-p", "2", "-l", "-d", str(tmp_path)]
    plain = subprocess.run(base, capture_output=True, text=True, timeout=600)
    flagged = subprocess.run(base + ["--meas"], capture_output=True, text=True, timeout=600)
    short = subprocess.run(base + ["-M"], capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0 and flagged.returncode == 0, (plain.stderr, flagged.stderr)
    assert short.stdout == flagged.stdout
    assert "RSRP" not in plain.stdout and "SINR" not in plain.stdout
    got = _rows(plain.stdout, flagged.stdout, "  RSRP  RSRQ  SINR", 18)
    with pkg.Searcher(0) as s:
        s.set_cell_meas(True)
        cells, _ = s.search_capbuf(CS.cap(4), pkg.f_search_set_for(CS.FC, 2), CS.FC, CS.FC, FS)
        _check_values(pkg, got, cells, s.last_cell_meas(1, 16)[0])
    assert set(got) == {233, 9}


@pytest.mark.gpu
def test_columns_follow_the_tdd_columns(tmp_path):
    pkg = load_pkg()
    pkg.itfile.write_it(str(tmp_path / "capbuf_0000.it"), {"capbuf": K.cap(2), "fc": np.array([int(K.FC)], np.int32)})
    base = [EXE, "-s", str(int(K.FC)), "-p", "2", "-x", "tdd", "--tdd-config", "-l", "-d", str(tmp_path)]
    plain = subprocess.run(base, capture_output=True, text=True, timeout=600)
    flagged = subprocess.run(base + ["--meas"], capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0 and flagged.returncode == 0, (plain.stderr, flagged.stderr)
    got = _rows(plain.stdout, flagged.stdout, "  RSRP  RSRQ  SINR", 18)
    with pkg.Searcher(0) as s:
        s.set_duplex(pkg.DUPLEX_TDD), s.set_tdd_config(True), s.set_cell_meas(True)
        cells, _ = s.search_capbuf(K.cap(2), pkg.f_search_set_for(K.FC, 2, 2.5e3), K.FC, K.FC, FS)
        info = s.last_cell_meas(1, 16)[0]
        _check_values(pkg, got, cells, info)
        assert {c.n_id_cell(): m.dl_mask for c, m in zip(cells, info)} == {n: pkg.tdd_dl_mask(cfg) for n, (cfg, _, _) in K.planted(2).items()}
