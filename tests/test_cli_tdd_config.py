"""host/CellSearch -x tdd --tdd-config: the uplink-downlink configuration and the DwPTS class as two more columns of the report,
on a recorded .it capture of two planted TDD cells (tests/tdd_config_cases.py, buffer 2: configuration 2 with a DwPTS of 10
symbols, and configuration 3 with the extended CP and a DwPTS of 10); without the flag the report is what it was."""
import os
import subprocess

import numpy as np
import pytest

import tdd_config_cases as K
from conftest import ROOT, load_pkg

EXE = os.path.join(ROOT, "host", "CellSearch")


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])


def test_help_lists_the_option():
    h = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "-T --tdd-config" in h and "-x --duplex fdd|tdd" in h


@pytest.mark.gpu
def test_report_gains_two_columns_and_is_unchanged_without_the_flag(tmp_path):
    pkg = load_pkg()
    pkg.itfile.write_it(str(tmp_path / "capbuf_0000.it"), {"capbuf": K.cap(2), "fc": np.array([int(K.FC)], np.int32)})
    base = [EXE, "-s", str(int(K.FC)), "-p", "2", "-x", "tdd", "-l", "-d", str(tmp_path)]
    plain = subprocess.run(base, capture_output=True, text=True, timeout=600)
    flagged = subprocess.run(base + ["--tdd-config"], capture_output=True, text=True, timeout=600)
    short = subprocess.run(base + ["-T"], capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0 and flagged.returncode == 0, (plain.stderr, flagged.stderr)
    assert short.stdout == flagged.stdout
    assert "UD" not in plain.stdout and "DwPTS" not in plain.stdout
    a, b = plain.stdout.splitlines(), flagged.stdout.splitlines()
    head = a.index("CID A      fc   foff RXPWR C nRB P  PR CrystalCorrectionFactor")
    legend = "UD: uplink-downlink configuration ; DW: DwPTS class (port-0 reference rows in the special subframe)"
    assert b[:head] == a[:head] and b[head] == legend and b[head + 1] == a[head] + " UD DW"
    rows_a, rows_b = a[head + 1:], b[head + 2:]
    assert len(rows_a) == len(rows_b) >= 2
    got = {}
    for ra, rb in zip(rows_a, rows_b):
        assert rb.startswith(ra) and len(rb) == len(ra) + 6, (ra, rb)
        got[int(ra.split()[0])] = tuple(rb[len(ra):].split())
    want = {n_id: (str(cfg), str(rows)) for n_id, (cfg, rows, _) in K.planted(2).items()}
    assert {k: got.get(k) for k in want} == want, got
    # in FDD the flag is accepted and estimates nothing
    fdd = subprocess.run([EXE, "-s", str(int(K.FC)), "-p", "2", "-l", "-d", str(tmp_path), "--tdd-config"], capture_output=True, text=True, timeout=600)
    assert fdd.returncode == 0 and all(line.endswith("  -  -") for line in fdd.stdout.splitlines() if line[:3].strip().isdigit() and "M " in line)
