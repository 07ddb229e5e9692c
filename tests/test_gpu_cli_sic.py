"""host/CellSearch --sic N: the search with cancellation rounds from the command line, on the S + W capture of tests/sic_cases.py
recorded as dongle bytes in a capbuf_0000.it file."""
import os
import re
import subprocess

import numpy as np
import pytest

import sic_cases as K
from conftest import ROOT, load_pkg

EXE = os.path.join(ROOT, "host", "CellSearch")
HEADER = "CID A      fc   foff RXPWR C nRB P  PR CrystalCorrectionFactor"


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "host"), "-s"])


def _run(args):
    return subprocess.run([EXE] + args, capture_output=True, text=True, timeout=120)


def test_sic_option_is_checked():
    assert "cancellation rounds must be 1..4" in _run(["-s", "739e6", "-l", "--sic", "5"]).stderr
    assert "cancellation rounds must be 1..4" in _run(["-s", "739e6", "-l", "--sic", "0"]).stderr
    assert "-S --sic N" in _run(["-h"]).stdout


@pytest.mark.gpu
def test_sic_lists_the_hidden_cell(tmp_path):
    load_pkg()
    it = __import__("importlib").import_module("lte_cell_scanner_amd.itfile")
    x, _ = K.pair_u8()
    it.write_it(str(tmp_path / "capbuf_0000.it"), {"capbuf": x, "fc": np.array([int(K.FC)], np.int32)})
    args = ["-s", str(int(K.FC)), "-p", "5", "-l", "-d", str(tmp_path)]      # 5 ppm of 739 MHz: the hypotheses -5, 0, 5 kHz
    plain = _run(args)
    assert plain.returncode == 0, plain.stderr
    rows = [l for l in plain.stdout.splitlines() if re.match(r"^ *\d+ +\d ", l)]
    assert len(rows) == 1 and rows[0].startswith(" 31 2 ") and HEADER + "\n" in plain.stdout and "cancellation round" not in plain.stdout
    sic = _run(args + ["--sic", "2"])
    assert sic.returncode == 0, sic.stderr
    assert HEADER + " R\n" in sic.stdout
    rows2 = [l for l in sic.stdout.splitlines() if re.match(r"^ *\d+ +\d ", l)]
    assert len(rows2) == 2 and rows2[1].startswith("232 2 ") and rows2[1].endswith(" 1")
    # round 0's row is the plain row (the plain run takes the batched byte route, --sic the single-buffer one: the 20-digit
    # correction factor may differ in its last digits between the two) plus the round
    a, b = rows[0].split(), rows2[0].split()
    assert b[-1] == "0" and a[:-1] == b[:-2] and abs(float(a[-1]) - float(b[-2])) < 1e-9
    assert "cell ID: 232" in sic.stdout and "cell ID: 232" not in plain.stdout
    # one round is the plain search with the extra column
    one = _run(args + ["-S", "1"])
    assert [l for l in one.stdout.splitlines() if re.match(r"^ *\d+ +\d ", l)] == [rows2[0]]
