"""GPU tests of the cancellation kernels (csrc/sic.hip) at their geometric edges: every case of tests/sic_edge_cases.py through
Searcher.sic_cancel against sic_ref.cancel on the values the device gets -- the reference is sic_ref, never the device.

The cases are hand-made records on noise captures (no search): both CP types, every id mod 6, 1 / 2 / 4 ports, FDD and TDD, both sides
of the frame-origin branch, the sfn wrap, frames before the record's, steps of 1 +- 3e-4, captures that end with a window or start with
a symbol, 9600 and 268800 samples, single-bit masks, lists with a refused record, batches with per-buffer carriers, u8.

The bound is the project's RESIDUAL_TOL (tests/test_gpu_sic.py: 1.281e-6 of the capture's rms), not a new number.  It is derivable
too: the table td and the residual are complex64, so per sample |err| <= 2^-24 (sum_c |y_c| + |res|) plus fp64 noise, and under the
table's condition (max |capture|, max |y_c| <= 5 rms, at most two cells) that is at most 2^-24 * 15 rms = 9e-7 rms.

Measured on the first run (MI355X), worst max |device - sic_ref| / rms per group:
  identity 1.929e-7 (id503_p2_ext_fdd), origin 1.329e-7, rates 1.336e-7, ends 1.262e-7, masks 1.366e-7, lists 1.275e-7;
  the extended-CP S + W capture: 1.354e-7 -- the 1.281e-7 of the normal-CP pair, a seventh of the bound, at every geometry."""
import numpy as np
import pytest

import sic_cases as K
import sic_edge_cases as E
import sic_ref as R
from conftest import load_pkg
from test_gpu_sic import RESIDUAL_TOL, assert_info_close

pytestmark = pytest.mark.gpu

WORST = {}                     # group -> (ratio, case)
RERUN = ("id503_p4_ext_tdd", "rate_norm_minus", "batch_2_0_1")


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def ctx(pkg):
    """{duplex: context}: one FDD and one TDD context for the whole file"""
    fdd, tdd = pkg.Searcher(0), pkg.Searcher(0)
    tdd.set_duplex(pkg.DUPLEX_TDD)
    yield {R.FDD: fdd, R.TDD: tdd}
    fdd.close()
    tdd.close()


def launch(pkg, ctx, c, as_c64=False, fs=None):
    """-> (the captures on the device [n_buf][...], the residual [n_buf][n_cap] complex64 on the device, info [n_buf][cells])"""
    import torch
    n_buf = len(c["bufs"])
    if c["u8"] and not as_c64:
        host, fmt = np.stack([E.capture(c, b) for b in range(n_buf)]), pkg.FMT_IQ_U8
    else:
        host, fmt = np.stack([E.seen(c, b).astype(np.complex64) for b in range(n_buf)]), pkg.FMT_C64      # (u8 - 127) / 128 is exact in complex64
    d = torch.from_numpy(np.ascontiguousarray(host)).to("cuda:0")
    res = torch.full((n_buf, c["n_cap"]), float("nan"), dtype=torch.complex64, device="cuda:0")           # a sample nobody writes stays NaN
    cells = [[E.cell_of(s) for s in buf["cells"]] for buf in c["bufs"]]
    cfg = None
    if any(buf["configs"] is not None for buf in c["bufs"]):
        cfg = [[pkg.TDD_NOT_ESTIMATED if v is None else v for v in (buf["configs"] or [None] * len(buf["cells"]))] for buf in c["bufs"]]
    info = ctx[c["duplex"]].sic_cancel(d.data_ptr(), fmt, n_buf, c["n_cap"], cells, [buf["fc"][0] for buf in c["bufs"]], [buf["fc"][1] for buf in c["bufs"]],
                                       c["fs"] if fs is None else fs, res.data_ptr(), c["mask"], ul_dl_config=cfg)
    torch.cuda.synchronize()
    return d, res, info


def compare(pkg, c, res, info):
    """the residual and the records of every buffer against reference(c) -> the case's worst max |device - sic_ref| / rms"""
    ref = E.reference(c)
    worst = 0.0
    for b, buf in enumerate(c["bufs"]):
        got = res[b].cpu().numpy().astype(np.complex128)
        assert np.isfinite(got).all()
        worst = max(worst, float(np.abs(got - ref[b]["res"]).max() / ref[b]["rms"]))
        assert len(info[b]) == len(buf["cells"])
        for i, spec in enumerate(buf["cells"]):
            got_i, ref_i = info[b][i], ref[b]["info"][i]
            if spec["refused"]:
                assert got_i.n_sym == 0 and got_i.n_pss == 0 and not got_i.cancelled and got_i.ul_dl_config == pkg.TDD_NOT_ESTIMATED
                continue
            assert got_i.cancelled and got_i.n_pss == ref_i["n_pss"]
            assert_info_close(got_i, ref_i)
            for comp in range(4):
                if not (c["mask"] >> comp) & 1:
                    assert got_i.power[comp] == 0.0                      # exactly
            config = None if buf["configs"] is None else buf["configs"][i]
            known = c["duplex"] == R.TDD and config is not None and 0 <= config <= 6
            assert got_i.ul_dl_config == (config if known else pkg.TDD_NOT_ESTIMATED)
    return worst


@pytest.mark.parametrize("name", [c["name"] for c in E.CASES])
def test_case_against_sic_ref(pkg, ctx, name):
    c = E.BY_NAME[name]
    d, res, info = launch(pkg, ctx, c)
    worst = compare(pkg, c, res, info)
    print("%s: max |device - sic_ref| / rms = %.3e" % (name, worst))
    if worst > WORST.get(c["group"], (0.0, ""))[0]:
        WORST[c["group"]] = (worst, name)
    assert worst < RESIDUAL_TOL


def test_worst_ratio_per_group():
    """after the cases above (file order): what the docstring of this file and DESIGN.md record"""
    for group in E.GROUPS:
        print("group %-8s worst max |device - sic_ref| / rms = %.3e (%s)" % ((group,) + WORST.get(group, (float("nan"), "not run"))))
    assert all(WORST[g][0] < RESIDUAL_TOL for g in WORST)


def test_exact_zeros_and_untouched_buffer(pkg, ctx):
    import torch
    for tag in ("norm", "ext"):
        _, _, info = launch(pkg, ctx, E.BY_NAME["short_%s_no_sss" % tag])
        got = info[0][0]
        assert got.gain == 0 and got.power[0] == 0.0 and got.power[1] == 0.0 and got.n_pss == 1 and got.power[2] > 0 and got.cancelled
    d, res, info = launch(pkg, ctx, E.BY_NAME["batch_2_0_1"])
    assert info[1] == [] and torch.equal(res[1], d[1])                   # the cell-less buffer: its capture, bit for bit
    assert not torch.equal(res[0], d[0]) and not torch.equal(res[2], d[2])


def test_u8_route_equals_complex64_route(pkg, ctx):
    import torch
    c = E.BY_NAME["list_two_cells_u8"]
    _, res8, info8 = launch(pkg, ctx, c)
    _, res64, info64 = launch(pkg, ctx, c, as_c64=True)
    assert torch.equal(res8, res64) and [bytes(i) for i in info8[0]] == [bytes(i) for i in info64[0]]
    assert compare(pkg, c, res64, info64) < RESIDUAL_TOL


@pytest.mark.parametrize("name", RERUN)
def test_second_run_is_bit_equal(pkg, ctx, name):
    import torch
    c = E.BY_NAME[name]
    _, first, info1 = launch(pkg, ctx, c)
    _, second, info2 = launch(pkg, ctx, c)
    assert torch.equal(first, second) and [[bytes(i) for i in b] for b in info1] == [[bytes(i) for i in b] for b in info2]


def test_refusal_of_more_than_16_frames(pkg, ctx):
    """at 1.0 Msps a 268800-sample capture spans 27 frames of a cell: LCS_ERR_BAD_ARG, and the context is none the worse for it"""
    import torch
    before = E.BY_NAME["list_two_cells"]
    _, res0, info0 = launch(pkg, ctx, before)
    with pytest.raises(pkg.SearcherError, match="LCS_ERR_BAD_ARG.*more than 16 frames"):
        launch(pkg, ctx, E.BY_NAME["long_norm_15_frames"], fs=1.0e6)
    _, res1, info1 = launch(pkg, ctx, before)
    assert torch.equal(res0, res1) and [bytes(i) for i in info0[0]] == [bytes(i) for i in info1[0]]


def test_extended_cp_pair(pkg, ctx):
    """the extended-CP twin of test_gpu_sic.py's pair tests, the one new test that runs a search: S + W of sic_cases.ext_pair()"""
    import torch
    x = K.ext_pair()
    S = ctx[R.FDD]
    cells, rounds, info = S.search_capbuf_sic(x, K.F_SET, K.FC, K.FC, K.FS)
    assert [c.n_id_cell() for c in cells] == [K.ID_S, K.ID_W] and rounds == [0, 1] and all(c.cp_type == 2 for c in cells)
    d = torch.from_numpy(np.ascontiguousarray(x.astype(np.complex64))).to("cuda:0")
    res = torch.full((x.size,), float("nan"), dtype=torch.complex64, device="cuda:0")
    got_info = S.sic_cancel(d.data_ptr(), pkg.FMT_C64, 1, x.size, [cells[:1]], K.FC, K.FC, K.FS, res.data_ptr())[0]
    torch.cuda.synchronize()
    seen = d.cpu().numpy().astype(np.complex128)
    want, ref = R.cancel(seen, cells[:1], K.FC, K.FC, K.FS)
    err = np.abs(res.cpu().numpy().astype(np.complex128) - want).max() / np.sqrt(np.mean(np.abs(seen) ** 2))
    print("residual, extended-CP S + W: max |device - sic_ref| / rms = %.3e" % err)
    assert err < RESIDUAL_TOL
    assert_info_close(got_info[0], ref[0])
    assert got_info[0].n_sym == 959 and got_info[0].n_pss == ref[0]["n_pss"]
