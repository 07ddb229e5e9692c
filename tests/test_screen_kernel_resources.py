"""The instantiations of k_xcorr_i8x3 in the SHIPPED library (tools/code_objects.py reads the code objects' own metadata): the
three-digit grid form, the two-digit screen and the three-digit list form all keep the co-residency rules of DESIGN 3.3 -- 256
threads, at most 232 registers (two workgroups per CU leave 48 per SIMD lane to the collapse), no more LDS than the 77312 bytes the
kernel had before the screen, no spill, no scratch."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_BEFORE_THE_SCREEN = 77312


def test_every_form_of_the_int8_kernel_keeps_the_co_residency_rules():
    spec = importlib.util.spec_from_file_location("code_objects", os.path.join(ROOT, "tools", "code_objects.py"))
    co = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(co)
    lib = os.path.join(ROOT, "lte-cell-scanner_amd", "liblcs_amd.so")
    if not os.path.exists(lib):
        pytest.skip("library not built")
    ks = {k: v for k, v in co.kernels_of(lib).items() if "k_xcorr_i8x3" in k}
    forms = {"ILi3ELb0EE": "three digits, grid", "ILi2ELb0EE": "two digits, grid (the screen)", "ILi3ELb1EE": "three digits, list"}
    for tag, what in forms.items():
        hit = [v for k, v in ks.items() if tag in k]
        assert len(hit) == 1, (what, sorted(ks))
        v = hit[0]
        assert v["vgpr_count"] + v["agpr_count"] <= 232, (what, v)
        assert v["group_segment_fixed_size"] <= LDS_BEFORE_THE_SCREEN, (what, v)
        assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (what, v)
    assert len(ks) == len(forms), sorted(ks)
    screen = next(v for k, v in ks.items() if "ILi2ELb0EE" in k)
    exact = next(v for k, v in ks.items() if "ILi3ELb0EE" in k)
    assert screen["vgpr_count"] <= exact["vgpr_count"] - 48          # the second accumulator set and its float copies are gone
