"""CPU: `from eps.executor import AokGroupedGemm` (moe/gemms/bf16/aok.py:3) resolves in the shim; its C-ABI entry checks the struct's size first."""
import ctypes
import importlib
import json
import os
import sys

from conftest import PKG, ROOT


def test_aok_grouped_gemm_resolves_with_the_shim_first():
    records = json.load(open(os.path.join(ROOT, "tests", "golden", "import_surface.json")))["records"]
    hits = [r for r in records if (r["module"], r["name"]) == ("eps.executor", "AokGroupedGemm")]
    assert hits and hits[0]["file"] == "srt/layers/moe/gemms/bf16/aok.py" and hits[0]["level"] == "module"   # the fixture really records it
    sys.path.insert(0, PKG)
    try:
        mod = importlib.import_module("eps.executor")
    finally:
        sys.path.remove(PKG)
    assert os.path.dirname(os.path.dirname(mod.__file__)) == PKG
    assert callable(mod.silu) and callable(mod.AokGroupedGemm(4).run) and mod.AokGroupedGemm(4).num_local_experts == 4


def test_struct_size_is_checked_before_anything_is_launched():
    from fluent_mi355.gemm import FlGemmBf16Args, lib
    a = FlGemmBf16Args()
    a.struct_bytes = ctypes.sizeof(FlGemmBf16Args) - 8
    assert lib.fl_grouped_gemm_bf16(ctypes.byref(a), None) == 1 and b"struct_bytes" in lib.fl_last_error()   # FL_ERR_INVALID
    a.struct_bytes = ctypes.sizeof(FlGemmBf16Args)
    assert lib.fl_grouped_gemm_bf16(ctypes.byref(a), None) != 0 and b"struct_bytes" not in lib.fl_last_error()   # accepted size: refused for its zeroed sizes
    a.num_groups, a.N, a.K = 1, 64, 96
    assert lib.fl_grouped_gemm_bf16(ctypes.byref(a), None) == 3 and b"multiple of 64" in lib.fl_last_error()
