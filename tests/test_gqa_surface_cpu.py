"""CPU: the names srt/layers/attention/flashinfer_backend.py takes from `flashinfer` resolve in the shim, the host helpers of
`flashinfer.decode` return what flashinfer's do, and the C entry of the paged GQA kernel refuses a struct of another layout."""
import ctypes
import importlib

import pytest
import torch

NAMES = [("flashinfer", "BatchDecodeWithPagedKVCacheWrapper"), ("flashinfer", "BatchPrefillWithPagedKVCacheWrapper"),
         ("flashinfer", "run_device_plan_prefill_graph"), ("flashinfer.cascade", "merge_state"), ("flashinfer.decode", "_get_range_buf"),
         ("flashinfer.decode", "get_seq_lens"), ("flashinfer.decode", "_grouped_size_compiled_for_decode_kernels")]


@pytest.mark.parametrize("module,name", NAMES)
def test_name_resolves_in_the_shim(module, name):
    mod = importlib.import_module(module)
    assert "sglang-fluentllm_amd" in mod.__file__ and callable(getattr(mod, name))


def test_decode_host_helpers():
    from flashinfer import run_device_plan_prefill_graph
    from flashinfer.decode import _get_range_buf, _grouped_size_compiled_for_decode_kernels, get_seq_lens

    r = _get_range_buf(5, "cpu")
    assert r.dtype == torch.int32 and r.tolist() == [0, 1, 2, 3, 4]
    indptr, last = torch.tensor([0, 3, 3, 4], dtype=torch.int32), torch.tensor([2, 0, 16], dtype=torch.int32)
    assert get_seq_lens(indptr, last, 16).tolist() == [34, 0, 16]
    assert [_grouped_size_compiled_for_decode_kernels(h, 8) for h in (8, 16, 24, 32, 64, 128)] == [True, True, False, True, True, False]
    with pytest.raises(RuntimeError, match="plan record"):
        run_device_plan_prefill_graph(None, None, None, None, 1, 8, 4)


def test_c_entry_refuses_another_struct_layout_and_zeroed_sizes():
    from fluent_mi355 import lib
    from fluent_mi355.prefill import FlGqaPagedArgs

    a = FlGqaPagedArgs()
    a.struct_bytes = ctypes.sizeof(FlGqaPagedArgs) - 8
    assert lib.fl_gqa_paged_attention_bf16(ctypes.byref(a), None) == 1 and b"struct_bytes" in lib.fl_last_error()
    a.struct_bytes = ctypes.sizeof(FlGqaPagedArgs)
    assert lib.fl_gqa_paged_attention_bf16(ctypes.byref(a), None) == 1 and b"struct_bytes" not in lib.fl_last_error()
