"""CPU: fl_gemm_w8a8 refuses a foreign argument struct and unsupported shapes before it touches the device (no launch, no GPU needed)."""
import ctypes

import pytest


def args(**kw):
    from fluent_mi355.gemm import FlGemmW8A8Args
    a = FlGemmW8A8Args()
    a.struct_bytes = ctypes.sizeof(FlGemmW8A8Args)
    a.M, a.N, a.K, a.lda, a.ldb, a.ldc, a.sa_stride, a.sb_stride = 4, 32, 64, 64, 64, 32, 1, 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw, word", [(dict(struct_bytes=8), "struct_bytes"), (dict(K=24), "K = 24"), (dict(N=40), "N = 40"),
                                      (dict(elem_type=2), "elem_type"), (dict(tile_rows=64), "tile_rows"), (dict(lda=72), "lda"),
                                      (dict(sa_stride=2), "scale strides"), (dict(), "null pointer")])
def test_fl_gemm_w8a8_refuses_before_any_launch(kw, word):
    from fluent_mi355._lib import lib
    a = args(**kw)
    assert lib.fl_gemm_w8a8(ctypes.byref(a), None) == 1 and word in lib.fl_last_error().decode()


def test_empty_batch_is_ok_and_quantisers_refuse_ragged_rows():
    from fluent_mi355._lib import lib
    a = args(M=0)
    assert lib.fl_gemm_w8a8(ctypes.byref(a), None) == 0
    assert lib.fl_quant_per_token_fp8(None, 2, 12, None, None, None) == 1 and "K=12" in lib.fl_last_error().decode()
    assert lib.fl_quant_per_token_group_int8(None, 2, 256, 96, 1e-10, None, None, None) == 1
    assert lib.fl_quant_per_tensor_fp8(None, 12, None, None, 0, None) == 1
