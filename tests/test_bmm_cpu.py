"""CPU: the host side of csrc/bmm_bf16.hip — the split-K picker behind `fl_gemm_bf16_nt_splitk_workspace_bytes` over a grid of shapes
(its four invariants, the shapes it refuses, and the splits tests/test_bmm_dispatch_gpu.py builds its cases on), and the argument
checks of `fl_bmm_bf16_nt` / `fl_gemm_bf16_nt_splitk`, which come before anything is dereferenced or launched.  No call here passes
its checks with M > 0: it would launch."""
import ctypes
import itertools

import pytest

MS = (1, 33, 64, 65, 256, 1000, 5000)
NS = (64, 128, 192, 256, 512, 768)
KS = (64, 192, 448, 576, 1024, 1536, 4096, 6144, 7168, 8192)
# (M, N, K) -> ksplit: r1 .. r7 of tests/test_bmm_dispatch_gpu.py, then the router shape of tests/test_bmm_gpu.py at its four T.
# A retuned picker fails here first: the GPU cases were chosen for these splits and must then be chosen again.
PINNED = {(5, 64, 64): 1, (5, 64, 192): 3, (200, 192, 448): 7, (65, 64, 7168): 112, (1, 64, 8192): 128, (3, 768, 6144): 24,
          (130, 512, 6144): 12, (1, 256, 7168): 56, (33, 256, 7168): 56, (256, 256, 7168): 14, (1000, 256, 7168): 14}


@pytest.fixture(scope="module")
def lib():
    from fluent_mi355 import bmm  # noqa: F401  (declares the argument types of the three entry points)
    from fluent_mi355._lib import lib as lib_
    return lib_


@pytest.fixture(scope="module")
def host_ptr():
    """the address of a 64-byte-aligned host buffer (never dereferenced: every call below is refused by its argument checks)"""
    raw = ctypes.create_string_buffer(4096 + 64)
    addr = (ctypes.addressof(raw) + 63) & ~63
    assert addr % 64 == 0
    yield addr
    del raw


def test_splitk_workspace_bytes_invariants_over_the_grid(lib):
    for M, N, K in itertools.product(MS, NS, KS):
        nbytes = int(lib.fl_gemm_bf16_nt_splitk_workspace_bytes(M, N, K))
        assert nbytes > 0 and nbytes % (4 * M * N) == 0, (M, N, K, nbytes)
        ks = nbytes // (4 * M * N)
        assert K % ks == 0, (M, N, K, ks)
        kc = K // ks
        assert kc % 64 == 0 and kc * 256 <= 131072, (M, N, K, ks)      # 128-byte slab rows; both 64-row slabs within 128 KiB of LDS


def test_splitk_workspace_bytes_is_zero_for_shapes_the_form_does_not_serve(lib):
    f = lib.fl_gemm_bf16_nt_splitk_workspace_bytes
    for M, N, K in ((33, 96, 7168), (33, 32, 7168), (33, 2112 + 32, 7168), (33, 256, 7168 + 32), (33, 256, 48), (33, 256, 16),
                    (0, 256, 7168), (-1, 256, 7168), (33, 0, 7168), (33, -64, 7168), (33, 256, 0), (33, 256, -64)):
        assert int(f(M, N, K)) == 0, (M, N, K)


@pytest.mark.parametrize("shape,ks", sorted(PINNED.items()))
def test_splitk_pick_of_the_gpu_cases_is_pinned(lib, shape, ks):
    M, N, K = shape
    assert int(lib.fl_gemm_bf16_nt_splitk_workspace_bytes(M, N, K)) == ks * 4 * M * N


def test_fl_bmm_bf16_nt_refuses_before_any_launch(lib, host_ptr):
    p = host_ptr

    def call(A=p, B=p, C=p, batch=2, M=8, N=64, K=64, sAb=8 * 64, sAm=64, sBb=64 * 64, sBn=64, sCb=8 * 64, sCm=64, f32=0):
        return lib.fl_bmm_bf16_nt(A, B, C, batch, M, N, K, sAb, sAm, sBb, sBn, sCb, sCm, f32, None)

    for kwargs, reason in ((dict(N=48), b"N=48 must be a multiple of 32"),
                           (dict(K=24), b"K=24 of 16"),
                           (dict(sAm=12), b"operand rows must be 16-byte aligned"),
                           (dict(A=p + 2), b"operand rows must be 16-byte aligned"),
                           (dict(sCm=6), b"output rows must be 8-byte (bf16) / 16-byte (f32) aligned"),
                           (dict(C=p + 8, f32=1), b"output rows must be 8-byte (bf16) / 16-byte (f32) aligned")):
        assert call(**kwargs) == 1, kwargs
        assert reason in lib.fl_last_error(), (kwargs, lib.fl_last_error())
    assert call(M=0) == 0 and call(batch=0) == 0                       # nothing to do: not an error, and nothing is launched


def test_fl_gemm_bf16_nt_splitk_refuses_before_any_launch(lib, host_ptr):
    p = host_ptr
    M, N, K = 33, 256, 7168
    need = int(lib.fl_gemm_bf16_nt_splitk_workspace_bytes(M, N, K))
    assert need > 0

    def call(M=M, N=N, ws_bytes=need):
        return lib.fl_gemm_bf16_nt_splitk(p, p, p, M, N, K, K, K, N, 1, p, ws_bytes, None)

    assert call(N=96) == 1 and b"N=96, K=7168 must be multiples of 64" in lib.fl_last_error()
    assert call(ws_bytes=need - 1) == 1 and b"workspace too small" in lib.fl_last_error()
    assert call(M=0) == 0
