"""P1 / P2: ragged bf16 MHA prefill attention and the attention-state merge (csrc/mha_prefill_bf16.hip) — what
`flashinfer.BatchPrefillWithRaggedKVCacheWrapper.forward / forward_return_lse` (srt/layers/attention/flashinfer_mla_backend.py:449,
layers/attention/chunker.py:304) and `flashinfer.merge_state` (models/deepseek_v2.py:1037-1071) run on the DeepSeek-V3 / LongCat MLA
prompt path — and absorbed paged MLA attention over token-indexed KV (csrc/mla_prefill_bf16.hip), what
`flashinfer.BatchMLAPagedAttentionWrapper.run` (flashinfer_mla_backend.py:472-541) runs with page size 1 — and P3: paged GQA attention
(head dim 128, csrc/gqa_paged_bf16.hip, and over an fp8 e4m3 KV cache csrc/gqa_paged_fp8kv.hip), what `flashinfer.BatchDecodeWithPagedKVCacheWrapper` / `BatchPrefillWithPagedKVCacheWrapper` /
the 128/128 ragged wrapper run for the GQA models (srt/layers/attention/flashinfer_backend.py); its decode form allocates the workspace
of its KV split with torch.empty.  This module validates, fills the C struct and launches; nothing in it computes, copies or synchronises, and the only
allocations are the outputs.  Anything the kernel does not serve raises RuntimeError — there is no library fallback.

The log-sum-exp all three functions speak is BASE 2: lse = log2 sum_j 2^(sm_scale * log2(e) * q.k_j) (flashinfer's convention)."""
from __future__ import annotations

import ctypes
import math

import torch

from ._lib import check, cu_count, lib, stream_ptr

_vp, _i64, _i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32


class FlPrefillArgs(ctypes.Structure):
    """Mirror of `struct FlPrefillArgs` in include/fluent_mi355.h (field order is ABI)."""

    _fields_ = [
        ("struct_bytes", _i32), ("batch", _i32), ("num_q_tokens", _i64), ("num_kv_tokens", _i64), ("num_heads", _i32),
        ("head_dim_qk", _i32), ("head_dim_vo", _i32), ("causal", _i32), ("sm_scale", ctypes.c_float), ("reserved", _i32),
        ("q", _vp), ("q_stride_token", _i64), ("q_stride_head", _i64),
        ("k", _vp), ("k_stride_token", _i64), ("k_stride_head", _i64),
        ("v", _vp), ("v_stride_token", _i64), ("v_stride_head", _i64),
        ("qo_indptr", _vp), ("kv_indptr", _vp), ("out", _vp), ("lse", _vp),
    ]


lib.fl_mha_prefill_ragged_bf16.argtypes = [ctypes.POINTER(FlPrefillArgs), _vp]
lib.fl_mha_prefill_ragged_bf16.restype = ctypes.c_int
lib.fl_merge_state.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _i64, ctypes.c_int, _vp]
lib.fl_merge_state.restype = ctypes.c_int

HEAD_DIM_QK, HEAD_DIM_VO = 192, 128


def _operand(name, t, head_dim):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"mha_prefill_ragged: {name} must be a CUDA/HIP tensor")
    if t.dtype != torch.bfloat16:
        raise RuntimeError(f"mha_prefill_ragged: {name} is {t.dtype}; only bfloat16 is served")
    if t.dim() != 3 or t.shape[2] != head_dim:
        raise RuntimeError(f"mha_prefill_ragged: {name} must be [tokens, heads, {head_dim}] (head dims other than "
                           f"{HEAD_DIM_QK}/{HEAD_DIM_VO} are not served), got {tuple(t.shape)}")
    if t.numel() and (t.stride(2) != 1 or t.stride(0) % 8 or t.stride(1) % 8 or t.data_ptr() % 16):
        raise RuntimeError(f"mha_prefill_ragged: {name} needs a contiguous last dimension and 16-byte aligned rows, strides {t.stride()}")


def _indptr(name, t, device):
    if not torch.is_tensor(t) or t.device != device or t.dtype != torch.int32 or t.dim() != 1 or t.numel() < 1 or not t.is_contiguous():
        raise RuntimeError(f"mha_prefill_ragged: {name} must be a contiguous int32 [batch + 1] tensor on {device}")


def mha_prefill_ragged(q, k, v, qo_indptr, kv_indptr, causal: bool, sm_scale: float | None = None, return_lse: bool = False):
    """q [Tq, H, 192], k [Tk, H, 192], v [Tk, H, 128] bf16 (any token / head strides with 16-byte aligned rows; nothing is copied),
    qo_indptr / kv_indptr int32 [B + 1] on the same device.  Returns o [Tq, H, 128] bf16, and with `return_lse` also the BASE-2
    lse [Tq, H] f32.  `causal` is bottom-right aligned (row i of a request sees keys j <= i + kv_len - qo_len); a row that sees no key
    gets o = 0, lse = -inf.  Rows of q that belong to no request are left unwritten."""
    _operand("q", q, HEAD_DIM_QK)
    _operand("k", k, HEAD_DIM_QK)
    _operand("v", v, HEAD_DIM_VO)
    H = q.shape[1]
    if k.shape[1] != H or v.shape[1] != H:
        raise RuntimeError(f"mha_prefill_ragged: MHA only — q has {H} heads, k {k.shape[1]}, v {v.shape[1]}")
    if k.shape[0] != v.shape[0] or k.device != q.device or v.device != q.device:
        raise RuntimeError("mha_prefill_ragged: k and v must have the same tokens and sit on q's device")
    _indptr("qo_indptr", qo_indptr, q.device)
    _indptr("kv_indptr", kv_indptr, q.device)
    if kv_indptr.numel() != qo_indptr.numel():
        raise RuntimeError("mha_prefill_ragged: qo_indptr and kv_indptr differ in length")
    o = torch.empty(q.shape[0], H, HEAD_DIM_VO, dtype=torch.bfloat16, device=q.device)
    lse = torch.empty(q.shape[0], H, dtype=torch.float32, device=q.device) if return_lse else None
    a = FlPrefillArgs()
    a.struct_bytes = ctypes.sizeof(FlPrefillArgs)
    a.batch, a.num_q_tokens, a.num_kv_tokens, a.num_heads = qo_indptr.numel() - 1, q.shape[0], k.shape[0], H
    a.head_dim_qk, a.head_dim_vo, a.causal = HEAD_DIM_QK, HEAD_DIM_VO, int(bool(causal))
    a.sm_scale = float(HEAD_DIM_QK ** -0.5 if sm_scale is None else sm_scale)
    a.q, a.q_stride_token, a.q_stride_head = q.data_ptr(), q.stride(0), q.stride(1)
    a.k, a.k_stride_token, a.k_stride_head = k.data_ptr(), k.stride(0), k.stride(1)
    a.v, a.v_stride_token, a.v_stride_head = v.data_ptr(), v.stride(0), v.stride(1)
    a.qo_indptr, a.kv_indptr, a.out = qo_indptr.data_ptr(), kv_indptr.data_ptr(), o.data_ptr()
    a.lse = lse.data_ptr() if return_lse else None
    check(lib.fl_mha_prefill_ragged_bf16(ctypes.byref(a), stream_ptr(q.device)), "fl_mha_prefill_ragged_bf16")
    return (o, lse) if return_lse else o


def merge_state(v_a, s_a, v_b, s_b):
    """Attention states (v [T, H, D] bf16, s [T, H] f32 base-2 lse) over two disjoint key sets -> the state over their union.  A side
    whose s is -inf returns the other side unchanged; both -inf: v = 0, s = -inf."""
    for n, v, s in (("a", v_a, s_a), ("b", v_b, s_b)):
        if not (torch.is_tensor(v) and torch.is_tensor(s) and v.is_cuda and s.device == v.device):
            raise RuntimeError(f"merge_state: v_{n} / s_{n} must be CUDA/HIP tensors on one device")
        if v.dtype != torch.bfloat16 or s.dtype != torch.float32 or v.dim() != 3 or s.shape != v.shape[:2]:
            raise RuntimeError(f"merge_state: v_{n} bf16 [T, H, D] with s_{n} f32 [T, H], got {v.dtype} {tuple(v.shape)} / {s.dtype} {tuple(s.shape)}")
        if not (v.is_contiguous() and s.is_contiguous()):
            raise RuntimeError(f"merge_state: v_{n} / s_{n} must be contiguous")
    if v_a.shape != v_b.shape or v_b.device != v_a.device or v_a.shape[2] % 8:
        raise RuntimeError(f"merge_state: the two states differ in shape or device, or D is no multiple of 8: {tuple(v_a.shape)} / {tuple(v_b.shape)}")
    v, s = torch.empty_like(v_a), torch.empty_like(s_a)
    check(lib.fl_merge_state(v_a.data_ptr(), s_a.data_ptr(), v_b.data_ptr(), s_b.data_ptr(), v.data_ptr(), s.data_ptr(),
                             s_a.numel(), v_a.shape[2], stream_ptr(v_a.device)), "fl_merge_state")
    return v, s


class FlMlaPrefillArgs(ctypes.Structure):
    """Mirror of `struct FlMlaPrefillArgs` in include/fluent_mi355.h (field order is ABI)."""

    _fields_ = [
        ("struct_bytes", _i32), ("batch", _i32), ("num_q_tokens", _i64), ("num_kv_slots", _i64), ("num_kv_indices", _i64),
        ("num_heads", _i32), ("head_dim_ckv", _i32), ("head_dim_kpe", _i32), ("causal", _i32), ("sm_scale", ctypes.c_float),
        ("reserved", _i32),
        ("q_nope", _vp), ("q_nope_stride_token", _i64), ("q_nope_stride_head", _i64),
        ("q_pe", _vp), ("q_pe_stride_token", _i64), ("q_pe_stride_head", _i64),
        ("ckv", _vp), ("ckv_stride_slot", _i64), ("kpe", _vp), ("kpe_stride_slot", _i64),
        ("qo_indptr", _vp), ("kv_indptr", _vp), ("kv_indices", _vp), ("kv_len_arr", _vp), ("out", _vp), ("lse", _vp),
    ]


lib.fl_mla_prefill_paged_bf16.argtypes = [ctypes.POINTER(FlMlaPrefillArgs), _vp]
lib.fl_mla_prefill_paged_bf16.restype = ctypes.c_int

HEAD_DIM_CKV, HEAD_DIM_KPE = 512, 64


def _mla_rows(name, t, shape, what):
    """bf16 CUDA/HIP tensor of `shape` (None = any size) with a contiguous last dimension and 16-byte aligned rows"""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"mla_prefill_paged: {name} must be a CUDA/HIP tensor")
    if t.dtype != torch.bfloat16:
        raise RuntimeError(f"mla_prefill_paged: {name} is {t.dtype}; only bfloat16 is served")
    if t.dim() != len(shape) or any(w is not None and d != w for d, w in zip(t.shape, shape)):
        raise RuntimeError(f"mla_prefill_paged: {name} must be {what} (head dims other than {HEAD_DIM_CKV}/{HEAD_DIM_KPE} and page "
                           f"sizes other than 1 are not served), got {tuple(t.shape)}")
    if t.numel() and (t.stride(-1) != 1 or any(t.stride(i) % 8 for i in range(t.dim() - 1)) or t.data_ptr() % 16):
        raise RuntimeError(f"mla_prefill_paged: {name} needs a contiguous last dimension and 16-byte aligned rows, strides {t.stride()}")


def _i32_array(name, t, device, n=None):
    if (not torch.is_tensor(t) or t.device != device or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous()
            or (n is not None and t.numel() < n)):
        raise RuntimeError(f"mla_prefill_paged: {name} must be a contiguous int32 vector on {device}"
                           + (f" with at least {n} entries" if n is not None else ""))


def mla_prefill_paged(q_nope, q_pe, ckv, kpe, qo_indptr, kv_indptr, kv_indices, kv_len_arr, causal: bool, sm_scale: float,
                      out=None, lse=None, return_lse: bool = False):
    """q_nope [T, H, 512], q_pe [T, H, 64], ckv [N, 512] or [N, 1, 512], kpe [N, 64] or [N, 1, 64] bf16 (any 16-byte aligned token /
    head strides — the two column ranges of one [N, 1, 576] buffer are fine; nothing is copied); qo_indptr / kv_indptr int32 [>= B + 1],
    kv_indices int32 (one slot = one token), kv_len_arr int32 [>= B] on the same device, B = len(qo_indptr) - 1.  Writes o [T, H, 512]
    bf16 into `out` (allocated when None) and, with `return_lse` or `lse` given, the BASE-2 lse [T, H] f32.  Request b attends over
    kv_len = max(0, min(kv_len_arr[b], kv_indptr[b + 1] - kv_indptr[b])) keys; `causal` is bottom-right aligned; a row that sees no key
    gets o = 0, lse = -inf; rows of no request are left unwritten; slot indices are clamped into [0, N)."""
    if q_nope is None or not torch.is_tensor(q_nope) or q_nope.dim() != 3:
        raise RuntimeError("mla_prefill_paged: q_nope must be a [tokens, heads, 512] tensor")
    T, H = q_nope.shape[:2]
    _mla_rows("q_nope", q_nope, (T, H, HEAD_DIM_CKV), "[tokens, heads, 512]")
    _mla_rows("q_pe", q_pe, (T, H, HEAD_DIM_KPE), "[tokens, heads, 64] with q_nope's tokens and heads")
    dev = q_nope.device
    if torch.is_tensor(ckv) and ckv.dim() == 3 and torch.is_tensor(kpe) and kpe.dim() == 3:
        _mla_rows("ckv_cache", ckv, (None, 1, HEAD_DIM_CKV), "[slots, 1, 512]")
        _mla_rows("kpe_cache", kpe, (ckv.shape[0], 1, HEAD_DIM_KPE), "[slots, 1, 64] with ckv_cache's slots")
    else:
        _mla_rows("ckv_cache", ckv, (None, HEAD_DIM_CKV), "[slots, 512] or [slots, 1, 512]")
        _mla_rows("kpe_cache", kpe, (ckv.shape[0], HEAD_DIM_KPE), "[slots, 64] with ckv_cache's slots")
    if q_pe.device != dev or ckv.device != dev or kpe.device != dev:
        raise RuntimeError("mla_prefill_paged: q_nope, q_pe, ckv_cache and kpe_cache must sit on one device")
    _i32_array("qo_indptr", qo_indptr, dev, 1)
    B = qo_indptr.numel() - 1
    _i32_array("kv_indptr", kv_indptr, dev, B + 1)
    _i32_array("kv_indices", kv_indices, dev)
    _i32_array("kv_len_arr", kv_len_arr, dev, B)
    if out is None:
        out = torch.empty(T, H, HEAD_DIM_CKV, dtype=torch.bfloat16, device=dev)
    elif (not torch.is_tensor(out) or out.dtype != torch.bfloat16 or out.device != dev or tuple(out.shape) != (T, H, HEAD_DIM_CKV)
          or not out.is_contiguous()):
        raise RuntimeError(f"mla_prefill_paged: out must be a contiguous bf16 [{T}, {H}, {HEAD_DIM_CKV}] tensor on {dev}")
    if lse is None:
        lse = torch.empty(T, H, dtype=torch.float32, device=dev) if return_lse else None
    elif (not torch.is_tensor(lse) or lse.dtype != torch.float32 or lse.device != dev or tuple(lse.shape) != (T, H)
          or not lse.is_contiguous()):
        raise RuntimeError(f"mla_prefill_paged: lse must be a contiguous f32 [{T}, {H}] tensor on {dev}")
    a = FlMlaPrefillArgs()
    a.struct_bytes = ctypes.sizeof(FlMlaPrefillArgs)
    a.batch, a.num_q_tokens, a.num_kv_slots, a.num_kv_indices, a.num_heads = B, T, ckv.shape[0], kv_indices.numel(), H
    a.head_dim_ckv, a.head_dim_kpe, a.causal, a.sm_scale = HEAD_DIM_CKV, HEAD_DIM_KPE, int(bool(causal)), float(sm_scale)
    a.q_nope, a.q_nope_stride_token, a.q_nope_stride_head = q_nope.data_ptr(), q_nope.stride(0), q_nope.stride(1)
    a.q_pe, a.q_pe_stride_token, a.q_pe_stride_head = q_pe.data_ptr(), q_pe.stride(0), q_pe.stride(1)
    a.ckv, a.ckv_stride_slot, a.kpe, a.kpe_stride_slot = ckv.data_ptr(), ckv.stride(0), kpe.data_ptr(), kpe.stride(0)
    a.qo_indptr, a.kv_indptr, a.kv_indices = qo_indptr.data_ptr(), kv_indptr.data_ptr(), kv_indices.data_ptr()
    a.kv_len_arr, a.out, a.lse = kv_len_arr.data_ptr(), out.data_ptr(), (lse.data_ptr() if lse is not None else None)
    check(lib.fl_mla_prefill_paged_bf16(ctypes.byref(a), stream_ptr(dev)), "fl_mla_prefill_paged_bf16")
    return (out, lse) if return_lse else out


class FlGqaPagedArgs(ctypes.Structure):
    """Mirror of `struct FlGqaPagedArgs` in include/fluent_mi355.h (field order is ABI)."""

    _fields_ = [
        ("struct_bytes", _i32), ("batch", _i32), ("num_q_tokens", _i64), ("num_kv_slots", _i64), ("num_kv_indices", _i64),
        ("num_qo_heads", _i32), ("num_kv_heads", _i32), ("head_dim", _i32), ("causal", _i32), ("sm_scale", ctypes.c_float),
        ("decode_form", _i32), ("num_splits", _i32), ("reserved", _i32),
        ("q", _vp), ("q_stride_token", _i64), ("q_stride_head", _i64),
        ("k", _vp), ("k_stride_slot", _i64), ("k_stride_head", _i64),
        ("v", _vp), ("v_stride_slot", _i64), ("v_stride_head", _i64),
        ("qo_indptr", _vp), ("kv_indptr", _vp), ("kv_indices", _vp), ("out", _vp), ("lse", _vp),
        ("workspace", _vp), ("workspace_bytes", _i64),
    ]


lib.fl_gqa_paged_attention_bf16.argtypes = [ctypes.POINTER(FlGqaPagedArgs), _vp]
lib.fl_gqa_paged_attention_bf16.restype = ctypes.c_int
lib.fl_gqa_paged_attention_fp8kv.argtypes = [ctypes.POINTER(FlGqaPagedArgs), ctypes.c_float, ctypes.c_float, _vp]
lib.fl_gqa_paged_attention_fp8kv.restype = ctypes.c_int

GQA_HEAD_DIM, GQA_MAX_GROUP, GQA_DECODE_ROWS, GQA_MAX_SPLITS = 128, 16, 16, 16


def gqa_num_splits(batch: int, num_kv_heads: int, cus: int) -> int:
    """Slices the decode form cuts every request's KV into.  From SHAPES only (a captured graph stays valid when lengths change): enough
    workgroups for two per CU, at most 16.  The rule is a GUESS: no other S was ever timed beside it.  The first measurement
    (profiles/gqa_paged_first_measurement.txt; Hkv = 8, seq 4096, 256 CUs): B = 128 -> S = 1, 0.72 of 8 TB/s; B = 16 -> S = 4, 0.67;
    B = 1 -> the cap of 16 (the rule asks for 64) leaves half the CUs idle, 15.8 us = 0.13."""
    return max(1, min(GQA_MAX_SPLITS, -(-2 * cus // max(1, batch * num_kv_heads))))


def _gqa_rows(name, t, heads, dev, dtype=torch.bfloat16):
    if not torch.is_tensor(t) or not t.is_cuda or t.device != dev:
        raise RuntimeError(f"gqa_paged_attention: {name} must be a CUDA/HIP tensor on {dev}")
    if t.dtype != dtype:
        raise RuntimeError(f"gqa_paged_attention: {name} is {t.dtype}; " + (
            f"the other pool is {dtype}" if dtype != torch.bfloat16 else "only bfloat16 is served" if name == "q" else
            "only bfloat16 and float8_e4m3fn pools (both alike) are served"))
    if t.dim() != 3 or t.shape[2] != GQA_HEAD_DIM or (heads is not None and t.shape[1] != heads):
        raise RuntimeError(f"gqa_paged_attention: {name} must be [rows, {heads or 'heads'}, {GQA_HEAD_DIM}] (other head dims, page sizes "
                           f"other than 1 and the HND layout are not served), got {tuple(t.shape)}")
    per16 = 16 // t.element_size()   # elements in 16 bytes: 8 (bf16) or 16 (fp8)
    if t.numel() and (t.stride(2) != 1 or t.stride(0) % per16 or t.stride(1) % per16 or t.data_ptr() % 16):
        raise RuntimeError(f"gqa_paged_attention: {name} needs a contiguous last dimension and 16-byte aligned rows, strides {t.stride()}")


def _gqa_i32(name, t, dev, n=None):
    if (not torch.is_tensor(t) or t.device != dev or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous()
            or (n is not None and t.numel() < n)):
        raise RuntimeError(f"gqa_paged_attention: {name} must be a contiguous int32 vector on {dev}"
                           + (f" with at least {n} entries" if n is not None else ""))


def gqa_paged_attention(q, k_pool, v_pool, qo_indptr, kv_indptr, kv_indices, causal: bool, sm_scale: float | None = None,
                        out=None, lse=None, return_lse: bool = False, q_len_fixed: bool = False, k_scale=None, v_scale=None):
    """q [T, Hq, 128] bf16, k_pool / v_pool [slots, Hkv, 128] both bf16 or both float8_e4m3fn — the pools' dtype picks the kernel,
    csrc/gqa_paged_bf16.hip or csrc/gqa_paged_fp8kv.hip (any 16-byte aligned slot / head strides; nothing is copied),
    Hq % Hkv == 0 with a group of at most 16 heads.  qo_indptr int32 [B + 1] or None (= one query token per request: decode, T == B),
    kv_indptr int32 [>= B + 1], kv_indices int32 (one slot = one token) or None (= identity: request b's keys are rows
    kv_indptr[b] .. kv_indptr[b + 1] of the pools themselves — the ragged form).  Writes o [T, Hq, 128] bf16 into `out` (allocated when
    None) and, with `return_lse` or `lse` given, the BASE-2 lse [T, Hq] f32.  `causal` is bottom-right aligned; a row that sees no key
    gets o = 0, lse = -inf; rows of no request are left unwritten; slot indices are clamped into [0, slots).

    Which kernel form runs is decided from shapes alone (no host synchronisation): the decode form — waves split the KV, the KV of a
    request is cut into gqa_num_splits() slices and merged by a second kernel — when every request has one query token (qo_indptr None)
    or, with `q_len_fixed`, T / B tokens with T / B * (Hq / Hkv) <= 16; the row form otherwise.

    fp8 pools: o = v_scale softmax(sm_scale k_scale q K8^T + mask) V8, and the lse carries k_scale; the bytes are dequantised exactly, q and
    P stay bf16.  `k_scale` / `v_scale` are None (= 1.0) or finite positive Python numbers; a tensor is refused (reading it would
    synchronise the host and break a capture).  bf16 pools take no scale other than None / 1.0."""
    if not torch.is_tensor(q) or q.dim() != 3:
        raise RuntimeError("gqa_paged_attention: q must be a [tokens, heads, 128] tensor")
    dev = q.device
    T, Hq = q.shape[:2]
    _gqa_rows("q", q, None, dev)
    if not torch.is_tensor(k_pool) or k_pool.dim() != 3:
        raise RuntimeError("gqa_paged_attention: k_pool must be a [slots, kv heads, 128] tensor")
    Hkv = k_pool.shape[1]
    fp8 = k_pool.dtype == torch.float8_e4m3fn
    _gqa_rows("k_pool", k_pool, None, dev, k_pool.dtype if fp8 else torch.bfloat16)
    _gqa_rows("v_pool", v_pool, Hkv, dev, k_pool.dtype)
    scales = []
    for name, s in (("k_scale", k_scale), ("v_scale", v_scale)):
        if s is not None and (isinstance(s, bool) or not isinstance(s, (int, float)) or not math.isfinite(s) or s <= 0):
            raise RuntimeError(f"gqa_paged_attention: {name}={s!r}; a scale is None or a finite positive Python number (a tensor would "
                               "have to be read on the host)")
        if s is not None and not fp8 and float(s) != 1.0:
            raise RuntimeError(f"gqa_paged_attention: {name}={s!r} with bf16 pools; only an fp8 KV cache is scaled")
        scales.append(1.0 if s is None else float(s))
    if v_pool.shape[0] != k_pool.shape[0]:
        raise RuntimeError("gqa_paged_attention: k_pool and v_pool differ in slots")
    if Hkv < 1 or Hq % Hkv or Hq // Hkv > GQA_MAX_GROUP:
        raise RuntimeError(f"gqa_paged_attention: {Hq} query heads over {Hkv} KV heads; the group must be whole and at most {GQA_MAX_GROUP}")
    G = Hq // Hkv
    _gqa_i32("kv_indptr", kv_indptr, dev, 1)
    if qo_indptr is None:
        B = kv_indptr.numel() - 1
        if T != B:
            raise RuntimeError(f"gqa_paged_attention: without qo_indptr every request has one query token, got {T} tokens for {B} requests")
    else:
        _gqa_i32("qo_indptr", qo_indptr, dev, 1)
        B = qo_indptr.numel() - 1
        _gqa_i32("kv_indptr", kv_indptr, dev, B + 1)
    if kv_indices is not None:
        _gqa_i32("kv_indices", kv_indices, dev)
    if out is None:
        out = torch.empty(T, Hq, GQA_HEAD_DIM, dtype=torch.bfloat16, device=dev)
    elif (not torch.is_tensor(out) or out.dtype != torch.bfloat16 or out.device != dev or tuple(out.shape) != (T, Hq, GQA_HEAD_DIM)
          or not out.is_contiguous()):
        raise RuntimeError(f"gqa_paged_attention: out must be a contiguous bf16 [{T}, {Hq}, {GQA_HEAD_DIM}] tensor on {dev}")
    if lse is None:
        lse = torch.empty(T, Hq, dtype=torch.float32, device=dev) if return_lse else None
    elif (not torch.is_tensor(lse) or lse.dtype != torch.float32 or lse.device != dev or tuple(lse.shape) != (T, Hq)
          or not lse.is_contiguous()):
        raise RuntimeError(f"gqa_paged_attention: lse must be a contiguous f32 [{T}, {Hq}] tensor on {dev}")
    decode = qo_indptr is None or (bool(q_len_fixed) and B > 0 and T % B == 0 and T // B * G <= GQA_DECODE_ROWS)
    S = gqa_num_splits(B, Hkv, cu_count(dev)) if decode and B > 0 else 1
    # the partial states of the splits: from the caching allocator (under capture: the graph's pool), not the caller's workspace buffer
    ws = torch.empty(S * T * Hq * (GQA_HEAD_DIM + 1), dtype=torch.float32, device=dev) if S > 1 else None
    a = FlGqaPagedArgs()
    a.struct_bytes = ctypes.sizeof(FlGqaPagedArgs)
    a.batch, a.num_q_tokens, a.num_kv_slots = B, T, k_pool.shape[0]
    a.num_kv_indices = k_pool.shape[0] if kv_indices is None else kv_indices.numel()
    a.num_qo_heads, a.num_kv_heads, a.head_dim, a.causal = Hq, Hkv, GQA_HEAD_DIM, int(bool(causal))
    a.sm_scale = float(GQA_HEAD_DIM ** -0.5 if sm_scale is None else sm_scale)
    a.decode_form, a.num_splits = int(decode), S
    a.q, a.q_stride_token, a.q_stride_head = q.data_ptr(), q.stride(0), q.stride(1)
    a.k, a.k_stride_slot, a.k_stride_head = k_pool.data_ptr(), k_pool.stride(0), k_pool.stride(1)
    a.v, a.v_stride_slot, a.v_stride_head = v_pool.data_ptr(), v_pool.stride(0), v_pool.stride(1)
    a.qo_indptr = qo_indptr.data_ptr() if qo_indptr is not None else None
    a.kv_indptr = kv_indptr.data_ptr()
    a.kv_indices = kv_indices.data_ptr() if kv_indices is not None else None
    a.out, a.lse = out.data_ptr(), (lse.data_ptr() if lse is not None else None)
    a.workspace, a.workspace_bytes = (ws.data_ptr(), ws.numel() * 4) if ws is not None else (None, 0)
    if fp8:
        check(lib.fl_gqa_paged_attention_fp8kv(ctypes.byref(a), scales[0], scales[1], stream_ptr(dev)), "fl_gqa_paged_attention_fp8kv")
    else:
        check(lib.fl_gqa_paged_attention_bf16(ctypes.byref(a), stream_ptr(dev)), "fl_gqa_paged_attention_bf16")
    return (out, lse) if return_lse else out
