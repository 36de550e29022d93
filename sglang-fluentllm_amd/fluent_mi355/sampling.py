"""S1: the sampler's kernels (csrc/sampling.hip) — softmax, top-k / top-p renormalisation and top-k / top-p / min-p sampling over f32
rows, what `flashinfer.sampling` serves to srt/layers/sampler.py:94-110 and srt/speculative/eagle_{worker,utils}.py.  This module
validates, fills `FlSamplingArgs` and launches once on torch's current stream; nothing in it computes, copies or synchronises and the only
allocation is the output.  Anything the kernels do not serve raises RuntimeError — there is no library fallback.

Keep rules (p(k) the k-th largest value of a row, S its sum, M(x) = sum{p_j : p_j > x}):
  top-k: p_i >= p(k), ties kept, k >= V keeps everything;  top-p: M(p_i) < top_p * S_base, top_p >= 1 keeps everything positive;
  "joint": both on the input row (S_base = S), intersected;  "top_k_first": top-p on the top-k survivors (S_base = their mass);
  min-p: p_i >= min_p * max_j p_j (one f32 multiply).
Per-row parameters are Python scalars or device tensors with one entry per ROW of probs (with `indices`, sample b reads row indices[b]
and that row's parameters, as flashinfer does)."""
from __future__ import annotations

import ctypes

import torch

from ._lib import check, lib, stream_ptr

_vp, _i64, _i32, _f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float
TOP_K, TOP_P, TOP_K_THEN_P, JOINT, MIN_P = range(5)
MAX_VOCAB = 1 << 22


class FlSamplingArgs(ctypes.Structure):
    """Mirror of `struct FlSamplingArgs` in include/fluent_mi355.h (field order is ABI)."""

    _fields_ = [
        ("struct_bytes", _i32), ("mode", _i32), ("batch", _i32), ("vocab", _i32), ("num_rows", _i64), ("row_pitch", _i64),
        ("probs", _vp), ("indices", _vp), ("top_k", _vp), ("top_k_is_i64", _i32), ("reserved", _i32), ("top_k_val", _i64),
        ("top_p", _vp), ("min_p", _vp), ("temperature", _vp), ("u", _vp),
        ("top_p_val", _f32), ("min_p_val", _f32), ("temperature_val", _f32), ("reserved2", _i32), ("out", _vp),
    ]


for _name in ("fl_sampling_softmax", "fl_sampling_renorm", "fl_sampling_sample"):
    getattr(lib, _name).argtypes = [ctypes.POINTER(FlSamplingArgs), _vp]
    getattr(lib, _name).restype = ctypes.c_int


def _rows(what, name, t):
    """f32 [B, V] on the device with a contiguous last dimension (any row pitch); returns the filled argument struct"""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"{what}: {name} must be a CUDA/HIP tensor (nothing is served on the CPU)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{what}: {name} is {t.dtype}; only float32 is served")
    if t.dim() != 2 or t.shape[1] < 1 or t.shape[1] > MAX_VOCAB:
        raise RuntimeError(f"{what}: {name} must be [batch, vocab] with 1 <= vocab <= {MAX_VOCAB}, got {tuple(t.shape)}")
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise RuntimeError(f"{what}: {name} needs a contiguous last dimension and non-overlapping rows, strides {t.stride()}")
    a = FlSamplingArgs()
    a.struct_bytes = ctypes.sizeof(FlSamplingArgs)
    a.batch, a.vocab, a.num_rows = t.shape[0], t.shape[1], t.shape[0]
    a.row_pitch = t.stride(0) if t.shape[0] > 1 else t.shape[1]
    a.probs = t.data_ptr()
    return a


def _per_row(what, name, v, rows, device, dtypes):
    """(pointer, scalar) of a per-row parameter: a Python number, or a contiguous device tensor of `rows` entries ([rows] or [rows, 1])"""
    if not torch.is_tensor(v):
        return None, v
    if v.dim() == 2 and v.shape[1] == 1:
        v = v.view(-1) if v.is_contiguous() else v[:, 0]
    if v.dim() == 0 and not v.is_cuda:
        return None, v.item()
    if v.device != device or v.dtype not in dtypes or v.dim() != 1 or v.numel() != rows or (rows > 1 and v.stride(0) != 1):
        raise RuntimeError(f"{what}: {name} must be a number or a contiguous {' / '.join(str(d) for d in dtypes)} tensor of {rows} entries "
                           f"(one per row) on {device}, got {v.dtype} {tuple(v.shape)} on {v.device}")
    return v, None


def _fill_filters(what, a, probs, top_k, top_p, min_p, keep):
    """per-row top_k / top_p / min_p into the struct; `keep` collects the tensors whose pointers the struct holds"""
    rows, dev = probs.shape[0], probs.device
    if top_k is not None:
        t, s = _per_row(what, "top_k", top_k, rows, dev, (torch.int32, torch.int64))
        if t is not None:
            keep.append(t)
            a.top_k, a.top_k_is_i64 = t.data_ptr(), int(t.dtype == torch.int64)
        else:
            a.top_k_val = int(s)
    if top_p is not None:
        t, s = _per_row(what, "top_p", top_p, rows, dev, (torch.float32,))
        if t is not None:
            keep.append(t)
            a.top_p = t.data_ptr()
        else:
            a.top_p_val = float(s)
    if min_p is not None:
        t, s = _per_row(what, "min_p", min_p, rows, dev, (torch.float32,))
        if t is not None:
            keep.append(t)
            a.min_p = t.data_ptr()
        else:
            a.min_p_val = float(s)


def softmax(logits, temperature=None):
    """softmax(logits / temperature) per row: f32 [B, V] -> f32 [B, V]; temperature None (1), a number or a [B] / [B, 1] f32 device tensor.
    A row of -inf gives zeros."""
    a = _rows("sampling.softmax", "logits", logits)
    t, s = _per_row("sampling.softmax", "temperature", temperature, logits.shape[0], logits.device, (torch.float32,))
    a.temperature, a.temperature_val = (t.data_ptr() if t is not None else None), float(1.0 if s is None else s)
    out = torch.empty(logits.shape, dtype=torch.float32, device=logits.device)
    a.out = out.data_ptr()
    check(lib.fl_sampling_softmax(ctypes.byref(a), stream_ptr(logits.device)), "fl_sampling_softmax")
    return out


def renorm(probs, top_k=None, top_p=None, order="joint"):
    """The kept entries of each row divided by their sum, the dropped ones exactly 0: a new f32 [B, V].  top_k and / or top_p as in the
    module docstring; with both, `order` is "joint" or "top_k_first"."""
    a = _rows("sampling.renorm", "probs", probs)
    a.mode = _mode("sampling.renorm", top_k, top_p, None, order)
    keep = []
    _fill_filters("sampling.renorm", a, probs, top_k, top_p, None, keep)
    out = torch.empty(probs.shape, dtype=torch.float32, device=probs.device)
    a.out = out.data_ptr()
    check(lib.fl_sampling_renorm(ctypes.byref(a), stream_ptr(probs.device)), "fl_sampling_renorm")
    return out


def _mode(what, top_k, top_p, min_p, order):
    if order not in ("joint", "top_k_first"):
        raise RuntimeError(f'{what}: filter order {order!r}; "joint" and "top_k_first" are served')
    if min_p is not None:
        if top_k is not None or top_p is not None:
            raise RuntimeError(f"{what}: min_p is served on its own (renormalise with top_k / top_p first, as the reference's sampler does)")
        return MIN_P
    if top_k is None and top_p is None:
        raise RuntimeError(f"{what}: give top_k, top_p or min_p")
    if top_p is None:
        return TOP_K
    if top_k is None:
        return TOP_P
    return JOINT if order == "joint" else TOP_K_THEN_P


def sample(probs, u, top_k=None, top_p=None, min_p=None, order="joint", indices=None):
    """One token id per entry of `u` (f32 [B] uniforms in [0, 1) on the device): the smallest kept index of the row whose running kept mass
    in vocabulary order exceeds u * S_kept -> int32 [B].  Sample b reads row b of probs, or row indices[b] (int32 [B]) when given."""
    what = "sampling.sample"
    a = _rows(what, "probs", probs)
    a.mode = _mode(what, top_k, top_p, min_p, order)
    dev = probs.device
    if not torch.is_tensor(u) or u.device != dev or u.dtype != torch.float32 or u.dim() != 1 or (u.numel() > 1 and u.stride(0) != 1):
        raise RuntimeError(f"{what}: u must be a contiguous float32 vector on {dev}")
    if indices is not None:
        if (not torch.is_tensor(indices) or indices.device != dev or indices.dtype != torch.int32 or indices.dim() != 1
                or indices.numel() != u.numel() or (indices.numel() > 1 and indices.stride(0) != 1)):
            raise RuntimeError(f"{what}: indices must be a contiguous int32 vector on {dev} with one entry per sample ({u.numel()})")
        a.indices = indices.data_ptr()
    elif u.numel() != probs.shape[0]:
        raise RuntimeError(f"{what}: u has {u.numel()} entries for {probs.shape[0]} rows (give indices to map samples to rows)")
    if u.numel() and probs.shape[0] == 0:
        raise RuntimeError(f"{what}: samples asked of an empty probs")
    keep = []
    _fill_filters(what, a, probs, top_k, top_p, min_p, keep)
    a.batch, a.u = u.numel(), u.data_ptr()
    out = torch.empty(u.numel(), dtype=torch.int32, device=dev)
    a.out = out.data_ptr()
    check(lib.fl_sampling_sample(ctypes.byref(a), stream_ptr(dev)), "fl_sampling_sample")
    return out
