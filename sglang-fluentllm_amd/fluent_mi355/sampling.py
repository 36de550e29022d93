"""S1: the sampler's kernels (csrc/sampling.hip) — softmax, top-k / top-p renormalisation and top-k / top-p / min-p sampling over f32
rows, what `flashinfer.sampling` serves to srt/layers/sampler.py:94-110 and srt/speculative/eagle_{worker,utils}.py.  This module
validates, fills `FlSamplingArgs` and launches once on torch's current stream; nothing in it computes, copies or synchronises and the only
allocation is the output (the speculative verify step at the end of the file also keeps a few KB of tickets and slice sums per stream).
Anything the kernels do not serve raises RuntimeError — there is no library fallback.

Keep rules (p(k) the k-th largest value of a row, S its sum, M(x) = sum{p_j : p_j > x}):
  top-k: p_i >= p(k), ties kept, k >= V keeps everything;  top-p: M(p_i) < top_p * S_base, top_p >= 1 keeps everything positive;
  "joint": both on the input row (S_base = S), intersected;  "top_k_first": top-p on the top-k survivors (S_base = their mass);
  min-p: p_i >= min_p * max_j p_j (one f32 multiply).
Per-row parameters are Python scalars or device tensors with one entry per ROW of probs (with `indices`, sample b reads row indices[b]
and that row's parameters, as flashinfer does)."""
from __future__ import annotations

import ctypes

import torch

from ._lib import check, cu_count, lib, stream_ptr

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


# ---- S2: speculative chain verification (csrc/spec_verify.hip): the accept / reject step that ends an EAGLE / MTP verify step
# (srt/speculative/eagle_utils.py:231-289).  Semantics are stated in include/fluent_mi355.h.


class FlSpecVerifyArgs(ctypes.Structure):
    """Mirror of `struct FlSpecVerifyArgs` in include/fluent_mi355.h (field order is ABI)."""

    _fields_ = [
        ("struct_bytes", _i32), ("batch", _i32), ("num_draft", _i32), ("vocab", _i32), ("num_slices", _i32), ("target_predict_is_i64", _i32),
        ("accept_index_pitch", _i64), ("predicts", _vp), ("accept_index", _vp), ("accept_token_num", _vp), ("candidates", _vp),
        ("target_predict", _vp), ("uniform_samples", _vp), ("uniform_final", _vp), ("target_probs", _vp), ("draft_probs", _vp),
        ("target_pitch_b", _i64), ("target_pitch_d", _i64), ("draft_pitch_b", _i64), ("draft_pitch_d", _i64),
        ("threshold_single", _f32), ("threshold_acc", _f32), ("slice_sums", _vp), ("tickets", _vp),
    ]


for _name in ("fl_spec_verify_greedy", "fl_spec_verify_sample"):
    getattr(lib, _name).argtypes = [ctypes.POINTER(FlSpecVerifyArgs), _vp]
    getattr(lib, _name).restype = ctypes.c_int

MAX_DRAFT, MAX_SLICES = 32, 512
_SLICE_MIN_ELEMS = 8192        # shortest slice the rule below makes: 2,048 vectors = one round of eight loads per lane with a draft row
_WORKSPACE_MAX_BYTES = 16 << 20
_workspace = {}                # (device index, stream) -> (tickets u32 [>= B] all zero between launches, slice sums f32 [>= B * S])


def choose_num_slices(batch, vocab, cus):
    """Workgroups per request of the sampling kernel.  By the first measurement (profiles/spec_verify_first_measurement.txt, V = 129,280 on
    256 CUs): 8 slices beat one while single workgroups would leave 15 CUs in 16 idle (B = 1, 4, 16: 12.1-13.8 us against 14.8-15.3);
    at B = 64 and 256 the hand-over through memory costs more than the shorter walk saves (21.1-23.0 against 19.8-19.9, 62-68 against
    43-47) and one workgroup per request it is.  The 16 lies between two measured points (B = 16 wins, B = 64 does not); it is not a
    tuned threshold."""
    if batch * 16 > cus:
        return 1
    return max(1, min(8, -(-vocab // _SLICE_MIN_ELEMS)))


def _verify_common(what, predicts, accept_index, accept_token_num, candidates):
    """validates the tensors both kernels share; returns the struct with them filled in"""
    if not all(torch.is_tensor(t) and t.is_cuda for t in (predicts, accept_index, accept_token_num, candidates)):
        raise RuntimeError(f"{what}: predicts, accept_index, accept_token_num and candidates must be CUDA/HIP tensors (nothing is served on the CPU)")
    dev = candidates.device
    if candidates.dim() != 2 or candidates.dtype != torch.int32 or not candidates.is_contiguous():
        raise RuntimeError(f"{what}: candidates must be a contiguous int32 [batch, draft tokens], got {candidates.dtype} {tuple(candidates.shape)}")
    B, D = candidates.shape
    if not 1 <= D <= MAX_DRAFT or B > 65535 or B * D >= 1 << 31:
        raise RuntimeError(f"{what}: {D} draft tokens (1 .. {MAX_DRAFT} are served) or batch {B} (up to 65535)")
    for name, t, n in (("predicts", predicts, B * D), ("accept_token_num", accept_token_num, B)):
        if t.device != dev or t.dtype != torch.int32 or t.numel() != n or not t.is_contiguous():
            raise RuntimeError(f"{what}: {name} must be a contiguous int32 tensor of {n} elements on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    if (accept_index.device != dev or accept_index.dtype != torch.int32 or accept_index.dim() != 2 or accept_index.shape[0] != B
            or accept_index.shape[1] < D or (B and accept_index.stride(1) != 1) or (B > 1 and accept_index.stride(0) < accept_index.shape[1])):
        raise RuntimeError(f"{what}: accept_index must be int32 [{B}, >= {D}] on {dev} with a contiguous last dimension, got {accept_index.dtype} "
                           f"{tuple(accept_index.shape)} strides {accept_index.stride()}")
    a = FlSpecVerifyArgs()
    a.struct_bytes = ctypes.sizeof(FlSpecVerifyArgs)
    a.batch, a.num_draft = B, D
    a.accept_index_pitch = accept_index.stride(0) if B > 1 else accept_index.shape[1]
    a.predicts, a.accept_index, a.accept_token_num = predicts.data_ptr(), accept_index.data_ptr(), accept_token_num.data_ptr()
    a.candidates = candidates.data_ptr()
    return a


def verify_chain_greedy(predicts, accept_index, accept_token_num, candidates, target_predict):
    """In place: the leading run of chain positions whose candidate equals the target's prediction at the position before it."""
    what = "sampling.verify_chain_greedy"
    a = _verify_common(what, predicts, accept_index, accept_token_num, candidates)
    if (not torch.is_tensor(target_predict) or target_predict.device != candidates.device or target_predict.dtype not in (torch.int32, torch.int64)
            or target_predict.shape != candidates.shape or not target_predict.is_contiguous()):
        raise RuntimeError(f"{what}: target_predict must be a contiguous int32 / int64 {tuple(candidates.shape)} on {candidates.device}")
    a.target_predict, a.target_predict_is_i64 = target_predict.data_ptr(), int(target_predict.dtype == torch.int64)
    check(lib.fl_spec_verify_greedy(ctypes.byref(a), stream_ptr(candidates.device)), "fl_spec_verify_greedy")


def _verify_workspace(dev, batch, slices):
    """(tickets, slice sums) of one launch.  Eager calls on one stream share a pair (the kernel leaves its tickets at zero; launches on one
    stream are ordered), grown on demand; another stream gets its own, so two streams never share tickets; a call made while the stream
    is CAPTURING gets a fresh pair from the graph's private pool (the kvmove.py rule).  Zeroed by a fill kernel, not a memset."""
    need = 4 * batch * (slices + 1)
    if need > _WORKSPACE_MAX_BYTES:
        raise RuntimeError(f"sampling.chain_speculative_sampling: batch {batch} x {slices} slices needs {need} B of workspace, over the {_WORKSPACE_MAX_BYTES} B bound")
    if torch.cuda.is_current_stream_capturing():
        return torch.zeros(batch, dtype=torch.int32, device=dev), torch.empty(batch * slices, dtype=torch.float32, device=dev)
    key = (dev.index, stream_ptr(dev))
    ws = _workspace.get(key)
    if ws is None or ws[0].numel() < batch or ws[1].numel() < batch * slices:
        ws = _workspace[key] = (torch.zeros(batch, dtype=torch.int32, device=dev), torch.empty(batch * slices, dtype=torch.float32, device=dev))
    return ws


def chain_speculative_sampling(predicts, accept_index, accept_token_num, candidates, uniform_samples, uniform_samples_for_final_sampling,
                               target_probs, draft_probs, threshold_single=1.0, threshold_acc=1.0, num_slices=None):
    """In place: the accept tests of a drafted chain against the target's probabilities and the final token from max(q - p, 0), one launch.
    `num_slices` (private: tests and timing) forces the number of workgroups per request; None = choose_num_slices."""
    what = "sampling.chain_speculative_sampling"
    a = _verify_common(what, predicts, accept_index, accept_token_num, candidates)
    dev, (B, D) = candidates.device, candidates.shape
    for name, t in (("target_probs", target_probs), ("draft_probs", draft_probs)):
        if not torch.is_tensor(t) or t.device != dev or t.dtype != torch.float32:
            raise RuntimeError(f"{what}: {name} must be a float32 tensor on {dev} (only float32 is served)")
        if t.dim() != 3 or t.shape[:2] != (B, D) or t.shape != target_probs.shape or not 1 <= t.shape[2] <= MAX_VOCAB:
            raise RuntimeError(f"{what}: {name} must be [{B}, {D}, vocab] with 1 <= vocab <= {MAX_VOCAB}, got {tuple(t.shape)}")
        if B and (t.stride(2) != 1 or (D > 1 and t.stride(1) < t.shape[2])):
            raise RuntimeError(f"{what}: {name} needs a contiguous last dimension and non-overlapping rows, strides {t.stride()}")
    for name, t, shape in (("uniform_samples", uniform_samples, (B, D)), ("uniform_samples_for_final_sampling", uniform_samples_for_final_sampling, (B,))):
        if not torch.is_tensor(t) or t.device != dev or t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise RuntimeError(f"{what}: {name} must be a contiguous float32 {shape} on {dev}")
    V = target_probs.shape[2]
    S = choose_num_slices(B, V, cu_count(dev)) if num_slices is None else int(num_slices)
    if not 1 <= S <= MAX_SLICES:
        raise RuntimeError(f"{what}: {S} slices (1 .. {MAX_SLICES} are served)")
    a.vocab, a.num_slices = V, S
    a.uniform_samples, a.uniform_final = uniform_samples.data_ptr(), uniform_samples_for_final_sampling.data_ptr()
    a.target_probs, a.draft_probs = target_probs.data_ptr(), draft_probs.data_ptr()
    a.target_pitch_b, a.target_pitch_d = (target_probs.stride(0) if B > 1 else D * V), (target_probs.stride(1) if D > 1 else V)
    a.draft_pitch_b, a.draft_pitch_d = (draft_probs.stride(0) if B > 1 else D * V), (draft_probs.stride(1) if D > 1 else V)
    a.threshold_single, a.threshold_acc = float(threshold_single), float(threshold_acc)
    ws = None
    if S > 1 and B:
        ws = _verify_workspace(dev, B, S)
        a.tickets, a.slice_sums = ws[0].data_ptr(), ws[1].data_ptr()
    check(lib.fl_spec_verify_sample(ctypes.byref(a), stream_ptr(dev)), "fl_spec_verify_sample")
