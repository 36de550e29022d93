"""Construction-time dependencies of `FlashMLABackend(model_runner)`: its base class
`FlashInferMLAAttnBackend.__init__` (python/sglang/srt/layers/attention/flashinfer_mla_backend.py:124-142) builds
`flashinfer.BatchPrefillWithRaggedKVCacheWrapper(workspace, "NHD")` and three `flashinfer.BatchMLAPagedAttentionWrapper(
workspace, backend="auto")`, and its indices updaters call `.plan(...)` / `.begin_forward(...)` on them
(:344, :622-650).  Both are LIVE.  `BatchPrefillWithRaggedKVCacheWrapper`: the ragged bf16 MHA prefill of the prompt path
(forward_normal_extend :449, the chunked-prefix path layers/attention/chunker.py:281-312) runs on csrc/mha_prefill_bf16.hip.
`BatchMLAPagedAttentionWrapper`: absorbed paged MLA attention (forward_absorbed :486-541 — prompts under a captured prefill graph and
with flashinfer_mla_disable_ragged — and decode / verify of the plain backend :472-483) runs on csrc/mla_prefill_bf16.hip.  Both go
through fluent_mi355/prefill.py; what the kernels do not serve raises RuntimeError — loudly, not by a silent fall-back.  (On the FP8 MLA
decode / verify path of FlashMLABackend every attention call goes to `flash_mla_fp8` / `flash_mla_swap` instead,
flashmla_backend.py:105-256.)"""
from __future__ import annotations


class _InertWrapper:
    _what = "flashinfer attention wrapper"

    def __init__(self, float_workspace_buffer=None, *args, use_cuda_graph: bool = False, **kwargs):
        self._float_workspace_buffer = float_workspace_buffer
        self._use_cuda_graph = bool(use_cuda_graph)
        # attributes the reference's fast_mla_decode_plan / graph paths read or assign (flashinfer_mla_backend.py:760-820)
        self._kv_indices_buf = kwargs.get("kv_indices")
        self._kv_indptr_buf = kwargs.get("kv_indptr")
        self._qo_indptr_buf = kwargs.get("qo_indptr")
        self._kv_len_arr_buf = kwargs.get("kv_len_arr")
        self._init_args, self._init_kwargs = args, kwargs
        self.last_plan = None

    def plan(self, *args, **kwargs):
        self.last_plan = (args, kwargs)

    begin_forward = plan

    def end_forward(self):
        self.last_plan = None

    def run(self, *args, **kwargs):
        raise RuntimeError(f"{self._what}.run: not on the FP8 MLA decode / grouped-GEMM hot path this library replaces "
                           "(flashmla_backend.py routes decode and verify to flash_mla_fp8 / flash_mla_swap); paged MLA "
                           "attention through flashinfer has no MI355X implementation here")

    forward = run
    forward_return_lse = run
    run_return_lse = run


class BatchPrefillWithRaggedKVCacheWrapper(_InertWrapper):
    """flashinfer.BatchPrefillWithRaggedKVCacheWrapper(workspace, kv_layout) — flashinfer_mla_backend.py:124-126, used by
    forward_extend's ragged prefill (:449) and the prefix chunker (chunker.py:268-312).  `plan` / `begin_forward` only RECORD
    (no device access, never raise); `run` / `forward` return o [Tq, H, 128] bf16, `run_return_lse` / `forward_return_lse`
    (o, lse) with lse [Tq, H] f32 in BASE 2 (log2 of the sum of 2^(sm_scale * log2(e) * q.k)), the base `flashinfer.merge_state`
    reads.  Served: bf16, MHA, head dims 192 / 128, NHD, causal (bottom-right aligned) or not; per-call `causal`, `sm_scale`,
    `logits_soft_cap` override the plan's, `sm_scale=None` = head_dim_qk ** -0.5.  Everything else raises RuntimeError."""
    _what = "BatchPrefillWithRaggedKVCacheWrapper"

    def __init__(self, float_workspace_buffer=None, kv_layout: str = "NHD", *args, **kwargs):
        super().__init__(float_workspace_buffer, *args, **kwargs)
        self._kv_layout = kv_layout
        self._plan = None

    def plan(self, qo_indptr=None, kv_indptr=None, num_qo_heads=None, num_kv_heads=None, head_dim_qk=None, head_dim_vo=None,
             *args, **kwargs):
        self.last_plan = ((qo_indptr, kv_indptr, num_qo_heads, num_kv_heads, head_dim_qk, head_dim_vo) + args, kwargs)
        self._plan = dict(kwargs, qo_indptr=qo_indptr, kv_indptr=kv_indptr, num_qo_heads=num_qo_heads, num_kv_heads=num_kv_heads,
                          head_dim_qk=head_dim_qk, head_dim_vo=head_dim_qk if head_dim_vo is None else head_dim_vo, extra_args=args)

    begin_forward = plan

    def end_forward(self):
        self.last_plan = self._plan = None

    def _run(self, q, k, v, return_lse, causal=None, sm_scale=None, logits_soft_cap=None, **kwargs):
        from fluent_mi355 import prefill

        what, pl = self._what, self._plan
        if pl is None:
            raise RuntimeError(f"{what}.run before plan / begin_forward")
        if self._kv_layout != "NHD":
            raise RuntimeError(f"{what}: kv_layout {self._kv_layout!r}; only NHD is served")
        causal = pl.get("causal", False) if causal is None else causal
        sm_scale = pl.get("sm_scale") if sm_scale is None else sm_scale
        cap = pl.get("logits_soft_cap") if logits_soft_cap is None else logits_soft_cap
        if cap is not None and cap > 0:
            raise RuntimeError(f"{what}: logits_soft_cap={cap} is not served by the MI355X prefill kernel")
        if pl["extra_args"] or pl.get("custom_mask") is not None or pl.get("packed_custom_mask") is not None:
            raise RuntimeError(f"{what}: custom masks are not served")
        # every other option of flashinfer's plan / run must sit at its neutral value: nothing is silently ignored
        neutral = {"pos_encoding_mode": "NONE", "window_left": -1, "use_fp16_qk_reduction": False, "rope_scale": None, "rope_theta": None,
                   "k_scale": None, "v_scale": None, "out": None, "lse": None}
        given = [(n, pl[n]) for n in neutral if n in pl] + [(n, x) for n, x in kwargs.items() if n != "enable_pdl"]
        for name, val in given:
            if name not in neutral or ((val is not None) if neutral[name] is None else (val != neutral[name])):
                raise RuntimeError(f"{what}: {name}={val!r} is not served")
        if pl["num_kv_heads"] != pl["num_qo_heads"]:
            raise RuntimeError(f"{what}: MHA only (num_qo_heads={pl['num_qo_heads']}, num_kv_heads={pl['num_kv_heads']})")
        if (pl["head_dim_qk"], pl["head_dim_vo"]) != (prefill.HEAD_DIM_QK, prefill.HEAD_DIM_VO):
            raise RuntimeError(f"{what}: head dims {pl['head_dim_qk']}/{pl['head_dim_vo']}; only 192/128 are served")
        return prefill.mha_prefill_ragged(q, k, v, pl["qo_indptr"], pl["kv_indptr"], bool(causal), sm_scale, return_lse)

    def run(self, q=None, k=None, v=None, *args, return_lse: bool = False, **kwargs):
        if args:
            raise RuntimeError(f"{self._what}.run: unexpected positional arguments")
        return self._run(q, k, v, return_lse, **kwargs)

    def run_return_lse(self, q=None, k=None, v=None, **kwargs):
        return self._run(q, k, v, True, **kwargs)

    def forward(self, q=None, k=None, v=None, causal=None, **kwargs):
        return self._run(q, k, v, False, causal=causal, **kwargs)

    def forward_return_lse(self, q=None, k=None, v=None, causal=None, **kwargs):
        return self._run(q, k, v, True, causal=causal, **kwargs)


class BatchMLAPagedAttentionWrapper(_InertWrapper):
    """flashinfer.BatchMLAPagedAttentionWrapper(workspace, backend="auto", use_cuda_graph=..., qo_indptr=..., kv_indptr=...,
    kv_indices=..., kv_len_arr=...) — flashinfer_mla_backend.py:128-142 and the cuda-graph capture paths (:196-311).
    `plan(qo_indptr, kv_indptr, kv_indices, kv_len_arr, num_heads, head_dim_ckv, head_dim_kpe, page_size, causal, sm_scale,
    q_data_type, kv_data_type)` RECORDS and never raises; built without `use_cuda_graph` it touches no device, with it the four arrays
    are also copied (device-side, non-blocking; skipped where the argument already is the buffer) into the constructor's buffers, which
    `run` then reads: a captured launch sees the next plan's values.  `run(q_nope, q_pe, ckv_cache, kpe_cache, out=None, lse=None,
    return_lse=False)` returns `out` [T, H, 512] bf16, or `(out, lse)` with lse [T, H] f32 in BASE 2.  Served: bf16 on both sides, head
    dims 512 / 64, page size 1, causal (bottom-right aligned) or not.  Everything else raises RuntimeError at `run`."""
    _what = "BatchMLAPagedAttentionWrapper"
    _PLAN = ("qo_indptr", "kv_indptr", "kv_indices", "kv_len_arr", "num_heads", "head_dim_ckv", "head_dim_kpe", "page_size", "causal",
             "sm_scale", "q_data_type", "kv_data_type")

    def __init__(self, float_workspace_buffer=None, use_cuda_graph: bool = False, qo_indptr=None, kv_indptr=None, kv_indices=None,
                 kv_len_arr=None, backend: str = "auto", **kwargs):
        super().__init__(float_workspace_buffer, use_cuda_graph=use_cuda_graph, qo_indptr=qo_indptr, kv_indptr=kv_indptr,
                         kv_indices=kv_indices, kv_len_arr=kv_len_arr, **kwargs)
        self._backend = backend
        self._plan = None

    def plan(self, *args, **kwargs):
        import torch

        self.last_plan = (args, kwargs)
        pl = dict(zip(self._PLAN, args))
        pl.update(kwargs)
        pl["extra_args"] = args[len(self._PLAN):]
        if self._use_cuda_graph:
            for name in self._PLAN[:4]:
                src, buf = pl.get(name), getattr(self, f"_{name}_buf")
                if torch.is_tensor(src) and torch.is_tensor(buf) and buf.dim() == 1 and src.dim() == 1 and src.numel() <= buf.numel():
                    if src.data_ptr() != buf.data_ptr() or src.device != buf.device:
                        buf[:src.numel()].copy_(src, non_blocking=True)
                    # (kv_indices: the whole buffer — kv_indptr bounds what is read, as under flashinfer)
                    pl[name] = buf if name == "kv_indices" else buf[:src.numel()]
        self._plan = pl

    begin_forward = plan

    def end_forward(self):
        self.last_plan = self._plan = None

    def run(self, q_nope=None, q_pe=None, ckv_cache=None, kpe_cache=None, *args, out=None, lse=None, return_lse: bool = False, **kwargs):
        from fluent_mi355 import prefill
        import torch

        what, pl = self._what, self._plan
        if pl is None:
            raise RuntimeError(f"{what}.run before plan")
        if args or pl["extra_args"]:
            raise RuntimeError(f"{what}: unexpected positional arguments")
        for name, val in kwargs.items():   # kv_len / page_table / profiler_buffer and anything unknown: nothing is silently ignored
            if name != "enable_pdl":
                raise RuntimeError(f"{what}.run: {name}= is not served")
        missing = [n for n in self._PLAN if n not in pl]
        unknown = [n for n in pl if n not in self._PLAN and n not in ("extra_args", "use_profiler")]
        if missing or unknown or pl.get("use_profiler"):
            raise RuntimeError(f"{what}: plan lacks {missing}, has unserved {unknown or 'use_profiler'}")
        if pl["page_size"] != 1:
            raise RuntimeError(f"{what}: page_size={pl['page_size']}; only token-indexed KV (page size 1) is served")
        if (pl["head_dim_ckv"], pl["head_dim_kpe"]) != (prefill.HEAD_DIM_CKV, prefill.HEAD_DIM_KPE):
            raise RuntimeError(f"{what}: head dims {pl['head_dim_ckv']}/{pl['head_dim_kpe']}; only 512/64 are served")
        if pl["q_data_type"] != torch.bfloat16 or pl["kv_data_type"] != torch.bfloat16:
            raise RuntimeError(f"{what}: q / kv data types {pl['q_data_type']} / {pl['kv_data_type']}; only bfloat16 is served")
        if not torch.is_tensor(q_nope) or q_nope.dim() != 3 or q_nope.shape[1] != pl["num_heads"]:
            raise RuntimeError(f"{what}: q_nope must be a [tokens, {pl['num_heads']}, 512] tensor")
        return prefill.mla_prefill_paged(q_nope, q_pe, ckv_cache, kpe_cache, pl["qo_indptr"], pl["kv_indptr"], pl["kv_indices"],
                                         pl["kv_len_arr"], bool(pl["causal"]), float(pl["sm_scale"]), out=out, lse=lse,
                                         return_lse=return_lse)

    forward = run

    def run_return_lse(self, q_nope=None, q_pe=None, ckv_cache=None, kpe_cache=None, **kwargs):
        kwargs.pop("return_lse", None)
        return self.run(q_nope, q_pe, ckv_cache, kpe_cache, return_lse=True, **kwargs)

    forward_return_lse = run_return_lse
