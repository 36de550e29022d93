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
    reads.  Served: bf16, NHD, causal (bottom-right aligned) or not, with head dims 192 / 128 and MHA (csrc/mha_prefill_bf16.hip) or head
    dims 128 / 128 and num_qo_heads a multiple of num_kv_heads, group <= 16 (the paged GQA kernel without an index table,
    csrc/gqa_paged_bf16.hip; flashinfer_backend.py:524-541); per-call `causal`, `sm_scale`, `logits_soft_cap` override the plan's,
    `sm_scale=None` = head_dim_qk ** -0.5.  Everything else raises RuntimeError."""
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
        import torch

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
        if (pl["head_dim_qk"], pl["head_dim_vo"]) == (prefill.GQA_HEAD_DIM, prefill.GQA_HEAD_DIM):
            # 128/128, MHA or GQA: the paged GQA kernel in identity-index mode (csrc/gqa_paged_bf16.hip)
            if not pl["num_kv_heads"] or pl["num_qo_heads"] % pl["num_kv_heads"]:
                raise RuntimeError(f"{what}: num_qo_heads={pl['num_qo_heads']} is no multiple of num_kv_heads={pl['num_kv_heads']}")
            for name, t, heads in (("q", q, pl["num_qo_heads"]), ("k", k, pl["num_kv_heads"]), ("v", v, pl["num_kv_heads"])):
                if not torch.is_tensor(t) or t.dim() != 3 or t.shape[1] != heads:
                    raise RuntimeError(f"{what}: {name} must be a [tokens, {heads}, 128] tensor as planned")
                if t.dtype != torch.bfloat16:   # (the binding would take fp8 k / v for a cache; fresh activations are bf16)
                    raise RuntimeError(f"{what}: {name} is {t.dtype}; only bfloat16 is served")
            return prefill.gqa_paged_attention(q, k, v, pl["qo_indptr"], pl["kv_indptr"], None, bool(causal), sm_scale,
                                               return_lse=return_lse)
        if pl["num_kv_heads"] != pl["num_qo_heads"]:
            raise RuntimeError(f"{what}: MHA only (num_qo_heads={pl['num_qo_heads']}, num_kv_heads={pl['num_kv_heads']})")
        if (pl["head_dim_qk"], pl["head_dim_vo"]) != (prefill.HEAD_DIM_QK, prefill.HEAD_DIM_VO):
            raise RuntimeError(f"{what}: head dims {pl['head_dim_qk']}/{pl['head_dim_vo']}; only 192/128 and 128/128 are served")
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


class _PagedGqaWrapper:
    """What BatchDecodeWithPagedKVCacheWrapper and BatchPrefillWithPagedKVCacheWrapper share: `plan` RECORDS and never raises (built with
    `use_cuda_graph` it also copies the index arrays into the constructor's buffers — device-side, non-blocking, skipped where the argument
    already is the buffer — which `run` then reads: a captured launch sees the next plan's values); `run` checks everything and launches
    csrc/gqa_paged_bf16.hip or, for a plan with `kv_data_type` / `data_type` float8_e4m3fn, csrc/gqa_paged_fp8kv.hip through
    fluent_mi355.prefill.gqa_paged_attention.  Served: bf16 q; a bf16 or float8_e4m3fn KV cache (the pools must have the planned type), the
    fp8 one with `k_scale` / `v_scale` = None (1.0) or finite positive Python numbers: o = v_scale softmax(sm_scale k_scale q K^T) V, the
    lse carries k_scale; head dims 128 / 128, page size 1, NHD, num_qo_heads a multiple of num_kv_heads with a group of at most 16, causal
    (bottom-right aligned) or not; `sm_scale=None` = 128 ** -0.5.
    Refused at `run` with RuntimeError: logits_soft_cap > 0, window_left != -1, k_scale / v_scale other than None or 1.0 on a bf16 cache,
    a zero, negative, non-finite or tensor scale, float8_e5m2 / uint8 or any other KV type, fp8 q, pools that are not of the planned type,
    custom masks, positional encodings, other head dims, page sizes or layouts, a single-tensor KV cache, any other option."""
    _what = "paged GQA wrapper"

    def _init(self, float_workspace_buffer, kv_layout, use_cuda_graph, bufs):
        self._float_workspace_buffer = float_workspace_buffer   # kept, never used: the split's workspace comes from the caching allocator
        self._kv_layout = kv_layout
        self._use_cuda_graph = bool(use_cuda_graph)
        self._bufs = bufs          # plan name -> the constructor's graph buffer (or None)
        self._plan = self.last_plan = None
        indptr = bufs.get("kv_indptr")
        self._fixed_batch_size = indptr.numel() - 1 if self._use_cuda_graph and indptr is not None else 0

    @property
    def is_cuda_graph_enabled(self):
        return self._use_cuda_graph

    @property
    def device(self):
        return getattr(self._float_workspace_buffer, "device", None)

    def _record(self, pl):
        import torch

        self.last_plan = pl
        if self._use_cuda_graph:
            for name, buf in self._bufs.items():
                src = pl.get(name)
                if torch.is_tensor(src) and torch.is_tensor(buf) and buf.dim() == 1 and src.dim() == 1 and src.numel() <= buf.numel():
                    if src.data_ptr() != buf.data_ptr() or src.device != buf.device:
                        buf[:src.numel()].copy_(src, non_blocking=True)
                    # (kv_indices: the whole buffer — kv_indptr bounds what is read, as under flashinfer)
                    pl[name] = buf if name == "kv_indices" else buf[:src.numel()]
        self._plan = pl

    def end_forward(self):
        self._plan = self.last_plan = None

    def _launch(self, q, paged_kv_cache, run_opts, return_lse, out=None, lse=None):
        import math

        from fluent_mi355 import prefill
        import torch

        what, pl = self._what, self._plan
        if pl is None:
            raise RuntimeError(f"{what}.run before plan / begin_forward")
        if self._kv_layout != "NHD":
            raise RuntimeError(f"{what}: kv_layout {self._kv_layout!r}; only NHD is served")
        opts = dict(pl["options"])
        opts.update({n: v for n, v in run_opts.items() if v is not None})
        causal, sm_scale = bool(opts.pop("causal", False)), opts.pop("sm_scale", None)
        if (opts.pop("logits_soft_cap", None) or 0) > 0:
            raise RuntimeError(f"{what}: logits_soft_cap is not served by the MI355X GQA kernel")
        if opts.pop("window_left", -1) != -1:
            raise RuntimeError(f"{what}: sliding windows (window_left != -1) are not served")
        q_dt, kv_dt = opts.pop("q_data_type", None), opts.pop("kv_data_type", None)
        if q_dt is not None and q_dt not in (torch.bfloat16, "bfloat16"):
            raise RuntimeError(f"{what}: q_data_type={q_dt}; only bfloat16 is served")
        fp8 = kv_dt in (torch.float8_e4m3fn, "float8_e4m3fn")
        if kv_dt is not None and not fp8 and kv_dt not in (torch.bfloat16, "bfloat16"):
            raise RuntimeError(f"{what}: kv_data_type={kv_dt}; only bfloat16 and float8_e4m3fn are served")
        scales = {}
        for name in ("k_scale", "v_scale"):
            s = scales[name] = opts.pop(name, None)
            if s is None:
                continue
            if not fp8:
                if float(s) != 1.0:
                    raise RuntimeError(f"{what}: {name}={s!r}; an fp8 / scaled KV cache is not served with a bfloat16 plan")
                scales[name] = None
            elif isinstance(s, bool) or not isinstance(s, (int, float)) or not math.isfinite(s) or s <= 0:
                raise RuntimeError(f"{what}: {name}={s!r}; a scale is None or a finite positive Python number (a tensor would have to be "
                                   "read on the host, which a captured launch cannot do)")
        if opts.pop("pos_encoding_mode", "NONE") != "NONE":
            raise RuntimeError(f"{what}: positional encodings inside attention are not served")
        opts.pop("non_blocking", None)
        opts.pop("enable_pdl", None)
        q_len_fixed = bool(opts.pop("q_len_fixed", False))
        left = {n: v for n, v in opts.items() if v is not None and v is not False}   # custom masks, rope_*, anything unknown
        if left or pl["extra_args"]:
            raise RuntimeError(f"{what}: {sorted(left) or 'extra positional arguments'} not served")
        if pl["page_size"] != 1:
            raise RuntimeError(f"{what}: page_size={pl['page_size']}; only token-indexed KV (page size 1) is served")
        if pl["head_dim"] != prefill.GQA_HEAD_DIM or pl["head_dim_vo"] not in (None, prefill.GQA_HEAD_DIM):
            raise RuntimeError(f"{what}: head dims {pl['head_dim']}/{pl['head_dim_vo']}; only 128/128 are served")
        if not (isinstance(paged_kv_cache, (tuple, list)) and len(paged_kv_cache) == 2):
            raise RuntimeError(f"{what}: paged_kv_cache must be the (k_pool, v_pool) tuple; a single-tensor KV cache is not served")
        k_pool, v_pool = paged_kv_cache
        if torch.is_tensor(k_pool) and k_pool.dim() == 4 and torch.is_tensor(v_pool) and v_pool.dim() == 4:   # [pages, page_size = 1, Hkv, 128]
            if k_pool.shape[1] != 1 or v_pool.shape[1] != 1:
                raise RuntimeError(f"{what}: KV cache pages of {k_pool.shape[1]} tokens; only page size 1 is served")
            k_pool, v_pool = k_pool[:, 0], v_pool[:, 0]
        if (not torch.is_tensor(q) or q.dim() != 3 or q.shape[1] != pl["num_qo_heads"] or not torch.is_tensor(k_pool) or k_pool.dim() != 3
                or k_pool.shape[1] != pl["num_kv_heads"]):
            raise RuntimeError(f"{what}: q must be [tokens, {pl['num_qo_heads']}, 128] and the pools [slots, {pl['num_kv_heads']}, 128] as planned")
        want = torch.float8_e4m3fn if fp8 else torch.bfloat16
        if k_pool.dtype != want or not torch.is_tensor(v_pool) or v_pool.dtype != want:
            raise RuntimeError(f"{what}: the plan says a {want} KV cache, the pools are {k_pool.dtype} / {getattr(v_pool, 'dtype', None)}")
        return prefill.gqa_paged_attention(q, k_pool, v_pool, pl.get("qo_indptr"), pl["kv_indptr"], pl["kv_indices"], causal, sm_scale,
                                           out=out, lse=lse, return_lse=return_lse, q_len_fixed=q_len_fixed, **scales)


class BatchDecodeWithPagedKVCacheWrapper(_PagedGqaWrapper):
    """flashinfer.BatchDecodeWithPagedKVCacheWrapper — one query token per request over the paged (k_pool, v_pool) of a GQA model
    (flashinfer_backend.py:581,749,1137): the decode form of csrc/gqa_paged_bf16.hip with its split over the KV.  `_plan_info` is
    deliberately not defined: the reference then takes its `begin_forward` branch (:731)."""
    _what = "BatchDecodeWithPagedKVCacheWrapper"

    def __init__(self, float_workspace_buffer=None, kv_layout: str = "NHD", use_cuda_graph: bool = False, use_tensor_cores: bool = False,
                 paged_kv_indptr_buffer=None, paged_kv_indices_buffer=None, paged_kv_last_page_len_buffer=None, **kwargs):
        self._init(float_workspace_buffer, kv_layout, use_cuda_graph,
                   {"kv_indptr": paged_kv_indptr_buffer, "kv_indices": paged_kv_indices_buffer, "last_page_len": paged_kv_last_page_len_buffer})
        self._paged_kv_indptr_buf, self._paged_kv_indices_buf = paged_kv_indptr_buffer, paged_kv_indices_buffer
        self._paged_kv_last_page_len_buf = paged_kv_last_page_len_buffer
        self.use_tensor_cores = self._use_tensor_cores = bool(use_tensor_cores)
        self._init_kwargs = kwargs

    def plan(self, indptr=None, indices=None, last_page_len=None, num_qo_heads=None, num_kv_heads=None, head_dim=None, page_size=None,
             pos_encoding_mode="NONE", window_left=-1, logits_soft_cap=None, q_data_type=None, kv_data_type=None, data_type=None,
             sm_scale=None, rope_scale=None, rope_theta=None, non_blocking=True, *args, **kwargs):
        options = dict(kwargs, pos_encoding_mode=pos_encoding_mode, window_left=window_left, logits_soft_cap=logits_soft_cap,
                       q_data_type=q_data_type, kv_data_type=data_type if kv_data_type is None else kv_data_type, sm_scale=sm_scale,
                       rope_scale=rope_scale, rope_theta=rope_theta)
        self._record({"kv_indptr": indptr, "kv_indices": indices, "last_page_len": last_page_len, "num_qo_heads": num_qo_heads,
                      "num_kv_heads": num_kv_heads, "head_dim": head_dim, "head_dim_vo": None, "page_size": page_size,
                      "options": options, "extra_args": args})

    begin_forward = plan

    def run(self, q=None, paged_kv_cache=None, *args, sm_scale=None, logits_soft_cap=None, k_scale=None, v_scale=None, window_left=None,
            return_lse: bool = False, out=None, lse=None, **kwargs):
        if args:
            raise RuntimeError(f"{self._what}.run: unexpected positional arguments")
        opts = dict(kwargs, sm_scale=sm_scale, logits_soft_cap=logits_soft_cap, k_scale=k_scale, v_scale=v_scale, window_left=window_left)
        return self._launch(q, paged_kv_cache, opts, return_lse, out, lse)   # one token per request: no mask to apply

    forward = run

    def run_return_lse(self, q=None, paged_kv_cache=None, **kwargs):
        kwargs.pop("return_lse", None)
        return self.run(q, paged_kv_cache, return_lse=True, **kwargs)

    forward_return_lse = run_return_lse


class BatchPrefillWithPagedKVCacheWrapper(_PagedGqaWrapper):
    """flashinfer.BatchPrefillWithPagedKVCacheWrapper — prompts, extend over a cached prefix and speculative verify over the paged
    (k_pool, v_pool) of a GQA model (flashinfer_backend.py:512,542,980).  Rows per (request, KV head) are not known on the host without a
    synchronisation: the decode form of the kernel runs only when the plan says `q_len_fixed` and T / B * (Hq / Hkv) <= 16, the row form
    otherwise."""
    _what = "BatchPrefillWithPagedKVCacheWrapper"

    def __init__(self, float_workspace_buffer=None, kv_layout: str = "NHD", use_cuda_graph: bool = False, qo_indptr_buf=None,
                 paged_kv_indptr_buf=None, paged_kv_indices_buf=None, paged_kv_last_page_len_buf=None, custom_mask_buf=None,
                 mask_indptr_buf=None, backend: str = "auto", **kwargs):
        self._init(float_workspace_buffer, kv_layout, use_cuda_graph,
                   {"qo_indptr": qo_indptr_buf, "kv_indptr": paged_kv_indptr_buf, "kv_indices": paged_kv_indices_buf,
                    "last_page_len": paged_kv_last_page_len_buf})
        self._qo_indptr_buf, self._paged_kv_indptr_buf, self._paged_kv_indices_buf = qo_indptr_buf, paged_kv_indptr_buf, paged_kv_indices_buf
        self._paged_kv_last_page_len_buf = paged_kv_last_page_len_buf
        self._custom_mask_buf, self._mask_indptr_buf, self._backend = custom_mask_buf, mask_indptr_buf, backend
        self._init_kwargs = kwargs

    def plan(self, qo_indptr=None, paged_kv_indptr=None, paged_kv_indices=None, paged_kv_last_page_len=None, num_qo_heads=None,
             num_kv_heads=None, head_dim_qk=None, page_size=None, head_dim_vo=None, custom_mask=None, causal=False, sm_scale=None,
             q_data_type=None, kv_data_type=None, non_blocking=True, q_len_fixed=False, *args, **kwargs):
        options = dict(kwargs, custom_mask=custom_mask, causal=causal, sm_scale=sm_scale, q_data_type=q_data_type,
                       kv_data_type=kv_data_type, q_len_fixed=q_len_fixed)
        self._record({"qo_indptr": qo_indptr, "kv_indptr": paged_kv_indptr, "kv_indices": paged_kv_indices,
                      "last_page_len": paged_kv_last_page_len, "num_qo_heads": num_qo_heads, "num_kv_heads": num_kv_heads,
                      "head_dim": head_dim_qk, "head_dim_vo": head_dim_vo, "page_size": page_size, "options": options, "extra_args": args})

    begin_forward = plan

    def run(self, q=None, paged_kv_cache=None, *args, causal=None, sm_scale=None, window_left=None, logits_soft_cap=None, k_scale=None,
            v_scale=None, return_lse: bool = False, out=None, lse=None, **kwargs):
        if args:
            raise RuntimeError(f"{self._what}.run: unexpected positional arguments")
        if self._plan is not None and self._plan.get("qo_indptr") is None:
            raise RuntimeError(f"{self._what}: the plan has no qo_indptr")
        opts = dict(kwargs, causal=causal, sm_scale=sm_scale, window_left=window_left, logits_soft_cap=logits_soft_cap, k_scale=k_scale,
                    v_scale=v_scale)
        return self._launch(q, paged_kv_cache, opts, return_lse, out, lse)

    forward = run

    def run_return_lse(self, q=None, paged_kv_cache=None, **kwargs):
        kwargs.pop("return_lse", None)
        return self.run(q, paged_kv_cache, return_lse=True, **kwargs)

    forward_return_lse = run_return_lse


def run_device_plan_prefill_graph(*args, **kwargs):
    """The fork's device-side re-plan of a REPLAYED verify graph (flashinfer_backend.py:739,970,1092) rewrites flashinfer's internal plan
    record, which the MI355X GQA kernel has no counterpart of (it reads lengths on the device and needs no plan).  The name resolves so
    that flashinfer_backend.py imports; the call is refused."""
    raise RuntimeError("flashinfer.run_device_plan_prefill_graph: there is no flashinfer plan record to update on MI355X — the paged GQA "
                       "kernel reads qo_indptr / kv_indptr on the device at every launch; call begin_forward on the wrapper instead")
