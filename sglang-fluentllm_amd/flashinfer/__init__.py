"""Drop-in subset of `flashinfer` (reference fork: 3rdparty/flashinfer feature/longcat_main): ONLY the entry points on
the FP8 MLA-decode / grouped-GEMM hot path: quantization.quant_1x128, sgl_per_token_group_quant_fp8,
silu_and_mul, activation.silu_and_mul_fuse_block_quant, comm.trtllm_{allreduce,reducescatter,allgather}_fusion, and
moe_fused_gate (the router selection feeding the EP dispatch, srt/layers/moe/topk.py:33,715) and
apply_rope_with_cos_sin_cache_inplace (q_pe / k_pe rotation before K5/K4, srt/layers/rotary_embedding.py:31,203), plus the
rmsnorm / fused_add_rmsnorm / norm._rmsnorm_fused_parallel (layernorm.py:26-31,293), topk_softmax / routing_flash (topk.py:33,845), the
two attention-wrapper classes FlashMLABackend's base class constructs (flashinfer_mla_backend.py:124-142; attention_wrappers.py):
both LIVE: BatchPrefillWithRaggedKVCacheWrapper — the ragged bf16 MHA prefill (192/128) of the prompt path, with `merge_state` for
its chunked-prefix form (csrc/mha_prefill_bf16.hip; lse in base 2) — and BatchMLAPagedAttentionWrapper — absorbed paged MLA attention
(576/512, bf16, page size 1, ragged and causal; csrc/mla_prefill_bf16.hip) — and `comm.vllm_ar` (C4), and the submodule `sampling`
(softmax, top-k / top-p renormalisation, top-k / top-p / min-p sampling; csrc/sampling.hip) — taken from the submodule, as the reference does."""
from fluent_mi355.gemm import sgl_per_token_group_quant_fp8, silu_and_mul  # noqa: F401
# the W8A8 dense path (per-token x per-channel scales, csrc/gemm_w8a8.hip + the row quantisers of csrc/quant_act.hip)
from fluent_mi355.gemm import (fp8_scaled_mm, int8_scaled_mm, sgl_per_tensor_quant_fp8, sgl_per_token_group_quant_int8,  # noqa: F401
                               sgl_per_token_quant_fp8)
from fluent_mi355.router import moe_fused_gate, routing_flash, topk_softmax  # noqa: F401
from fluent_mi355.rope import FusedSetKVBufferArg, apply_rope_with_cos_sin_cache_inplace  # noqa: F401

from .attention_wrappers import BatchMLAPagedAttentionWrapper, BatchPrefillWithRaggedKVCacheWrapper  # noqa: F401
# the GQA models' default attention backend (srt/layers/attention/flashinfer_backend.py): paged GQA attention, head dim 128, bf16, page
# size 1 (csrc/gqa_paged_bf16.hip), with the host helpers of `decode` and `cascade` that file imports
from .attention_wrappers import (BatchDecodeWithPagedKVCacheWrapper, BatchPrefillWithPagedKVCacheWrapper,  # noqa: F401
                                 run_device_plan_prefill_graph)

from . import activation, cascade, comm, decode, norm, quantization, sampling  # noqa: F401
from .norm import fused_add_rmsnorm, gemma_fused_add_rmsnorm, gemma_rmsnorm, rmsnorm  # noqa: F401

import torch as _torch


from fluent_mi355.bmm import dsv3_router_gemm  # noqa: F401,E402  (hand-written bf16 MFMA GEMM, csrc/bmm_bf16.hip)


def dsv3_fused_a_gemm(hidden_states, weight_t):
    """models/deepseek_v2.py:46,785-793: the <= 16-token min-latency q_a/kv_a projection, behind
    `use_min_latency_fused_a_gemm` (an sm90 switch): hidden [T, K] x weight_t [K, N] with weight_t k-contiguous (the
    transposed view of the [N, K] parameter, as the call site passes it) -> the same hand-written MFMA kernel."""
    from fluent_mi355.bmm import bmm as _bmm

    return _bmm(hidden_states.unsqueeze(0), weight_t.unsqueeze(0))[0]


def merge_state(v_a, s_a, v_b, s_b):
    """models/deepseek_v2.py:43,1037-1071: the chunked-prefill attention merge — two states (v [T, H, D] bf16, s [T, H] f32 lse in
    BASE 2, as `forward_return_lse` returns it) over disjoint key sets -> (v, s) over their union (csrc/mha_prefill_bf16.hip)."""
    from fluent_mi355.prefill import merge_state as _merge

    return _merge(v_a, s_a, v_b, s_b)
