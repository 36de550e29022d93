"""eps.executor.silu(gate_up bf16 [M, 2I], exclusive_sum, num_tokens_hint) -> bf16 [M, I]
(python/sglang/srt/layers/moe/executors/fp8_eps_executor.py:62) and eps.executor.AokGroupedGemm(num_local_experts)
.run(input, weight, None, exclusive_sum, num_tokens_hint) -> bf16 [M, N] (moe/gemms/bf16/aok.py:3,18; moe/executors/eps_executor.py:35,48)."""
from fluent_mi355.gemm import AokGroupedGemm, silu  # noqa: F401
