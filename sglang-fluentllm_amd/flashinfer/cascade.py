"""`flashinfer.cascade` as srt/layers/attention/flashinfer_backend.py takes it (:550): merge_state, the attention-state merge of
csrc/mha_prefill_bf16.hip (base-2 lse) that `flashinfer.merge_state` already is."""
from fluent_mi355.prefill import merge_state  # noqa: F401
