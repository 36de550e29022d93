"""`flashinfer.sampling` for gfx950: the names srt/layers/sampler.py:15-20 and srt/speculative/eagle_worker.py:29 / eagle_utils.py:22 take
from it, with flashinfer's signatures, on the hand-written kernels of csrc/sampling.hip (through fluent_mi355/sampling.py, which states
the keep rules).  Uniforms are `torch.rand(B, generator=generator)` on the probabilities' device — torch's generator is graph-safe, so
a captured call draws fresh numbers on every replay.  `deterministic` is accepted: the kernels always are.  `check_nan=True` tests the
probabilities with torch (a host synchronisation, off on the reference's path) and raises ValueError.  The speculative accept / reject step
(`verify_chain_greedy`, `chain_speculative_sampling_target_only`: eagle_utils.py:234,273) runs on csrc/spec_verify.hip, one launch each,
in place; unlike upstream, `draft_probs` is only read.  Absent on purpose: `top_k_top_p_sampling_from_logits` and the
mask variants."""
import torch

from fluent_mi355 import sampling as _s


def softmax(logits, temperature=None, enable_pdl=None):
    """f32 logits [B, V] -> f32 probabilities; temperature None, a number or a [B] / [B, 1] tensor (eagle_worker.py:308,322)"""
    return _s.softmax(logits, temperature)


def top_k_renorm_probs(probs, top_k):
    """keep p_i >= (k-th largest), ties included, and renormalise (sampler.py:96, eagle_utils.py:252); top_k an int or an int tensor [B]"""
    return _s.renorm(probs, top_k=top_k)


def top_p_renorm_probs(probs, top_p):
    """keep the shortest descending prefix whose mass reaches top_p, ties at its last value included, and renormalise (sampler.py:97,
    eagle_utils.py:258); top_p a float or an f32 tensor [B]"""
    return _s.renorm(probs, top_p=top_p)


top_k_renorm_prob = top_k_renorm_probs
top_p_renorm_prob = top_p_renorm_probs


def _uniforms(probs, indices, generator, check_nan):
    if not torch.is_tensor(probs) or not probs.is_cuda:
        raise RuntimeError("flashinfer.sampling: probs must be a CUDA/HIP tensor (nothing is served on the CPU)")
    if check_nan and bool(torch.isnan(probs).any()):
        raise ValueError("flashinfer.sampling: NaN in probs")
    n = probs.shape[0] if indices is None else indices.shape[0]
    return torch.rand(n, device=probs.device, generator=generator)


def top_k_top_p_sampling_from_probs(probs, top_k, top_p, indices=None, filter_apply_order="top_k_first", deterministic=True, generator=None,
                                    check_nan=False):
    """int32 [B] token ids under top-k and top-p (sampler.py:104-110 passes filter_apply_order="joint")"""
    if filter_apply_order not in ("joint", "top_k_first"):
        raise RuntimeError(f'flashinfer.sampling: filter_apply_order {filter_apply_order!r}; "joint" and "top_k_first" are served')
    return _s.sample(probs, _uniforms(probs, indices, generator, check_nan), top_k=top_k, top_p=top_p, order=filter_apply_order, indices=indices)


def min_p_sampling_from_probs(probs, min_p, indices=None, deterministic=True, generator=None, check_nan=False):
    """int32 [B] token ids among p_i >= min_p * max_j p_j (sampler.py:98-100)"""
    return _s.sample(probs, _uniforms(probs, indices, generator, check_nan), min_p=min_p, indices=indices)


def verify_chain_greedy(predicts, accept_index, accept_token_num, candidates, target_predict, batch_size=None, num_draft_tokens=None):
    """accept the leading drafted tokens that equal the target's argmax (eagle_utils.py:234-242); writes predicts, accept_index and
    accept_token_num in place.  candidates int32 [B, D] (column 0 the verified root), target_predict int32 / int64 [B, D]"""
    if torch.is_tensor(candidates) and candidates.dim() == 2 and (batch_size not in (None, candidates.shape[0])
                                                                  or num_draft_tokens not in (None, candidates.shape[1])):
        raise RuntimeError(f"flashinfer.sampling.verify_chain_greedy: batch_size {batch_size} / num_draft_tokens {num_draft_tokens} do not "
                           f"match candidates {tuple(candidates.shape)}")
    _s.verify_chain_greedy(predicts, accept_index, accept_token_num, candidates, target_predict)


def chain_speculative_sampling_target_only(predicts, accept_index, accept_token_num, candidates, uniform_samples,
                                           uniform_samples_for_final_sampling, target_probs, draft_probs, threshold_single=1.0,
                                           threshold_acc=1.0, deterministic=True):
    """accept drafted token j while coin_j <= p_target(token_j) / threshold_acc or p_target(token_j) >= threshold_single, then draw the
    final token from max(target - draft, 0) (eagle_utils.py:273-289); writes predicts, accept_index and accept_token_num in place.
    target_probs / draft_probs f32 [B, D, V], uniform_samples f32 [B, D], uniform_samples_for_final_sampling f32 [B]"""
    _s.chain_speculative_sampling(predicts, accept_index, accept_token_num, candidates, uniform_samples, uniform_samples_for_final_sampling,
                                  target_probs, draft_probs, threshold_single, threshold_acc)
