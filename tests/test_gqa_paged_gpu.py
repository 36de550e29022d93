"""GPU: paged GQA attention, head dim 128, bf16 (csrc/gqa_paged_bf16.hip) through the public interface —
`flashinfer.BatchDecodeWithPagedKVCacheWrapper`, `BatchPrefillWithPagedKVCacheWrapper` and the 128/128 form of
`BatchPrefillWithRaggedKVCacheWrapper` — against a plain fp64 statement on the CPU computed from the same bf16 inputs: K / V gathered by
kv_indices, every KV head repeated G times, softmax(scale QK^T + mask) V per request and head, lse in base 2, a row without a visible key
= 0 / -inf.  The KV pools are larger than the tokens used, kv_indices is a random permutation into them, slot 0 (where a wrong index or a
clamp would land) is poisoned.  Shapes sit on the kernel's edges: 64 tokens per KV tile, 16 per wave in the decode form, 128 rows per
workgroup in the row form, 16 rows as the limit of the decode form, and the split counts the committed rule gives on 256 CUs.  Bounds: the
project's own for this arithmetic (bf16 operands, fp32 accumulation, bf16 P and output; tests/test_prefill_gpu.py): rel-MAE < 6e-3,
max-abs < 5e-2, finite lse within 2e-3, -inf positions exactly equal; the fp32 split merge gets no wider bound."""
import pytest
import torch

from helpers import rel_mae

pytestmark = pytest.mark.gpu
SCALE = 128 ** -0.5
LN2 = 0.6931471805599453
DEV = torch.device("cuda:0")


def indptr(lens):
    return torch.tensor([0] + list(lens), dtype=torch.int32).cumsum(0).to(torch.int32)


def ref_attention(q, k, v, qo_lens, kv_lens, causal):
    """fp64 over request-contiguous k / v [sum(kv_lens), Hkv, 128]: (o [Tq, Hq, 128], lse [Tq, Hq] base 2); causal is bottom-right aligned"""
    G = q.shape[1] // k.shape[1]
    q, k, v = q.double(), k.double().repeat_interleave(G, 1), v.double().repeat_interleave(G, 1)
    o = torch.zeros(q.shape, dtype=torch.float64)
    lse = torch.full(q.shape[:2], float("-inf"), dtype=torch.float64)
    qs = ks = 0
    for ql, kl in zip(qo_lens, kv_lens):
        if ql and kl:
            s = torch.einsum("ihd,jhd->hij", q[qs:qs + ql], k[ks:ks + kl]) * SCALE
            if causal:
                s.masked_fill_(torch.arange(kl)[None, :] > torch.arange(ql)[:, None] + (kl - ql), float("-inf"))
            o[qs:qs + ql] = torch.einsum("hij,jhd->ihd", torch.softmax(s, -1).nan_to_num(0.0), v[ks:ks + kl])
            lse[qs:qs + ql] = (torch.logsumexp(s, -1) / LN2).t()
        qs, ks = qs + ql, ks + kl
    return o, lse


def make_case(qo_lens, kv_lens, Hq, Hkv, rescale=False):
    """q, the two pools, kv_indices (a permutation that avoids the poisoned slot 0) — on the CPU"""
    g = torch.Generator().manual_seed(5 + len(qo_lens) + sum(kv_lens) + Hq)
    Tq, Tk = sum(qo_lens), sum(kv_lens)
    q = torch.randn(Tq, Hq, 128, generator=g).to(torch.bfloat16)
    kp, vp = (torch.randn(Tk + 37, Hkv, 128, generator=g).to(torch.bfloat16) for _ in range(2))
    kp[0], vp[0] = 3e4, 3e4
    idx = (torch.randperm(Tk + 36, generator=g)[:Tk] + 1).to(torch.int32)
    if rescale:   # q x 8, keys in rising order of the first head's score: the row maximum moves tile after tile and slice after slice
        q = (q.float() * 8).to(torch.bfloat16)
        idx = idx[torch.argsort(kp[idx.long(), 0].float() @ q[0, 0].float())]
    return q, kp, vp, idx


def check(o, lse, ro, rl, what):
    o = o.float().cpu()
    rel, mabs = rel_mae(o, ro), float((o.double() - ro).abs().max())
    lerr = 0.0
    if lse is not None:
        lse, fin = lse.cpu(), torch.isfinite(rl)
        lerr = float((lse[fin].double() - rl[fin]).abs().max()) if fin.any() else 0.0
        assert torch.equal(torch.isneginf(lse), torch.isneginf(rl)) and not torch.isnan(lse).any(), what
    print(f"{what}: rel-MAE {rel:.2e}, max-abs {mabs:.2e}, lse {lerr:.1e}")
    assert torch.isfinite(o).all() and rel < 6e-3 and mabs < 5e-2 and lerr < 2e-3, (what, rel, mabs, lerr)


def workspace():
    return torch.empty(16, dtype=torch.uint8, device=DEV)


def run_paged(qo_lens, kv_lens, Hq, Hkv, causal, q_len_fixed=False, rescale=False):
    """qo_lens None: the decode wrapper (one token per request), else the paged prefill wrapper; returns (o, lse, ref o, ref lse)"""
    import flashinfer

    decode = qo_lens is None
    qo_lens = [1] * len(kv_lens) if decode else qo_lens
    q, kp, vp, idx = make_case(qo_lens, kv_lens, Hq, Hkv, rescale)
    ones = torch.ones(len(kv_lens), dtype=torch.int32, device=DEV)
    if decode:
        w = flashinfer.BatchDecodeWithPagedKVCacheWrapper(workspace(), "NHD")
        w.begin_forward(indptr(kv_lens).to(DEV), idx.to(DEV), ones, Hq, Hkv, 128, 1, data_type=torch.bfloat16, q_data_type=torch.bfloat16)
        o, lse = w.forward_return_lse(q.to(DEV), (kp.to(DEV), vp.to(DEV)), sm_scale=SCALE, logits_soft_cap=0.0, k_scale=1.0, v_scale=None)
    else:
        w = flashinfer.BatchPrefillWithPagedKVCacheWrapper(workspace(), "NHD")
        w.begin_forward(indptr(qo_lens).to(DEV), indptr(kv_lens).to(DEV), idx.to(DEV), ones, Hq, Hkv, 128, 1, q_data_type=torch.bfloat16,
                        kv_data_type=torch.bfloat16, custom_mask=None, non_blocking=True, q_len_fixed=q_len_fixed)
        o, lse = w.forward_return_lse(q.to(DEV), (kp.to(DEV), vp.to(DEV)), causal=causal, sm_scale=SCALE, window_left=-1)
    torch.cuda.synchronize()
    assert o.shape == q.shape and o.dtype == torch.bfloat16 and lse.shape == q.shape[:2] and lse.dtype == torch.float32
    return (o, lse) + ref_attention(q, kp[idx.long()], vp[idx.long()], qo_lens, kv_lens, causal)


# S = clamp(ceil(2 * 256 / (B * Hkv)), 1, 16) on 256 CUs: B * Hkv = 4 -> 16 slices (most of the 1-key request's are empty), 320 -> 2, 512 -> 1
DECODE = [(4, 4, [1, 63, 64, 65, 300], False), (8, 2, [1, 63, 64, 65, 300], False), (16, 1, [1, 63, 64, 65, 300], False),
          (8, 2, [1000, 1], False), (16, 8, [1 + i % 130 for i in range(40)], False), (16, 8, [1 + (7 * i) % 130 for i in range(64)], False),
          (4, 1, [4000], True)]   # 16 slices of 4 tiles


@pytest.mark.parametrize("Hq,Hkv,kv_lens,rescale", DECODE)
def test_decode_matches_fp64(Hq, Hkv, kv_lens, rescale):
    check(*run_paged(None, kv_lens, Hq, Hkv, False, rescale=rescale), f"decode Hq={Hq} Hkv={Hkv} B={len(kv_lens)} rescale={rescale}")


PREFILL = [
    ([129, 64, 1, 0], [129, 64, 1, 0], 2, True, False),   # crossed row tile (258 rows), exact KV tile, single token, empty request
    ([5, 130], [133, 194], 2, True, False),               # bottom-right offset with a prefix
    ([33, 128], [200, 0], 2, False, False),               # second request: empty KV -> 0 / -inf
    ([40], [8], 2, True, False),                          # tokens 0..31 see no key
    ([4, 4, 4], [4, 67, 260], 2, True, True),             # verify, 4 tokens x G = 4 = 16 rows: decode form, causal inside the block
    ([4, 4, 4], [4, 67, 260], 1, True, True),             # verify, 4 tokens x G = 8 = 32 rows: row form
]


@pytest.mark.parametrize("qo_lens,kv_lens,Hkv,causal,q_len_fixed", PREFILL)
def test_paged_prefill_extend_verify_match_fp64(qo_lens, kv_lens, Hkv, causal, q_len_fixed):
    check(*run_paged(qo_lens, kv_lens, 8, Hkv, causal, q_len_fixed), f"paged {qo_lens} x {kv_lens} Hkv={Hkv} causal={causal} fixed={q_len_fixed}")


def ragged(qo_lens, kv_lens, Hq, Hkv, q, k, v, causal):
    import flashinfer

    w = flashinfer.BatchPrefillWithRaggedKVCacheWrapper(workspace(), "NHD")
    w.begin_forward(indptr(qo_lens).to(DEV), indptr(kv_lens).to(DEV), Hq, Hkv, 128, q_data_type=torch.bfloat16)
    return w.forward_return_lse(q.to(DEV), k.to(DEV), v.to(DEV), causal=causal, sm_scale=SCALE, logits_soft_cap=0.0)


@pytest.mark.parametrize("qo_lens,kv_lens,causal", [([129, 64, 1, 0], [129, 64, 1, 0], True), ([33, 128], [200, 0], False)])
def test_ragged_128_gqa_matches_fp64(qo_lens, kv_lens, causal):
    q, kp, vp, _ = make_case(qo_lens, kv_lens, 8, 2)
    kp, vp = kp[1:], vp[1:]   # (without the poisoned row; 36 surplus rows follow the last request)
    o, lse = ragged(qo_lens, kv_lens, 8, 2, q, kp, vp, causal)
    torch.cuda.synchronize()
    n = sum(kv_lens)
    check(o, lse, *ref_attention(q, kp[:n], vp[:n], qo_lens, kv_lens, causal), f"ragged {qo_lens} x {kv_lens}")


def test_ragged_over_new_tokens_merged_with_paged_over_the_prefix_equals_causal_attention_over_the_whole_context():
    """flashinfer_backend.py:534-550; the second request has no prefix"""
    import flashinfer
    import flashinfer.cascade

    new, prefix, Hq, Hkv = [70, 33, 5], [100, 0, 260], 8, 2
    q, kp, vp, idx = make_case(new, prefix, Hq, Hkv)
    g = torch.Generator().manual_seed(3)
    kn, vn = (torch.randn(sum(new), Hkv, 128, generator=g).to(torch.bfloat16) for _ in range(2))
    o1, s1 = ragged(new, new, Hq, Hkv, q, kn, vn, True)
    w = flashinfer.BatchPrefillWithPagedKVCacheWrapper(workspace(), "NHD")
    w.begin_forward(indptr(new).to(DEV), indptr(prefix).to(DEV), idx.to(DEV), torch.ones(3, dtype=torch.int32, device=DEV), Hq, Hkv, 128, 1,
                    q_data_type=torch.bfloat16, kv_data_type=torch.bfloat16)
    o2, s2 = w.forward_return_lse(q.to(DEV), (kp.to(DEV), vp.to(DEV)), causal=False, sm_scale=SCALE)
    o, s = flashinfer.cascade.merge_state(o1, s1, o2, s2)
    torch.cuda.synchronize()
    cat = lambda a, b: torch.cat([torch.cat(t) for t in zip(a.split(prefix), b.split(new))])
    ro, rl = ref_attention(q, cat(kp[idx.long()], kn), cat(vp[idx.long()], vn), new, [a + b for a, b in zip(prefix, new)], True)
    check(o, s, ro, rl, "ragged + paged prefix")


def test_captured_decode_replays_with_new_lengths_and_indices():
    import flashinfer

    Hq, Hkv, lens_a, lens_b = 8, 2, [300, 5, 64], [1, 190, 129]
    q, kp, vp, idx_b = make_case([1, 1, 1], lens_b, Hq, Hkv)
    idx_a = torch.arange(1, 1 + sum(lens_a), dtype=torch.int32)
    kp, vp = torch.cat([kp, kp]), torch.cat([vp, vp])   # (room for lens_a's slots)
    bufs = [torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(512, dtype=torch.int32, device=DEV), torch.ones(3, dtype=torch.int32, device=DEV)]
    w = flashinfer.BatchDecodeWithPagedKVCacheWrapper(workspace(), "NHD", use_cuda_graph=True, paged_kv_indptr_buffer=bufs[0],
                                                      paged_kv_indices_buffer=bufs[1], paged_kv_last_page_len_buffer=bufs[2])
    plan = lambda lens, idx: w.begin_forward(indptr(lens).to(DEV), idx.to(DEV), bufs[2], Hq, Hkv, 128, 1, data_type=torch.bfloat16,
                                             q_data_type=torch.bfloat16, non_blocking=True)
    qd, kv = q.to(DEV), (kp.to(DEV), vp.to(DEV))
    plan(lens_b, idx_b)
    eager = w.forward(qd, kv, sm_scale=SCALE).clone()   # (also loads the kernels before the capture)
    plan(lens_a, idx_a)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = w.forward(qd, kv, sm_scale=SCALE)
    plan(lens_b, idx_b)
    ro, _ = ref_attention(q, kp[idx_b.long()], vp[idx_b.long()], [1, 1, 1], lens_b, False)
    for replay in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager), replay
    check(out, None, ro, None, "graph replay")


def test_unsupported_calls_are_refused_at_run():
    import flashinfer

    q, kv = torch.zeros(2, 8, 128, dtype=torch.bfloat16, device=DEV), tuple(torch.zeros(8, 2, 128, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    ip, ones = indptr([3, 4]).to(DEV), torch.ones(2, dtype=torch.int32, device=DEV)

    def planned(head_dim=128, page_size=1):
        d = flashinfer.BatchDecodeWithPagedKVCacheWrapper(workspace(), "NHD")
        d.begin_forward(ip, torch.arange(7, dtype=torch.int32, device=DEV), ones, 8, 2, head_dim, page_size, data_type=torch.bfloat16)
        p = flashinfer.BatchPrefillWithPagedKVCacheWrapper(workspace(), "NHD")
        p.begin_forward(indptr([1, 1]).to(DEV), ip, torch.arange(7, dtype=torch.int32, device=DEV), ones, 8, 2, head_dim, page_size)
        return d, p

    for w in planned():
        w.forward(q, kv)   # the served call, so that each refusal below is about ONE thing
        for bad in (dict(logits_soft_cap=30.0), dict(window_left=128), dict(k_scale=0.5)):
            with pytest.raises(RuntimeError):
                w.forward(q, kv, **bad)
        with pytest.raises(RuntimeError):
            w.forward(q.half(), kv)
        with pytest.raises(RuntimeError):
            w.forward(q, kv[0])
    for w in planned(head_dim=64) + planned(page_size=16):
        with pytest.raises(RuntimeError):
            w.forward(q, kv)
