"""GPU: ragged bf16 MHA prefill attention (192/128) and merge_state (csrc/mha_prefill_bf16.hip) through the public interface,
`flashinfer.BatchPrefillWithRaggedKVCacheWrapper` and `flashinfer.merge_state`, against a plain fp64 statement on the CPU computed from
the same bf16 inputs: per request and head softmax(scale QK^T + mask) V, lse in base 2, a row without a visible key = 0 / -inf.
Shapes sit on the kernel's tile edges (128 query rows per workgroup, 32 per wave, 64 KV tokens per tile).  Bounds: the project's own
for this arithmetic (bf16 operands, fp32 accumulation, bf16 P, bf16 output; tests/test_mla_gpu.py): rel-MAE < 6e-3, max-abs < 5e-2,
finite lse within 2e-3, -inf positions exactly equal."""
import pytest
import torch

from helpers import rel_mae

pytestmark = pytest.mark.gpu
SCALE = 192 ** -0.5
LN2 = 0.6931471805599453


def ref_attention(q, k, v, qo_lens, kv_lens, causal):
    """fp64: (o [Tq, H, 128], lse [Tq, H] base 2); causal is bottom-right aligned"""
    q, k, v = q.double().cpu(), k.double().cpu(), v.double().cpu()
    o = torch.zeros(q.shape[0], q.shape[1], v.shape[2], dtype=torch.float64)
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


def indptr(lens, dev):
    return torch.tensor([0] + list(lens), dtype=torch.int32).cumsum(0).to(torch.int32).to(dev)


def planned(qo_lens, kv_lens, H, dev, num_kv_heads=None):
    import flashinfer

    w = flashinfer.BatchPrefillWithRaggedKVCacheWrapper(torch.empty(16, dtype=torch.uint8, device=dev), "NHD")
    w.begin_forward(indptr(qo_lens, dev), indptr(kv_lens, dev), H, H if num_kv_heads is None else num_kv_heads, 192, 128,
                    q_data_type=torch.bfloat16)
    return w


def check(o, lse, ro, rl, what):
    o, lse = o.float().cpu(), lse.cpu()
    fin = torch.isfinite(rl)
    rel, mabs = rel_mae(o, ro), float((o.double() - ro).abs().max())
    lerr = float((lse[fin].double() - rl[fin]).abs().max()) if fin.any() else 0.0
    print(f"{what}: rel-MAE {rel:.2e}, max-abs {mabs:.2e}, lse {lerr:.1e}")
    assert torch.isfinite(o).all() and torch.equal(torch.isneginf(lse), torch.isneginf(rl)) and not torch.isnan(lse).any()
    assert rel < 6e-3 and mabs < 5e-2 and lerr < 2e-3, (what, rel, mabs, lerr)


CASES = [
    ([1], [1], 1, True, ""),
    ([129, 64, 1, 0], [129, 64, 1, 0], 2, True, ""),      # crossed row tile, exact KV tile, single token, empty request
    ([5, 130], [133, 194], 2, True, ""),                  # bottom-right offset with a prefix
    ([33, 128], [200, 0], 2, False, ""),                  # second request: empty KV -> 0 / -inf
    ([40], [8], 1, True, ""),                             # rows 0..31 see no key
    ([257], [257], 16, True, "strided"),                  # v = kv[..., 128:], q a view of [T, H * 192], as the reference passes them
    ([70], [200], 1, False, "rescale"),                   # q x 8, keys sorted by score: the row maximum rises tile after tile
]


@pytest.mark.parametrize("qo_lens,kv_lens,H,causal,variant", CASES)
def test_prefill_matches_fp64(qo_lens, kv_lens, H, causal, variant):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7 + len(qo_lens) + sum(kv_lens))
    Tq, Tk = sum(qo_lens), sum(kv_lens)
    q = torch.randn(Tq, H * 192, generator=g).to(torch.bfloat16)
    k = torch.randn(Tk, H, 192, generator=g).to(torch.bfloat16)
    kv = torch.randn(Tk, H, 256, generator=g).to(torch.bfloat16)
    if variant == "rescale":
        q = (q.float() * 8).to(torch.bfloat16)
        k = k[torch.argsort(k[:, 0].float() @ q[0].float())]
    qd, kd, kvd = q.to(dev).view(Tq, H, 192), k.to(dev), kv.to(dev)
    vd = kvd[..., 128:] if variant == "strided" else kvd[..., 128:].contiguous()
    o, lse = planned(qo_lens, kv_lens, H, dev).forward_return_lse(qd, kd, vd, causal=causal, sm_scale=SCALE)
    torch.cuda.synchronize()
    assert o.shape == (Tq, H, 128) and o.dtype == torch.bfloat16 and lse.shape == (Tq, H) and lse.dtype == torch.float32
    ro, rl = ref_attention(q.view(Tq, H, 192), k, kv[..., 128:], qo_lens, kv_lens, causal)
    check(o, lse, ro, rl, f"prefill {qo_lens} x {kv_lens} H={H} causal={causal} {variant}")


def test_chunked_prefix_composition_equals_causal_attention_over_the_whole_context():
    """chunker.py:281-312 + deepseek_v2.py:1037-1071: causal attention over the new tokens, merged with non-causal attention over each
    prefix chunk.  Request 1's prefix ends inside chunk A (chunk B is empty for it), request 2 has no prefix at all."""
    import flashinfer

    dev, H = torch.device("cuda:0"), 2
    new, chunk_a, chunk_b = [70, 33, 5], [100, 40, 0], [50, 0, 0]
    g = torch.Generator().manual_seed(11)
    mk = lambda T, D: torch.randn(T, H, D, generator=g).to(torch.bfloat16)
    q, kn, vn = mk(sum(new), 192), mk(sum(new), 192), mk(sum(new), 128)
    ka, va, kb, vb = mk(sum(chunk_a), 192), mk(sum(chunk_a), 128), mk(sum(chunk_b), 192), mk(sum(chunk_b), 128)
    qd = q.to(dev)
    o, s = planned(new, new, H, dev).forward_return_lse(qd, kn.to(dev), vn.to(dev), causal=True, sm_scale=SCALE)
    for lens, kc, vc in ((chunk_a, ka, va), (chunk_b, kb, vb)):
        oc, sc = planned(new, lens, H, dev).forward_return_lse(qd, kc.to(dev), vc.to(dev), causal=False, sm_scale=SCALE)
        o, s = flashinfer.merge_state(o, s, oc, sc)
    torch.cuda.synchronize()
    # the whole context of every request: [chunk A; chunk B; new]
    cat = lambda a, b, n: torch.cat([torch.cat(t) for t in zip(a.split(chunk_a), b.split(chunk_b), n.split(new))])
    total = [x + y + z for x, y, z in zip(chunk_a, chunk_b, new)]
    ro, rl = ref_attention(q, cat(ka, kb, kn), cat(va, vb, vn), new, total, True)
    check(o, s, ro, rl, "chunked prefix")


def test_unsupported_calls_are_refused_at_run():
    dev = torch.device("cuda:0")
    q, k, v = (torch.zeros(4, 16, d, dtype=torch.bfloat16, device=dev) for d in (192, 192, 128))
    w = planned([4], [4], 16, dev)
    with pytest.raises(RuntimeError):
        w.forward(q, k, v, causal=True, logits_soft_cap=30.0)
    with pytest.raises(RuntimeError):
        w.forward(q.half(), k, v, causal=True)
    with pytest.raises(RuntimeError):
        planned([4], [4], 16, dev, num_kv_heads=1).forward(q, k[:, :1], v[:, :1], causal=True)
