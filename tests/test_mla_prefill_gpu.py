"""GPU: absorbed paged MLA attention (576/512, bf16, page size 1; csrc/mla_prefill_bf16.hip) through the public interface,
`flashinfer.BatchMLAPagedAttentionWrapper`, against a plain fp64 statement on the CPU computed from the same bf16 inputs:
s = scale (q_nope . ckv[slot] + q_pe . kpe[slot]), o = softmax(s + mask) ckv[slot], lse in base 2, a row without a visible key = 0 / -inf.
Shapes sit on the kernel's tile edges (R = 64 flattened (token, head) rows per workgroup, 16 per wave; K = 32 KV tokens per tile); every
case gathers through shuffled indices into a pool larger than its KV.  Bounds: the project's own for this arithmetic (bf16 operands, fp32
accumulation, bf16 P, bf16 output; tests/test_mla_gpu.py, tests/test_prefill_gpu.py): rel-MAE < 6e-3, max-abs < 5e-2, finite lse within
2e-3, -inf positions exactly equal, no NaN."""
import pytest
import torch

from helpers import rel_mae

pytestmark = pytest.mark.gpu
SCALE = 192 ** -0.5
LN2 = 0.6931471805599453
R, K = 64, 32


def ref_mla(qn, qp, ckv, kpe, q_lens, kv_lens, slots, causal):
    """fp64: (o [T, H, 512], lse [T, H] base 2); slots[b] = the request's key slots in order; causal is bottom-right aligned"""
    q = torch.cat([qn, qp], -1).double()
    kv = torch.cat([ckv, kpe], -1).double()
    o = torch.zeros(q.shape[0], q.shape[1], 512, dtype=torch.float64)
    lse = torch.full(q.shape[:2], float("-inf"), dtype=torch.float64)
    qs = 0
    for ql, kl, sl in zip(q_lens, kv_lens, slots):
        if ql and kl:
            k = kv[sl[:kl]]
            s = torch.einsum("ihd,jd->hij", q[qs:qs + ql], k) * SCALE
            if causal:
                s.masked_fill_(torch.arange(kl)[None, :] > torch.arange(ql)[:, None] + (kl - ql), float("-inf"))
            o[qs:qs + ql] = torch.einsum("hij,jd->ihd", torch.softmax(s, -1).nan_to_num(0.0), k[:, :512])
            lse[qs:qs + ql] = (torch.logsumexp(s, -1) / LN2).t()
        qs += ql
    return o, lse


def i32(x, dev):
    return torch.as_tensor(x, dtype=torch.int32).to(dev)


def indptr(lens):
    return torch.tensor([0] + list(lens)).cumsum(0)


def make_case(q_lens, kv_lens, H, seed, span_extra=0, variant=""):
    """bf16 inputs on the CPU; kv_indptr spans kv_len + span_extra entries per request (the surplus points at other live slots)"""
    g = torch.Generator().manual_seed(seed)
    T, spans = sum(q_lens), [k + span_extra for k in kv_lens]
    N = sum(spans) + 37
    q = torch.randn(T, H, 576, generator=g).to(torch.bfloat16)
    pool = torch.randn(N, 1, 576, generator=g).to(torch.bfloat16)
    perm = torch.randperm(N, generator=g)[:sum(spans)]
    slots = list(perm.split(spans))
    if variant == "rescale":   # q x 8, keys in rising order of their score against row (0, 0): the maximum rises tile after tile
        q = (q.float() * 8).to(torch.bfloat16)
        slots = [sl[torch.argsort(pool[sl, 0].float() @ q[0, 0].float())] for sl in slots]
    return q, pool, slots, spans


def check(o, lse, ro, rl, what):
    o, lse = o.float().cpu(), lse.cpu()
    fin = torch.isfinite(rl)
    rel = rel_mae(o, ro) if float(ro.abs().sum()) > 0 else float(o.abs().sum())
    mabs = float((o.double() - ro).abs().max())
    lerr = float((lse[fin].double() - rl[fin]).abs().max()) if fin.any() else 0.0
    print(f"{what}: rel-MAE {rel:.2e}, max-abs {mabs:.2e}, lse {lerr:.1e}")
    assert torch.isfinite(o).all() and torch.equal(torch.isneginf(lse), torch.isneginf(rl)) and not torch.isnan(lse).any()
    assert rel < 6e-3 and mabs < 5e-2 and lerr < 2e-3, (what, rel, mabs, lerr)


CASES = [
    ("a", [1], [1], 1, True, ""),                                      # a single pair
    ("b", [R // 16 + 1, 4, 1, 0], [R // 16 + 1, 4, 1, 0], 16, True, ""),   # tile crossing a token, exact tile, single token, empty request
    ("c", [3, 5], [K + 2, 2 * K + 1], 128, True, ""),                  # several row tiles per token; prefix offset
    ("d", [7], [3 * K], 24, True, ""),                                 # H divides neither R nor the wave's rows
    ("e", [6], [2], 16, True, ""),                                     # tokens 0..3 see no key -> 0 / -inf
    ("f", [1, 1, 1], [K, 1, 2 * K + 5], 16, False, ""),                # the decode form
    ("g", [9], [K + 7], 16, True, "views"),                            # operands as views of fused buffers; out= a caller tensor
    ("h", [3], [6 * K], 16, False, "rescale"),                         # the row maximum rises tile after tile
    ("i", [5], [K + 3], 16, True, "short"),                            # kv_len_arr smaller than the indptr span
]


@pytest.mark.parametrize("name,q_lens,kv_lens,H,causal,variant", CASES)
def test_mla_prefill_matches_fp64(name, q_lens, kv_lens, H, causal, variant):
    import flashinfer

    dev = torch.device("cuda:0")
    q, pool, slots, spans = make_case(q_lens, kv_lens, H, 100 + ord(name), span_extra=9 if variant == "short" else 0, variant=variant)
    T = sum(q_lens)
    qd, pd = q.to(dev), pool.to(dev)
    if variant == "views":
        qn, qp, ckv, kpe = qd[..., :512], qd[..., 512:], pd[..., :512], pd[..., 512:]
    else:
        qn, qp, ckv, kpe = qd[..., :512].contiguous(), qd[..., 512:].contiguous(), pd[:, 0, :512].contiguous(), pd[:, 0, 512:].contiguous()
    w = flashinfer.BatchMLAPagedAttentionWrapper(torch.empty(16, dtype=torch.uint8, device=dev), backend="auto")
    w.plan(i32(indptr(q_lens), dev), i32(indptr(spans), dev), i32(torch.cat(slots), dev), i32(kv_lens, dev), H, 512, 64, 1, causal,
           SCALE, torch.bfloat16, torch.bfloat16)
    out = torch.full((T, H, 512), float("nan"), dtype=torch.bfloat16, device=dev) if variant == "views" else None
    o, lse = w.run(qn, qp, ckv, kpe, out=out, return_lse=True)
    torch.cuda.synchronize()
    assert o.shape == (T, H, 512) and o.dtype == torch.bfloat16 and lse.shape == (T, H) and lse.dtype == torch.float32
    assert out is None or o is out
    ro, rl = ref_mla(q[..., :512], q[..., 512:], pool[:, 0, :512], pool[:, 0, 512:], q_lens, kv_lens, slots, causal)
    check(o, lse, ro, rl, f"mla prefill {name} {q_lens} x {kv_lens} H={H} causal={causal} {variant}")


def test_graph_replay_reads_the_next_plan():
    """use_cuda_graph=True: `run` captured under plan A (one launch on one stream: one kernel node, no branches), replayed after plan B
    (same T and B, other lengths and indices) = fp64 of B, replay after replay"""
    import flashinfer

    dev, H = torch.device("cuda:0"), 16
    ql_a, kl_a, ql_b, kl_b = [5, 3], [K + 5, 3], [2, 6], [9, 2 * K + 2]
    q, pool, slots_a, _ = make_case(ql_a, kl_a, H, 7)
    slots_b = list(torch.randperm(pool.shape[0], generator=torch.Generator().manual_seed(8))[:sum(kl_b)].split(kl_b))
    qd, pd = q.to(dev), pool.to(dev)
    qn, qp, ckv, kpe = qd[..., :512], qd[..., 512:], pd[..., :512], pd[..., 512:]
    bufs = dict(qo_indptr=torch.zeros(3, dtype=torch.int32, device=dev), kv_indptr=torch.zeros(3, dtype=torch.int32, device=dev),
                kv_indices=torch.zeros(256, dtype=torch.int32, device=dev), kv_len_arr=torch.zeros(2, dtype=torch.int32, device=dev))
    w = flashinfer.BatchMLAPagedAttentionWrapper(torch.empty(16, dtype=torch.uint8, device=dev), use_cuda_graph=True, backend="auto", **bufs)
    out, lse = torch.zeros(8, H, 512, dtype=torch.bfloat16, device=dev), torch.zeros(8, H, dtype=torch.float32, device=dev)

    def plan(q_lens, kv_lens, slots):
        w.plan(i32(indptr(q_lens), dev), i32(indptr(kv_lens), dev), i32(torch.cat(slots), dev), i32(kv_lens, dev), H, 512, 64, 1, True,
               SCALE, torch.bfloat16, torch.bfloat16)

    plan(ql_a, kl_a, slots_a)
    w.run(qn, qp, ckv, kpe, out=out, lse=lse)   # warm-up outside the capture
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        w.run(qn, qp, ckv, kpe, out=out, lse=lse)
    plan(ql_b, kl_b, slots_b)
    ro, rl = ref_mla(q[..., :512], q[..., 512:], pool[:, 0, :512], pool[:, 0, 512:], ql_b, kl_b, slots_b, True)
    for i in range(2):
        out.zero_()
        gr.replay()
        torch.cuda.synchronize()
        check(out, lse, ro, rl, f"graph replay {i} under plan B")


def test_unsupported_calls_are_refused_at_run():
    import flashinfer

    dev, H = torch.device("cuda:0"), 16
    q = torch.zeros(2, H, 576, dtype=torch.bfloat16, device=dev)
    pool = torch.zeros(8, 1, 576, dtype=torch.bfloat16, device=dev)
    ops = (q[..., :512], q[..., 512:], pool[..., :512], pool[..., 512:])

    def planned(page_size=1, dim=512, dtype=torch.bfloat16):
        w = flashinfer.BatchMLAPagedAttentionWrapper(torch.empty(16, dtype=torch.uint8, device=dev), backend="auto")
        w.plan(i32([0, 2], dev), i32([0, 2], dev), i32([3, 5], dev), i32([2], dev), H, dim, 64, page_size, True, SCALE, dtype, torch.bfloat16)
        return w

    with pytest.raises(RuntimeError):
        planned(page_size=64).run(*ops)
    with pytest.raises(RuntimeError):
        planned().run(ops[0].half(), ops[1].half(), *ops[2:])
    with pytest.raises(RuntimeError):
        planned(dim=256).run(q[..., :256], q[..., 512:], pool[..., :256], pool[..., 512:])
    with pytest.raises(RuntimeError):
        planned().run(*ops, kv_len=i32([2], dev))
    with pytest.raises(RuntimeError):
        flashinfer.BatchMLAPagedAttentionWrapper(torch.empty(16, dtype=torch.uint8, device=dev), backend="auto").run(*ops)
