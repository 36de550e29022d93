"""GPU: speculative chain verification (csrc/spec_verify.hip) against fp64 loops on the CPU over the same inputs.
Accept decisions are exact: every coin is built a factor 2 away from its threshold (asserted on the reference).  The final token t must have
weight w_t = max(q - p, 0) > 0, must not be the rejected token, and must bracket u * sum(w) in the fp64 running weight (vocabulary order)
within 1e-5 of sum(w) — the bound tests/test_sampling_gpu.py applies to the sampler's inverse CDF (an f32 sum of <= 129,280 non-negative terms)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
SENTINEL = -7


def run(fn, cand, *inputs, A=None, **kw):
    """calls fn on the device with sentinel-filled outputs -> (predicts, accept_index, accept_token_num) on the CPU"""
    B, D = cand.shape
    pred = torch.full((B * D,), SENTINEL, dtype=torch.int32, device="cuda")
    ai = torch.full((B, D + 1 if A is None else A), -1, dtype=torch.int32, device="cuda")
    num = torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda")
    fn(pred, ai, num, cand.cuda(), *[t.cuda() for t in inputs], **kw)
    return pred.cpu(), ai.cpu(), num.cpu()


def check_accepted(out, n, accepted_pred):
    """n, the whole accept_index and the accepted predicts are exact; everything else keeps its fill value"""
    pred, ai, num = out
    B, D = len(n), pred.numel() // len(n)
    assert num.tolist() == n
    for b in range(B):
        assert ai[b].tolist() == [b * D + j for j in range(n[b] + 1)] + [-1] * (ai.shape[1] - n[b] - 1)
        assert pred[b * D:b * D + n[b]].tolist() == accepted_pred[b][:n[b]]
        assert (pred[b * D + n[b] + 1:(b + 1) * D] == SENTINEL).all() and pred[b * D + n[b]] != SENTINEL


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("B,D", [(1, 2), (3, 4), (65, 8)])
def test_greedy(B, D, dtype):
    from flashinfer.sampling import verify_chain_greedy

    g = torch.Generator().manual_seed(B * 100 + D)
    tp = torch.randint(0, 1000, (B, D), generator=g)
    cand = torch.randint(0, 1000, (B, D), generator=g)
    for b in range(B):
        m = (D - 1, 0, (D - 1) // 2)[b % 3]                     # matching prefix, then a sure mismatch
        cand[b, 1:m + 1] = tp[b, :m]
        if m + 1 < D:
            cand[b, m + 1] = tp[b, m] + 1
    n, want = [], []
    for b in range(B):                                          # the rule, as a plain loop
        last = 0
        for j in range(1, D):
            if cand[b, j] != tp[b, last]:
                break
            last = j
        n.append(last)
        want.append(tp[b, :last + 1].tolist())
    assert {0, D - 1, (D - 1) // 2} <= set(n) or B == 1
    out = run(verify_chain_greedy, cand.int(), tp.to(dtype), batch_size=B, num_draft_tokens=D)
    check_accepted(out, n, want)
    assert all(out[0][b * D + n[b]] == want[b][n[b]] for b in range(B))


@functools.lru_cache(maxsize=None)
def case(V, D, draft):
    """B = 6 requests on the CPU with the fp64 reference: accepted prefixes 0 / D-1 / middle, candidates = the target's argmax"""
    B = 6
    g = torch.Generator().manual_seed(V + 10 * D)
    q = torch.softmax(3.0 * torch.randn(B, D, V, generator=g), -1)
    p = torch.zeros_like(q) if draft == "zero" else q * torch.where(torch.rand(B, D, V, generator=g) < 0.5, 0.5, 1.5)
    cand = torch.cat([torch.zeros(B, 1, dtype=torch.long), q[:, :-1].argmax(-1)], 1).int()
    pt = q[:, :-1].gather(2, cand[:, 1:, None].long())[..., 0].double()         # [B, D-1]
    n = [(D - 1, 0, (D - 1) // 2)[b % 3] for b in range(B)]
    coins = torch.rand(B, D, generator=g)
    for b in range(B):
        coins[b, :D - 1] = (pt[b] * torch.where(torch.arange(D - 1) < n[b], 0.5, 2.0)).float()
    ratio = coins[:, :D - 1].double() / pt
    assert (((ratio - 0.5).abs() < 1e-6) | ((ratio - 2).abs() < 1e-6)).all() and (pt < 0.99).all() and (pt > 1e-4).all()   # decidable in f32, far below threshold_single = 1
    w = q.double()[torch.arange(B), n] - torch.stack([p[b, n[b]].double() if n[b] < D - 1 else torch.zeros(V, dtype=torch.float64) for b in range(B)])
    w = w.clamp(min=0)
    rej = [int(cand[b, n[b] + 1]) if n[b] < D - 1 else -1 for b in range(B)]
    for b in range(B):
        if rej[b] >= 0:
            w[b, rej[b]] = 0
    u = torch.rand(B, generator=g)
    u[0], u[1] = 0.0, 1 - 2.0 ** -24
    return dict(q=q, p=p, cand=cand, coins=coins, u=u, n=n, w=w, rej=rej)


def check_final(pred, c, u):
    B, D = c["cand"].shape
    t = torch.tensor([int(pred[b * D + c["n"][b]]) for b in range(B)])
    w, rows = c["w"], torch.arange(B)
    assert (t >= 0).all() and (t < w.shape[1]).all() and (w[rows, t] > 0).all() and all(int(t[b]) != c["rej"][b] for b in range(B))
    C = w.cumsum(-1)
    S, hi, lo = C[:, -1], C[rows, t], torch.where(t > 0, C[rows, (t - 1).clamp(min=0)], 0.0)
    slack = float((torch.maximum(lo - u.double() * S, u.double() * S - hi) / S).max())
    print(f"worst CDF slack {slack:.2e} of sum(w)")
    assert slack <= 1e-5, slack
    first = (w > 0).long().argmax(-1)
    assert torch.equal(t[u == 0], first[u == 0])                # u = 0: the first index with positive weight


@pytest.mark.parametrize("draft", ["zero", "mixed"])
@pytest.mark.parametrize("D", [2, 5])
@pytest.mark.parametrize("S", [1, 3, 7, "empty"])
@pytest.mark.parametrize("V", [4099, 129280])
def test_sample(V, S, D, draft):
    from fluent_mi355.sampling import chain_speculative_sampling

    c = case(V, D, draft)
    assert {0, D - 1, (D - 1) // 2} == set(c["n"])
    S = V // 2048 + 3 if S == "empty" else S                     # more slices than 2,048-element load granules: some are empty
    dp = c["p"].cuda()
    out = run(chain_speculative_sampling, c["cand"], c["coins"], c["u"], c["q"], dp, num_slices=S)
    assert torch.equal(dp.cpu(), c["p"])                        # draft_probs is only read
    check_accepted(out, c["n"], [c["cand"][b, 1:].tolist() for b in range(6)])
    check_final(out[0], c, c["u"])


def test_thresholds_and_edge_cases():
    from flashinfer.sampling import chain_speculative_sampling_target_only

    B, D, V = 5, 3, 64
    q = torch.full((B, D, V), 0.4 / 62)
    q[:, :, 5], q[:, :, 9] = 0.4, 0.2
    cand = torch.tensor([[0, 5, 9], [0, 9, 5], [0, V, 5], [0, -1, 5], [0, 5, 9]], dtype=torch.int32)
    # request 0: pt = 0.4 >= 0.3 with coin 0.95 > 0.4 / 0.5, then pt = 0.2 < 0.3 with 0.2 < coin 0.3 < 0.2 / 0.5: both accepted
    # request 1: pt = 0.2 with coin 0.45 > 0.4: rejected.  2, 3: candidate out of range.  4: accepted once, then weights all zero
    coins = torch.tensor([[0.95, 0.3, 0], [0.45, 0, 0], [0, 0, 0], [0, 0, 0], [0.1, 0.9, 0]])
    p = torch.zeros(B, D, V)
    p[4, 1] = q[4, 1]
    out = run(chain_speculative_sampling_target_only, cand, coins, torch.full((B,), 0.5), q, p, threshold_single=0.3, threshold_acc=0.5)
    check_accepted(out, [2, 0, 0, 0, 1], [[5, 9], [], [], [], [5]])
    assert out[0][4 * D + 1] == 0                               # every weight zero: token 0
    assert out[0][1 * D] != 9 and 0 <= out[0][2 * D] < V        # the rejected token is never drawn


def test_graph_replays_equal_eager():
    from fluent_mi355.sampling import chain_speculative_sampling

    c = case(4099, 5, "mixed")
    B, D = c["cand"].shape
    dev = [c[k].cuda() for k in ("cand", "coins", "u", "q", "p")]
    outs = [torch.full((B * D,), SENTINEL, dtype=torch.int32, device="cuda"), torch.full((B, D), -1, dtype=torch.int32, device="cuda"),
            torch.zeros(B, dtype=torch.int32, device="cuda")]
    chain_speculative_sampling(*outs, *dev, num_slices=3)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        chain_speculative_sampling(*outs, *dev, num_slices=3)
    g = torch.Generator().manual_seed(5)
    for _ in range(2):
        coins = c["coins"] * torch.where(torch.rand(B, D, generator=g) < 0.5, 1.0, 4.0)      # other accept patterns, still decidable
        u = torch.rand(B, generator=g)
        dev[1].copy_(coins.cuda()); dev[2].copy_(u.cuda())
        for o, fill in zip(outs, (SENTINEL, -1, 0)):
            o.fill_(fill)
        gr.replay()
        torch.cuda.synchronize()
        eager = run(chain_speculative_sampling, c["cand"], coins, u, c["q"], c["p"], A=D, num_slices=3)
        assert all(torch.equal(o.cpu(), e) for o, e in zip(outs, eager))


def test_refusals():
    from flashinfer.sampling import chain_speculative_sampling_target_only as sample, verify_chain_greedy

    def args(B=2, D=3, V=64, A=None, dtype=torch.float32, device="cuda"):
        z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=device)
        return [z(B * D), z(B, D if A is None else A), z(B), z(B, D), z(B, D, dt=torch.float32), z(B, dt=torch.float32), z(B, D, V, dt=dtype), z(B, D, V, dt=dtype)]

    for bad in (args(device="cpu"), args(dtype=torch.float16), args(A=2), args(D=33)):
        with pytest.raises(RuntimeError):
            sample(*bad)
    for bad in (args(device="cpu"), args(A=2), args(D=33)):
        with pytest.raises(RuntimeError):
            verify_chain_greedy(*bad[:4], bad[3])
    sample(*args())                                             # the same arguments, unspoiled, are served
    torch.cuda.synchronize()
