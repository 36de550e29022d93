"""GPU: flashinfer.sampling (csrc/sampling.hip) against plain fp64 statements on the CPU computed from the same f32 inputs.
Keep rules (p(k) the k-th largest value, S the row sum, M(x) = sum{p_j : p_j > x}): top-k keeps p_i >= p(k) (ties kept, k >= V all);
top-p keeps M(p_i) < top_p * S_base (top_p >= 1: everything positive); "joint" intersects both on the input row; "top_k_first" runs top-p
on the top-k survivors; min-p keeps p_i >= min_p * max p (one f32 multiply).  Every top_p is CONSTRUCTED half-way between two breakpoints
of the descending cumulative mass (>= 5e-5 from either, ~50 x the fp32 summation error), so the kept SET is exact and compared exactly.
Bounds: kept values within 2e-6 relative of p_i / S_kept (an fp32 sum of <= 129,280 non-negative terms plus one division); a sampled id r
satisfies C_kept(r-1) - eps <= u S_kept <= C_kept(r) + eps, eps = 1e-5 S_kept; softmax within 1e-6 absolute.
Worst measured on MI355X: renormalised values 1.6e-7 relative (top-k) and 1.9e-7 (top-p); no sample outside its bracket (slack 0, from
u = 0); softmax 1.3e-7 absolute."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
#        V, B, sigma, columns of the buffer the rows are a view of
CASES = {"a": (33, 3, 3.0, 33), "b": (4099, 5, 3.0, 4099), "c": (4096, 300, 3.0, 4096), "d": (129280, 2, 3.0, 129280),
         "flat": (4099, 5, 0.3, 4099), "strided": (4098, 5, 3.0, 4103)}
KS = (1, 2, 50, None, 1 << 30)     # None -> V
RANKS = (1, 2, 17, None)           # None -> the last rank with p(j) >= 1e-4
MIN_PS = (0.0, 0.05, 1.0)


@functools.lru_cache(maxsize=None)
def case(name):
    """f32 probs [B, V] on the CPU (a view of a [B, cols] buffer) with its fp64 descending order, per-row top_k, constructed top_p, min_p"""
    V, B, sigma, cols = CASES[name]
    g = torch.Generator().manual_seed(1000 + sum(map(ord, name)))
    buf = torch.zeros(B, cols)
    buf[:, :V] = torch.softmax(sigma * torch.randn(B, V, generator=g), -1)
    probs = buf[:, :V]
    srt = probs.double().sort(-1, descending=True).values
    top_k = torch.tensor([V if KS[b % 5] is None else KS[b % 5] for b in range(B)], dtype=torch.int32)
    keep_k = probs >= srt.gather(1, (top_k.long().clamp(max=V) - 1)[:, None]).float()
    min_p = torch.tensor([MIN_PS[b % 3] for b in range(B)], dtype=torch.float32)
    keep_m = probs >= (min_p * probs.max(-1).values)[:, None]           # one f32 multiply
    return dict(probs=probs, buf=buf, srt=srt, top_k=top_k, keep_k=keep_k, min_p=min_p, keep_m=keep_m)


def constructed_top_p(c, s_base=None, cap=None):
    """per row: rank j from RANKS (capped by `cap`), top_p = (C(j) - p(j) / 2) / s_base -> (f32 top_p [B], keep mask = ranks 1..j and ties)"""
    srt, probs = c["srt"], c["probs"]
    B, V = probs.shape
    C = srt.cumsum(-1)
    last = (srt >= 1e-4).sum(-1)
    ranks = [RANKS[(b + (2 if B < 4 else 0)) % 4] for b in range(B)]          # few rows: start at the deep ranks
    j = torch.tensor([int(last[b]) if ranks[b] is None else min(ranks[b], V) for b in range(B)])
    if cap is not None:
        j = torch.minimum(j, cap.long().clamp(max=V))
    pj = srt.gather(1, (j - 1)[:, None])[:, 0]
    nxt = srt.gather(1, j.clamp(max=V - 1)[:, None])[:, 0]
    assert (pj / 2 >= 5e-5).all() and ((nxt != pj) | (j == V)).all()   # the cut is decidable in fp32
    top_p = (C.gather(1, (j - 1)[:, None])[:, 0] - pj / 2) / (1.0 if s_base is None else s_base)
    assert (top_p < 1 - 1e-5).all()
    return top_p.float(), probs >= pj.float()[:, None]


def dev_rows(c):
    buf = c["buf"].cuda()
    return buf[:, :c["probs"].shape[1]]


def check_renorm(out, c, keep, what):
    out, p = out.cpu(), c["probs"].double()
    ref = torch.where(keep, p, 0.0) / torch.where(keep, p, 0.0).sum(-1, keepdim=True)
    assert out.dtype == torch.float32 and torch.equal(out != 0, keep), f"{what}: kept set differs in {int(((out != 0) != keep).sum())} places"
    rel = float(((out.double() - ref).abs()[keep] / ref[keep]).max())
    print(f"{what}: worst relative error of a kept value {rel:.2e}")
    assert rel <= 2e-6, (what, rel)


@pytest.mark.parametrize("name", CASES)
def test_top_k_renorm(name):
    from flashinfer.sampling import top_k_renorm_probs

    c = case(name)
    check_renorm(top_k_renorm_probs(dev_rows(c), c["top_k"].cuda()), c, c["keep_k"], f"top_k_renorm {name}")


@pytest.mark.parametrize("name", CASES)
def test_top_p_renorm(name):
    from flashinfer.sampling import top_p_renorm_probs

    c = case(name)
    top_p, keep = constructed_top_p(c)
    top_p[-1], keep[-1] = 1.0, c["probs"][-1] > 0          # top_p = 1 keeps everything positive
    check_renorm(top_p_renorm_probs(dev_rows(c), top_p.cuda()), c, keep, f"top_p_renorm {name}")


def filters(c, mode):
    """(kwargs of fluent_mi355.sampling.sample on the CPU, keep mask)"""
    if mode == "top_k":
        return dict(top_k=c["top_k"]), c["keep_k"]
    if mode == "top_p":
        top_p, keep = constructed_top_p(c)
        return dict(top_p=top_p), keep
    if mode == "joint":
        top_p, keep = constructed_top_p(c)
        return dict(top_k=c["top_k"], top_p=top_p, order="joint"), keep & c["keep_k"]
    if mode == "top_k_first":
        s_k = torch.where(c["keep_k"], c["probs"].double(), 0.0).sum(-1)
        top_p, keep = constructed_top_p(c, s_base=s_k, cap=c["top_k"])
        return dict(top_k=c["top_k"], top_p=top_p, order="top_k_first"), keep & c["keep_k"]
    return dict(min_p=c["min_p"]), c["keep_m"]


def check_ids(ids, rows, u, c, keep, what):
    """every id is kept and brackets u S_kept in the fp64 running kept mass (vocabulary order)"""
    assert ids.dtype == torch.int32
    ids, rows, u = ids.cpu().long(), rows.long(), u.double()
    assert ids.shape == rows.shape and (ids >= 0).all() and (ids < keep.shape[1]).all()
    assert keep[rows, ids].all(), f"{what}: {int((~keep[rows, ids]).sum())} ids outside the kept set"
    Ck = torch.where(keep, c["probs"].double(), 0.0).cumsum(-1)
    S = Ck[rows, -1]
    hi, lo = Ck[rows, ids], torch.where(ids > 0, Ck[rows, (ids - 1).clamp(min=0)], 0.0)
    slack = float((torch.maximum(lo - u * S, u * S - hi) / S).max())
    print(f"{what}: worst CDF slack {slack:.2e} of S_kept")
    assert slack <= 1e-5, (what, slack)
    first = keep.long().argmax(-1)
    assert torch.equal(ids[u == 0], first[rows[u == 0]])                       # u = 0 returns the first kept index


@pytest.mark.parametrize("mode", ["top_k", "top_p", "joint", "top_k_first", "min_p"])
@pytest.mark.parametrize("name", CASES)
def test_sample_with_explicit_u(name, mode):
    from fluent_mi355.sampling import sample

    c = case(name)
    kw, keep = filters(c, mode)
    B = c["probs"].shape[0]
    g = torch.Generator().manual_seed(7)
    u1 = torch.cat([torch.tensor([0.0, 1 - 2.0 ** -24, 0.5]), torch.rand(257, generator=g)])
    used = torch.arange(min(B, 5))                                             # many samples onto few rows, through `indices`
    rows, u = used.repeat_interleave(u1.numel()), u1.repeat(used.numel())
    ids = sample(dev_rows(c), u.cuda(), indices=rows.int().cuda(), **{k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()})
    check_ids(ids, rows, u, c, keep, f"sample {name} {mode}")
    if "top_k" in kw:                                                          # top_k = 1: the argmax for every u
        one = c["top_k"][rows] == 1
        assert one.any() and torch.equal(ids.cpu().long()[one], c["probs"].argmax(-1)[rows[one]])


def test_public_interface_as_the_sampler_calls_it():
    from flashinfer.sampling import min_p_sampling_from_probs, softmax, top_k_top_p_sampling_from_probs

    c = case("c")
    B, V = c["probs"].shape
    probs, rows = dev_rows(c), torch.arange(B)
    top_ps, keep_p = constructed_top_p(c)
    top_ks, min_ps = c["top_k"].cuda(), c["min_p"].cuda()                      # int32 holding 1 << 30; f32
    assert top_ks.dtype == torch.int32 and int(top_ks.max()) == 1 << 30

    def gen(seed):
        return torch.Generator(device="cuda").manual_seed(seed)

    a = top_k_top_p_sampling_from_probs(probs, top_ks, top_ps.cuda(), filter_apply_order="joint", generator=gen(3))
    a2 = top_k_top_p_sampling_from_probs(probs, top_ks, top_ps.cuda(), filter_apply_order="joint", generator=gen(3))
    a3 = top_k_top_p_sampling_from_probs(probs, top_ks, top_ps.cuda(), filter_apply_order="joint", generator=gen(4))
    m = min_p_sampling_from_probs(probs, min_ps, generator=gen(3))
    for ids, keep in ((a, keep_p & c["keep_k"]), (m, c["keep_m"])):
        assert ids.dtype == torch.int32 and ids.shape == (B,) and keep[rows, ids.cpu().long()].all()
    assert torch.equal(a, a2) and not torch.equal(a, a3)

    # one captured launch with its torch.rand: fresh uniforms and kept ids on every replay
    top_k_top_p_sampling_from_probs(probs, top_ks, top_ps.cuda(), filter_apply_order="joint")
    torch.cuda.synchronize()
    tp = top_ps.cuda()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        ids = top_k_top_p_sampling_from_probs(probs, top_ks, tp, filter_apply_order="joint")
    for _ in range(2):
        ids.fill_(-1)
        gr.replay()
        torch.cuda.synchronize()
        assert (keep_p & c["keep_k"])[rows, ids.cpu().long()].all()

    g = torch.Generator().manual_seed(11)
    logits = 3.0 * torch.randn(6, 4099, generator=g)
    logits[2] = float("-inf")
    temps = 0.5 + 1.5 * torch.rand(6, generator=g)
    out = softmax(logits.cuda(), temps.cuda().view(-1, 1)).cpu()
    ref = torch.softmax(logits.double() / temps.double()[:, None], -1).nan_to_num(0.0)
    err = float((out.double() - ref).abs().max())
    print(f"softmax: worst absolute error {err:.2e}")
    assert err <= 1e-6 and torch.equal(out[2], torch.zeros(4099))


def test_refusals():
    from flashinfer.sampling import min_p_sampling_from_probs, top_k_renorm_probs, top_k_top_p_sampling_from_probs

    probs = torch.softmax(torch.randn(4, 64), -1)
    with pytest.raises(RuntimeError):
        top_k_top_p_sampling_from_probs(probs.cuda().bfloat16(), 5, 0.9)
    with pytest.raises(RuntimeError):
        top_k_top_p_sampling_from_probs(probs, 5, 0.9)
    with pytest.raises(RuntimeError):
        top_k_renorm_probs(probs.cuda(), torch.full((3,), 5, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError):
        top_k_top_p_sampling_from_probs(probs.cuda(), 5, 0.9, filter_apply_order="bogus")
    probs[1, 7] = float("nan")
    with pytest.raises(ValueError):
        min_p_sampling_from_probs(probs.cuda(), 0.1, check_nan=True)
