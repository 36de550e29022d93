"""GPU box: first measurement of flashinfer.sampling (csrc/sampling.hip) at the real vocabulary, V = 129,280, B in {1, 16, 128, 256}:
softmax, top_k_top_p_sampling_from_probs (joint, per-row k and p) and min_p_sampling_from_probs, each beside the same operation as a plain
torch statement (sort -> cumsum -> mask -> multinomial; softmax: torch.softmax) timed in the same run.  us per call from device events
around a window of at least 0.3 s after a warm-up window: hipGraph replays for this library, back-to-back calls on one stream for torch.  Roofline: every byte the operation must move once
(B V 4 in, plus B V 4 out for softmax) at 8 TB/s.  Rows are softmax(3 randn): peaked, like a model's.
usage: python tools/time_sampling.py   (FLUENT_MI355_LIB selects another build of the library)
       python tools/time_sampling.py verify   — instead: the speculative verify step (csrc/spec_verify.hip) as eagle_utils.py:249-289 issues it,
       D = 2 and 4, B = 1 … 256: softmax -> top-k renorm -> top-p renorm -> chain_speculative_sampling_target_only, eager and as one captured
       graph; the chain kernel alone at the chosen number of slices and at 1, 8 and 16 (timed twice each, alternating), the accept /
       final-sample step as a plain torch statement (gather, cumsum, searchsorted), and verify_chain_greedy.  A library built with
       `make SVFLAGS=-DFL_SV_THREADFENCE` (through FLUENT_MI355_LIB) times the cache-wide-fence form of the slice hand-over."""
import os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "sglang-fluentllm_amd"))
import torch
from flashinfer import sampling
dev = torch.device("cuda:0")
HBM, V = 8e12, 129280
class Eager:
    """back to back on the current stream (the torch statements: their sort and multinomial allocate and are not captured)"""
    def __init__(self, fn, calls): self.fn, self.calls = fn, calls
    def replay(self):
        for _ in range(self.calls): self.fn()
def timeit(fn, graph=True, calls=4, window_s=0.3):
    fn(); torch.cuda.synchronize()
    if graph:
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(calls): fn()
    else:
        gr = Eager(fn, calls)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    def window(replays):
        e0.record()
        for _ in range(replays): gr.replay()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (calls * replays)
    us = window(5)   # warm-up: code objects loaded, clocks up; sizes the timed window
    return window(max(5, int(window_s * 1e6 / (us * calls))))
def torch_top_k_top_p(probs, top_ks, top_ps):
    """the keep rules of this library's "joint" order as a plain torch statement"""
    srt, idx = probs.sort(dim=-1, descending=True)
    before = srt.cumsum(dim=-1) - srt
    srt[before >= top_ps.view(-1, 1)] = 0.0
    srt[torch.arange(probs.shape[1], device=probs.device).view(1, -1) >= top_ks.view(-1, 1)] = 0.0
    return idx.gather(1, torch.multinomial(srt, 1)).view(-1).to(torch.int32)
def torch_min_p(probs, min_ps):
    kept = torch.where(probs >= min_ps.view(-1, 1) * probs.max(dim=-1, keepdim=True).values, probs, 0.0)
    return torch.multinomial(kept, 1).view(-1).to(torch.int32)
def torch_chain(cand, coins, u, q, p, thr_single=1.0, thr_acc=1.0):
    """the accept rule and the final sample of chain_speculative_sampling_target_only as a plain torch statement -> (n, final token)"""
    B, D, _ = q.shape
    rows = torch.arange(B, device=q.device)
    pt = q[:, :-1].gather(2, cand[:, 1:, None].long())[..., 0]
    n = ((coins[:, :-1] <= pt / thr_acc) | (pt >= thr_single)).long().cumprod(1).sum(1)
    w = (q[rows, n] - torch.where((n < D - 1)[:, None], p[rows, n], 0.0)).clamp_(min=0)
    rejected = cand.gather(1, (n + 1).clamp(max=D - 1)[:, None])[:, 0].long()
    w[rows, rejected] = torch.where(n < D - 1, 0.0, w[rows, rejected])
    c = w.cumsum(-1)
    return n, torch.searchsorted(c, (u * c[:, -1])[:, None], right=True)[:, 0]
def verify_step():
    from fluent_mi355 import _lib, sampling as s2
    g = torch.Generator(device=dev).manual_seed(0)
    for D in (2, 4):
        for B in (1, 4, 16, 64, 256):
            logits = 3.0 * torch.randn(B * D, V, device=dev, generator=g)
            temps = 0.5 + torch.rand(B * D, 1, device=dev, generator=g)
            top_ks = torch.randint(20, 100, (B * D,), device=dev, generator=g).to(torch.int32)
            top_ps = 0.8 + 0.19 * torch.rand(B * D, device=dev, generator=g)
            q = sampling.top_p_renorm_probs(sampling.top_k_renorm_prob(sampling.softmax(logits, temps), top_ks), top_ps).view(B, D, V)
            p = torch.zeros_like(q)                      # what eagle_utils.py:266 passes
            cand = torch.cat([torch.zeros(B, 1, dtype=torch.int64, device=dev), q[:, :-1].argmax(-1)], 1).to(torch.int32)
            coins, u = torch.rand(B, D, device=dev, generator=g), torch.rand(B, device=dev, generator=g)   # argmax candidates: accepted with the target's own probability
            pred, ai, num = torch.zeros(B * D, dtype=torch.int32, device=dev), torch.full((B, D), -1, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
            tp = q.argmax(-1)
            def chain(S=None): s2.chain_speculative_sampling(pred, ai, num, cand, coins, u, q, p, num_slices=S)
            def step():
                t = sampling.top_p_renorm_probs(sampling.top_k_renorm_prob(sampling.softmax(logits, temps), top_ks), top_ps).view(B, D, V)
                sampling.chain_speculative_sampling_target_only(pred, ai, num, cand, coins, u, t, p)
            by_slices = {}
            for _ in range(2):                           # alternating: the spread shows beside the difference
                for S in (None, 1, 8, 16):
                    by_slices.setdefault("chosen" if S is None else S, []).append(round(timeit(lambda: chain(S)), 1))
            print(json.dumps({"D": D, "B": B, "mean_accepted": round(float(num.float().mean()), 2), "chosen_slices": s2.choose_num_slices(B, V, _lib.cu_count(dev)),
                              "chain_us_by_slices": by_slices,
                              "torch_gather_cumsum_searchsorted_us": round(timeit(lambda: torch_chain(cand, coins, u, q, p), graph=False), 1),
                              "greedy_us": round(timeit(lambda: sampling.verify_chain_greedy(pred, ai, num, cand, tp), calls=16), 1),
                              "verify_step_graph_us": round(timeit(step, calls=2), 1), "verify_step_eager_us": round(timeit(step, graph=False, calls=2), 1)}), flush=True)
print(json.dumps({"device": torch.cuda.get_device_name(dev), "vocab": V}))
if sys.argv[1:] == ["verify"]:
    verify_step()
    sys.exit(0)
g = torch.Generator(device=dev).manual_seed(0)
for B in (1, 16, 128, 256):
    logits = 3.0 * torch.randn(B, V, device=dev, generator=g)
    probs = torch.softmax(logits, -1)
    temps = 0.5 + torch.rand(B, 1, device=dev, generator=g)
    top_ks = torch.randint(20, 100, (B,), device=dev, generator=g).to(torch.int32)
    top_ps = 0.8 + 0.19 * torch.rand(B, device=dev, generator=g)
    min_ps = 0.02 + 0.1 * torch.rand(B, device=dev, generator=g)
    rows = (
        ("softmax", 2, lambda: sampling.softmax(logits, temps), lambda: torch.softmax(logits / temps, -1)),
        ("top_k_top_p_sampling_from_probs joint", 1, lambda: sampling.top_k_top_p_sampling_from_probs(probs, top_ks, top_ps, filter_apply_order="joint"),
         lambda: torch_top_k_top_p(probs, top_ks, top_ps)),
        ("min_p_sampling_from_probs", 1, lambda: sampling.min_p_sampling_from_probs(probs, min_ps), lambda: torch_min_p(probs, min_ps)),
    )
    for name, passes, ours, plain in rows:
        us, us_t = timeit(ours), timeit(plain, graph=False)
        floor_us = passes * B * V * 4 / HBM * 1e6
        print(json.dumps({"op": name, "B": B, "hip_us": round(us, 1), "roofline_us": round(floor_us, 2), "fraction_of_8TBs_read_once": round(floor_us / us, 3),
                          "torch_us": round(us_t, 1), "torch_over_hip": round(us_t / us, 1)}), flush=True)
