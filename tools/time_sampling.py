"""GPU box: first measurement of flashinfer.sampling (csrc/sampling.hip) at the real vocabulary, V = 129,280, B in {1, 16, 128, 256}:
softmax, top_k_top_p_sampling_from_probs (joint, per-row k and p) and min_p_sampling_from_probs, each beside the same operation as a plain
torch statement (sort -> cumsum -> mask -> multinomial; softmax: torch.softmax) timed in the same run.  us per call from device events
around a window of at least 0.3 s after a warm-up window: hipGraph replays for this library, back-to-back calls on one stream for torch.  Roofline: every byte the operation must move once
(B V 4 in, plus B V 4 out for softmax) at 8 TB/s.  Rows are softmax(3 randn): peaked, like a model's.
usage: python tools/time_sampling.py   (FLUENT_MI355_LIB selects another build of the library)"""
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
print(json.dumps({"device": torch.cuda.get_device_name(dev), "vocab": V}))
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
