"""GPU box: absorbed paged MLA attention (P2, csrc/mla_prefill_bf16.hip) at prompt sizes — one causal prompt of 4096 tokens at H = 128
and H = 16 without a prefix, and 8 x 512 new tokens over a 2,048-token prefix at H = 16; slots are a random permutation of the pool.
Device events around a window of at least 0.5 s of hipGraph replays after a warm-up window; clocks (MHz) and power (W) are read while
the window runs.  FLOPs: 2 (576 + 512) per visible (row, key) pair.  Peak: 2.5 PFLOP/s dense bf16 matrix rate.
usage: python tools/time_mla_prefill.py   (FLUENT_MI355_LIB selects another build of the library)"""
import os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "sglang-fluentllm_amd"))
import torch
import flashinfer
dev = torch.device("cuda:0")
PEAK = 2.5e15
def sensors():
    out = {}
    for name in ("clock_rate", "power_draw", "temperature"):
        try: out[name] = getattr(torch.cuda, name)(dev)
        except Exception as ex: out[name] = f"not available ({type(ex).__name__})"
    return out
def timeit(fn, calls=4, window_s=0.5):
    fn(); torch.cuda.synchronize()
    s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s): fn()
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(calls): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    def window(replays):
        e0.record()
        for _ in range(replays): gr.replay()
        e1.record()
        busy = sensors()   # read while the replays are still running: clocks and power UNDER this load
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (calls * replays), busy
    us, _ = window(10)   # warm-up: code objects loaded, clocks up; sizes the timed window
    return window(max(10, int(window_s * 1e6 / (us * calls))))
print(json.dumps({"device": torch.cuda.get_device_name(dev), "idle": sensors()}))
g = torch.Generator(device=dev).manual_seed(0)
for B, new, prefix, H in ((1, 4096, 0, 128), (1, 4096, 0, 16), (8, 512, 2048, 16)):
    T, kv = B * new, new + prefix
    q = torch.randn(T, H, 576, device=dev, generator=g).to(torch.bfloat16)
    pool = torch.randn(B * kv + 1000, 1, 576, device=dev, generator=g).to(torch.bfloat16)   # ckv / kpe are its two column ranges
    idx = torch.randperm(pool.shape[0], device=dev, generator=g)[:B * kv].to(torch.int32)
    qo = (torch.arange(B + 1, device=dev) * new).to(torch.int32)
    ki = (torch.arange(B + 1, device=dev) * kv).to(torch.int32)
    lens = torch.full((B,), kv, dtype=torch.int32, device=dev)
    out = torch.empty(T, H, 512, dtype=torch.bfloat16, device=dev)
    w = flashinfer.BatchMLAPagedAttentionWrapper(torch.empty(16, dtype=torch.uint8, device=dev), backend="auto")
    w.plan(qo, ki, idx, lens, H, 512, 64, 1, True, 192 ** -0.5, torch.bfloat16, torch.bfloat16)
    us, busy = timeit(lambda: w.run(q[..., :512], q[..., 512:], pool[..., :512], pool[..., 512:], out=out))
    pairs = B * H * (new * prefix + new * (new + 1) // 2)   # token i of a request sees prefix + i + 1 keys
    flops = 2 * (576 + 512) * pairs
    print(json.dumps({"B": B, "new_tokens": new, "prefix": prefix, "H": H, "us": round(us, 1), "tflops_visible": round(flops / us / 1e6, 1),
                      "fraction_of_2.5_pflops_peak": round(flops / (us * 1e-6) / PEAK, 3), "under_load": busy}))
    del q, pool, out
