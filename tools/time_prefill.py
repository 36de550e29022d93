"""GPU box: causal ragged bf16 MHA prefill (P1, csrc/mha_prefill_bf16.hip) at prompt sizes — one request of 4096 tokens and 8 x 2048,
at H = 16 and H = 128.  Device events around a window of at least 0.5 s of hipGraph replays after a warm-up window; clocks (MHz) and
power (W) are read while the window runs.  FLOPs are the causal half of the square: B H T^2 (192 + 128), i.e. 2 T^2 (d_qk + d_vo) / 2
per request and head.  Peak: 2.5 PFLOP/s dense bf16 matrix rate.
usage: python tools/time_prefill.py   (FLUENT_MI355_LIB selects another build of the library)"""
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
for H in (16, 128):
    for B, T in ((1, 4096), (8, 2048)):
        q = torch.randn(B * T, H * 192, device=dev, generator=g).to(torch.bfloat16).view(B * T, H, 192)
        k = torch.randn(B * T, H, 192, device=dev, generator=g).to(torch.bfloat16)
        v = torch.randn(B * T, H, 256, device=dev, generator=g).to(torch.bfloat16)[..., 128:]   # the reference's view of kv
        ind = (torch.arange(B + 1, device=dev) * T).to(torch.int32)
        w = flashinfer.BatchPrefillWithRaggedKVCacheWrapper(torch.empty(16, dtype=torch.uint8, device=dev), "NHD")
        w.begin_forward(ind, ind, H, H, 192, 128, q_data_type=torch.bfloat16)
        us, busy = timeit(lambda: w.forward(q, k, v, causal=True, sm_scale=192 ** -0.5))
        flops = B * H * T * T * (192 + 128)
        print(json.dumps({"B": B, "T": T, "H": H, "us": round(us, 1), "tflops_causal": round(flops / us / 1e6, 1),
                          "fraction_of_2.5_pflops_peak": round(flops / (us * 1e-6) / PEAK, 3), "under_load": busy}))
        del q, k, v
