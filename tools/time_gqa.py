"""GPU box: paged GQA attention (P3, csrc/gqa_paged_bf16.hip and, over an fp8 e4m3 KV cache, csrc/gqa_paged_fp8kv.hip) through the
flashinfer wrappers at serving sizes, each next to torch.nn.functional.scaled_dot_product_attention on gathered, head-repeated K / V in the
same process.  Every shape prints a bf16 line and, beside it, an fp8 line ("kv": "fp8"; pools (randn / scale).to(float8_e4m3fn), the scales
passed as k_scale / v_scale; 1 byte per K / V element in the bytes formula).
  decode  (B, Hq, Hkv, seq): bound by the K + V stream, B seq Hkv 128 x 2 x (2 or 1) bytes, reported as a fraction of 8 TB/s;
  prefill (causal 4096-token prompt; 8 x 512 tokens over a 2048-token prefix): 2 (128 + 128) Hq x visible (query, key) pairs FLOPs,
          reported as a fraction of the 2.5 PFLOP/s dense bf16 matrix peak.
Device events around a window of at least 0.5 s of hipGraph replays after a warm-up window (tools/time_prefill.py's method); the KV pool is
token-indexed through a random permutation.  `S` is the number of KV slices fluent_mi355.prefill.gqa_num_splits chose from the shapes.
usage: python tools/time_gqa.py [--no-sdpa]   (FLUENT_MI355_LIB selects another build of the library)"""
import os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "sglang-fluentllm_amd"))
import torch
import torch.nn.functional as F
import flashinfer
from fluent_mi355 import cu_count
from fluent_mi355.prefill import gqa_num_splits
dev = torch.device("cuda:0")
PEAK_FLOPS, PEAK_BYTES, SCALE = 2.5e15, 8e12, 128 ** -0.5
FP8, K_SCALE, V_SCALE, SDPA = torch.float8_e4m3fn, 0.5, 2.0, "--no-sdpa" not in sys.argv
def timeit(fn, calls=4, window_s=0.5):
    fn(); torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(calls): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    def window(replays):
        e0.record()
        for _ in range(replays): gr.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (calls * replays)
    us = window(10)   # warm-up: code objects loaded, clocks up; sizes the timed window
    return window(max(10, int(window_s * 1e6 / (us * calls))))
def sdpa_us(q, k, v, **kw):
    if not SDPA: return "not measured (--no-sdpa)"
    try: return round(timeit(lambda: F.scaled_dot_product_attention(q, k, v, scale=SCALE, **kw)), 1)
    except Exception as ex: return f"not measured ({type(ex).__name__})"
def pools(tokens, Hkv, g):
    kp, vp = (torch.randn(tokens + 64, Hkv, 128, device=dev, generator=g).to(torch.bfloat16) for _ in range(2))
    return kp, vp, torch.randperm(tokens + 64, device=dev, generator=g)[:tokens].to(torch.int32)
def pools8(tokens, Hkv, g):
    return tuple((torch.randn(tokens + 64, Hkv, 128, device=dev, generator=g) / s).to(FP8) for s in (K_SCALE, V_SCALE))
ws = lambda: torch.empty(16, dtype=torch.uint8, device=dev)
print(json.dumps({"device": torch.cuda.get_device_name(dev), "cus": cu_count(dev)}))
g = torch.Generator(device=dev).manual_seed(0)
for B, Hq, Hkv, seq in ((1, 32, 8, 4096), (16, 32, 8, 4096), (128, 32, 8, 4096), (64, 64, 8, 8192)):
    kp, vp, idx = pools(B * seq, Hkv, g)
    q = torch.randn(B, Hq, 128, device=dev, generator=g).to(torch.bfloat16)
    w = flashinfer.BatchDecodeWithPagedKVCacheWrapper(ws(), "NHD")
    w.begin_forward((torch.arange(B + 1, device=dev) * seq).to(torch.int32), idx, torch.ones(B, dtype=torch.int32, device=dev), Hq, Hkv, 128, 1,
                    data_type=torch.bfloat16, q_data_type=torch.bfloat16)
    us = timeit(lambda: w.forward(q, (kp, vp), sm_scale=SCALE))
    gather = lambda p: p[idx.long()].view(B, seq, Hkv, 128).transpose(1, 2).repeat_interleave(Hq // Hkv, 1).contiguous()
    kg, vg = gather(kp), gather(vp)
    nbytes = B * seq * Hkv * 128 * 2 * 2
    print(json.dumps({"decode": [B, Hq, Hkv, seq], "S": gqa_num_splits(B, Hkv, cu_count(dev)), "us": round(us, 1),
                      "kv_tb_per_s": round(nbytes / us / 1e6, 2), "fraction_of_8_tb_per_s": round(nbytes / (us * 1e-6) / PEAK_BYTES, 3),
                      "sdpa_us": sdpa_us(q.view(B, Hq, 1, 128), kg, vg)}))
    del kp, vp, kg, vg
    kv8 = pools8(B * seq, Hkv, g)
    w.begin_forward((torch.arange(B + 1, device=dev) * seq).to(torch.int32), idx, torch.ones(B, dtype=torch.int32, device=dev), Hq, Hkv, 128, 1,
                    data_type=FP8, q_data_type=torch.bfloat16)
    us8 = timeit(lambda: w.forward(q, kv8, sm_scale=SCALE, k_scale=K_SCALE, v_scale=V_SCALE))
    print(json.dumps({"decode": [B, Hq, Hkv, seq], "kv": "fp8", "us": round(us8, 1), "bf16_over_fp8": round(us / us8, 2),
                      "kv_tb_per_s": round(nbytes / 2 / us8 / 1e6, 2), "fraction_of_8_tb_per_s": round(nbytes / 2 / (us8 * 1e-6) / PEAK_BYTES, 3)}))
    del kv8
for name, B, q_len, prefix, Hq, Hkv in (("prompt 1 x 4096", 1, 4096, 0, 32, 8), ("extend 8 x 512 over 2048", 8, 512, 2048, 32, 8)):
    kv_len = prefix + q_len
    kp, vp, idx = pools(B * kv_len, Hkv, g)
    q = torch.randn(B * q_len, Hq, 128, device=dev, generator=g).to(torch.bfloat16)
    w = flashinfer.BatchPrefillWithPagedKVCacheWrapper(ws(), "NHD")
    w.begin_forward((torch.arange(B + 1, device=dev) * q_len).to(torch.int32), (torch.arange(B + 1, device=dev) * kv_len).to(torch.int32), idx,
                    torch.ones(B, dtype=torch.int32, device=dev), Hq, Hkv, 128, 1, q_data_type=torch.bfloat16, kv_data_type=torch.bfloat16)
    us = timeit(lambda: w.forward(q, (kp, vp), causal=True, sm_scale=SCALE))
    gather = lambda p: p[idx.long()].view(B, kv_len, Hkv, 128).transpose(1, 2).repeat_interleave(Hq // Hkv, 1).contiguous()
    mask = torch.arange(kv_len, device=dev)[None, :] <= torch.arange(q_len, device=dev)[:, None] + prefix   # bottom-right aligned
    flops = 2 * (128 + 128) * Hq * B * (q_len * prefix + q_len * (q_len + 1) // 2)
    print(json.dumps({"prefill": name, "Hq": Hq, "Hkv": Hkv, "us": round(us, 1), "tflops": round(flops / us / 1e6, 1),
                      "fraction_of_2.5_pflops_peak": round(flops / (us * 1e-6) / PEAK_FLOPS, 3),
                      "sdpa_us": sdpa_us(q.view(B, q_len, Hq, 128).transpose(1, 2), gather(kp), gather(vp), attn_mask=mask)}))
    del kp, vp
    kv8 = pools8(B * kv_len, Hkv, g)
    w.begin_forward((torch.arange(B + 1, device=dev) * q_len).to(torch.int32), (torch.arange(B + 1, device=dev) * kv_len).to(torch.int32), idx,
                    torch.ones(B, dtype=torch.int32, device=dev), Hq, Hkv, 128, 1, q_data_type=torch.bfloat16, kv_data_type=FP8)
    us8 = timeit(lambda: w.forward(q, kv8, causal=True, sm_scale=SCALE, k_scale=K_SCALE, v_scale=V_SCALE))
    print(json.dumps({"prefill": name, "kv": "fp8", "us": round(us8, 1), "bf16_over_fp8": round(us / us8, 2),
                      "tflops": round(flops / us8 / 1e6, 1), "fraction_of_2.5_pflops_peak": round(flops / (us8 * 1e-6) / PEAK_FLOPS, 3)}))
    del kv8
