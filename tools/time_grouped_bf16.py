"""GPU box: bf16 grouped GEMM of the MoE experts (G5, csrc/grouped_gemm_bf16.hip) at the LongCat / DeepSeek expert shapes — w13 (N = 4096,
K = 7168) and w2 (N = 7168, K = 2048), E = 32 local experts, eight routed rows per token spread uniformly (8 T / 32 rows per expert):
T = 128 and 512 in the 32-row form, T = 16384 in the 128-row form.  Device events around a window of at least 0.5 s of hipGraph replays after
a warm-up window; clocks (MHz) and power (W) are read while the window runs.
  decode figure : bytes of the touched weight panels (E N K 2) / time, against 8 TB/s HBM
  compute figure: 2 M N K / time, against the 2.5 PFLOP/s dense bf16 matrix rate
For context only: a per-expert torch.matmul loop over HOST-known offsets on the same inputs (eager launches, device events), and the largest
difference between the two results.
usage: python tools/time_grouped_bf16.py [--out FILE]   (FLUENT_MI355_LIB selects another build of the library)"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "sglang-fluentllm_amd"))
import torch
from fluent_mi355.gemm import m_grouped_gemm_bf16_nt_offset
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_gemm_bf16_first_measurement.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "needs an MI355X: nothing here is a measurement without one"
dev = torch.device("cuda:0")
PEAK_FLOPS, PEAK_BYTES = 2.5e15, 8e12
def sensors():
    out = {}
    for name in ("clock_rate", "power_draw", "temperature"):
        try: out[name] = getattr(torch.cuda, name)(dev)
        except Exception as ex: out[name] = f"not available ({type(ex).__name__})"
    return out
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
        busy = sensors()   # read while the replays are still running: clocks and power UNDER this load
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (calls * replays), busy
    us, _ = window(10)   # warm-up: code objects loaded, clocks up; sizes the timed window
    return window(max(10, int(window_s * 1e6 / (us * calls))))
def time_eager(fn, window_s=0.5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    def window(n):
        e0.record()
        for _ in range(n): fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n
    us = window(5)
    return window(max(5, int(window_s * 1e6 / us)))
lines = [json.dumps({"device": torch.cuda.get_device_name(dev), "idle": sensors(), "note": "first measurement, untuned"})]
print(lines[0], flush=True)
g = torch.Generator(device=dev).manual_seed(0)
E = 32
for name, N, K in (("w13", 4096, 7168), ("w2", 7168, 2048)):
    w = (0.05 * torch.randn(E, N, K, device=dev, generator=g)).to(torch.bfloat16)
    for T, tile_rows in ((128, 32), (512, 32), (16384, 128)):
        per = 8 * T // E
        M = per * E
        a = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
        out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        offs = [per * e for e in range(E + 1)]
        ex = torch.tensor(offs, dtype=torch.int32, device=dev)
        us, busy = timeit(lambda: m_grouped_gemm_bf16_nt_offset(a, w, out, ex, tile_rows))
        ref = torch.empty_like(out)
        def loop():
            for e in range(E): torch.matmul(a[offs[e]:offs[e + 1]], w[e].t(), out=ref[offs[e]:offs[e + 1]])
        loop(); torch.cuda.synchronize()
        us_loop = time_eager(loop)
        diff = max(float((out[i:i + 8192].float() - ref[i:i + 8192].float()).abs().max()) for i in range(0, M, 8192))
        flops, wbytes = 2.0 * M * N * K, 2.0 * E * N * K
        lines.append(json.dumps({
            "gemm": name, "N": N, "K": K, "E": E, "T": T, "rows_per_expert": per, "tile_rows": tile_rows, "us": round(us, 1),
            "weight_TB_per_s": round(wbytes / us / 1e6, 2), "fraction_of_8_TB_per_s": round(wbytes / (us * 1e-6) / PEAK_BYTES, 3),
            "tflops": round(flops / us / 1e6, 1), "fraction_of_2.5_pflops_peak": round(flops / (us * 1e-6) / PEAK_FLOPS, 3),
            "torch_matmul_loop_us": round(us_loop, 1), "max_abs_diff_vs_torch_loop": diff, "under_load": busy}))
        print(lines[-1], flush=True)
        del a, out, ref
    del w
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
