"""GPU box: the W8A8 dense GEMM (G6, csrc/gemm_w8a8.hip) in both element types beside torch's own 8-bit paths, same process.
Every timed call streams ANOTHER copy of the weight (>= 600 MB of copies per shape: more than L2 + the 256 MB memory-side cache), so the
decode rows measure HBM, not a cache.  One hipGraph of `copies` calls, 30 replays between two events, after a warm-up replay.
Fractions: decode rows (M <= 128) weight bytes / time over 8 TB/s; M = 4096 2 M N K / time over the 5 PFLOP/s 8-bit matrix peak.
usage: python tools/time_w8a8.py [--out profiles/gemm_w8a8_first_measurement.txt]   (clock and power are not sampled)"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "sglang-fluentllm_amd"))
import torch
import flashinfer
from fluent_mi355.gemm import gemm_w8a8_nt
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemm_w8a8_first_measurement.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: a CPU run measures nothing"
dev = torch.device("cuda:0")
HBM, PEAK = 8e12, 5e15


def timeit(fns):
    """mean seconds per call of the calls in `fns`, or the exception's first line if the first call is refused"""
    try:
        fns[0](); torch.cuda.synchronize()
    except Exception as ex:   # torch's path may not exist for this shape / build: that is a result too
        return f"n/a ({type(ex).__name__}: {str(ex).splitlines()[0][:60]})"
    s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for f in fns: f()
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for f in fns: f()
    gr.replay(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(30): gr.replay()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / (30 * len(fns))


def row(M, N, K, elem):
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    copies = -(-600_000_000 // (N * K))
    i8 = elem == "int8"
    dt = torch.int8 if i8 else torch.float8_e4m3fn
    a = torch.randint(-100, 101, (M, K), device=dev, generator=g).to(torch.float32).to(dt)
    ws = [torch.randint(-100, 101, (N, K), device=dev, generator=g).to(torch.float32).to(dt) for _ in range(copies)]
    sa = torch.rand(M, 1, device=dev, generator=g) * 1e-2
    sb = torch.rand(N, device=dev, generator=g) * 1e-2
    mm = flashinfer.int8_scaled_mm if i8 else flashinfer.fp8_scaled_mm
    ours = timeit([lambda w=w: mm(a, w.t(), sa, sb, torch.bfloat16) for w in ws])
    # M = 128 is the measured point under the form threshold (the library takes the 32-row form there): time the 128-row form as well
    forced = timeit([lambda w=w: gemm_w8a8_nt(dt, a, w.t(), sa, sb, torch.bfloat16, tile_rows=128) for w in ws]) if M == 128 else None
    if i8:
        ref = timeit([lambda w=w: (torch._int_mm(a, w.t()).float() * sa * sb).to(torch.bfloat16) for w in ws])
    else:
        ref = timeit([lambda w=w: torch._scaled_mm(a, w.t(), scale_a=sa, scale_b=sb.view(1, N), out_dtype=torch.bfloat16) for w in ws])
    frac = lambda t: (f"{N * K / t / HBM:6.3f} of 8 TB/s" if M <= 128 else f"{2 * M * N * K / t / PEAK:6.3f} of 5 PFLOP/s") if isinstance(t, float) else ""
    us = lambda t: f"{t * 1e6:9.1f} us" if isinstance(t, float) else t
    return f"{elem:5s} M={M:5d} N={N:5d} K={K:5d} copies={copies:3d} | ours {us(ours)} {frac(ours)} | torch {us(ref)} {frac(ref)}" + (
        f" | ours, 128-row form forced {us(forced)} {frac(forced)}" if forced is not None else "")


lines = ["W8A8 dense GEMM, first measurement, untuned (tools/time_w8a8.py; " + torch.cuda.get_device_name(0) + "; clock / power not sampled)",
         "torch column: torch._scaled_mm with row-wise scales (fp8), torch._int_mm + the f32 scaling statement (int8)"]
for N, K in ((7168, 2048), (2112, 7168), (4096, 7168)):
    for M in (32, 128, 4096):
        for elem in ("fp8", "int8"):
            lines.append(row(M, N, K, elem))
            print(lines[-1], flush=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
