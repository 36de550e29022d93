#!/usr/bin/env python3
"""bench.py — BASELINE.json metric on MI355X: DeepSeek-V3 MLA decode, per-token FP8 KV, bs=128 seq=4096, TP=1.

One "step" = one decode token for the whole batch through the MLA hot path of all 61 layers: per layer
K5 (quantise+store the new latent K), K4 (quantise Q), K1 (paged FP8 MLA decode + split combine), each layer with
its OWN KV cache (61 x 338 MB = 20.6 GB resident in HBM, so nothing is re-served from the 256 MB Infinity Cache).
All inputs are resident in HBM before the timed region.  Multi-GPU = DP-attention (each rank owns its
requests and pages, no data-path collective): weak scaling, value = total tokens/s over all ranks.

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times `--steps` steps and prints the headline (`value`, `ms_per_step`);
`--dump-outputs DIR` also writes what the last timed step returned.  `--full` adds every other measurement to the same line: `roofline`
(live HIP-event timing of the dominant kernel on its launch stream), `gemm`, `variants`, `cpu_baseline` (the oracle's restatement of
the reference's torch-native CPU attention path, bounded sample) and, at N > 1, the config-4 sub-record `cfg4`.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "sglang-fluentllm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

LAYERS = 61
BS, SEQ, H, S_Q = 128, 4096, 128, 1
SCALE = 192 ** -0.5
FUSED_QUANT = os.environ.get("FLUENT_BENCH_FUSED_QUANT", "0") == "1"   # headline = the reference's unmodified call sequence (K5, K4, K1)
K4_IN_K1 = os.environ.get("FLUENT_BENCH_K4_IN_K1", "0") == "1"   # experiment switch, see layer_call
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md); measured float4-copy ceiling ~6290 GB/s


class GpuSampler:
    matched = False   # the hwmon node was chosen by the device's PCI address
    """~10 Hz sampler of shader clock and socket power around a measured loop (VERDICT r5 item 3: the power-cap argument belongs in the
    driver's record).  Sources, first that answers: the amdgpu hwmon files of the device (no subprocess: freq1_input Hz, power1_average /
    power1_input uW, power1_cap uW), then `rocm-smi --showpower --showclocks`.  Every field is None when nothing answers — the headline
    never depends on it."""

    def __init__(self, index=0, period=0.1):
        import threading
        self.index, self.period = index, period
        self.stop_ev, self.samples, self.thread = threading.Event(), [], None
        self.hw = self._find_hwmon(index)
        self.cap = None

    @staticmethod
    def _find_hwmon(index):
        """hwmon directory of HIP device `index`: the drm card whose PCI address is the device's (a box may expose the sysfs nodes of GPUs this
        process cannot open: "the first card" reads somebody else's idle — or busy — chip); without a PCI match, the first candidate."""
        import glob
        cands = []
        for card in sorted(glob.glob("/sys/class/drm/card[0-9]*")):
            if "-" in os.path.basename(card):
                continue
            for hm in sorted(glob.glob(os.path.join(card, "device/hwmon/hwmon*"))):
                if os.path.exists(os.path.join(hm, "freq1_input")) and (os.path.exists(os.path.join(hm, "power1_average"))
                                                                          or os.path.exists(os.path.join(hm, "power1_input"))):
                    cands.append((os.path.basename(os.path.realpath(os.path.join(card, "device"))).lower(), hm))
        if not cands:
            return None
        try:
            pr = torch.cuda.get_device_properties(index)
            want = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}."
            for addr, hm in cands:
                if addr.startswith(want):
                    GpuSampler.matched = True
                    return hm
        except Exception:
            pass
        return cands[index][1] if index < len(cands) else cands[0][1]

    @staticmethod
    def _rd(path):
        try:
            with open(path) as f:
                return float(f.read().strip())
        except Exception:
            return None

    def _one(self):
        if self.hw is not None:
            f = self._rd(os.path.join(self.hw, "freq1_input"))
            pw = self._rd(os.path.join(self.hw, "power1_average"))
            if pw is None:
                pw = self._rd(os.path.join(self.hw, "power1_input"))
            if self.cap is None:
                c = self._rd(os.path.join(self.hw, "power1_cap"))
                self.cap = c / 1e6 if c else None
            if f is not None or pw is not None:
                return (f / 1e6 if f else None, pw / 1e6 if pw else None)
        import re
        import subprocess
        try:
            r = subprocess.run(["rocm-smi", "-d", str(self.index), "--showpower", "--showclocks", "--showmaxpower"], capture_output=True,
                               text=True, timeout=5).stdout
            pw = re.findall(r"(?:Average|Current)[^:]*Power[^:]*:\s*([0-9.]+)", r)
            sc = re.findall(r"sclk clock level[^(]*\((\d+)Mhz\)", r)
            mx = re.findall(r"Max Graphics Package Power[^:]*:\s*([0-9.]+)", r)
            if mx and self.cap is None:
                self.cap = float(mx[0])
            return (float(sc[0]) if sc else None, float(pw[0]) if pw else None)
        except Exception:
            return (None, None)

    def _loop(self):
        while not self.stop_ev.is_set():
            self.samples.append(self._one())
            self.stop_ev.wait(self.period)

    def __enter__(self):
        import threading
        self.thread = threading.Thread(target=self._loop, daemon=True)
        self.thread.start()
        return self

    def __exit__(self, *exc):
        self.stop_ev.set()
        self.thread.join(timeout=10)
        return False

    def summary(self):
        sc = [s for s, _ in self.samples if s]
        pw = [p for _, p in self.samples if p]
        return {"sclk_mhz_mean": round(sum(sc) / len(sc)) if sc else None, "power_w_mean": round(sum(pw) / len(pw), 1) if pw else None,
                "power_w_max": round(max(pw), 1) if pw else None, "power_cap_w": round(self.cap, 1) if self.cap else None,
                "samples": len(self.samples),
                "source": ("hwmon (PCI address of the device)" if GpuSampler.matched else "hwmon (first card: no PCI match)") if self.hw is not None else "rocm-smi"}


def sampled_loop(fn, seconds=2.5, chunk=4, index=0):
    """Runs fn() back to back for ~`seconds` under the sampler: (seconds per call, sampler summary).  The clock / power fields describe THIS
    loop (same launches as the timed measurement, just long enough for a 10 Hz sampler to see them)."""
    fn()
    torch.cuda.synchronize()
    n = 0
    with GpuSampler(index) as sm:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.time()
        e0.record()
        while time.time() - t0 < seconds:
            for _ in range(chunk):
                fn()
            n += chunk
            torch.cuda.synchronize()
        e1.record()
        torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / n, sm.summary()


def algorithmic_bytes(bs, seq, h, s_q):
    """per (request, layer): seq*644 KV + s_q*H*644 Q (after K4) + s_q*H*1024 out + 4*ceil(seq/64)."""
    return bs * (seq * 644 + s_q * h * 644 + s_q * h * 1024 + 4 * ((seq + 63) // 64))


def build_workload(dev, layers, bs, seq, h, seed):
    import flash_mla_fp8 as fm

    g = torch.Generator(device=dev).manual_seed(seed)
    npg = (seq + 63) // 64
    pages = bs * npg + 1
    slots = pages * 64
    key = torch.randn(slots, 1, 576, device=dev, generator=g, dtype=torch.float32).to(torch.bfloat16)
    caches = []
    for l in range(layers):
        k_lora = torch.empty(slots, 1, 512, dtype=torch.uint8, device=dev)
        k_scale = torch.empty(slots, 1, 1, dtype=torch.float32, device=dev)
        k_rope = torch.empty(slots, 1, 64, dtype=torch.bfloat16, device=dev)
        # same statistics per layer, different physical content (rolled) — values matter only for DVFS realism
        idx = ((torch.arange(slots, device=dev, dtype=torch.int64) + 64 * 7 * l) % slots).to(torch.int32)
        fm.quantize_and_cache_k(key, k_lora, k_scale, k_rope, idx, 512)
        caches.append((k_lora, k_scale, k_rope))
    del key
    perm = torch.randperm(pages - 1, device=dev, generator=g).to(torch.int32) + 1  # page 0 = padding page, unused
    block_table = perm.view(bs, npg).contiguous()
    seqlens = torch.full((bs,), seq, dtype=torch.int32, device=dev)
    q = torch.randn(bs, S_Q, h, 576, device=dev, generator=g, dtype=torch.float32).to(torch.bfloat16)
    k_new = torch.randn(bs, 1, 576, device=dev, generator=g, dtype=torch.float32).to(torch.bfloat16)
    # slot of the newest token of every request (the decode step writes it before attending: flashmla_backend.py:188-197)
    out_loc = (block_table[:, (seq - 1) // 64].to(torch.int64) * 64 + (seq - 1) % 64).to(torch.int32)
    return dict(caches=caches, block_table=block_table, seqlens=seqlens, q=q, k_new=k_new, out_loc=out_loc, pages=pages)


def layer_call(fm, wl, l, meta, ns, fused=None):
    fused = FUSED_QUANT if fused is None else fused
    k_lora, k_scale, k_rope = wl["caches"][l]
    pages = wl["pages"]
    if K4_IN_K1:      # K5 alone, K4 inside K1's request prologue (flash_mla_fp8.flash_mla_ckv_fp8_per_token_bf16_q)
        fm.quantize_and_cache_k(wl["k_new"], k_lora, k_scale, k_rope, wl["out_loc"], 512)
        return fm.flash_mla_ckv_fp8_per_token_bf16_q(wl["q"], k_lora.view(pages, 64, 1, 512), k_rope.view(pages, 64, 1, 64),
                                                     k_scale.view(pages, 64, 1, 1), wl["block_table"], wl["seqlens"], 512, meta, ns, SCALE, True)
    if fused:   # K5 + K4 in one launch (flash_mla_fp8.quantize_q_and_cache_k): 2 launches per layer instead of 3
        qn, qs, qr = fm.quantize_q_and_cache_k(wl["q"], wl["k_new"], k_lora, k_scale, k_rope, wl["out_loc"], 512)
    else:             # the call sequence of the unmodified FlashMLABackend.forward_decode (flashmla_backend.py:188-206)
        fm.quantize_and_cache_k(wl["k_new"], k_lora, k_scale, k_rope, wl["out_loc"], 512)
        qn, qs, qr = fm.quantize_ckv_per_token_head(wl["q"], 512)
    return fm.flash_mla_ckv_fp8_per_token(qn, qr, k_lora.view(pages, 64, 1, 512), k_rope.view(pages, 64, 1, 64), qs,
                                          k_scale.view(pages, 64, 1, 1), wl["block_table"], wl["seqlens"], 512, meta, ns,
                                          SCALE, True)


DUMP_SAMPLE = 1 << 17   # elements of every layer's `o` that --dump-outputs keeps


def dump_outputs(path, held):
    """--dump-outputs: what the last timed step handed back, per layer (o bf16 [bs, s_q, H, 512], lse f32 [bs, H, s_q]), as float32 .npy:
    `lse.npy` [layers, bs, H, s_q] whole; `o_sample.npy` [layers, DUMP_SAMPLE] = the same fixed, seeded sample of elements of every layer's
    flattened o (all of o in float32 is 61 x 33.5 MB).  32 MB + 4 MB at the headline shape."""
    import numpy as np

    os.makedirs(path, exist_ok=True)
    o0 = held[0][0]
    idx = torch.randint(0, o0.numel(), (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(576)).to(o0.device)
    np.save(os.path.join(path, "o_sample.npy"), torch.stack([o.reshape(-1)[idx].float() for o, _ in held]).cpu().numpy())
    np.save(os.path.join(path, "lse.npy"), torch.stack([lse.float() for _, lse in held]).cpu().numpy())


def k1_ragged_variant(dev, layers=61):
    """SURVEY section 8(d) variant of the headline workload: cfg2 with RAGGED lengths uniform in 2048..6144 (mean 4096): K1 only,
    `layers` layer caches captured in one hipGraph, HIP events on the launch stream -> us per launch + achieved algorithmic GB/s."""
    import flash_mla_fp8 as fm

    g = torch.Generator(device=dev).manual_seed(77)
    lens = torch.randint(2048, 6145, (BS,), device=dev, generator=g, dtype=torch.int32)
    npg = ((lens + 63) // 64).tolist()
    mp, pages = max(npg), sum(npg) + 1
    slots = pages * 64
    key = torch.randn(slots, 1, 576, device=dev, generator=g, dtype=torch.float32).to(torch.bfloat16)
    caches = []
    for l in range(layers):
        k_lora = torch.empty(slots, 1, 512, dtype=torch.uint8, device=dev)
        k_scale = torch.empty(slots, 1, 1, dtype=torch.float32, device=dev)
        k_rope = torch.empty(slots, 1, 64, dtype=torch.bfloat16, device=dev)
        idx = ((torch.arange(slots, device=dev, dtype=torch.int64) + 64 * 7 * l) % slots).to(torch.int32)
        fm.quantize_and_cache_k(key, k_lora, k_scale, k_rope, idx, 512)
        caches.append((k_lora, k_scale, k_rope))
    del key
    perm = (torch.randperm(pages - 1, device=dev, generator=g).to(torch.int32) + 1).cpu()
    bt = torch.zeros(BS, mp, dtype=torch.int32)
    o = 0
    for b, n in enumerate(npg):
        bt[b, :n] = perm[o:o + n]
        o += n
    bt = bt.to(dev)
    q = torch.randn(BS, S_Q, H, 576, device=dev, generator=g, dtype=torch.float32).to(torch.bfloat16)
    qn, qs, qr = fm.quantize_ckv_per_token_head(q, 512)
    meta, ns = fm.get_mla_metadata(lens, S_Q * H, 1)

    def k1(l):
        k_lora, k_scale, k_rope = caches[l]
        fm.flash_mla_ckv_fp8_per_token(qn, qr, k_lora.view(pages, 64, 1, 512), k_rope.view(pages, 64, 1, 64), qs,
                                       k_scale.view(pages, 64, 1, 1), bt, lens, 512, meta, ns, SCALE, True)

    for l in range(layers):
        k1(l)
    torch.cuda.synchronize()
    s2 = torch.cuda.Stream()
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s2):
        k1(0)
    torch.cuda.current_stream().wait_stream(s2)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for l in range(layers):
            k1(l)
    gr.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 5
    e0.record()
    for _ in range(reps):
        gr.replay()
    e1.record()
    torch.cuda.synchronize()
    t = e0.elapsed_time(e1) * 1e-3 / (reps * layers)
    alg = int(sum(int(L) * 644 + S_Q * H * 644 + S_Q * H * 1024 + 4 * ((int(L) + 63) // 64) for L in lens.tolist()))
    return {"workload": "cfg2 ragged: bs=128, lengths uniform in 2048..6144, H=128, K1 only", "us_per_launch": round(t * 1e6, 2),
            "GBs": round(alg / t / 1e9, 1), "hbm_frac": round(alg / t / 1e9 / HBM_PEAK_GBS, 4), "algorithmic_bytes_per_launch": alg,
            "splits": int(ns[-1]) - BS}


def kernel_variants(dev, n_caches=16, launches=64):
    """The other decode kernels of the path at the cfg2 batch (bs=128, seq=4096), measured like the headline's K1 (one hipGraph of `launches`
    launches cycling over `n_caches` distinct caches = 5.4 GB and more: nothing is re-served from the 256 MB Infinity Cache; HIP events on the
    launch stream): cfg2_h16 = K1 for the TP8 shard (H=16: BASELINE.md section 4 row 2), k2_fp8 / k2_bf16 =
    flash_mla_with_kvcache over a plain fp8 / bf16 [.,576] cache (flashmla_backend.py:163-175,227-254)."""
    import flash_mla_fp8 as fm
    import flash_mla_swap as fsw

    out = {}
    g = torch.Generator(device=dev).manual_seed(5)
    npg = SEQ // 64
    pages = BS * npg + 1
    bt = (torch.randperm(pages - 1, device=dev, generator=g).to(torch.int32) + 1).view(BS, npg).contiguous()
    lens = torch.full((BS,), SEQ, dtype=torch.int32, device=dev)

    def timed(call):
        for l in range(n_caches):
            call(l)
        torch.cuda.synchronize()
        s2 = torch.cuda.Stream()
        s2.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s2):
            call(0)
        torch.cuda.current_stream().wait_stream(s2)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for i in range(launches):
                call(i % n_caches)
        gr.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 5
        e0.record()
        for _ in range(reps):
            gr.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / (reps * launches)

    def record(name, workload, t, alg, **extra):
        out[name] = dict(workload=workload, us_per_launch=round(t * 1e6, 2), GBs=round(alg / t / 1e9, 1),
                         hbm_frac=round(alg / t / 1e9 / HBM_PEAK_GBS, 4), algorithmic_bytes_per_launch=alg, **extra)

    # ---- K1, TP8 shard: H = 16 (every rank of an attention-TP8 group runs this shape over the replicated latent cache) ----
    try:
        h = 16
        wl = build_workload(dev, n_caches, BS, SEQ, h, seed=77)
        meta, ns = fm.get_mla_metadata(wl["seqlens"], h, 1)
        qn, qs, qr = fm.quantize_ckv_per_token_head(wl["q"], 512)
        pg = wl["pages"]

        def k1(l):
            k_lora, k_scale, k_rope = wl["caches"][l]
            fm.flash_mla_ckv_fp8_per_token(qn, qr, k_lora.view(pg, 64, 1, 512), k_rope.view(pg, 64, 1, 64), qs, k_scale.view(pg, 64, 1, 1),
                                           wl["block_table"], wl["seqlens"], 512, meta, ns, SCALE, True)
        record("cfg2_h16", "cfg2 TP8 shard: bs=128 seq=4096 H=16, per-token fp8 KV, K1 only", timed(k1),
               algorithmic_bytes(BS, SEQ, h, 1), kernel="mla_decode_y_kernel<0,false,1> (4-wave instantiation; split requests merged inside the kernel)", parts=int(meta.shape[0]),
               splits=int(ns[-1]) - BS)
        del wl
    except Exception as ex_:
        out["cfg2_h16"] = {"error": f"{type(ex_).__name__}: {ex_}"[:300]}
    torch.cuda.empty_cache()
    # ---- K2: flash_mla_with_kvcache over ONE [.,576] cache tensor ----
    for name, dtype, mod, esz in (("k2_fp8", torch.float8_e4m3fn, fm, 1), ("k2_bf16", torch.bfloat16, fsw, 2)):
        try:
            # N(0,1) values (random BYTES would be fp8 values up to 448: scores of 1e6)
            base = torch.randn(pages, 64, 1, 576, device=dev, generator=g)
            caches = [torch.roll(base, 7 * l, 0).to(dtype) for l in range(n_caches)]
            del base
            q = torch.randn(BS, 1, H, 576, device=dev, generator=g).to(dtype)
            one = torch.ones(1, device=dev)
            meta, ns = mod.get_mla_metadata(lens, H, 1)
            if dtype == torch.bfloat16:
                call = lambda l: mod.flash_mla_with_kvcache(q, caches[l], bt, lens, 512, meta, ns, SCALE, True)   # noqa: E731
            else:
                call = lambda l: mod.flash_mla_with_kvcache(q, caches[l], bt, lens, 512, meta, ns, SCALE, True, one, one)   # noqa: E731
            alg = BS * (SEQ * 576 * esz + H * 576 * esz + H * 1024 + 4 * npg)
            record(name, f"cfg2 batch, {'plain fp8' if esz == 1 else 'bf16'} [.,576] cache: bs=128 seq=4096 H=128, flash_mla_with_kvcache", timed(call),
                   alg, parts=int(meta.shape[0]))
            del caches
        except Exception as ex_:
            out[name] = {"error": f"{type(ex_).__name__}: {ex_}"[:300]}
        torch.cuda.empty_cache()
    return out


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _physical_cores():
    """physical cores visible to this process (SMT siblings counted once)"""
    try:
        cores = set()
        allowed = os.sched_getaffinity(0)
        for c in allowed:
            with open(f"/sys/devices/system/cpu/cpu{c}/topology/thread_siblings_list") as f:
                cores.add(f.read().strip())
        return max(1, len(cores))
    except OSError:
        return os.cpu_count() or 1


def cpu_baseline(budget_s=28.0):
    """The reference's CPU path for this op (TorchNativeAttnBackend.forward_decode, torch_native_backend.py:309-343) as
    restated in oracle/mla_ref.py, bf16 KV, on ALL physical cores of the box (SURVEY section 8d / BASELINE.md section 3):
    2 warm-ups, then the median of >= 5 runs, (a) at BASELINE config 1 (bs=1, H=16, seq=128) and (b) at config 2's shape per
    request (H=128, seq=4096) on a reduced batch (stated), scaled to tokens/s of the 61-layer decode step."""
    from oracle import mla_ref

    ncores = _physical_cores()
    torch.set_num_threads(ncores)
    g = torch.Generator().manual_seed(0)

    def case(bs_s, h, seq):
        npg = (seq + 63) // 64
        slots = (bs_s * npg + 1) * 64
        kv = torch.randn(slots, 1, 576, generator=g).to(torch.bfloat16)
        perm = torch.randperm(bs_s * npg, generator=g) + 1
        r2t = (perm.view(bs_s, npg, 1) * 64 + torch.arange(64).view(1, 1, 64)).view(bs_s, -1).to(torch.int32)
        q = torch.randn(bs_s, h, 576, generator=g).to(torch.bfloat16)
        return (q, kv, r2t, torch.arange(bs_s), torch.full((bs_s,), seq, dtype=torch.int64), SCALE)

    def median_time(args, budget):
        t_all = time.perf_counter()
        for _ in range(2):
            mla_ref.torch_native_decode(*args)
        times = []
        while len(times) < 5 or (len(times) < 9 and time.perf_counter() - t_all < budget):
            t0 = time.perf_counter()
            mla_ref.torch_native_decode(*args)
            times.append(time.perf_counter() - t0)
        return sorted(times)[len(times) // 2], len(times)

    t1, n1 = median_time(case(1, 16, 128), 2.0)
    bs_s = 2
    t2, n2 = median_time(case(bs_s, H, SEQ), budget_s)
    per_req_layer = t2 / bs_s
    return {"value": round(1.0 / (per_req_layer * LAYERS), 4), "unit": "tokens/s", "cores": ncores, "kind": "port",
            "cpu_model": _cpu_model(), "cfg1_ms_per_layer_call": round(t1 * 1e3, 3),
            "sample": f"oracle.mla_ref.torch_native_decode (reference torch_native_backend.py:309-343 restated), bf16 KV, "
                      f"torch.set_num_threads({ncores}) = all physical cores; config 2 shape at bs={bs_s} of 128 (H={H}, seq={SEQ}): "
                      f"median of {n2} layer-calls after 2 warm-ups = {per_req_layer * 1e3:.1f} ms per request-layer, x{LAYERS} "
                      f"layers -> tokens/s; config 1 (bs=1, H=16, seq=128): median of {n1} = {t1 * 1e3:.3f} ms per layer-call"}


def gemm_roofline(dev):
    """BASELINE config 3 (north_star's second half): DeepSeek-V3 MoE w13 grouped GEMM [rows, 7168] x [256 experts, 4096, 7168],
    FP8 block-scaled, top-8 routing, TP=1 — fp8 MFMA fraction in the compute regime (T = 16384 tokens, 512 rows per expert)
    and the weight-stream HBM fraction in the decode regime (T = 128).  HIP events on the launch stream.
    Operands: N(0,1) values through the path's own quantisation (weights: 128x128 blocks scaled to amax/448 like an FP8
    checkpoint; activations: flashinfer 1x128 quantiser) — what the matrix pipe sees in service.  The compute-regime
    number is ALSO taken on uniformly random bytes (`T16384_random_bytes`, round 1's operands): the chip is power-capped
    by operand toggling (probes/probe_mfma_peak.hip: 3.9-4.2 PFLOP/s on random bits, 4.7-4.9 on zeros), so the two differ."""
    import deep_gemm
    from fluent_mi355.gemm import per_token_group_quant_fp8

    HID, INTER, E, TOPK = 7168, 2048, 256, 8
    N = 2 * INTER
    g = torch.Generator(device=dev).manual_seed(0)
    # one expert's worth of N(0,1) weights, block-quantised; the other experts are row-rotated copies (distinct memory,
    # same statistics: generating 7.5 G normals would dominate the bench's run time)
    wf = torch.randn(N, HID, device=dev, generator=g)
    blk = wf.view(N // 128, 128, HID // 128, 128)
    amax = blk.abs().amax(dim=(1, 3), keepdim=True).clamp_min(1e-12)
    w1 = (blk / (amax / 448.0)).clamp(-448, 448).to(torch.float8_e4m3fn).view(N, HID)
    ws1 = (amax / 448.0).view(N // 128, HID // 128) * 0.02
    del wf, blk
    w = torch.empty(E, N, HID, dtype=torch.float8_e4m3fn, device=dev)
    ws = torch.empty(E, N // 128, HID // 128, dtype=torch.float32, device=dev)
    for e in range(E):
        r = (e * 5) % (N // 128)
        w[e].view(torch.uint8).copy_(torch.roll(w1.view(torch.uint8), 128 * r, 0))
        ws[e].copy_(torch.roll(ws1, r, 0))
    del w1, ws1
    res = {"workload": "w13 grouped GEMM, 256 experts top-8 uniform routing, hidden 7168, 2 x inter 4096, fp8 e4m3 1x128 / 128x128 block scales",
           "operands": "N(0,1) through the path's quantisers (weights 128x128-block amax/448, activations 1x128)",
           "kernel": ("grouped_gemm_fp8_big3_kernel (192 x 256 tile, one wave per SIMD; FLUENT_GEMM_BIG=2 selects the 256 x 256 8-wave kernel)"
                      if os.environ.get("FLUENT_GEMM_BIG", "3")[:1] == "3" else "FLUENT_GEMM_BIG=" + os.environ.get("FLUENT_GEMM_BIG", "")),
           "binding": "compute regime: the refill's bytes through the CU's vector-memory path + the format's 1 VALU multiply per accumulator register "
                      "and k block (profiles/r06_gemm_big3_bounding_ladder.txt); decode regime (T128): HBM"}

    def timed(T, iters, xq, xs, ex, M, sample=None):
        out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)

        def run():
            deep_gemm.m_grouped_gemm_fp8_fp8_bf16_nt_offset((xq, xs), (w, ws), out, ex, use_pdl=True)

        run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            run()
        e1.record()
        torch.cuda.synchronize()
        if sample is not None:   # clock / power of the same launches over ~2 s
            try:
                s_, smp = sampled_loop(run, 2.0, 8)
                smp["ms_sampled_loop"] = round(s_ * 1e3, 3)
                sample.update(smp)
            except Exception as ex_:
                sample["error"] = f"{type(ex_).__name__}: {ex_}"[:200]
        return e0.elapsed_time(e1) * 1e-3 / iters

    for T, iters in ((128, 20), (16384, 3)):
        M = T * TOPK
        ids = torch.stack([torch.randperm(E, device=dev, generator=g)[:TOPK] for _ in range(min(T, 2048))])
        ids = ids.repeat((T + ids.shape[0] - 1) // ids.shape[0], 1)[:T].reshape(-1)
        counts = torch.bincount(ids, minlength=E)
        ex = torch.zeros(E + 1, dtype=torch.int32, device=dev)
        ex[1:] = torch.cumsum(counts, 0)
        xq = torch.empty(M, HID, dtype=torch.float8_e4m3fn, device=dev)
        xs = torch.empty(M, HID // 128, dtype=torch.float32, device=dev)
        for i in range(0, M, 16384):   # the path's own 1x128 quantiser on N(0,1) rows
            q_, s_ = per_token_group_quant_fp8(torch.randn(min(16384, M - i), HID, device=dev, generator=g).to(torch.bfloat16))
            xq[i:i + q_.shape[0]].copy_(q_)
            xs[i:i + q_.shape[0]].copy_(s_)
        smp = {} if T == 16384 else None
        t = timed(T, iters, xq, xs, ex, M, smp)
        flops = 2.0 * M * N * HID
        hit = int((counts > 0).sum())
        byts = hit * (N * HID) + M * (HID + HID // 128 * 4) + M * N * 2
        res[f"T{T}"] = {"ms": round(t * 1e3, 3), "TFLOPs": round(flops / t / 1e12, 1),
                        "mfma_frac": round(flops / t / 1e12 / 5000.0, 4), "GBs": round(byts / t / 1e9, 1),
                        "hbm_frac": round(byts / t / 1e9 / HBM_PEAK_GBS, 4), "rows_per_expert": round(M / E, 1)}
        if smp is not None:
            res[f"T{T}"].update({"sclk_mhz_mean": smp.get("sclk_mhz_mean"), "power_w_mean": smp.get("power_w_mean"),
                                 "power_cap_w": smp.get("power_cap_w"), "sampler": smp})
        if T == 16384:
            # what `binding` means in numbers: the bytes the 192 x 256 kernel pulls through each CU's vector-memory path (every tile refills
            # (192 + 256) rows x 128 B per k block, whatever L2 / HBM serves them) against what that path was measured to sustain per CU
            # (profiles/r06_gemm_big3_bounding_ladder.txt (4), r02_probe_dma_rate.txt: ~42-45 GB/s from HBM, ~120 from L2)
            tiles = int(((counts + 191) // 192).sum()) * (N // 256)
            refill = tiles * (HID // 128) * (192 + 256) * 128
            cus = torch.cuda.get_device_properties(dev).multi_processor_count
            res[f"T{T}"].update({"refill_bytes_per_launch": refill, "refill_GBs_per_cu": round(refill / t / 1e9 / cus, 1),
                                 "refill_GBs_per_cu_measured_ceilings": {"hbm_sourced": 45, "l2_resident": 120}})
        if T == 16384:   # the same launch on uniformly random bytes (maximal operand toggling; round 1's operands)
            flat = w.view(-1).view(torch.uint8)
            step = 1 << 28
            for i in range(0, flat.numel(), step):
                n = min(step, flat.numel() - i)
                b = torch.randint(0, 255, (n,), device=dev, generator=g, dtype=torch.int16)
                flat[i:i + n] = torch.where((b & 0x7F) == 0x7F, b - 1, b).to(torch.uint8)
            xq2 = (torch.randn(M, HID, device=dev, generator=g) / 10).to(torch.float8_e4m3fn)
            t2 = timed(T, iters, xq2, xs, ex, M)
            res["T16384_random_bytes"] = {"ms": round(t2 * 1e3, 3), "TFLOPs": round(flops / t2 / 1e12, 1),
                                          "mfma_frac": round(flops / t2 / 1e12 / 5000.0, 4)}
            del xq2
        del xq, xs
    # SURVEY section 8(d) variants of the compute regime (operands: the random bytes left in `w`, N(0,1)/10 activations):
    # Zipf-skewed routing at T=16384 (expert e drawn with weight 1/(e+1): a few experts take thousands of rows, a long tail
    # gets none) and T=32768 with uniform routing
    for name, T, zipf in (("T16384_zipf", 16384, True), ("T32768", 32768, False)):
        M = T * TOPK
        if zipf:
            wgt = 1.0 / torch.arange(1, E + 1, device=dev, dtype=torch.float32)
            ids = torch.multinomial(wgt.expand(2048, E), TOPK, replacement=False, generator=g)
        else:
            ids = torch.stack([torch.randperm(E, device=dev, generator=g)[:TOPK] for _ in range(2048)])
        ids = ids.repeat((T + 2047) // 2048, 1)[:T].reshape(-1)
        counts = torch.bincount(ids, minlength=E)
        ex = torch.zeros(E + 1, dtype=torch.int32, device=dev)
        ex[1:] = torch.cumsum(counts, 0)
        xq = (torch.randn(M, HID, device=dev, generator=g) / 10).to(torch.float8_e4m3fn)
        xs = torch.rand(M, HID // 128, device=dev, generator=g) * 1e-2 + 1e-3
        t = timed(T, 3, xq, xs, ex, M)
        flops = 2.0 * M * N * HID
        res[name] = {"ms": round(t * 1e3, 3), "TFLOPs": round(flops / t / 1e12, 1), "mfma_frac": round(flops / t / 1e12 / 5000.0, 4),
                     "experts_hit": int((counts > 0).sum()), "max_rows_per_expert": int(counts.max())}
        del xq, xs
    # ---- w2 (the K = 2048 GEMM: 16 k blocks per tile, set-up / epilogue-heavy) and the whole MoE layer of fp8_eps_executor.py:33-82
    #      (1x128 quant -> grouped w13 -> SiLU*mul -> 1x128 quant -> grouped w2) at T = 16384, operands as above ----
    try:
        import flashinfer
        from eps.executor import silu
        T, INTER = 16384, N // 2
        M = T * TOPK
        ids = torch.stack([torch.randperm(E, device=dev, generator=g)[:TOPK] for _ in range(2048)])
        ids = ids.repeat((T + 2047) // 2048, 1)[:T].reshape(-1)
        counts = torch.bincount(ids, minlength=E)
        ex = torch.zeros(E + 1, dtype=torch.int32, device=dev)
        ex[1:] = torch.cumsum(counts, 0)
        w2 = torch.empty(E, HID, INTER, dtype=torch.float8_e4m3fn, device=dev)
        flat = w2.view(-1).view(torch.uint8)
        for i in range(0, flat.numel(), 1 << 28):
            n = min(1 << 28, flat.numel() - i)
            b = torch.randint(0, 255, (n,), device=dev, generator=g, dtype=torch.int16)
            flat[i:i + n] = torch.where((b & 0x7F) == 0x7F, b - 1, b).to(torch.uint8)
        w2s = torch.rand(E, HID // 128, INTER // 128, device=dev, generator=g) * 1e-2
        x = (torch.randn(M, HID, device=dev, generator=g) / 10).to(torch.bfloat16)
        mp = (M + E * 31) // 32 * 32
        xq = torch.empty(M, HID, dtype=torch.float8_e4m3fn, device=dev)
        xs = torch.empty((HID // 128, mp), dtype=torch.float32, device=dev).permute(-1, -2)
        gate_up = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        dq = torch.empty(M, INTER, dtype=torch.float8_e4m3fn, device=dev)
        ds = torch.empty((INTER // 128, mp), dtype=torch.float32, device=dev).permute(-1, -2)
        out = torch.empty(M, HID, dtype=torch.bfloat16, device=dev)

        def layer():
            flashinfer.quantization.quant_1x128(x, xq, xs, ex, E, (M + 3) // 4 * 4, mp, HID)
            deep_gemm.m_grouped_gemm_fp8_fp8_bf16_nt_offset((xq, xs), (w, ws), gate_up, ex, use_pdl=True)
            a_ = silu(gate_up, ex, M)
            flashinfer.quantization.quant_1x128(a_, dq, ds, ex, E, (M + 3) // 4 * 4, mp, INTER)
            deep_gemm.m_grouped_gemm_fp8_fp8_bf16_nt_offset((dq, ds), (w2, w2s), out, ex, use_pdl=True)

        def g2():
            deep_gemm.m_grouped_gemm_fp8_fp8_bf16_nt_offset((dq, ds), (w2, w2s), out, ex, use_pdl=True)

        def tm(fn, iters=3):
            fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3 / iters

        layer()
        t2, tl = tm(g2), tm(layer)
        f2 = 2.0 * M * HID * INTER
        fl = 2.0 * M * (N * HID + HID * INTER)
        res["T16384_w2"] = {"workload": "w2 grouped GEMM [7168, 2048] per expert, same routing", "ms": round(t2 * 1e3, 3),
                            "TFLOPs": round(f2 / t2 / 1e12, 1), "mfma_frac": round(f2 / t2 / 1e12 / 5000.0, 4)}
        res["T16384_moe_layer"] = {"workload": "quant_1x128 -> w13 -> SiLU*mul -> quant_1x128 -> w2 (fp8_eps_executor.py:33-82)",
                                   "ms": round(tl * 1e3, 3), "TFLOPs": round(fl / tl / 1e12, 1),
                                   "mfma_frac": round(fl / tl / 1e12 / 5000.0, 4)}
        del w2, w2s, x, xq, xs, gate_up, dq, ds, out
    except Exception as ex_:   # the headline record must not depend on this add-on
        res["T16384_w2"] = {"error": f"{type(ex_).__name__}: {ex_}"[:200]}
    res["mfma_frac"] = res["T16384"]["mfma_frac"]          # of the 5 PFLOP/s dense fp8 peak
    res["T128_hbm_frac"] = res["T128"]["hbm_frac"]         # weight stream, of 8 TB/s
    del w, ws
    torch.cuda.empty_cache()
    return res


def dense_roofline(dev, T=256):
    """G4 — the dense block-fp8 decode projections (deep_gemm.gemm_fp8_fp8_bf16_nt behind Fp8LinearMethod,
    layers/dense/gemms/fp8/deep_geem.py:14-102) at T tokens, weights not re-served from cache (8 distinct copies in one hipGraph),
    and B1, the bf16 absorption bmm's / router GEMM.  `hbm_frac` = weight bytes / time / 8 TB/s.  At T = 256 these GEMMs sit AT the
    fp8 ridge point of the chip (2 T = 512 flop per weight byte vs 5 PF / 8 TB/s = 625): both roofs bind, see DESIGN.md."""
    import deep_gemm
    from fluent_mi355.bmm import bmm
    from fluent_mi355.gemm import per_token_group_quant_fp8

    g = torch.Generator(device=dev).manual_seed(5)
    res = {"tokens": T}

    def graph_time(fn, copies, reps=10):
        fn(0)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn(0)
        torch.cuda.current_stream().wait_stream(s)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for c in range(copies):
                fn(c)
        gr.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            gr.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / (reps * copies)

    # `frac_of_floor` = max(weight bytes / 8 TB/s, flops / 5 PFLOP/s) / measured: the binding roof of the two
    for N, K, Ts in ((2176, 7168, (T, 32)), (7168, 2048, (T, 32)), (14336, 7168, (T, 32))):
        Ws = [(torch.randint(0, 120, (N, K), device=dev, generator=g, dtype=torch.uint8).view(torch.float8_e4m3fn),
               torch.rand((N + 127) // 128, K // 128, device=dev, generator=g) * 1e-2) for _ in range(8)]
        for Tt in Ts:
            x = torch.randn(Tt, K, device=dev, generator=g).to(torch.bfloat16)
            xq, xs = per_token_group_quant_fp8(x, column_major_scales=True)
            out = torch.empty(Tt, N, dtype=torch.bfloat16, device=dev)
            t = graph_time(lambda c: deep_gemm.gemm_fp8_fp8_bf16_nt((xq, xs), Ws[c], out), 8)
            floor = max(N * K / (HBM_PEAK_GBS * 1e9), 2.0 * Tt * N * K / 5e15)
            res[f"fp8_{N}x{K}" + ("" if Tt == T else f"_T{Tt}")] = {
                "us": round(t * 1e6, 1), "weight_GBs": round(N * K / t / 1e9, 1), "hbm_frac": round(N * K / t / 1e9 / HBM_PEAK_GBS, 3),
                "TFLOPs": round(2.0 * Tt * N * K / t / 1e12, 1), "floor_us": round(floor * 1e6, 2), "frac_of_floor": round(floor / t, 3)}
        del Ws
    Hh = 128
    q = torch.randn(T, Hh, 192, device=dev, generator=g).to(torch.bfloat16)
    wkc = (torch.randn(Hh, 512, 128, device=dev, generator=g) * 0.05).to(torch.bfloat16).transpose(1, 2)      # [H, 128, 512], k-contiguous
    wvc = (torch.randn(Hh, 128, 512, device=dev, generator=g) * 0.05).to(torch.bfloat16).transpose(1, 2)      # [H, 512, 128]
    Q = torch.empty(T, Hh, 576, dtype=torch.bfloat16, device=dev)
    att = torch.randn(T, Hh, 512, device=dev, generator=g).to(torch.bfloat16)
    xr = torch.randn(T, 7168, device=dev, generator=g).to(torch.bfloat16)
    wr = (torch.randn(256, 7168, device=dev, generator=g) * 0.02).to(torch.bfloat16)
    import flashinfer
    for name, fn, wbytes in (("bmm_q_absorb_H128", lambda c: bmm(q[..., :128].transpose(0, 1), wkc, out=Q[..., :512].transpose(0, 1)), Hh * 128 * 512 * 2),
                             ("bmm_v_absorb_H128", lambda c: bmm(att.transpose(0, 1), wvc), Hh * 128 * 512 * 2),
                             ("router_gemm_256x7168", lambda c: flashinfer.dsv3_router_gemm(xr, wr, out_dtype=torch.float32), 256 * 7168 * 2)):
        t = graph_time(fn, 4)
        res[name] = {"us": round(t * 1e6, 1), "weight_GBs": round(wbytes / t / 1e9, 1)}
    return res


def fail_line(a, msg, rank=0):
    """A failure of the launch itself is still ONE JSON line on stdout (rank 0) and a non-zero exit code — never a bare SystemExit."""
    if rank == 0:
        print(json.dumps({"metric": "decode tokens/s (MLA-attention-bound, 61 layers) + achieved HBM GB/s, DeepSeek-V3 MLA bs=128 seq=4k",
                          "value": None, "unit": "tokens/s", "n_gpus": a.gpus, "steps": a.steps, "warmup": a.warmup, "error": msg}), flush=True)
    sys.exit(2)


def _free_port():
    import socket

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def self_launch(a):
    """Re-run this script as `--gpus N` ranks of ONE node: python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr
    127.0.0.1 --master-port P bench.py <same arguments>.  The children inherit stdout: rank 0's JSON line is this process's line."""
    import subprocess

    if not a.dry_launch:
        n = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if n < a.gpus:
            return fail_line(a, f"--gpus {a.gpus} but only {n} HIP device(s) are visible")
    port = int(os.environ.get("MASTER_PORT") or _free_port())
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL / peer mappings across processes need it on this driver
    r = subprocess.run(cmd, env=env)
    if r.returncode != 0:
        fail_line(a, f"torch.distributed.run exited with code {r.returncode} (the ranks' own messages are on stderr)")
    sys.exit(0)


def dry_launch(a, world, rank):
    """--dry-launch: the ranks meet over gloo (CPU), agree on their count with one all-reduce, rank 0 prints one line."""
    import torch.distributed as dist

    seen = 1
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)
        t = torch.ones(1, dtype=torch.int64)
        dist.all_reduce(t)
        seen = int(t.item())
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"dry_launch": True, "n_gpus": a.gpus, "world_size": world, "ranks_seen": seen, "steps": a.steps, "warmup": a.warmup}),
              flush=True)
    sys.exit(0 if seen == world == a.gpus else 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure roofline, gemm, variants, cpu_baseline and (N > 1) the config-4 sub-record")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (rank 0) as DIR/o_sample.npy and DIR/lse.npy (float32): see dump_outputs")
    ap.add_argument("--layers", type=int, default=LAYERS, help=argparse.SUPPRESS)
    ap.add_argument("--no-cpu-baseline", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-graph", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-gemm", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--mode", choices=["mla", "cfg4"], default="mla",
                    help="mla (default): the headline DP-attention MLA decode bench; cfg4: BASELINE config 4, attention-TP + EP MoE "
                         "decoder layers with the path's collectives (all-gather, reduce-scatter, EP all-to-all) over RCCL")
    ap.add_argument("--dry-launch", action="store_true",
                    help="launch plumbing only: --gpus N ranks rendezvous over gloo on the CPU, rank 0 prints one line (no GPU needed)")
    a = ap.parse_args()

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` launches ITSELF: one rank per GPU under torch.distributed.run (what the driver's multi-GPU form does by
        # hand); rank 0 of the children prints the one JSON line on this process's stdout.
        return self_launch(a)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus > 1 and world != a.gpus:
        return fail_line(a, f"--gpus {a.gpus} but the launcher set WORLD_SIZE={world}: launch with --nproc-per-node {a.gpus}", rank)
    if a.dry_launch:
        return dry_launch(a, world, rank)
    if not torch.cuda.is_available() or torch.cuda.device_count() <= local_rank:
        return fail_line(a, f"rank {rank} needs device cuda:{local_rank}; {torch.cuda.device_count() if torch.cuda.is_available() else 0} visible", rank)
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    dist = None
    if world > 1:
        import torch.distributed as dist_

        dist = dist_
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    if a.mode == "cfg4":
        return main_cfg4(a, dev, world, rank, dist)

    import flash_mla_fp8 as fm

    layers = a.layers
    wl = build_workload(dev, layers, BS, SEQ, H, seed=1234 + rank)
    meta, ns = fm.get_mla_metadata(wl["seqlens"], S_Q * H, 1)
    torch.cuda.synchronize()

    # (o, lse) of every layer of the latest step() call — of the captured step under a hipGraph, where each replay refills them.  Held only
    # when they are to be written: a run without --dump-outputs frees each layer's outputs at once, as it always did
    keep = a.dump_outputs is not None and rank == 0
    held = []

    def step():
        # K3 once per decode step, as the reference's backend does in init_forward_metadata (flashmla_backend.py:307-321)
        m_step, ns_step = fm.get_mla_metadata(wl["seqlens"], S_Q * H, 1)
        if keep:
            held[:] = [layer_call(fm, wl, l, m_step, ns_step) for l in range(layers)]
            return
        for l in range(layers):
            layer_call(fm, wl, l, m_step, ns_step)

    # eager warm-up (also sizes the caching allocator), then capture one step in a hipGraph like the reference's
    # decode path (model_executor/cuda_graph_runner.py:433-434)
    step()
    torch.cuda.synchronize()
    graph = None
    if not a.no_graph:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step()
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
    run = graph.replay if graph is not None else step
    graph_ok = graph is not None
    for _ in range(a.warmup):
        run()

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        run()
    barrier()
    dt = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    ms_per_step = dt / a.steps * 1e3
    tokens_per_s = world * BS / (ms_per_step * 1e-3) * (layers / LAYERS)   # (a step of fewer layers is scaled to the 61-layer step)
    if keep:
        dump_outputs(a.dump_outputs, held)
        del held[:]

    # ==== everything below the headline is measured under --full only: a plain run goes straight to its result line ====
    # ---- sub-records of the same step (rank 0, N = 1): (a) the optional fused quant launch (flash_mla_fp8.quantize_q_and_cache_k: an
    #      extension entry point an integrator may call instead of K5 + K4 — NOT what the unmodified FlashMLABackend calls, hence
    #      not the headline), (b) the quant launches alone, so that K1's share of the timed step can be read off ----
    step_variants = None
    if a.full and rank == 0 and world == 1 and graph is not None:
        def timed_graph(body, reps):
            s3 = torch.cuda.Stream()
            s3.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s3):
                body()
            torch.cuda.current_stream().wait_stream(s3)
            gx = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gx):
                body()
            gx.replay()
            torch.cuda.synchronize()
            t0_ = time.perf_counter()
            for _ in range(reps):
                gx.replay()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0_) / reps * 1e3

        def fused_step():
            m_step, ns_step = fm.get_mla_metadata(wl["seqlens"], S_Q * H, 1)
            for l in range(layers):
                layer_call(fm, wl, l, m_step, ns_step, fused=not FUSED_QUANT)

        def quant_only_step():
            fm.get_mla_metadata(wl["seqlens"], S_Q * H, 1)
            for l in range(layers):
                k_lora, k_scale, k_rope = wl["caches"][l]
                if FUSED_QUANT:
                    fm.quantize_q_and_cache_k(wl["q"], wl["k_new"], k_lora, k_scale, k_rope, wl["out_loc"], 512)
                else:
                    fm.quantize_and_cache_k(wl["k_new"], k_lora, k_scale, k_rope, wl["out_loc"], 512)
                    fm.quantize_ckv_per_token_head(wl["q"], 512)

        ms_other = timed_graph(fused_step, max(3, a.steps // 2))
        ms_quant = timed_graph(quant_only_step, max(3, a.steps // 2))

        def k3_only():   # K3 alone, 32 calls per replay (host clock around the replays: the replay overhead is in) (the reference runs it once per step on the host-critical path: flashmla_backend.py:380-387)
            for _ in range(32):
                fm.get_mla_metadata(wl["seqlens"], S_Q * H, 1)

        ms_k3 = timed_graph(k3_only, max(3, a.steps // 2)) / 32.0
        other = "K5, K4 separate (reference call sequence)" if FUSED_QUANT else "K5 + K4 fused (flash_mla_fp8.quantize_q_and_cache_k, extension)"
        step_variants = {"other_quant_form": {"quant_launch": other, "ms_per_step": round(ms_other, 4),
                                              "tokens_per_s": round(BS / (ms_other * 1e-3) * (layers / LAYERS), 1)},
                         "quant_launches_only_ms_per_step": round(ms_quant, 4),
                         "k3_us_per_call": round(ms_k3 * 1e3, 2),
                         "k1_us_per_launch_inside_the_timed_step": round((ms_per_step - ms_quant) * 1e3 / layers, 2)}

    # ---- roofline of the dominant kernel: K1 alone, HIP events on the launch stream (torch's current stream) ----
    roof = None
    if a.full and rank == 0:
        pages = wl["pages"]
        qn, qs, qr = fm.quantize_ckv_per_token_head(wl["q"], 512)

        def k1(l):
            k_lora, k_scale, k_rope = wl["caches"][l]
            fm.flash_mla_ckv_fp8_per_token(qn, qr, k_lora.view(pages, 64, 1, 512), k_rope.view(pages, 64, 1, 64), qs,
                                           k_scale.view(pages, 64, 1, 1), wl["block_table"], wl["seqlens"], 512, meta, ns,
                                           SCALE, True)

        for l in range(layers):
            k1(l)
        torch.cuda.synchronize()
        # launch-overhead-free: the K1 launches of all layers are captured once and replayed; HIP events bracket the
        # replays on the launch stream (torch's current stream)
        reps = 5
        k1_graph = None
        if not a.no_graph:
            s2 = torch.cuda.Stream()
            s2.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s2):
                k1(0)
            torch.cuda.current_stream().wait_stream(s2)
            k1_graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(k1_graph):
                for l in range(layers):
                    k1(l)
            k1_graph.replay()
            torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            if k1_graph is not None:
                k1_graph.replay()
            else:
                for l in range(layers):
                    k1(l)
        e1.record()
        torch.cuda.synchronize()
        per_launch_s = e0.elapsed_time(e1) * 1e-3 / (reps * layers)
        alg = algorithmic_bytes(BS, SEQ, H, S_Q)
        achieved = alg / per_launch_s / 1e9
        # HBM bytes per launch: NOT measured in this run — read from the committed rocprofv3 --pmc passes (FETCH_SIZE x 2 +
        # WRITE_SIZE, MI355X_MICROARCH.md) of the kernel this build dispatches at this workload; the source file is named
        traffic, traffic_src = None, None
        try:
            traffic_src = "profiles/r06_pmc_traffic.json"
            with open(os.path.join(ROOT, traffic_src)) as f:
                traffic = round(json.load(f)["hbm_bytes_per_launch"])
        except Exception:
            traffic_src = None
        # at H = 128 the kernel is near the fp8 ridge — the MFMA fraction beside the HBM fraction (2176 flop per
        # query row and token: QK 2 x 576, PV 2 x 512), and what the chip's clock / power did during the same launches
        flops = 2176.0 * S_Q * H * SEQ * BS
        mfma_frac = flops / per_launch_s / 5e15
        smp, smp_s = None, None
        try:
            def replay_once():
                if k1_graph is not None:
                    k1_graph.replay()
                else:
                    for l_ in range(layers):
                        k1(l_)
            smp_s, smp = sampled_loop(replay_once, 2.5, 4, local_rank)
            smp["us_per_launch_sampled_loop"] = round(smp_s / layers * 1e6, 2)
        except Exception as ex_:
            smp = {"error": f"{type(ex_).__name__}: {ex_}"[:200]}
        capped = bool(smp and smp.get("power_w_mean") and smp.get("power_cap_w") and smp["power_w_mean"] >= 0.93 * smp["power_cap_w"])
        # what binds: bytes (>= 0.6 of the HBM sheet rate is past the measured copy ceiling's 3/4) or the instruction stream under the
        # socket power limit (matrix-pipe duty + clock: DESIGN.md section 3)
        binding = "hbm" if achieved / HBM_PEAK_GBS >= 0.6 else "issue/power"
        roof = {"bound": "hbm", "binding": binding, "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4), "mfma_frac": round(mfma_frac, 4), "mfma_tflops": round(flops / per_launch_s / 1e12, 1),
                "sclk_mhz_mean": smp.get("sclk_mhz_mean") if smp else None, "power_w_mean": smp.get("power_w_mean") if smp else None,
                "power_cap_w": smp.get("power_cap_w") if smp else None, "power_capped": capped if smp and smp.get("power_w_mean") else None,
                "sampler": smp,
                "traffic": traffic, "traffic_source": traffic_src,
                "kernel": "mla_decode_y_kernel (no merge kernel: split requests are merged inside the decode kernel; none is split at this shape)",
                "us_per_launch": round(per_launch_s * 1e6, 2),
                "algorithmic_bytes_per_launch": alg}
    cpu = None
    gemm = None
    variants = None
    if a.full and rank == 0 and world == 1 and not a.no_gemm:
        wl = None
        torch.cuda.empty_cache()
        variants = {"cfg2_ragged": k1_ragged_variant(dev)}
        torch.cuda.empty_cache()
        try:
            variants.update(kernel_variants(dev))
        except Exception as ex_:   # an add-on: never at the expense of the headline record
            variants["kernel_variants_error"] = f"{type(ex_).__name__}: {ex_}"[:300]
        if step_variants is not None:
            variants["step"] = step_variants
        if os.environ.get("FLUENT_BENCH_CFG4_WORLD1", "1") != "0":
            # BASELINE config 4's decoder layer (data-connected: tools/cfg4_layer.py) at world 1 — every stage of the TP8/EP8 layer on ONE
            # GPU (all 128 heads, all 256 experts; collectives degenerate to their local kernels): ms per layer of the captured step + the
            # eager per-stage split.  An add-on: never at the expense of the headline record.
            try:
                torch.cuda.empty_cache()
                rec = measure_cfg4(a, dev, 1, 0, None, 2, 5, 2, stages=True)
                variants["cfg4_world1"] = {k: rec[k] for k in ("metric", "value", "unit", "ms_per_step", "ms_per_layer", "stage_ms", "config")}
            except Exception as ex_:
                variants["cfg4_world1"] = {"error": f"{type(ex_).__name__}: {ex_}"[:300]}
            torch.cuda.empty_cache()
        torch.cuda.empty_cache()
        gemm = gemm_roofline(dev)
        try:
            gemm["dense"] = dense_roofline(dev)
        except Exception as ex_:   # an add-on: never at the expense of the headline record
            gemm["dense"] = {"error": f"{type(ex_).__name__}: {ex_}"[:200]}
    if a.full and rank == 0 and world == 1 and not a.no_cpu_baseline:
        cpu = cpu_baseline()
    # ---- N > 1: BASELINE config 4 (attention-TP + EP MoE decoder layers, every collective of the path inside the captured step)
    #      as a sub-record of the SAME json line — what makes a multi-GPU record of this path more than N independent replicas.
    #      A watchdog prints the line without it if the collectives do not come back (the DP numbers above are already taken).
    cfg4 = None
    line = {}

    def emit():
        if rank == 0:
            line["cfg4"] = cfg4
            print(json.dumps(line), flush=True)

    want4 = os.environ.get("FLUENT_BENCH_CFG4", "1")   # "0": never; "force": also at N = 1 (exercises this code on a 1-GPU box)
    if a.full and ((world > 1 and want4 != "0") or want4 == "force"):
        # Every rank runs `bench.py --mode cfg4` as a CHILD process with its own rendezvous port: a hang is ended by the timeout
        # (the exact child is killed), and a hard fault in the multi-GPU transports — a peer mapping or a collective that aborts
        # the process — ends the child only: the DP record measured above is printed either way.
        import subprocess

        budget = float(os.environ.get("FLUENT_BENCH_CFG4_TIMEOUT_S", "240"))
        line.update(_headline(tokens_per_s, world, a, ms_per_step, layers, graph_ok, roof, gemm, variants, cpu))
        # the children build their own workload on the SAME GPU: the DP phase's 61 layer caches (20.6 GB), its graph and the graph pool go first
        wl = graph = run = step = None   # noqa: F841
        import gc

        gc.collect()
        torch.cuda.empty_cache()
        cmd = [sys.executable, os.path.abspath(__file__), "--mode", "cfg4", "--gpus", str(world), "--steps", str(max(3, min(a.steps, 10))),
               "--warmup", "2"]
        # Two attempts at most: the default routes first (decode-sized collectives and the EP exchange on the one-shot peer-mapped
        # transport — never run across real GPUs by its builder), then, if any rank's child failed or hung, everything on RCCL
        # (FLUENT_ONESHOT=0).  The ranks agree on the outcome with one all-reduce; the record names the route and the first failure.
        first_error = None
        for attempt, extra in enumerate(({}, {"FLUENT_ONESHOT": "0"})):
            env = dict(os.environ, MASTER_ADDR="127.0.0.1", FLUENT_BENCH_CFG4="0",
                       MASTER_PORT=str(int(os.environ.get("MASTER_PORT", "29500")) + 17 * (attempt + 1)), **extra)
            ok, rec, err = 0, None, None
            try:
                if dist is not None:
                    dist.barrier()
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=budget / 2)
                for ln in reversed(r.stdout.strip().splitlines()):
                    if ln.startswith("{"):
                        rec = json.loads(ln)
                        break
                ok = 1 if r.returncode == 0 and (rank != 0 or rec is not None) else 0
                if not ok:
                    err = f"config-4 child exited with code {r.returncode}: {r.stderr.strip()[-300:]}"
            except subprocess.TimeoutExpired:
                err = f"config-4 child did not finish within {budget / 2:.0f} s (collectives inside the captured step)"
            except Exception as ex:
                err = f"{type(ex).__name__}: {ex}"[:300]
            if dist is not None:
                flag = torch.tensor([ok], device=dev, dtype=torch.int32)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                ok = int(flag.item())
            if ok:
                if rec is not None:
                    cfg4 = {k: rec[k] for k in ("metric", "value", "unit", "ms_per_step", "ms_per_layer", "scaling", "config") if k in rec}
                    cfg4["attempt"] = "default routes (one-shot transport where it applies)" if attempt == 0 else "FLUENT_ONESHOT=0 (RCCL only)"
                    if first_error:
                        cfg4["first_attempt_error"] = first_error
                break
            first_error = first_error or err or "a peer rank's child failed"
            cfg4 = {"error": first_error + ("" if attempt == 0 else " | RCCL-only attempt: " + (err or "a peer rank's child failed")) + "; DP record only"}
    if not line:
        line.update(_headline(tokens_per_s, world, a, ms_per_step, layers, graph_ok, roof, gemm, variants, cpu))
    emit()
    if dist is not None:
        dist.destroy_process_group()


def _headline(tokens_per_s, world, a, ms_per_step, layers, graph_ok, roof, gemm, variants, cpu):
    return {
            "metric": "decode tokens/s (MLA-attention-bound, 61 layers) + achieved HBM GB/s, DeepSeek-V3 MLA bs=128 seq=4k",
            "value": round(tokens_per_s, 1), "unit": "tokens/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "fp8_e4m3 (KV, Q, P) x fp8 -> f32 acc; bf16 rope; bf16 out", "data": "synthetic",
            "config": {"workload": "DeepSeek-V3 MLA decode, per-token fp8 KV, bs=128/GPU seq=4096 H=128 (TP=1), page=64, "
                                   "pages randomly permuted, K3 metadata once + 61 layers x (K5 store + K4 quant-q + K1 decode) per step",
                       "bs_per_gpu": BS, "seq_len": SEQ, "heads": H, "layers_per_step": layers,
                       "parallelism": f"dp{world} (DP-attention, no data-path collective)", "hipgraph": graph_ok,
                       "launches_per_layer": 2 if FUSED_QUANT else 3,
                       "quant_launch": "K5 + K4 fused (flash_mla_fp8.quantize_q_and_cache_k)" if FUSED_QUANT else "K5, K4 separate"},
            "roofline": roof, "gemm": gemm, "variants": variants, "cpu_baseline": cpu}


def measure_cfg4(a, dev, world, rank, dist, layers, steps, warmup, stages=False):
    """-> the config-4 record (all ranks compute it; rank 0 prints / embeds it)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import cfg4_layer

    step, info = cfg4_layer.build(dev, world, rank, None, layers)
    step()
    torch.cuda.synchronize()
    graph, why = None, None
    if not a.no_graph:
        try:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                step()
            torch.cuda.current_stream().wait_stream(s)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step()
        except Exception as ex:   # a refused capture is reported, not hidden: the step then runs eagerly
            graph, why = None, f"{type(ex).__name__}: {ex}"[:200]
            torch.cuda.synchronize()
    run = graph.replay if graph is not None else step
    for _ in range(warmup):
        run()

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        run()
    barrier()
    dt = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    ms_per_step = dt / steps * 1e3
    stage_ms = info["_stage_times"]() if stages else None
    return {
            "stage_ms": stage_ms,
            "metric": "decode tokens/s, DeepSeek-V3 decoder layers at BASELINE config 4 (attention-TP + EP MoE, bs=256 seq=8k), scaled to 61 layers",
            "value": round(info["bs"] / (ms_per_step * 1e-3) * (layers / LAYERS), 1), "unit": "tokens/s", "n_gpus": world,
            "steps": steps, "warmup": warmup, "ms_per_step": round(ms_per_step, 4), "ms_per_layer": round(ms_per_step / layers, 4),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "fp8_e4m3 x fp8 -> f32 acc (attention, GEMMs); bf16 activations on the wire", "data": "synthetic",
            "config": {"workload": f"DeepSeek-V3 decoder layer x{layers}, data-connected (qkv_a -> C7 -> q_b -> absorb+RoPE+K5+K4 -> K1 -> bmm_v -> o_proj -> "
                                   f"C6 -> router -> EP -> experts || shared expert): TP{world} MLA decode (H={info['heads_per_rank']}/rank, bs=256 "
                                   f"seq=8192) + EP{world} MoE ({info['experts_per_rank']} experts/rank, top-8), all-gather + "
                                   "reduce-scatter + EP dispatch/combine inside the step",
                       "layers_per_step": layers, "parallelism": f"tp{world}/ep{world}", "hipgraph": graph is not None,
                       "hipgraph_refused": why, **{k: v for k, v in info.items() if not k.startswith("_")}},
            "roofline": None, "cpu_baseline": None}


def main_cfg4(a, dev, world, rank, dist):
    """BASELINE config 4 (TP8/EP8 decoder layers, bs=256, seq=8192): the multi-rank form of the path, every collective a
    real RCCL call inside the captured step.  The global batch is fixed (strong scaling); `value` = tokens/s of the job
    scaled to 61 layers.  Static shapes throughout, so the step is one hipGraph (eager if the capture is refused)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import cfg4_layer

    layers = a.layers if a.layers != LAYERS else (2 if world == 1 else 4)
    rec = measure_cfg4(a, dev, world, rank, dist, layers, a.steps, a.warmup)
    if rank == 0:
        print(json.dumps(rec))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
