"""GPU: paged GQA attention over an fp8 (e4m3fn) KV cache (csrc/gqa_paged_fp8kv.hip) through `flashinfer.BatchDecodeWithPagedKVCacheWrapper`
and `BatchPrefillWithPagedKVCacheWrapper`, against the fp64 statement of test_gqa_paged_gpu.py on the DEQUANTISED cache (k8 * k_scale,
v8 * v_scale, gathered by kv_indices).  Pools are (randn / scale) in e4m3fn, so the dequantised values have unit variance; they are larger
than the tokens used, kv_indices is a permutation that avoids slot 0, and slot 0 holds the NaN byte 0x7F: a stray fetch or a clamp shows up
as a non-finite output.  Bounds: `check`'s, unchanged (rel-MAE < 6e-3, max-abs < 5e-2, lse within 2e-3, -inf positions equal) — the
dequantisation is exact, the scales are applied in fp32 and the rest is the bf16 kernel's arithmetic.  Shapes sit on the 64-token edge of
the row form's tile, the 128-token edge of the decode form's, its 32 tokens per wave, and the split counts 16 / 1."""
import pytest
import torch

from test_gqa_paged_gpu import DEV, PREFILL, SCALE, check, indptr, ragged, ref_attention, workspace

pytestmark = pytest.mark.gpu
FP8 = torch.float8_e4m3fn


def make_case(qo_lens, kv_lens, Hq, Hkv, scales, rescale=False):
    """q, the two fp8 pools, kv_indices, and the dequantised pools (fp32) — on the CPU"""
    ks, vs = (1.0 if s is None else s for s in scales)
    g = torch.Generator().manual_seed(11 + len(qo_lens) + sum(kv_lens) + Hq)
    Tk = sum(kv_lens)
    q = torch.randn(sum(qo_lens), Hq, 128, generator=g).to(torch.bfloat16)
    kp, vp = ((torch.randn(Tk + 37, Hkv, 128, generator=g) / s).to(FP8) for s in (ks, vs))
    kp.view(torch.uint8)[0], vp.view(torch.uint8)[0] = 0x7F, 0x7F
    kd, vd = kp.float() * ks, vp.float() * vs
    idx = (torch.randperm(Tk + 36, generator=g)[:Tk] + 1).to(torch.int32)
    if rescale:   # q x 8, keys in rising order of the first head's score: the row maximum moves tile after tile and slice after slice
        q = (q.float() * 8).to(torch.bfloat16)
        idx = idx[torch.argsort(kd[idx.long(), 0] @ q[0, 0].float())]
    return q, kp, vp, idx, kd, vd


def run_paged(qo_lens, kv_lens, Hq, Hkv, causal, scales, q_len_fixed=False, rescale=False):
    """qo_lens None: the decode wrapper over [slots, Hkv, 128] pools, else the paged prefill wrapper over [pages, 1, Hkv, 128] pools"""
    import flashinfer

    decode = qo_lens is None
    qo_lens = [1] * len(kv_lens) if decode else qo_lens
    q, kp, vp, idx, kd, vd = make_case(qo_lens, kv_lens, Hq, Hkv, scales, rescale)
    ones = torch.ones(len(kv_lens), dtype=torch.int32, device=DEV)
    if decode:
        w = flashinfer.BatchDecodeWithPagedKVCacheWrapper(workspace(), "NHD")
        w.begin_forward(indptr(kv_lens).to(DEV), idx.to(DEV), ones, Hq, Hkv, 128, 1, data_type=FP8, q_data_type=torch.bfloat16)
        o, lse = w.forward_return_lse(q.to(DEV), (kp.to(DEV), vp.to(DEV)), sm_scale=SCALE, k_scale=scales[0], v_scale=scales[1])
    else:
        w = flashinfer.BatchPrefillWithPagedKVCacheWrapper(workspace(), "NHD")
        w.begin_forward(indptr(qo_lens).to(DEV), indptr(kv_lens).to(DEV), idx.to(DEV), ones, Hq, Hkv, 128, 1, q_data_type=torch.bfloat16,
                        kv_data_type="float8_e4m3fn", q_len_fixed=q_len_fixed)
        o, lse = w.forward_return_lse(q.to(DEV), (kp.to(DEV)[:, None], vp.to(DEV)[:, None]), causal=causal, sm_scale=SCALE,
                                      k_scale=scales[0], v_scale=scales[1])
    torch.cuda.synchronize()
    assert o.shape == q.shape and o.dtype == torch.bfloat16 and lse.shape == q.shape[:2] and lse.dtype == torch.float32
    return (o, lse) + ref_attention(q, kd[idx.long()], vd[idx.long()], qo_lens, kv_lens, causal)


EDGES = [1, 63, 64, 65, 127, 128, 129, 300]   # B * Hkv <= 32 -> 16 slices on 256 CUs, most of them empty
DECODE = [(4, 4, EDGES, False, (None, None)), (8, 2, EDGES, False, (0.5, 2.0)), (16, 1, EDGES, False, (0.37, 1.9)),
          (16, 8, [1 + (7 * i) % 130 for i in range(64)], False, (0.5, 2.0)),   # B * Hkv = 512 -> S = 1
          (4, 1, [4000], True, (0.37, 1.9))]                                    # 16 live slices of 2 tiles


@pytest.mark.parametrize("Hq,Hkv,kv_lens,rescale,scales", DECODE)
def test_decode_matches_fp64(Hq, Hkv, kv_lens, rescale, scales):
    check(*run_paged(None, kv_lens, Hq, Hkv, False, scales, rescale=rescale), f"fp8 decode Hq={Hq} Hkv={Hkv} B={len(kv_lens)} {scales}")


@pytest.mark.parametrize("qo_lens,kv_lens,Hkv,causal,q_len_fixed", PREFILL)
def test_paged_prefill_extend_verify_match_fp64(qo_lens, kv_lens, Hkv, causal, q_len_fixed):
    check(*run_paged(qo_lens, kv_lens, 8, Hkv, causal, (0.37, 1.9), q_len_fixed), f"fp8 paged {qo_lens} x {kv_lens} Hkv={Hkv} causal={causal}")


def test_ragged_bf16_over_new_tokens_merged_with_paged_fp8_over_the_prefix_equals_causal_attention_over_the_whole_context():
    """flashinfer_backend.py:534-550; the second request has no prefix.  The merge weighs the two states by their lse: it is right only if
    the fp8 state's lse carries k_scale"""
    import flashinfer
    import flashinfer.cascade

    new, prefix, Hq, Hkv, scales = [70, 33, 5], [100, 0, 260], 8, 2, (0.37, 1.9)
    q, kp, vp, idx, kd, vd = make_case(new, prefix, Hq, Hkv, scales)
    g = torch.Generator().manual_seed(3)
    kn, vn = (torch.randn(sum(new), Hkv, 128, generator=g).to(torch.bfloat16) for _ in range(2))
    o1, s1 = ragged(new, new, Hq, Hkv, q, kn, vn, True)
    w = flashinfer.BatchPrefillWithPagedKVCacheWrapper(workspace(), "NHD")
    w.begin_forward(indptr(new).to(DEV), indptr(prefix).to(DEV), idx.to(DEV), torch.ones(3, dtype=torch.int32, device=DEV), Hq, Hkv, 128, 1,
                    q_data_type=torch.bfloat16, kv_data_type=FP8)
    o2, s2 = w.forward_return_lse(q.to(DEV), (kp.to(DEV), vp.to(DEV)), causal=False, sm_scale=SCALE, k_scale=scales[0], v_scale=scales[1])
    o, s = flashinfer.cascade.merge_state(o1, s1, o2, s2)
    torch.cuda.synchronize()
    cat = lambda a, b: torch.cat([torch.cat(t) for t in zip(a.split(prefix), b.split(new))])
    ro, rl = ref_attention(q, cat(kd[idx.long()], kn.float()), cat(vd[idx.long()], vn.float()), new, [a + b for a, b in zip(prefix, new)], True)
    check(o, s, ro, rl, "ragged bf16 + paged fp8 prefix")


def test_captured_decode_replays_with_new_lengths_and_indices():
    import flashinfer

    Hq, Hkv, lens_a, lens_b, scales = 8, 2, [300, 5, 64], [1, 190, 129], (0.5, 2.0)
    q, kp, vp, idx_b, kd, vd = make_case([1, 1, 1], lens_b, Hq, Hkv, scales)
    idx_a = torch.arange(1, 1 + sum(lens_a), dtype=torch.int32)
    bufs = [torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(512, dtype=torch.int32, device=DEV), torch.ones(3, dtype=torch.int32, device=DEV)]
    w = flashinfer.BatchDecodeWithPagedKVCacheWrapper(workspace(), "NHD", use_cuda_graph=True, paged_kv_indptr_buffer=bufs[0],
                                                      paged_kv_indices_buffer=bufs[1], paged_kv_last_page_len_buffer=bufs[2])
    plan = lambda lens, idx: w.begin_forward(indptr(lens).to(DEV), idx.to(DEV), bufs[2], Hq, Hkv, 128, 1, data_type=FP8,
                                             q_data_type=torch.bfloat16, non_blocking=True)
    qd, kv = q.to(DEV), tuple(torch.cat([t.to(DEV).view(torch.uint8)] * 2).view(FP8) for t in (kp, vp))   # (room for lens_a's slots)
    run = lambda: w.forward(qd, kv, sm_scale=SCALE, k_scale=scales[0], v_scale=scales[1])
    plan(lens_b, idx_b)
    eager = run().clone()   # (also loads the kernels before the capture)
    plan(lens_a, idx_a)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    plan(lens_b, idx_b)
    ro, _ = ref_attention(q, kd[idx_b.long()], vd[idx_b.long()], [1, 1, 1], lens_b, False)
    for replay in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager), replay
    check(out, None, ro, None, "fp8 graph replay")


def test_unsupported_fp8_calls_are_refused_at_run():
    import flashinfer

    q = torch.zeros(2, 8, 128, dtype=torch.bfloat16, device=DEV)
    kv16 = tuple(torch.zeros(8, 2, 128, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    kv = tuple(torch.zeros(8, 2, 128, dtype=torch.uint8, device=DEV).view(FP8) for _ in range(2))
    ip, ones, idx = indptr([3, 4]).to(DEV), torch.ones(2, dtype=torch.int32, device=DEV), torch.arange(7, dtype=torch.int32, device=DEV)

    def planned(dt):
        d = flashinfer.BatchDecodeWithPagedKVCacheWrapper(workspace(), "NHD")
        d.begin_forward(ip, idx, ones, 8, 2, 128, 1, data_type=dt)
        p = flashinfer.BatchPrefillWithPagedKVCacheWrapper(workspace(), "NHD")
        p.begin_forward(indptr([1, 1]).to(DEV), ip, idx, ones, 8, 2, 128, 1, kv_data_type=dt)
        return d, p

    for w in planned(FP8):
        w.forward(q, kv, k_scale=0.5, v_scale=2)   # the served call, so that each refusal below is about ONE thing
        for bad in (dict(k_scale=0.0), dict(v_scale=-1.0), dict(k_scale=float("nan")), dict(v_scale=torch.ones(1, device=DEV))):
            with pytest.raises(RuntimeError):
                w.forward(q, kv, **bad)
        for pools in (kv16, tuple(t.view(torch.uint8) for t in kv), tuple(t.view(torch.float8_e5m2) for t in kv)):
            with pytest.raises(RuntimeError):
                w.forward(q, pools)
        with pytest.raises(RuntimeError):
            w.forward(q.to(FP8), kv)
    for w in planned(torch.bfloat16) + planned(torch.float8_e5m2):   # bf16 planned with fp8 pools; an e5m2 plan
        with pytest.raises(RuntimeError):
            w.forward(q, kv)
