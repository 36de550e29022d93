"""MI355X: G5, the bf16 grouped GEMM behind eps.executor.AokGroupedGemm (csrc/grouped_gemm_bf16.hip), against A.double() @ W[e].double().T per group.
Bound of tests/test_bmm_gpu.py: |got - bf16(ref)| <= |ref| 2^-7 + 2e-3 elementwise.  `out` is pre-filled with 7.0: rows outside the groups must keep it."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROUTING, ROWS = (3, 3, 4, 37, 167), 176   # leading offset, empty group, 1 row, 33 rows, 130 rows (cross the 32- / 128-row tile), trailing buffer rows
Z = functools.partial(torch.zeros, dtype=torch.bfloat16, device=DEV)


def reference(a, w, ex):
    ref = torch.full((a.shape[0], w.shape[1]), float("nan"), dtype=torch.float64)
    for e in range(len(ex) - 1):
        ref[ex[e]:ex[e + 1]] = a[ex[e]:ex[e + 1]].double() @ w[e].double().T
    return ref


@functools.lru_cache(maxsize=None)
def case(ex, M, N, K):
    # (A, W) bf16 on the host, seeded per case, and the fp64 reference [M, N] (rows outside the groups: NaN)
    g = torch.Generator().manual_seed(1000 * K + N + len(ex))
    a = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (0.05 * torch.randn(len(ex) - 1, N, K, generator=g)).to(torch.bfloat16)
    return a, w, reference(a, w, ex)


def check(out, ref):
    out, inside = out.cpu(), ~torch.isnan(ref[:, 0])
    assert bool((out[~inside] == 7.0).all()), "a row outside the groups was written"
    r = ref[inside]
    err = (out[inside].double() - r.to(torch.bfloat16).double()).abs()
    assert bool((err <= r.abs() * 2.0 ** -7 + 2e-3).all()), f"worst error {float(err.max()):.3e}"


def run_offset(ex, M, N, K, tile_rows, dense=False):
    from fluent_mi355.gemm import gemm_bf16_nt, m_grouped_gemm_bf16_nt_offset
    a, w, ref = case(ex, M, N, K)
    out = torch.full((M, N), 7.0, dtype=torch.bfloat16, device=DEV)
    if dense:
        gemm_bf16_nt(a.to(DEV), w[0].to(DEV), out, tile_rows)
    else:
        m_grouped_gemm_bf16_nt_offset(a.to(DEV), w.to(DEV), out, torch.tensor(ex, dtype=torch.int32, device=DEV), tile_rows)
    check(out, ref)


# K: one k block; exactly the ring depth (2 stages in the 128-row form, 3 in the 32-row form); 7 blocks.  N: half a weight tile, one tile, 2 1/2 tiles.
@pytest.mark.parametrize("tile_rows", [32, 128])
@pytest.mark.parametrize("K", [64, 128, 192, 448])
@pytest.mark.parametrize("N", [64, 128, 320])
def test_offset_mode_matches_fp64(N, K, tile_rows):
    run_offset(ROUTING, ROWS, N, K, tile_rows)


@pytest.mark.parametrize("tile_rows", [32, 128])
@pytest.mark.parametrize("E", [70, 260])
def test_many_mostly_empty_groups(E, tile_rows):
    """locate_tile past its first 64-lane round and past 256 groups: groups of 0 / 1 rows, the last one of 35"""
    ex = torch.tensor([2] + [i % 2 for i in range(E - 1)] + [35]).cumsum(0).tolist()
    run_offset(tuple(ex), ex[-1] + 3, 64, 64, tile_rows)


def test_all_groups_empty():
    run_offset((5, 5, 5, 5), 9, 64, 64, None)


@pytest.mark.parametrize("tile_rows", [32, 128])
@pytest.mark.parametrize("M", [1, 33, 130])
def test_dense_mode(M, tile_rows):
    run_offset((0, M), M, 320, 448, tile_rows, dense=True)


def test_capped_grid_walks_every_tile():
    import deep_gemm
    before = deep_gemm.get_num_sms()
    deep_gemm.set_num_sms(8)   # 30 tiles in the 32-row form
    try:
        for tile_rows in (32, 128):
            run_offset(ROUTING, ROWS, 320, 448, tile_rows)
    finally:
        deep_gemm.set_num_sms(before)
    assert deep_gemm.get_num_sms() == before


def test_graph_replay_follows_rewritten_routing():
    from fluent_mi355.gemm import AokGroupedGemm
    second = (0, 40, 41, 41, 170)
    a, w, ref1 = case(ROUTING, ROWS, 128, 192)
    ad, wd, gemm = a.to(DEV), w.to(DEV), AokGroupedGemm(4)
    ex = torch.tensor(ROUTING, dtype=torch.int32, device=DEV)
    gemm.run(ad, wd, None, ex, ROWS)   # warm-up outside the capture
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = gemm.run(ad, wd, None, ex, ROWS)
    for routing, ref in ((ROUTING, ref1), (second, reference(a, w, second))):
        ex.copy_(torch.tensor(routing, dtype=torch.int32))
        out.fill_(7.0)
        gr.replay()
        torch.cuda.synchronize()
        check(out, ref)


@pytest.mark.parametrize("hint", [16, 300])   # min(hint, M) / E < 64: the 32-row form; >= 64: the 128-row form
def test_executor_pipeline_w13_silu_w2(hint):
    """moe/executors/eps_executor.py:35-48 through the shim's names, against the fp64 composition rounded to bf16 at the same three points"""
    from eps.executor import AokGroupedGemm, silu
    g = torch.Generator().manual_seed(hint)
    E, H, I, M = 4, 128, 128, 300   # (silu serves I % 128 == 0)
    x = torch.randn(M, H, generator=g).to(torch.bfloat16)
    w13 = (0.05 * torch.randn(E, 2 * I, H, generator=g)).to(torch.bfloat16)
    w2 = (0.05 * torch.randn(E, H, I, generator=g)).to(torch.bfloat16)
    ex, gemm = torch.tensor(ROUTING, dtype=torch.int32, device=DEV), AokGroupedGemm(E)
    gate_up = gemm.run(x.to(DEV), w13.to(DEV), None, ex, hint)
    out = gemm.run(silu(gate_up, ex, hint), w2.to(DEV), None, ex, hint)
    assert out.shape == (M, H) and out.dtype == torch.bfloat16
    gu = reference(x, w13, ROUTING).to(torch.bfloat16).double()
    act = (gu[:, :I] * torch.sigmoid(gu[:, :I]) * gu[:, I:]).to(torch.bfloat16)
    out[:ROUTING[0]] = out[ROUTING[-1]:] = 7.0   # rows outside the groups of a fresh tensor are unspecified
    check(out, reference(act, w2, ROUTING))


@pytest.mark.parametrize("what,change", [
    ("third argument", lambda a: dict(third=Z(1))),
    ("float32 input", lambda a: dict(input=a["input"].float())),
    ("host input", lambda a: dict(input=a["input"].cpu())),
    ("non-contiguous input", lambda a: dict(input=Z(8, 128)[:, ::2])),
    ("non-contiguous weight", lambda a: dict(weight=Z(2, 64, 128)[:, :, ::2])),
    ("expert count", lambda a: dict(weight=Z(3, 64, 64))),
    ("int64 exclusive_sum", lambda a: dict(exclusive_sum=a["exclusive_sum"].long())),
    ("short exclusive_sum", lambda a: dict(exclusive_sum=a["exclusive_sum"][:2])),
    ("host exclusive_sum", lambda a: dict(exclusive_sum=a["exclusive_sum"].cpu())),
    ("K % 64", lambda a: dict(input=Z(8, 96), weight=Z(2, 64, 96))),
    ("N % 64", lambda a: dict(weight=Z(2, 96, 64)))])
def test_run_refuses_what_it_does_not_serve(what, change):
    from fluent_mi355.gemm import AokGroupedGemm
    a = dict(input=Z(8, 64), weight=Z(2, 64, 64), third=None, num_tokens_hint=8, exclusive_sum=torch.tensor([0, 4, 8], dtype=torch.int32, device=DEV))
    AokGroupedGemm(2).run(**a)   # the unmodified call is served
    a.update(change(a))
    with pytest.raises(RuntimeError):
        AokGroupedGemm(2).run(**a)
