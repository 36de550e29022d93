"""MI355X: G6, the W8A8 dense GEMM (csrc/gemm_w8a8.hip) behind flashinfer.fp8_scaled_mm / int8_scaled_mm, and its quantisers, against fp64.
GEMM inputs make the accumulator exact in any order (int8: i32; fp8: integers in [-8, 8], K <= 1040, partial sums < 2^24), so only the epilogue's
f32 roundings (cvt, sa, sb, bias: at most four, 2^-21 with a factor of two to spare) and the output rounding (half an ulp: r) remain:
    |got - ref| <= r |ref| + 2^-21 (|prod| + |bias|)   (+ 2^-24 for fp16),   r = 2^-8 bf16, 2^-11 fp16.
`out` is a view into a taller, wider buffer pre-filled with 7.0: everything outside [M, N] keeps it."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ELEMS = {"fp8": torch.float8_e4m3fn, "int8": torch.int8}
MS, NS = (1, 33, 130), (16, 80, 272)   # one row, across the 32- / 128-row tile; under a column tile, a ragged tile, several tiles


@functools.lru_cache(maxsize=None)
def operands(elem, K, correlated=False):
    """A [130, K], B [272, K] as int64 (exact), sa, sb f32, bias f64 — every smaller case is a leading slice."""
    g = torch.Generator().manual_seed(K + (7 if elem == "fp8" else 0))
    lim = 8 if elem == "fp8" else 127
    a = torch.randint(-lim, lim + 1, (max(MS), K), generator=g)
    b = torch.randint(-lim, lim + 1, (max(NS), K), generator=g)
    if correlated:   # column n repeats row n of A: sum a^2 ~ K 127^2 / 3
        b[:32] = a[:32]
    sa = 1e-3 + 0.02 * torch.rand(max(MS), generator=g)
    sb = 1e-3 + 0.02 * torch.rand(max(NS), generator=g)
    return a, b, sa, sb, torch.randn(max(NS), generator=g), (a.double() @ b.double().T)


def run(elem, M, N, K, tile_rows, out_dtype=torch.bfloat16, bias=True, broadcast=False, strided=False, correlated=False):
    from fluent_mi355.gemm import gemm_w8a8_nt
    a, b, sa, sb, bv, acc = operands(elem, K, correlated)
    dt = ELEMS[elem]
    a, b, sa, sb, acc = a[:M], b[:N], (sa[:1] if broadcast else sa[:M]), (sb[:1] if broadcast else sb[:N]), acc[:M, :N]
    bv = bv[:N].to(out_dtype)
    ad = a.float().to(dt).to(DEV)
    if strided:   # a column slice of a wider tensor
        wide = torch.full((M, K + 32), 3.0)
        wide[:, 16:16 + K] = a.float()
        ad = wide.to(dt).to(DEV)[:, 16:16 + K]
    buf = torch.full((M + 3, N + 8), 7.0, dtype=out_dtype, device=DEV)
    gemm_w8a8_nt(dt, ad, b.float().to(dt).to(DEV).t(), sa.to(DEV).view(-1, 1), sb.to(DEV), out_dtype, bv.to(DEV) if bias else None,
                 out=buf[:M, :N], tile_rows=tile_rows)
    got = buf.cpu().double()
    prod = acc * sa.double()[:, None] * sb.double()[None, :]
    babs = bv.double().abs()[None, :] if bias else 0.0
    ref = prod + (bv.double()[None, :] if bias else 0.0)
    r, extra = (2.0 ** -8, 0.0) if out_dtype == torch.bfloat16 else (2.0 ** -11, 2.0 ** -24)
    bound = r * ref.abs() + 2.0 ** -21 * (prod.abs() + babs) + extra
    err = (got[:M, :N] - ref).abs()
    print(f"{elem} M={M} N={N} K={K} tile_rows={tile_rows}: worst error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), f"worst error / bound {float((err / bound).max()):.3f}"
    got[:M, :N] = 7.0
    assert bool((got == 7.0).all()), "an element outside [M, N] was written"
    return acc


# K: under one MFMA k step; exactly the ring (2 x 128 in the 128-row form, 4 x 128 in the 32-row form); a ragged k tail; many blocks
@pytest.mark.parametrize("tile_rows", [32, 128])
@pytest.mark.parametrize("K", [16, 256, 512, 208, 1040])
@pytest.mark.parametrize("elem", ["fp8", "int8"])
def test_gemm_matches_fp64(elem, K, tile_rows):
    for M in MS:
        for N in NS:
            run(elem, M, N, K, tile_rows)


@pytest.mark.parametrize("tile_rows", [32, 128])
@pytest.mark.parametrize("variant", [dict(bias=False), dict(out_dtype=torch.float16), dict(broadcast=True), dict(strided=True)],
                         ids=["no_bias", "fp16_out", "broadcast_scales", "strided_a"])
@pytest.mark.parametrize("elem", ["fp8", "int8"])
def test_gemm_variants(elem, variant, tile_rows):
    run(elem, 33, 80, 208, tile_rows, **variant)


@pytest.mark.parametrize("tile_rows", [32, 128])
def test_int8_accumulator_stays_i32_past_2_to_24(tile_rows):
    acc = run("int8", 130, 80, 7168, tile_rows, correlated=True)
    assert float(acc.abs().max()) > 2.0 ** 24


def test_auto_form_and_empty_batch():
    from flashinfer import int8_scaled_mm
    run("int8", 130, 272, 208, None)   # tile_rows = 0: the library chooses
    w = torch.zeros(32, 16, dtype=torch.int8, device=DEV).t()
    out = int8_scaled_mm(torch.zeros(0, 16, dtype=torch.int8, device=DEV), w, torch.zeros(0, 1, device=DEV), torch.ones(32, device=DEV), torch.bfloat16)
    assert tuple(out.shape) == (0, 32)
    with pytest.raises(RuntimeError, match="mat_b"):
        int8_scaled_mm(torch.zeros(4, 16, dtype=torch.int8, device=DEV), w.contiguous(), torch.ones(4, device=DEV),   # row-major [K, N]
                       torch.ones(32, device=DEV), torch.bfloat16)


# ---------------------------------------------------------------------------------------------- quantisers
@functools.lru_cache(maxsize=None)
def rows(K):
    g = torch.Generator().manual_seed(K)
    x = (torch.randn(3, K, generator=g) * 10.0 ** (6 * torch.rand(3, K, generator=g) - 3)).to(torch.bfloat16)
    x[1] = 0
    return x


def check_q(x, q, s, qmax):
    """x [R, G] bf16, q [R, G], s [R] f32 (host): the fp8 / int8 bound of the rounding against the fp64 quotient"""
    t = (x.double() / s.double()[:, None]).clamp(-qmax, qmax)
    err = (q.double() - t).abs()
    bound = 2.0 ** -4 * t.abs() * (1 + 2.0 ** -10) + 2.0 ** -10 if qmax == 448 else torch.full_like(t, 0.5 + 2.0 ** -10)
    assert bool(torch.isfinite(s).all()) and bool((err <= bound).all()) and float(q.double().abs().max()) <= qmax, float((err / bound).max())


@pytest.mark.parametrize("K", [16, 208, 7168])
@pytest.mark.parametrize("elem", ["fp8", "int8"])
def test_per_token_quant(elem, K):
    import flashinfer
    x = rows(K)
    q, s = torch.empty(3, K, dtype=ELEMS[elem], device=DEV), torch.full((3, 1), float("nan"), device=DEV)
    if elem == "fp8":
        flashinfer.sgl_per_token_quant_fp8(x.to(DEV), q, s)
    else:
        flashinfer.sgl_per_token_group_quant_int8(x.to(DEV), q, s, K, 1e-10, -128, 127)
    qmax = 448 if elem == "fp8" else 127
    s_ref = x.float().abs().amax(1).clamp(min=1e-10) / qmax
    assert torch.equal(s.cpu()[:, 0], s_ref)   # bit-equal to the f32 statement
    check_q(x, q.cpu().float(), s_ref, qmax)
    assert bool((q[1].float() == 0).all())


def test_group_quant_int8():
    import flashinfer
    x = rows(384)
    q, s = torch.empty(3, 384, dtype=torch.int8, device=DEV), torch.empty(3, 3, device=DEV)
    flashinfer.sgl_per_token_group_quant_int8(x.to(DEV), q, s, 128, 1e-10, -128, 127)
    s_ref = x.float().view(9, 128).abs().amax(1).clamp(min=1e-10) / 127
    assert torch.equal(s.cpu().view(9), s_ref)
    check_q(x.view(9, 128), q.cpu().float().view(9, 128), s_ref, 127)


@pytest.mark.parametrize("is_static", [False, True])
def test_per_tensor_quant_fp8(is_static):
    import flashinfer
    x = rows(7168)
    s_ref = x.float().abs().amax().clamp(min=1e-10).view(1) / 448
    if is_static:
        s_ref = s_ref * 0.25   # a given scale under which the large values saturate
    q, s = torch.empty(3, 7168, dtype=torch.float8_e4m3fn, device=DEV), (s_ref.to(DEV) if is_static else torch.full((1,), 3e38, device=DEV))
    flashinfer.sgl_per_tensor_quant_fp8(x.to(DEV), q, s, is_static)
    assert torch.equal(s.cpu(), s_ref)
    check_q(x.view(1, -1), q.cpu().float().view(1, -1), s_ref, 448)


def test_quant_then_gemm_under_graph_capture_replays_bit_exact():
    import flashinfer
    g = torch.Generator().manual_seed(5)
    M, N, K = 5, 80, 208
    w = (torch.randn(N, K, generator=g) * 50).to(torch.float8_e4m3fn).to(DEV)
    sb = (1e-3 + 0.02 * torch.rand(N, generator=g)).to(DEV)
    xs = [torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV) for _ in range(3)]
    x, q, s = xs[0].clone(), torch.empty(M, K, dtype=torch.float8_e4m3fn, device=DEV), torch.empty(M, 1, device=DEV)

    def step():
        flashinfer.sgl_per_token_quant_fp8(x, q, s)
        return flashinfer.fp8_scaled_mm(q, w.t(), s, sb, torch.bfloat16)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for xi in xs[1:]:
        x.copy_(xi)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, step())
