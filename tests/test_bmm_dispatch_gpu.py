"""MI355X: every dispatch branch of the small bf16 GEMMs (csrc/bmm_bf16.hip: `bmm_bf16_nt_kernel<4 / 16>`, the five forms of
`bmm_bf16_wlds_kernel`, `router_partial_kernel` + `router_reduce_kernel`) through `fluent_mi355.bmm.bmm`, `flashinfer.dsv3_router_gemm` and
`flashinfer.dsv3_fused_a_gemm`, at shapes chosen for the branch and not for a call site.  tests/test_bmm_gpu.py holds the call-site shapes.

Two kinds of input per case:
* integers from {-3 .. 3} stored as bf16: every product and partial sum is an integer of magnitude <= 9 K <= 73,728 < 2^24, exact in fp32 under
  ANY accumulation order or split — the f32 output is `torch.equal` to the exact product, the bf16 output bit-equal to the exact product rounded
  once (RNE; sums above 256 land on ties).  No tolerance: a dropped, doubled or misplaced k step, a wrong row, column or split range shows.
* Gaussian (A ~ N(0,1), B ~ 0.05 N(0,1), 0.02 for the router shapes) against the fp64 product of the same bf16 values under the bounds of
  tests/test_bmm_gpu.py: bf16 out |got - bf16(ref)| <= 2^-7 |ref| + 2e-3 elementwise; f32 out max|got - ref| <= 1e-4 max|ref| + 1e-4.
An output handed in as a view lies in a parent filled with a sentinel, with spare rows behind row M - 1: nothing outside the view may change.
Operand views lie in parents whose margins hold 2^100: a read outside the view shows in the result.

Worst measured on MI355X (Gaussian cases): f32 out max|got - ref| 3.0e-6 against a bound of 1.8e-3 (g6, M = 16; 0.002 of its bound in every
case); bf16 out: one bf16 ulp where the fp32 sum sits beside a rounding boundary — worst err / (2^-7 |ref| + 2e-3) 0.76 (w3; 0.58 at g6,
0.49 at r7, 0.42 at r3, 0.30 at w2), bit-equal to bf16(ref) in 20 of the 31 bf16 cases.  Every integer case is exact."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
SENT = -(2.0 ** 100)      # exact in bf16 and f32; no result comes near it
MARGIN = 2.0 ** 100


@functools.lru_cache(maxsize=None)
def operands(kind, B, M, N, K, b_scale=0.05):
    """(a [B, M, K] bf16, w [B, N, K] bf16, the fp64 product [B, M, N] of exactly these values) on the CPU; shared, never written"""
    g = torch.Generator().manual_seed(B * 1000003 + M * 10007 + N * 101 + K + (kind == "int"))
    if kind == "int":
        a = torch.randint(-3, 4, (B, M, K), generator=g).to(BF16)
        w = torch.randint(-3, 4, (B, N, K), generator=g).to(BF16)
    else:
        a = torch.randn(B, M, K, generator=g).to(BF16)
        w = (torch.randn(B, N, K, generator=g) * b_scale).to(BF16)
    ref = torch.einsum("bmk,bnk->bmn", a.double(), w.double()) + 0.0    # (+ 0.0: an all-(-0) sum is +0 in the kernel's accumulator)
    return a, w, ref


def compare(got, ref, kind, label):
    """integer inputs: exact; Gaussian: the two bounds of tests/test_bmm_gpu.py.  Prints the figure before it asserts."""
    got = got.cpu()
    assert got.shape == ref.shape, (label, got.shape, ref.shape)
    if kind == "int":
        if got.dtype == F32:
            same = torch.equal(got, ref.float())
        else:
            same = torch.equal(got.contiguous().view(torch.int16), ref.float().to(BF16).view(torch.int16))
        print(f"{label}: exact {'ok' if same else 'MISMATCH'}")
        assert same, label
    elif got.dtype == F32:
        err, bound = float((got.double() - ref).abs().max()), 1e-4 * float(ref.abs().max()) + 1e-4
        print(f"{label}: f32 max|got - ref| {err:.3e} (bound {bound:.3e}, ratio {err / bound:.3f})")
        assert err <= bound, (label, err, bound)
    else:
        err = (got.double() - ref.to(BF16).double()).abs()
        ratio = float((err / (ref.abs() * 2.0 ** -7 + 2e-3)).max())
        print(f"{label}: bf16 max|got - bf16(ref)| {float(err.max()):.3e}, worst err / (2^-7 |ref| + 2e-3) {ratio:.3f}")
        assert ratio <= 1.0, (label, ratio)


def lay_a(a, layout):
    if layout == "callsite":      # x.transpose(0, 1) of a [M, B, K + 64] tensor (deepseek_v2.py:840: q_nope out of [T, H, 192])
        B, M, K = a.shape
        x = torch.full((M, B, K + 64), MARGIN, dtype=BF16, device=DEV)
        x[..., :K] = a.transpose(0, 1).to(DEV)
        return x[..., :K].transpose(0, 1)
    return a.to(DEV)


def lay_b(w, layout):
    """the [B, K, N] k-contiguous view of the weight rows [B, N, K]"""
    if layout == "b_stride_136":  # rows of a wider buffer: b_stride_n = K + 8
        B, N, K = w.shape
        buf = torch.full((B, N, K + 8), MARGIN, dtype=BF16, device=DEV)
        buf[..., :K] = w.to(DEV)
        return buf[..., :K].transpose(1, 2)
    return w.to(DEV).transpose(1, 2)


def lay_out(B, M, N, dtype, layout):
    """(sentinel-filled parent, view function): three spare rows behind row M - 1 in every layout"""
    if layout == "callsite":      # a transposed view into a wider tensor (deepseek_v2.py:840: out=Q[..., :512].transpose(0, 1))
        return torch.full((M + 3, B, N + 64), SENT, dtype=dtype, device=DEV), lambda p: p[:M, :, :N].transpose(0, 1)
    if layout == "c_plus_8_bytes":  # bf16: 8-byte aligned only, row stride N + 4 = 4 mod 8
        return torch.full((B, M + 3, N + 4), SENT, dtype=dtype, device=DEV), lambda p: p[:, :M, 4:]
    return torch.full((B, M + 3, N), SENT, dtype=dtype, device=DEV), lambda p: p[:, :M]


def run_bmm(kind, shape, dtype, label, a_layout=None, b_layout=None, c_layout=None):
    from fluent_mi355.bmm import bmm
    B, M, N, K = shape
    a, w, ref = operands(kind, B, M, N, K)
    parent, view = lay_out(B, M, N, dtype, c_layout)
    out = view(parent)
    assert out.shape == (B, M, N)
    res = bmm(lay_a(a, a_layout), lay_b(w, b_layout), out=out)
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr()
    got = out.cpu()
    view(parent).fill_(SENT)
    assert bool((parent == SENT).all()), f"{label}: an element outside the output view was written"
    compare(got, ref, kind, label)


# ---- bmm_bf16_nt_kernel: the generic kernel (dispatch: fl_bmm_bf16_nt, after the LDS-resident form has been ruled out;
#      ksplit = 16 / 4 when batch * ceil(M / 32) * (N / 32) < 512 and K >= 4096 / 1024, else 1: four n tiles per workgroup) ----
GENERIC = {
    # K = 16 is neither 128 nor 512 -> generic; K < 1024 -> ksplit 1; only the 16-step tail loop runs; one n tile: waves 1-3 have none
    "g1": dict(shape=(1, 1, 32, 16), dtypes=(F32, BF16)),
    # ksplit 1; K = 80 = 64 + 16: the 64-step loop once, the tail once; M = 70: a 6-row tail tile; 3 n tiles in one group (wave 3 idle)
    "g2": dict(shape=(3, 70, 96, 80), dtypes=(F32, BF16)),
    # ksplit 1; K = 208 = 128 + 64 + 16: all three loops once; 5 n tiles: the second group has one live tile
    "g3": dict(shape=(2, 33, 160, 208), dtypes=(F32, BF16)),
    # the absorption shape K = 128, N = 512, but f32 out: the LDS-resident form is bf16-only -> generic, ksplit 1 (K < 1024)
    "g4a": dict(shape=(2, 37, 512, 128), dtypes=(F32,)),
    # the same, bf16 out at parent[..., 4:] of a [B, M + 3, 516] tensor: C is 8-byte aligned only and c_stride_m = 516 is 4 mod 8 -> generic
    "g4b": dict(shape=(2, 37, 512, 128), dtypes=(BF16,), c_layout="c_plus_8_bytes"),
    # the same, bf16 out, weight rows of stride 136 != K -> generic
    "g4c": dict(shape=(2, 37, 512, 128), dtypes=(BF16,), b_layout="b_stride_136"),
    # 2 tiles < 512, 1024 <= K < 4096: the 4-wave k split, per = ceil(65 / 4) * 16 = 272: ranges 272, 272, 272, 224
    "g5": dict(shape=(1, 40, 32, 1040), dtypes=(F32, BF16)),
    # 3 tiles < 512, K >= 4096: the 16-wave k split, per = ceil(257 / 16) * 16 = 272: waves 0-14 take 272, wave 15 takes 32
    "g7": dict(shape=(1, 5, 96, 4112), dtypes=(F32, BF16)),
}


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("name,dtype", [(n, d) for n, c in GENERIC.items() for d in c["dtypes"]],
                         ids=lambda v: v if isinstance(v, str) else str(v).split(".")[-1])
def test_generic_kernel(name, dtype, kind):
    c = GENERIC[name]
    run_bmm(kind, c["shape"], dtype, f"{name} {kind} {dtype}", b_layout=c.get("b_layout"), c_layout=c.get("c_layout"))


# g6: the model's own dsv3_fused_a_gemm shape, <= 16 tokens, 7168 -> 2112: 66 tiles < 512 and K >= 4096 -> bmm_bf16_nt_kernel<16>,
# per = 448 = 3 * 128 + 64 for every wave.  bf16 through dsv3_fused_a_gemm (its only output type); f32 through bmm on the same operands.
@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("M", [1, 16])
def test_fused_a_gemm_at_the_model_shape(M, dtype, kind):
    import flashinfer
    a, w, ref = operands(kind, 1, 16, 2112, 7168)
    label = f"g6 M={M} {kind} {dtype}"
    if dtype == F32:
        from fluent_mi355.bmm import bmm
        parent, view = lay_out(1, M, 2112, F32, None)
        bmm(a[:, :M].to(DEV), lay_b(w, None), out=view(parent))
        torch.cuda.synchronize()
        got = view(parent)[0].cpu()
        view(parent).fill_(SENT)
        assert bool((parent == SENT).all()), f"{label}: an element outside the output view was written"
    else:
        got = flashinfer.dsv3_fused_a_gemm(a[0, :M].to(DEV), w[0].to(DEV).t())      # weight_t [K, N]: the k-contiguous view of [N, K]
        torch.cuda.synchronize()
        assert got.dtype == BF16
    compare(got, ref[0, :M], kind, label)


# ---- bmm_bf16_wlds_kernel<KS, MT2, BY_M>: bf16 out, K = 128 / 512, N K 2 <= 128 KiB, b_stride_n = K, 16-byte aligned output rows.
#      M <= 32: <.., 1, false>, wave w takes n tiles w, w + 4, ..; M > 32: <.., 1, true>, wave w takes token rows 32 w ..;
#      K = 128 and batch * ceil(M / 128) > 512: <8, 2, true>, two token tiles per wave.  An odd N / 32 is never sliced (n_splits 1). ----
WLDS = {}
for _N in (32, 96, 160):          # w1, K = 128 (CH == 1: two n tiles per trip): 1 / 3 / 5 tiles
    WLDS[f"w1 N={_N} M=1"] = dict(shape=(3, 1, _N, 128))     # <8,1,false>: by n; N = 160: five tiles over four waves (wave 0 takes 0 and 4)
    WLDS[f"w1 N={_N} M=33"] = dict(shape=(3, 33, _N, 128))   # <8,1,true>: by m; wave 1 has one live row; odd tile counts end a trip half way
for _N in (32, 96):               # w2, K = 512 (CH == 4)
    WLDS[f"w2 N={_N} M=7"] = dict(shape=(2, 7, _N, 512))     # <32,1,false>
    WLDS[f"w2 N={_N} M=40"] = dict(shape=(2, 40, _N, 512))   # <32,1,true>: wave 1 has 8 live rows
# w3: 520 > 512 workgroups of 128 rows -> <8,2,true>, 256 rows per workgroup: wave 0's second tile holds one live row, waves 1-3 none
WLDS["w3"] = dict(shape=(520, 33, 64, 128))
# w4: the call sites' layout — A = x.transpose(0, 1) of [M, B, K + 64], out a transposed view into a wider tensor
WLDS["w4 K=128"] = dict(shape=(3, 33, 160, 128), a_layout="callsite", c_layout="callsite")   # <8,1,true>
WLDS["w4 K=512"] = dict(shape=(2, 7, 96, 512), a_layout="callsite", c_layout="callsite")     # <32,1,false>


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("name", list(WLDS))
def test_lds_resident_weight_kernel(name, kind):
    c = WLDS[name]
    run_bmm(kind, c["shape"], BF16, f"{name} {kind}", a_layout=c.get("a_layout"), c_layout=c.get("c_layout"))


# ---- router_partial_kernel + router_reduce_kernel through dsv3_router_gemm(x [T, K], w [E, K]): E % 64 == 0, K % 64 == 0, rows 16-byte
#      aligned, workspace <= 64 MiB.  (T, E, K) -> (ksplit, kc) as rt_pick_ksplit chooses them (pinned in tests/test_bmm_cpu.py) ----
ROUTER = {
    "r1": ((5, 64, 64), (1, 64)),            # one split: the reduce adds one partial (lanes 1-7 of a group add nothing)
    "r2": ((5, 64, 192), (3, 64)),           # fewer than 8 splits: the clamped loads
    "r3": ((200, 192, 448), (7, 64)),        # M tail of 8 rows in the fourth m tile; three n tiles
    "r4": ((65, 64, 7168), (112, 64)),       # ksplit > 64: the second trip of the reduce loop; one row in the second m tile
    "r5": ((1, 64, 8192), (128, 64)),        # two full trips of the reduce loop
    "r6": ((3, 768, 6144), (24, 256)),       # kc = 256; twelve n tiles
    "r7": ((130, 512, 6144), (12, 512)),     # kc = 512: the largest slab; ksplit no multiple of 8; two rows in the third m tile
    "r8": ((33, 128, 1536), (24, 64)),       # x and w are column slices [:, 8 : 8 + K] of buffers with row stride K + 16
}


def router_operands(kind, T, E, K, strided=False):
    a, w, ref = operands(kind, 1, T, E, K, 0.02)
    if not strided:
        return a[0].to(DEV), w[0].to(DEV), ref[0]
    xb = torch.full((T, K + 16), MARGIN, dtype=BF16, device=DEV)
    wb = torch.full((E, K + 16), MARGIN, dtype=BF16, device=DEV)
    xb[:, 8:8 + K] = a[0].to(DEV)
    wb[:, 8:8 + K] = w[0].to(DEV)
    return xb[:, 8:8 + K], wb[:, 8:8 + K], ref[0]


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("name", list(ROUTER))
def test_splitk_router_path(name, dtype, kind):
    import flashinfer
    from fluent_mi355._lib import lib
    (T, E, K), (ks, kc) = ROUTER[name]
    need = int(lib.fl_gemm_bf16_nt_splitk_workspace_bytes(T, E, K))
    assert need == ks * 4 * T * E and K // ks == kc and 0 < need <= 64 << 20       # the case takes the branch it was written for
    x, w, ref = router_operands(kind, T, E, K, strided=name == "r8")
    out = flashinfer.dsv3_router_gemm(x, w, out_dtype=dtype)
    torch.cuda.synchronize()
    assert out.dtype == dtype
    compare(out, ref, kind, f"{name} {kind} {dtype}")
    if name in ("r3", "r4"):                                                        # the reduce adds in a fixed order: run to run bit-equal
        again = flashinfer.dsv3_router_gemm(x, w, out_dtype=dtype)
        torch.cuda.synchronize()
        assert torch.equal(out, again)


# f1: E = 96 is no multiple of 64 -> out of the split-K form into fl_bmm_bf16_nt: 2 x 3 tiles < 512, K >= 4096 -> bmm_bf16_nt_kernel<16>
@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
def test_router_gemm_falls_back_when_E_is_no_multiple_of_64(dtype, kind):
    import flashinfer
    from fluent_mi355._lib import lib
    T, E, K = 33, 96, 7168
    assert int(lib.fl_gemm_bf16_nt_splitk_workspace_bytes(T, E, K)) == 0
    x, w, ref = router_operands(kind, T, E, K)
    out = flashinfer.dsv3_router_gemm(x, w, out_dtype=dtype)
    torch.cuda.synchronize()
    assert out.dtype == dtype
    compare(out, ref, kind, f"f1 {kind} {dtype}")


# f2: the split-K workspace would be 14 * 4682 * 256 * 4 = 67,121,152 B > 64 MiB = 67,108,864 B -> fl_bmm_bf16_nt: 147 x 8 tiles >= 512
# -> the generic kernel WITHOUT k split at K = 7168 (56 trips of the 128-step loop).  One call; the reference is one fp32 product on the
# CPU, exact for these integers.
def test_router_gemm_falls_back_when_the_workspace_exceeds_its_cap():
    import flashinfer
    from fluent_mi355._lib import lib
    T, E, K = 4682, 256, 7168
    assert int(lib.fl_gemm_bf16_nt_splitk_workspace_bytes(T, E, K)) == 67121152 > 64 << 20
    g = torch.Generator().manual_seed(4682)
    x = torch.randint(-3, 4, (T, K), generator=g, dtype=torch.int8)
    w = torch.randint(-3, 4, (E, K), generator=g, dtype=torch.int8)
    out = flashinfer.dsv3_router_gemm(x.to(DEV).to(BF16), w.to(DEV).to(BF16), out_dtype=F32)
    torch.cuda.synchronize()
    ref = x.float() @ w.float().t()
    assert out.dtype == F32 and out.shape == (T, E)
    same = torch.equal(out.cpu(), ref)
    print(f"f2 int float32: exact {'ok' if same else 'MISMATCH'}")
    assert same


# f3: no tokens
def test_router_gemm_of_no_tokens_is_empty():
    import flashinfer
    w = torch.zeros(128, 256, dtype=BF16, device=DEV)
    for dtype in (F32, BF16):
        out = flashinfer.dsv3_router_gemm(torch.zeros(0, 256, dtype=BF16, device=DEV), w, out_dtype=dtype)
        assert out.shape == (0, 128) and out.dtype == dtype


# r10: a captured dsv3_router_gemm (two kernel nodes in sequence on one stream) reads its inputs at replay time and owns its workspace:
# the eager call's shared workspace is replaced between capture and replay, and the replays are not disturbed.
def test_captured_router_gemm_replays_with_new_inputs_and_its_own_workspace():
    import flashinfer
    from fluent_mi355 import bmm as bmm_mod
    T, E, K = 33, 256, 7168
    g = torch.Generator().manual_seed(10)
    x1, x2 = (torch.randint(-3, 4, (T, K), generator=g).to(BF16) for _ in range(2))
    w = torch.randint(-3, 4, (E, K), generator=g).to(BF16)
    big = torch.randint(-3, 4, (1100, K), generator=g).to(BF16)
    refs = [(xx.float() @ w.float().t()) for xx in (x1, x2, big)]                    # exact in fp32
    x, wd = x1.to(DEV), w.to(DEV)
    torch.cuda.synchronize()
    bmm_mod._splitk_ws.clear()                     # the eager workspace starts at its 8 MiB floor whatever ran before in this process
    eager = flashinfer.dsv3_router_gemm(x, wd)     # warm-up outside the capture
    torch.cuda.synchronize()
    assert torch.equal(eager.cpu(), refs[0])
    ws_before = dict(bmm_mod._splitk_ws)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = flashinfer.dsv3_router_gemm(x, wd)
    assert bmm_mod._splitk_ws.keys() == ws_before.keys() and all(bmm_mod._splitk_ws[k] is v for k, v in ws_before.items())   # the capture took no eager workspace
    # an eager call at T = 1100: 14 * 1100 * 256 * 4 B = 15.8 MB > 8 MiB — the shared eager workspace is regrown (the old one is freed)
    eager_big = flashinfer.dsv3_router_gemm(big.to(DEV), wd)
    torch.cuda.synchronize()
    (ws_now,) = bmm_mod._splitk_ws.values()
    assert ws_now.numel() >= 14 * 1100 * 256 * 4 and all(ws_now is not v for v in ws_before.values())
    assert torch.equal(eager_big.cpu(), refs[2])
    x.copy_(x2)                                    # new inputs, in place
    for _ in range(2):
        out.fill_(SENT)
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), refs[1])
