"""GPU: MFMA GEMM family vs torch fp64 matmul on bf16-rounded / fp32 inputs (the kernel's own inputs),
every operand layout, every epilogue, ragged M/N/K tails, split-K.  Every case first asserts the kernel variant the planner runs it
on (tests/test_gemm_plans_gpu.py covers every variant systematically)."""
import pytest
import torch

from tests import gemm_cases as G
from tests.gpu_util import report
from tests.test_planning_cpu import _tile_rows

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
# error of the OUTPUT rounding dominates for bf16 (2^-9 relative); accumulation is fp32
TOL = {torch.bfloat16: 6e-3, torch.float32: 2e-5}


def _mk(shape, dtype, scale=1.0):
    return (torch.randn(shape, device="cuda") * scale).to(dtype)


def _plan(A, B, M, N, K, family, impl=None, **kw):
    """assert the variant (gemm_cases.FAMILIES) and epilogue implementation (IMPLS) the planner picks for this call"""
    from xpretrain_amd import hip_ops as H
    p = H.gemm(A, B, M, N, K, plan_only=True, **kw)
    got = (G.FAMILIES[p["family"]], G.IMPLS[p["epi_impl"]])
    assert got[0] == family and (impl is None or got[1] == impl), (M, N, K, kw.keys(), got, family, impl)
    return p


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (256, 384, 768), (204, 132, 200), (8, 512, 768), (1000, 2304, 768)])
def test_nt_plain(dtype, M, N, K):
    from xpretrain_amd import hip_ops as H
    torch.manual_seed(M + N + K)
    A, B = _mk((M, K), dtype), _mk((N, K), dtype)
    # ragged k-tiles (K = 200) take the register-staged loader, N % 8 == 4 the 4-column epilogue
    _plan(A, B, M, N, K, "staged" if K == 200 else "direct", "row4" if N % 8 else "fast")
    C = H.gemm(A, B, M, N, K)
    ref = A.double() @ B.double().t()
    assert report(f"gemm_nt {dtype} {M}x{N}x{K}", C, ref, TOL[dtype]) <= TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(128, 128, 128), (204, 768, 2304), (52, 192, 136)])
def test_nn_b_kstrided(dtype, M, N, K):
    """dX = dY[M,K] . W[K,N]  (B stored [k][n])"""
    from xpretrain_amd import hip_ops as H
    torch.manual_seed(1)
    A, W = _mk((M, K), dtype), _mk((K, N), dtype)
    _plan(A, W, M, N, K, "staged" if N % 128 else "direct", "fast", b_kstrided=True)      # (k-strided B: N % 128 for DIRECT)
    C = H.gemm(A, W, M, N, K, b_kstrided=True)
    ref = A.double() @ W.double()
    assert report(f"gemm_nn {dtype} {M}x{N}x{K}", C, ref, TOL[dtype]) <= TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K,split", [(128, 128, 256, 1), (768, 3072, 1000, 1), (192, 136, 204, 1), (768, 768, 4000, 8)])
def test_tn_both_kstrided(dtype, M, N, K, split):
    """dW[M,N] = dY[K,M]^T . X[K,N]  (both stored [k][row]), optionally split-K over the long contraction."""
    from xpretrain_amd import hip_ops as H
    torch.manual_seed(2)
    Y, X = _mk((K, M), dtype), _mk((K, N), dtype)
    # (768 x 768 x 4000 in 8 slabs: 72 workgroups of the 256 family, below its default threshold of 96)
    _plan(Y, X, M, N, K, "staged" if M % 128 or N % 128 else "direct", "fast", a_kstrided=True, b_kstrided=True,
          out_dtype=torch.float32, split_k=split)
    if split == 1:
        C = H.gemm(Y, X, M, N, K, a_kstrided=True, b_kstrided=True, out_dtype=torch.float32)
    else:
        slabs = H.gemm(Y, X, M, N, K, a_kstrided=True, b_kstrided=True, split_k=split)
        C = H.splitk_reduce(slabs, torch.empty(M, N, device="cuda"))
    ref = Y.double().t() @ X.double()
    tol = 2e-5 if dtype == torch.float32 else 1e-5   # fp32 output: only accumulation error
    assert report(f"gemm_tn {dtype} {M}x{N}x{K} split{split}", C, ref, tol) <= tol


@pytest.mark.parametrize("dtype", DTYPES)
def test_epilogues(dtype):
    from xpretrain_amd import hip_ops as H
    from xpretrain_amd import _lib as L
    torch.manual_seed(3)
    M, N, K = 204, 384, 192
    A, B = _mk((M, K), dtype, 0.5), _mk((N, K), dtype, 0.2)
    bias = torch.randn(N, device="cuda")
    R = _mk((M, N), dtype)
    acc = A.double() @ B.double().t()
    tol = TOL[dtype]
    impl = "fast" if dtype == torch.bfloat16 else "row8"      # (fp32 output: the fast epilogue exists for EPI_NONE only)
    for epi in (L.EPI_BIAS, L.EPI_BIAS_QSCALE, L.EPI_BIAS_GELU, L.EPI_BIAS_RESID, L.EPI_GELU_BWD):
        _plan(A, B, M, N, K, "direct", impl, epilogue=epi, bias=bias, resid=R)
    _plan(A, B, M, N, K, "direct", "row8", epilogue=L.EPI_SCALE, out_dtype=torch.float32)
    C = H.gemm(A, B, M, N, K, epilogue=L.EPI_BIAS, bias=bias)
    assert report(f"epi_bias {dtype}", C, acc + bias.double(), tol) <= tol
    C = H.gemm(A, B, M, N, K, epilogue=L.EPI_BIAS_QSCALE, bias=bias, scale=0.125, scale_cols=128)
    ref = acc + bias.double(); ref[:, :128] *= 0.125
    assert report(f"epi_qscale {dtype}", C, ref, tol) <= tol
    aux = torch.empty(M, N, dtype=dtype, device="cuda")
    C = H.gemm(A, B, M, N, K, epilogue=L.EPI_BIAS_GELU, bias=bias, aux=aux)
    pre = acc + bias.double()
    assert report(f"epi_gelu.aux {dtype}", aux, pre, tol) <= tol
    assert report(f"epi_gelu.act {dtype}", C, pre * torch.sigmoid(1.702 * pre), tol) <= tol
    C = H.gemm(A, B, M, N, K, epilogue=L.EPI_BIAS_RESID, bias=bias, resid=R)
    assert report(f"epi_resid {dtype}", C, acc + bias.double() + R.double(), tol) <= tol
    C = H.gemm(A, B, M, N, K, epilogue=L.EPI_GELU_BWD, resid=R)
    x = R.double(); s = torch.sigmoid(1.702 * x)
    assert report(f"epi_gelu_bwd {dtype}", C, acc * (s * (1 + 1.702 * x * (1 - s))), tol) <= tol
    C = H.gemm(A, B, M, N, K, epilogue=L.EPI_SCALE, scale=3.0, out_dtype=torch.float32)
    assert report(f"epi_scale {dtype}", C, acc * 3.0, 2e-5) <= 2e-5


@pytest.mark.parametrize("dtype", DTYPES)
def test_patch_epilogue_and_row_remap(dtype):
    """conv-as-GEMM epilogue: rows (b,t,l) land in token slot b*S + Mp + t*L + l with + time[t] + pos[l]."""
    from xpretrain_amd import hip_ops as H
    from xpretrain_amd import _lib as L
    torch.manual_seed(4)
    Bsz, T, Lp, Mp, D, K = 2, 3, 10, 4, 128, 192
    S = Mp + T * Lp
    A, W = _mk((Bsz * T * Lp, K), dtype, 0.3), _mk((D, K), dtype, 0.3)
    tab_t, tab_l = torch.randn(T, D, device="cuda"), torch.randn(Lp, D, device="cuda")
    x = torch.zeros(Bsz * S, D, dtype=dtype, device="cuda")
    _plan(A, W, Bsz * T * Lp, D, K, "direct", "row8", out=x, epilogue=L.EPI_PATCH, tab1=tab_t, tab2=tab_l, tab_L=Lp,
          c_remap=(T * Lp, S, Mp))
    H.gemm(A, W, Bsz * T * Lp, D, K, out=x, epilogue=L.EPI_PATCH, tab1=tab_t, tab2=tab_l, tab_L=Lp,
           c_remap=(T * Lp, S, Mp))
    ref = (A.double() @ W.double().t()).view(Bsz, T, Lp, D) + tab_t.double()[None, :, None] + tab_l.double()[None, None]
    full = torch.zeros(Bsz, S, D, dtype=torch.float64, device="cuda")
    full[:, Mp:] = ref.view(Bsz, T * Lp, D)
    assert report(f"epi_patch {dtype}", x.view(Bsz, S, D), full, TOL[dtype]) <= TOL[dtype]
    # dW with the A operand's k-rows remapped the same way (token rows -> patch rows)
    dx = _mk((Bsz * S, D), dtype)
    _plan(dx, A, D, K, Bsz * T * Lp, "staged", "fast", a_kstrided=True, b_kstrided=True, lda=D, ldb=K, out_dtype=torch.float32,
          a_remap=(T * Lp, S, Mp))
    dW = H.gemm(dx, A, D, K, Bsz * T * Lp, a_kstrided=True, b_kstrided=True, lda=D, ldb=K, out_dtype=torch.float32,
                a_remap=(T * Lp, S, Mp))
    ref = dx.double().view(Bsz, S, D)[:, Mp:].reshape(-1, D).t() @ A.double()
    assert report(f"dW_patch_remap {dtype}", dW, ref, 2e-5) <= 2e-5


@pytest.mark.parametrize("dtype", DTYPES)
def test_colsum(dtype):
    from xpretrain_amd import hip_ops as H
    X = _mk((1000, 768), dtype)
    out = H.colsum(X, 1000, 768)
    assert report(f"colsum {dtype}", out, X.double().sum(0), 1e-5) <= 1e-5


def test_bad_arguments_raise():
    from xpretrain_amd import hip_ops as H
    A = torch.zeros(8, 12, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="multiples of"):
        H.gemm(A, A, 8, 8, 12)


# ---------------------------------------------------------------------------------------------- 256x256 family
@pytest.fixture
def force_gemm256(monkeypatch):
    monkeypatch.setenv("XPRETRAIN_GEMM256", "2")     # use the 256x256 family whenever its preconditions hold


def _params(shapes, bf16_fallback=()):
    """(M, N, K, dtype) with the ids of a stacked (M,N,K) x dtype parametrisation; the bf16 cases of `bf16_fallback` left out (they
    are test_gemm256_falls_back_to_128's)"""
    return [pytest.param(*s, dt, id="-".join(map(str, s)) + f"-dtype{i}") for s in shapes for i, dt in enumerate(DTYPES)
            if not (dt == torch.bfloat16 and s in bf16_fallback)]


def _family256(dtype):
    """the family a forced-256 test runs: the 256 family is bf16 only, fp32 parametrisations run the 128x128 family"""
    return "g256" if dtype == torch.bfloat16 else "direct"


@pytest.mark.parametrize("M,N,K,dtype", _params([(256, 256, 128), (1280, 512, 768), (1100, 768, 256), (304, 264, 128),
                                                  (2356, 768, 3072), (256, 256, 64), (300, 260, 96)],
                                                 bf16_fallback=[(256, 256, 64), (300, 260, 96)]))
def test_gemm256_nt(force_gemm256, dtype, M, N, K):
    from xpretrain_amd import hip_ops as H
    torch.manual_seed(M + N + K)
    A, B = _mk((M, K), dtype), _mk((N, K), dtype)
    _plan(A, B, M, N, K, _family256(dtype), "row4" if N % 8 else "fast")
    C = H.gemm(A, B, M, N, K)
    ref = A.double() @ B.double().t()
    assert report(f"gemm256_nt {dtype} {M}x{N}x{K}", C, ref, TOL[dtype]) <= TOL[dtype]


@pytest.mark.parametrize("M,N,K,dtype", _params([(1280, 768, 2304), (512, 256, 128), (2356, 3072, 768), (520, 256, 72)],
                                                 bf16_fallback=[(520, 256, 72)]))
def test_gemm256_nn(force_gemm256, dtype, M, N, K):
    from xpretrain_amd import hip_ops as H
    torch.manual_seed(1)
    A, W = _mk((M, K), dtype), _mk((K, N), dtype)
    _plan(A, W, M, N, K, "staged" if K % 32 else _family256(dtype), "fast", b_kstrided=True)
    C = H.gemm(A, W, M, N, K, b_kstrided=True)
    ref = A.double() @ W.double()
    assert report(f"gemm256_nn {dtype} {M}x{N}x{K}", C, ref, TOL[dtype]) <= TOL[dtype]


@pytest.mark.parametrize("layout,M,N,K,family,impl", [
    # one k-tile: the 256 family's pipeline needs >= 2 k-tiles in the last slab
    pytest.param("nt", 256, 256, 64, "direct", "fast", id="nt-256-256-64"),
    # N % 8 == 4: no 8-column epilogue, and the 256 family has only the fast one; K % 64 != 0 as well (ragged k-tile: staged)
    pytest.param("nt", 300, 260, 96, "staged", "row4", id="nt-300-260-96"),
    # K % 64 != 0 with a k-contiguous A (xp_gemm256_legal)
    pytest.param("nn", 520, 256, 72, "staged", "fast", id="nn-520-256-72"),
])
def test_gemm256_falls_back_to_128(force_gemm256, layout, M, N, K, family, impl):
    """bf16 problems the 256 family does not admit even when forced (XPRETRAIN_GEMM256=2): the planner runs them on the 128x128
    family.  (These were test_gemm256_nt / _nn cases; those now hold 256-admissible neighbours.)"""
    from xpretrain_amd import hip_ops as H
    bf = torch.bfloat16
    torch.manual_seed(M + N + K if layout == "nt" else 1)
    bks = layout == "nn"
    A, B = _mk((M, K), bf), _mk((K, N) if bks else (N, K), bf)
    _plan(A, B, M, N, K, family, impl, b_kstrided=bks)
    C = H.gemm(A, B, M, N, K, b_kstrided=bks)
    ref = A.double() @ (B.double() if bks else B.double().t())
    assert report(f"gemm256 fallback {layout} {M}x{N}x{K}", C, ref, TOL[bf]) <= TOL[bf]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K,split", [(768, 1024, 1000, 1), (256, 512, 77, 1), (768, 768, 4000, 8)])
def test_gemm256_tn(force_gemm256, dtype, M, N, K, split):
    from xpretrain_amd import hip_ops as H
    torch.manual_seed(2)
    Y, X = _mk((K, M), dtype), _mk((K, N), dtype)
    _plan(Y, X, M, N, K, _family256(dtype), "fast", a_kstrided=True, b_kstrided=True, out_dtype=torch.float32, split_k=split)
    if split == 1:
        C = H.gemm(Y, X, M, N, K, a_kstrided=True, b_kstrided=True, out_dtype=torch.float32)
    else:
        C = H.splitk_reduce(H.gemm(Y, X, M, N, K, a_kstrided=True, b_kstrided=True, split_k=split),
                            torch.empty(M, N, device="cuda"))
    ref = Y.double().t() @ X.double()
    assert report(f"gemm256_tn {dtype} {M}x{N}x{K} split{split}", C, ref, 2e-5) <= 2e-5


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm256_epilogues(force_gemm256, dtype):
    from xpretrain_amd import hip_ops as H
    from xpretrain_amd import _lib as L
    torch.manual_seed(3)
    M, N, K = 1100, 512, 192
    A, B = _mk((M, K), dtype, 0.5), _mk((N, K), dtype, 0.2)
    bias = torch.randn(N, device="cuda")
    R = _mk((M, N), dtype)
    acc = A.double() @ B.double().t()
    tol = TOL[dtype]
    for epi in (L.EPI_BIAS_QSCALE, L.EPI_BIAS_GELU, L.EPI_BIAS_RESID, L.EPI_GELU_BWD):
        _plan(A, B, M, N, K, _family256(dtype), "fast" if dtype == torch.bfloat16 else "row8", epilogue=epi, bias=bias, resid=R)
    C = H.gemm(A, B, M, N, K, epilogue=L.EPI_BIAS_QSCALE, bias=bias, scale=0.125, scale_cols=128)
    ref = acc + bias.double(); ref[:, :128] *= 0.125
    assert report(f"g256 epi_qscale {dtype}", C, ref, tol) <= tol
    aux = torch.empty(M, N, dtype=dtype, device="cuda")
    C = H.gemm(A, B, M, N, K, epilogue=L.EPI_BIAS_GELU, bias=bias, aux=aux)
    pre = acc + bias.double()
    assert report(f"g256 epi_gelu.aux {dtype}", aux, pre, tol) <= tol
    assert report(f"g256 epi_gelu.act {dtype}", C, pre * torch.sigmoid(1.702 * pre), tol) <= tol
    C = H.gemm(A, B, M, N, K, epilogue=L.EPI_BIAS_RESID, bias=bias, resid=R)
    assert report(f"g256 epi_resid {dtype}", C, acc + bias.double() + R.double(), tol) <= tol
    C = H.gemm(A, B, M, N, K, epilogue=L.EPI_GELU_BWD, resid=R)
    x = R.double(); s = torch.sigmoid(1.702 * x)
    assert report(f"g256 epi_gelu_bwd {dtype}", C, acc * (s * (1 + 1.702 * x * (1 - s))), tol) <= tol


@pytest.mark.parametrize("epi", ["none", "gelu_bwd"])
def test_gemm_fused_colsum(epi):
    """Column sums of the finished outputs from the GEMM epilogue (the bias gradient of the producing Linear), M not a
    multiple of the tile (rows >= M must not contribute), vs fp64."""
    from xpretrain_amd import hip_ops as H
    from xpretrain_amd import _lib as L
    torch.manual_seed(12)
    M, N, K = 8 * 2356 + 40, 768, 512
    bf = torch.bfloat16
    dY = (torch.randn(M, K, device="cuda") * 0.5).to(bf)
    W = (torch.randn(K, N, device="cuda") * 0.05).to(bf)          # [K, N]: read k-strided (the dX orientation)
    pre = torch.randn(M, N, device="cuda").to(bf)
    defer = H.DeferredReduce(dY.device)
    kw = dict(epilogue=L.EPI_GELU_BWD, resid=pre) if epi == "gelu_bwd" else {}
    assert _plan(dY, W, M, N, K, "g256", "fast", b_kstrided=True, colsum_defer=defer, **kw)["colsum_rows"] == 2 * ((M + 255) // 256)
    out, cs = H.gemm(dY, W, M, N, K, b_kstrided=True, colsum_defer=defer, **kw)
    assert len(defer.segs) == 1 and defer.segs[0].nrows == 2 * ((M + 255) // 256)      # the fused path was taken (256-row tiles)
    defer.flush()
    ref = dY.double() @ W.double()
    if epi == "gelu_bwd":
        s = torch.sigmoid(1.702 * pre.double())
        ref = ref * (s * (1 + 1.702 * pre.double() * (1 - s)))
    assert report(f"fused colsum {epi} out", out, ref, 6e-3) <= 6e-3
    assert report(f"fused colsum {epi}", cs, ref.sum(0), 2e-3) <= 2e-3
    # small problem: the library declines the fusion, the wrapper falls back to a separate pass with the same result
    out2, cs2 = H.gemm(dY[:300].contiguous(), W, 300, N, K, b_kstrided=True, colsum_defer=defer,
                       **({} if epi == "none" else dict(epilogue=L.EPI_GELU_BWD, resid=pre[:300].contiguous())))
    defer.flush()
    assert report(f"fallback colsum {epi}", cs2, out2.double().sum(0), 1e-5) <= 1e-5


# ---------------------------------------------------------------------------------------------- the real token count
@pytest.mark.parametrize("M", [18848, 18848 + 40, 18848 - 200])
def test_gemm256_token_count_all_epilogues(M):
    """The training step's row count (74 tiles of 256 rows, ragged last tile) through every fused epilogue of the family; rows past
    M are never written."""
    from xpretrain_amd import hip_ops as H
    from xpretrain_amd import _lib as L
    torch.manual_seed(M)
    bf = torch.bfloat16
    N, K = 768, 192
    assert _tile_rows(M, N, K) == 256
    A, B = _mk((M, K), bf, 0.5), _mk((N, K), bf, 0.2)
    bias = torch.randn(N, device="cuda")
    R = _mk((M, N), bf)
    for epi in range(L.EPI_GELU_BWD + 1):
        _plan(A, B, M, N, K, "g256", "fast", epilogue=epi, bias=bias, resid=R)
    acc = A.double() @ B.double().t()
    tol = TOL[bf]
    C = H.gemm(A, B, M, N, K)
    assert report("g256 none", C, acc, tol) <= tol
    C = H.gemm(A, B, M, N, K, epilogue=L.EPI_BIAS, bias=bias)
    assert report("g256 bias", C, acc + bias.double(), tol) <= tol
    C = H.gemm(A, B, M, N, K, epilogue=L.EPI_BIAS_QSCALE, bias=bias, scale=0.125, scale_cols=256)
    ref = acc + bias.double(); ref[:, :256] *= 0.125
    assert report("g256 qscale", C, ref, tol) <= tol
    aux = torch.full((M, N), float("nan"), dtype=bf, device="cuda")
    C = H.gemm(A, B, M, N, K, epilogue=L.EPI_BIAS_GELU, bias=bias, aux=aux)
    pre = acc + bias.double()
    assert report("g256 gelu.aux", aux, pre, tol) <= tol
    assert report("g256 gelu.act", C, pre * torch.sigmoid(1.702 * pre), tol) <= tol
    C2 = H.gemm(A, B, M, N, K, epilogue=L.EPI_BIAS_GELU, bias=bias)                 # forward-only: no pre-activation
    assert torch.equal(C2, C)
    C = H.gemm(A, B, M, N, K, epilogue=L.EPI_BIAS_RESID, bias=bias, resid=R)
    assert report("g256 resid", C, acc + bias.double() + R.double(), tol) <= tol
    C = H.gemm(A, B, M, N, K, epilogue=L.EPI_GELU_BWD, resid=R)
    x = R.double(); s = torch.sigmoid(1.702 * x)
    assert report("g256 gelu_bwd", C, acc * (s * (1 + 1.702 * x * (1 - s))), tol) <= tol
    big = torch.full((M + 300, N), 7.0, dtype=bf, device="cuda")
    H.gemm(A, B, M, N, K, out=big)
    assert bool((big[M:] == 7.0).all())


def test_gemm256_token_count_nn_and_f32():
    """the dX orientation (N side k-strided) and fp32 output at the training step's row count"""
    from xpretrain_amd import hip_ops as H
    torch.manual_seed(5)
    bf = torch.bfloat16
    M, N, K = 18848, 768, 256
    assert _tile_rows(M, N, K, b_kstrided=True) == 256
    A, W = _mk((M, K), bf, 0.5), _mk((K, N), bf, 0.2)
    _plan(A, W, M, N, K, "g256", "fast", b_kstrided=True, out_dtype=torch.float32)
    C = H.gemm(A, W, M, N, K, b_kstrided=True)
    ref = A.double() @ W.double()
    assert report("g256 nn", C, ref, TOL[bf]) <= TOL[bf]
    Cf = H.gemm(A, W, M, N, K, b_kstrided=True, out_dtype=torch.float32)
    assert report("g256 nn f32", Cf, ref, 2e-5) <= 2e-5
    B = _mk((N, K), bf, 0.2)
    Cf = H.gemm(A, B, M, N, K, out_dtype=torch.float32)
    assert report("g256 nt f32", Cf, A.double() @ B.double().t(), 2e-5) <= 2e-5


@pytest.mark.parametrize("M,N,K,split", [(3072, 768, 18848, 7), (768, 768, 18848, 27), (2304, 768, 9424, 9)])
# (the splits of earlier rounds; the planner's own splits of the step, and the grid identity at them: test_gemm_plans_gpu.py)
def test_dw_split_k_chunk_major_grid(M, N, K, split, tmp_path):
    """Weight-gradient shapes of the step (dW1, dWo, dWqkv): the split-K launch walks a 1-D grid over (k-chunk, tile) pairs,
    chunk-major per XCD (csrc/gemm256.hip).  Against fp64, and bit-identical to the (tile, z) grid (XPRETRAIN_DEBUG=dw_tile_major
    in a fresh process: it computes the same slabs) -- the mapping changes which CU computes a slab, never the slab."""
    import os
    import subprocess
    import sys
    from xpretrain_amd import hip_ops as H
    torch.manual_seed(M + split)
    bf = torch.bfloat16
    Y, X = _mk((K, M), bf, 0.3), _mk((K, N), bf, 0.3)
    assert _plan(Y, X, M, N, K, "g256", "fast", a_kstrided=True, b_kstrided=True, split_k=split)["flat_split"] == split
    slabs = H.gemm(Y, X, M, N, K, a_kstrided=True, b_kstrided=True, split_k=split)
    dw = H.splitk_reduce(slabs, torch.empty(M, N, device="cuda"))
    ref = Y.double().t() @ X.double()
    assert report(f"dW {M}x{N}x{K} split {split}", dw, ref, 2e-5) <= 2e-5
    case = str(tmp_path / "xp_chunk_major_case.pt")
    torch.save({"Y": Y.cpu(), "X": X.cpu(), "slabs": slabs.cpu()}, case)
    code = ("import torch, sys; sys.path.insert(0, '.');\n"
            "from xpretrain_amd import hip_ops as H\n"
            f"d = torch.load({case!r}); Y, X = d['Y'].cuda(), d['X'].cuda()\n"
            f"s = H.gemm(Y, X, {M}, {N}, {K}, a_kstrided=True, b_kstrided=True, split_k={split})\n"
            "assert torch.equal(s.cpu(), d['slabs'])\nprint('same')\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, XPRETRAIN_DEBUG="dw_tile_major"),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "same" in out.stdout, out.stderr[-1500:]


@pytest.mark.parametrize("M,N,K,S,Ms", [(18848, 768, 192, 2356, 4), (4712, 768, 3072, 2356, 4), (200, 256, 128, 50, 3), (40, 64, 64, 10, 4)])
def test_resid_epilogue_with_fp32_side_rows(M, N, K, S, Ms):
    """EPI_BIAS_RESID with the fp32 side rows of the residual stream (XpGemmDesc::resid_side / out_side): rows m with m % S < Ms take
    their residual operand from the fp32 side buffer and leave their fp32 result there as well as the rounded C row; all other rows
    are untouched by the feature.  256-wide family (the step's row count) and the 128x128 family (the smaller row counts)."""
    from xpretrain_amd import hip_ops as H
    from xpretrain_amd import _lib as L
    torch.manual_seed(M + N)
    bf = torch.bfloat16
    A, B = _mk((M, K), bf, 0.5), _mk((N, K), bf, 0.2)
    bias = torch.randn(N, device="cuda")
    R = _mk((M, N), bf)
    nb = (M + S - 1) // S
    rs = torch.randn(nb * Ms, N, device="cuda")
    os_ = torch.full((nb * Ms, N), float("nan"), device="cuda")
    _plan(A, B, M, N, K, "g256" if -(-M // 256) * -(-N // 256) >= 96 else "direct", "fast", epilogue=L.EPI_BIAS_RESID, bias=bias,
          resid=R)      # (the 256 family from 96 workgroups by default)
    C = H.gemm(A, B, M, N, K, epilogue=L.EPI_BIAS_RESID, bias=bias, resid=R, resid_side=rs, out_side=os_, side=(S, Ms))
    plain = H.gemm(A, B, M, N, K, epilogue=L.EPI_BIAS_RESID, bias=bias, resid=R)
    acc = A.double() @ B.double().t() + bias.double()
    rows = torch.arange(M, device="cuda")
    is_side = (rows % S) < Ms
    sidx = (rows // S) * Ms + rows % S
    # side rows: fp32 result = acc + bias + fp32 residual; C = that, rounded
    want = acc[is_side] + rs[sidx[is_side]].double()
    assert report("side rows fp32", os_[sidx[is_side]], want, 2e-5) <= 2e-5
    assert torch.equal(C[is_side], os_[sidx[is_side]].to(bf))
    assert torch.equal(C[~is_side], plain[~is_side])
    # side slots of rows >= M (a partial last sample) stay untouched
    touched = torch.zeros(nb * Ms, dtype=torch.bool, device="cuda"); touched[sidx[is_side]] = True
    assert bool(torch.isnan(os_[~touched]).all())
