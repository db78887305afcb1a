"""Inference kernels vs fp64 references at edge shapes, with derived
per-element bounds (tests/nn_ref.py; tests/test_nn_tolerances.py proves on the
CPU that a correct implementation meets each bound on these same inputs).

Covers every GEMM variant and every branch of the gemm_bf16 dispatcher, all
LayerNorm / softmax code paths and grid wraps, bias_act, gemv, featpack, the
flash attention kernel with partial Q blocks and a moving running max, the
LDS-pad variants, and the bindings' argument checks.
"""
import pytest
import torch

from tests import nn_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def nat():
    from arkflow_amd import ops
    return ops.require_native()  # GPU present ⇒ extension must load


def _poison(shape, dtype, dev):
    """Outputs are torch::empty and the caching allocator hands the block just
    freed to the next allocation of that size: fill it with NaN so a tile the
    kernel fails to write cannot inherit a plausible value."""
    t = torch.full(shape, float("nan"), dtype=dtype, device=dev)
    del t


def _to(dev, *ts):
    return tuple(None if t is None else t.to(dev) for t in ts)


# ----------------------------------------------------------------- GEMM family
@pytest.mark.parametrize("case", R.gemm_variant_cases(), ids=lambda c: c.id)
def test_gemm_variant(nat, dev, case):
    """Each gemm_bf16_variant id at (a) a ragged single tile, (b) a ragged
    20-tile grid (XCD remap with a remainder), (c) a single row (every staged
    row is the clamped row); shape 'x' is (b) under every epilogue, where the
    variants must also agree bitwise with variant 0 (same 16x16x32 MFMA in
    ascending-k order)."""
    A, Bt, bias = _to(dev, *R.gemm_inputs(case))
    bm, bn, _ = R.GEMM_VARIANTS[case.variant]
    _poison((case.M, case.N), torch.bfloat16, dev)
    C = nat.gemm_bf16_variant(A, Bt, bias, case.act, case.variant)
    ref, tol = R.gemm_ref(A, Bt, bias, case.act)
    R.assert_within(C, ref, tol, case.id, tile=(bm, bn))
    if case.shape == "x" and case.variant != 0:
        C0 = nat.gemm_bf16_variant(A, Bt, bias, case.act, 0)
        assert torch.equal(C, C0), \
            f"{case.id}: differs bitwise from variant 0 at " \
            f"{torch.nonzero(C != C0)[0].tolist()}"


@pytest.mark.parametrize("case", R.GEMM_DISPATCH_CASES, ids=lambda c: c.id)
def test_gemm_dispatch_branch(nat, dev, case):
    """One shape per branch of gemm_bf16: 8-phase BM=256+swizzle, the 128^2
    BK=32 fall-through, k64s and skinny; gelu + bias."""
    A, Bt, bias = _to(dev, *R.gemm_inputs(case))
    _poison((case.M, case.N), torch.bfloat16, dev)
    C = nat.gemm_bf16(A, Bt, bias, case.act)
    ref, tol = R.gemm_ref(A, Bt, bias, case.act)
    R.assert_within(C, ref, tol, case.id, tile=(128, 128))


@pytest.mark.parametrize("case,variant",
                         zip(R.GEMM_DISPATCH_CASES, R.GEMM_DISPATCH_VARIANTS),
                         ids=lambda p: getattr(p, "id", str(p)))
def test_gemm_dispatch_takes_documented_variant(nat, dev, case, variant):
    """gemm_bf16 runs the kernel its branch names: bitwise equal to
    gemm_bf16_variant with that id (pins the dispatcher-to-enum wiring)."""
    A, Bt, bias = _to(dev, *R.gemm_inputs(case))
    C = nat.gemm_bf16(A, Bt, bias, case.act)
    Cv = nat.gemm_bf16_variant(A, Bt, bias, case.act, variant)
    assert torch.equal(C, Cv), \
        f"{case.id}: gemm_bf16 differs bitwise from variant {variant}"


# ------------------------------------------------------------------- LayerNorm
def _check_ln(nat, dev, x, res, gamma, beta, what):
    x, res, gamma, beta = _to(dev, x, res, gamma, beta)
    _poison(tuple(x.shape), torch.bfloat16, dev)
    got = nat.layernorm_bf16(x, gamma, beta, R.LN_EPS, res)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    ref, tol = R.layernorm_ref(x, res, gamma, beta)
    R.assert_within(got, ref, tol, what)


@pytest.mark.parametrize("n", R.LN_WIDTHS)
def test_layernorm_widths(nat, dev, n):
    """Register-cached wave path (n <= 1024), streamed wave path (<= 2048) and
    block-per-row path (> 2048), at and around each threshold, with and
    without the fused residual; gamma and beta take both signs."""
    for rows in R.LN_ROWS:
        x, res, gamma, beta = R.ln_inputs(rows, n)
        _check_ln(nat, dev, x, None, gamma, beta, f"ln {rows}x{n}")
        _check_ln(nat, dev, x, res, gamma, beta, f"ln+res {rows}x{n}")


@pytest.mark.parametrize("rows,n", R.LN_WRAP)
def test_layernorm_grid_wrap(nat, dev, rows, n):
    """More rows than the capped grid covers in one sweep (wave path: 4096
    blocks x 4 rows; block path: 2048 blocks)."""
    x, res, gamma, beta = R.ln_inputs(rows, n)
    _check_ln(nat, dev, x, None, gamma, beta, f"ln {rows}x{n}")
    _check_ln(nat, dev, x, res, gamma, beta, f"ln+res {rows}x{n}")


@pytest.mark.parametrize("c,sigma", R.LN_ILL)
@pytest.mark.parametrize("n", R.LN_ILL_WIDTHS)
def test_layernorm_ill_conditioned_residual(nat, dev, n, c, sigma):
    """x = c, residual = sigma randn with |c| >> sigma: finite and within the
    bound on all three code paths. The one-pass E[f^2] - mean^2 variance these
    kernels used gave NaN (negative variance) or errors of tens here."""
    x, res, gamma, beta = R.ln_ill_inputs(n, c, sigma)
    _check_ln(nat, dev, x, res, gamma, beta, f"ln ill n={n} c={c} s={sigma}")


# --------------------------------------------------------------------- softmax
def _check_softmax(nat, dev, rows, n, scale):
    x, masked = R.softmax_inputs(rows, n, scale)
    xd = x.to(dev)
    _poison((rows, n), torch.bfloat16, dev)
    got = nat.softmax_bf16(xd, scale)
    ref, tol = R.softmax_ref(xd, scale)
    what = f"softmax {rows}x{n} scale={scale}"
    R.assert_within(got, ref, tol, what)
    rowsum = got.double().sum(-1)
    worst = float((rowsum - 1.0).abs().max())
    assert worst <= R.SM_ROWSUM_TOL, f"{what}: |row sum - 1| = {worst}"
    if masked is not None:
        assert bool((got[masked.to(dev)] == 0).all()), \
            f"{what}: masked position not exactly 0"


@pytest.mark.parametrize("scale", R.SM_SCALES)
@pytest.mark.parametrize("n", R.SM_WIDTHS)
def test_softmax_widths(nat, dev, n, scale):
    """Widths where 1 of 256 threads holds data up to two loop trips per
    thread, with a dominant logit, an all-equal row, masked (-inf) entries
    and +-3e4 logits."""
    for rows in R.SM_ROWS:
        _check_softmax(nat, dev, rows, n, scale)


def test_softmax_grid_wrap(nat, dev):
    rows, n = R.SM_WRAP
    _check_softmax(nat, dev, rows, n, 0.125)


# -------------------------------------------------------------------- bias_act
@pytest.mark.parametrize("act", (0, 1, 2, 3))
def test_bias_act(nat, dev, act):
    shapes = [(R.BA_ROWS, n) for n in R.BA_WIDTHS] + [R.BA_WRAP]
    for rows, n in shapes:
        x, bias = _to(dev, *R.bias_act_inputs(rows, n))
        for b in (None, bias):
            _poison((rows, n), torch.bfloat16, dev)
            got = nat.bias_act_bf16(x, b, act)
            ref, tol = R.bias_act_ref(x, b, act)
            R.assert_within(
                got, ref, tol,
                f"bias_act {rows}x{n} act={act} bias={b is not None}")


# ------------------------------------------------------------------------ gemv
@pytest.mark.parametrize("M", R.GEMV_M)
def test_gemv(nat, dev, M):
    for K in R.GEMV_K:
        x, w = _to(dev, *R.gemv_inputs(M, K))
        _poison((M,), torch.float32, dev)
        got = nat.gemv_bf16_f32(x, w, R.GEMV_BIAS)
        assert got.dtype == torch.float32 and got.shape == (M,)
        ref, tol = R.gemv_ref(x, w, R.GEMV_BIAS)
        R.assert_within(got, ref, tol, f"gemv {M}x{K}")


# -------------------------------------------------------------------- featpack
def _check_featpack(nat, dev, nf, kpad, n, dtype):
    cols = R.featpack_sources(nf, n, dtype)
    out = torch.full((n, kpad), float("nan"), dtype=torch.bfloat16,
                     device=dev)
    nat.featpack([c.to(dev) for c in cols], out)
    what = f"featpack nf={nf} kpad={kpad} n={n} {dtype}"
    if nf < kpad:
        pad = out[:, nf:]
        assert bool((pad == 0).all()), f"{what}: pad column not exactly 0"
    R.assert_bf16_identical(out, R.featpack_ref(cols, kpad), what)


@pytest.mark.parametrize("dtype", (torch.float32, torch.float64),
                         ids=("f32", "f64"))
@pytest.mark.parametrize("nf,kpad", R.FP_SHAPES)
def test_featpack(nat, dev, nf, kpad, dtype):
    """Exact bf16 rounding (ties to even, signed zero, denormal, overflow,
    inf, NaN) and zeroed pad columns, into a NaN-prefilled output."""
    for n in R.FP_ROWS:
        _check_featpack(nat, dev, nf, kpad, n, dtype)


@pytest.mark.parametrize("dtype", (torch.float32, torch.float64),
                         ids=("f32", "f64"))
def test_featpack_grid_wrap(nat, dev, dtype):
    n, nf, kpad = R.FP_WRAP
    _check_featpack(nat, dev, nf, kpad, n, dtype)


# ------------------------------------------------------------------- attention
@pytest.mark.parametrize("family", R.ATTN_FAMILIES)
@pytest.mark.parametrize("shape", R.ATTN_SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_attention_flash(nat, dev, shape, family):
    """Flash kernel through both entry points at S=192 and S=320 (a partial
    last 128-row Q block after full ones), including inputs whose running max
    grows with every KV tile, sits in the first tile, or reaches tens."""
    qkv, scale = R.attention_inputs(shape, family)
    qkv = qkv.to(dev)
    q, k, v = R.split_qkv(qkv)
    ref, tol = R.attention_ref(q, k, v, scale)
    B, H, S, D = shape
    what = f"attn {shape} {family}"
    _poison((B, H, S, D), torch.bfloat16, dev)
    got = nat.attention_bf16(q, k, v, scale)
    R.assert_within(got, ref, tol, what + " [B,H,S,D]", tile=(128, D))
    _poison((B, S, H * D), torch.bfloat16, dev)
    got2 = nat.attention_qkv_bf16(qkv, scale)
    R.assert_within(got2, R.heads_to_rows(ref), R.heads_to_rows(tol),
                    what + " qkv", tile=(128, D))


def test_attention_pad_variants_identical(nat, dev):
    """pad only changes the LDS layout of the S=128 kernel: 4, 16 and 20 must
    reproduce the default 8 bit for bit (and 8 must meet the bound)."""
    shape = (2, 3, 128, 64)
    qkv, scale = R.attention_inputs(shape, "randn")
    qkv = qkv.to(dev)
    base = nat.attention_qkv_bf16(qkv, scale, 8)
    q, k, v = R.split_qkv(qkv)
    ref, tol = R.attention_ref(q, k, v, scale)
    R.assert_within(base, R.heads_to_rows(ref), R.heads_to_rows(tol),
                    "attn S=128 pad=8", tile=(32, 64))
    for pad in (4, 16, 20):
        _poison(tuple(base.shape), torch.bfloat16, dev)
        got = nat.attention_qkv_bf16(qkv, scale, pad)
        assert torch.equal(got, base), f"pad={pad} differs from pad=8"


# ------------------------------------------------------------- binding hygiene
def _still_clean(dev):
    torch.cuda.synchronize()
    assert int((torch.arange(8, device=dev) * 2).sum()) == 56


def test_bad_arguments_raise_before_launch(nat, dev):
    bf = torch.bfloat16
    A = torch.randn(4, 64, device=dev).to(bf)
    Bt = torch.randn(8, 64, device=dev).to(bf)
    bias = torch.randn(8, device=dev)
    for variant in (None, 0, 2, 8):
        def call(a, b, bi):
            if variant is None:
                return nat.gemm_bf16(a, b, bi, 0)
            return nat.gemm_bf16_variant(a, b, bi, 0, variant)
        with pytest.raises(RuntimeError):  # K = 48
            call(A[:, :48].contiguous(), Bt[:, :48].contiguous(), None)
        with pytest.raises(RuntimeError):  # fp16 inputs
            call(A.half(), Bt.half(), None)
        with pytest.raises(RuntimeError):  # bias of the wrong length
            call(A, Bt, torch.randn(9, device=dev))
        with pytest.raises(RuntimeError):  # K mismatch
            call(A, Bt[:, :32].contiguous(), None)
        with pytest.raises(RuntimeError):  # rank
            call(A.reshape(2, 2, 64), Bt, None)
        with pytest.raises(RuntimeError):  # host bias
            call(A, Bt, bias.cpu())
    for variant in (99, -1):
        with pytest.raises(RuntimeError):  # not a variant id
            nat.gemm_bf16_variant(A, Bt, bias, 0, variant)
    x = torch.randn(3, 64, device=dev).to(bf)
    g = torch.randn(64, device=dev)
    b = torch.randn(64, device=dev)
    with pytest.raises(RuntimeError):  # host gamma
        nat.layernorm_bf16(x, g.cpu(), b, 1e-5, None)
    with pytest.raises(RuntimeError):  # host beta
        nat.layernorm_bf16(x, g, b.cpu(), 1e-5, None)
    with pytest.raises(RuntimeError):  # gamma of the wrong length
        nat.layernorm_bf16(x, g[:56].contiguous(), b, 1e-5, None)
    with pytest.raises(RuntimeError):  # host residual
        nat.layernorm_bf16(x, g, b, 1e-5, x.cpu())
    with pytest.raises(RuntimeError):  # residual of another shape
        nat.layernorm_bf16(x, g, b, 1e-5, x[:2].contiguous())
    q = torch.randn(1, 1, 128, 64, device=dev).to(bf)
    with pytest.raises(RuntimeError):  # k shorter than q
        nat.attention_bf16(q, q[:, :, :64].contiguous(), q, 0.125)
    with pytest.raises(RuntimeError):  # v of another dtype
        nat.attention_bf16(q, q, q.half(), 0.125)
    with pytest.raises(RuntimeError):  # bias_act bias of the wrong length
        nat.bias_act_bf16(x, torch.randn(63, device=dev), 0)
    with pytest.raises(RuntimeError):  # more sources than output columns
        nat.featpack([torch.zeros(4, device=dev)] * 3,
                     torch.empty(4, 2, dtype=bf, device=dev))
    _still_clean(dev)


def test_empty_inputs_return_without_launch(nat, dev):
    bf = torch.bfloat16
    A = torch.empty(0, 64, dtype=bf, device=dev)
    Bt = torch.randn(8, 64, device=dev).to(bf)
    bias = torch.randn(8, device=dev)
    assert nat.gemm_bf16(A, Bt, bias, 2).shape == (0, 8)
    for variant in (0, 1, 3, 6, 8, 11):
        assert nat.gemm_bf16_variant(A, Bt, bias, 2, variant).shape == (0, 8)
    w = torch.randn(64, device=dev).to(bf)
    out = nat.gemv_bf16_f32(A, w, 0.5)
    assert out.shape == (0,) and out.dtype == torch.float32
    assert nat.bias_act_bf16(A, torch.randn(64, device=dev), 1).shape == \
        (0, 64)
    nat.featpack([torch.empty(0, device=dev)],
                 torch.empty(0, 32, dtype=bf, device=dev))
    nat.featpack([torch.empty(0, dtype=torch.float64, device=dev)],
                 torch.empty(0, 32, dtype=bf, device=dev))
    g = torch.randn(64, device=dev)
    assert nat.layernorm_bf16(A, g, g, 1e-5, None).shape == (0, 64)
    _still_clean(dev)
