"""The bounds in tests/nn_ref.py are conditions on the kernels, so prove on
the CPU that a correct implementation meets them on the very inputs the GPU
tests in tests/test_nn_kernels.py use, and that they reject the defects they
were written to catch."""
import numpy as np
import pytest
import torch

from tests import nn_ref as R


def test_act_eps_constant_matches_measurement():
    worst = max(R.measure_act_eps().values())
    assert 2.0 * worst <= R.ACT_EPS <= 2.0 * worst * 1.01, (worst, R.ACT_EPS)


# ------------------------------------------------------------------------ GEMM
_BY_VARIANT = {}
for _c in R.gemm_variant_cases():
    _BY_VARIANT.setdefault(_c.variant, []).append(_c)


def test_gemm_cases_cover_every_epilogue_and_shape():
    for v, cases in _BY_VARIANT.items():
        bm, bn, ks = R.GEMM_VARIANTS[v]
        assert {(c.act, c.has_bias) for c in cases if c.shape == "x"} == \
            set(R.EPILOGUES)
        for K in ks:
            shapes = {c.shape for c in cases if c.K == K}
            assert {"a", "c"} <= shapes and shapes & {"b", "x"}, (v, K)
        m, n = 5 * bm - 7, 4 * bn - 1
        assert -(-m // bm) * -(-n // bn) == 20
    assert len({c.seed for cs in _BY_VARIANT.values() for c in cs}) == \
        sum(map(len, _BY_VARIANT.values()))


@pytest.mark.parametrize("variant", sorted(_BY_VARIANT))
def test_gemm_bound_holds_for_fp32_reference(variant):
    for case in _BY_VARIANT[variant]:
        A, Bt, bias = R.gemm_inputs(case)
        ref, tol = R.gemm_ref(A, Bt, bias, case.act)
        R.assert_within(R.gemm_emulate(A, Bt, bias, case.act), ref, tol,
                        case.id, tile=R.GEMM_VARIANTS[variant][:2])


@pytest.mark.parametrize("case", R.GEMM_DISPATCH_CASES, ids=lambda c: c.id)
def test_gemm_dispatch_bound_holds_for_fp32_reference(case):
    A, Bt, bias = R.gemm_inputs(case)
    ref, tol = R.gemm_ref(A, Bt, bias, case.act)
    R.assert_within(R.gemm_emulate(A, Bt, bias, case.act), ref, tol, case.id,
                    tile=(128, 128))


def test_gemm_bound_rejects_one_dropped_term_at_k32():
    """The old max(3e-2 mean|ref| + 0.2, 0.5) absolute bound passed results
    with one of 32 terms missing; this one must not."""
    case = next(c for c in _BY_VARIANT[0] if c.K == 32 and c.shape == "a")
    A, Bt, bias = R.gemm_inputs(case)
    ref, tol = R.gemm_ref(A, Bt, bias, R.ACT_NONE)
    broken = A.clone()
    broken[:, 17] = 0  # every output loses its k = 17 term
    got = R.gemm_emulate(broken, Bt, bias, R.ACT_NONE)
    out = ~((got.double() - ref).abs() <= tol)
    assert out.float().mean() > 0.8
    with pytest.raises(AssertionError, match=r"tile \(0, 0\) of 128x128"):
        R.assert_within(got, ref, tol, "dropped term", tile=(128, 128))


def test_gemv_bound_holds_for_fp32_reference():
    for M in R.GEMV_M:
        for K in R.GEMV_K:
            x, w = R.gemv_inputs(M, K)
            ref, tol = R.gemv_ref(x, w, R.GEMV_BIAS)
            got = x.float() @ w.float() + R.GEMV_BIAS
            R.assert_within(got, ref, tol, f"gemv {M}x{K}")


def test_bias_act_bound_holds_for_fp32_reference():
    for rows, n in [(R.BA_ROWS, n) for n in R.BA_WIDTHS] + [R.BA_WRAP]:
        x, bias = R.bias_act_inputs(rows, n)
        for act in (0, 1, 2, 3):
            for b in (None, bias):
                z = x.float() if b is None else x.float() + b
                ref, tol = R.bias_act_ref(x, b, act)
                R.assert_within(R.kernel_act_f32(z, act).to(R.BF16), ref, tol,
                                f"bias_act {rows}x{n} act={act}")


# ------------------------------------------------------------------- LayerNorm
def _ln_all_inputs():
    for n in R.LN_WIDTHS:
        for rows in R.LN_ROWS:
            x, res, g, b = R.ln_inputs(rows, n)
            yield f"{rows}x{n}", x, None, g, b
            yield f"{rows}x{n}+res", x, res, g, b
    for rows, n in R.LN_WRAP:
        x, res, g, b = R.ln_inputs(rows, n)
        yield f"{rows}x{n}", x, None, g, b
        yield f"{rows}x{n}+res", x, res, g, b
    for n in R.LN_ILL_WIDTHS:
        for c, s in R.LN_ILL:
            yield (f"ill n={n} c={c} s={s}",) + R.ln_ill_inputs(n, c, s)


def test_layernorm_bound_holds_for_fp32_reference():
    for what, x, res, g, b in _ln_all_inputs():
        ref, tol = R.layernorm_ref(x, res, g, b)
        R.assert_within(R.layernorm_emulate(x, res, g, b), ref, tol, what)


def _wave_kernel_emulation(x, res, gamma, beta, two_pass, eps=R.LN_EPS):
    """NumPy emulation of the wave-per-row LayerNorm kernel's fp32 arithmetic
    in its own order: lane l accumulates vectors l, l + 64, ... element by
    element (squares fused as fma), then the shfl_down tree 32, 16, ..., 1.
    two_pass=False is the one-pass var = E[f^2] - mean^2 the kernel used."""
    f32, f64 = np.float32, np.float64
    X, Rr = x.float().numpy(), res.float().numpy()
    G, Bb = gamma.numpy().astype(f32), beta.numpy().astype(f32)
    rows, n = X.shape
    nv = n // 8

    def tree(v):
        v = v.copy()
        for off in (32, 16, 8, 4, 2, 1):
            nxt = v.copy()
            nxt[:64 - off] = v[:64 - off] + v[off:]
            v = nxt
        return v[0]

    def fma(a, b, c):
        return f32(f64(a) * f64(b) + f64(c))

    out = np.empty((rows, n), f32)
    for r in range(rows):
        f = (X[r] + Rr[r]).astype(f32)
        lanes = [[f[i * 8 + j] for i in range(lane, nv, 64) for j in range(8)]
                 for lane in range(64)]
        s = np.zeros(64, f32)
        q = np.zeros(64, f32)
        for lane, vals in enumerate(lanes):
            for v in vals:
                s[lane] = s[lane] + v
                if not two_pass:
                    q[lane] = fma(v, v, q[lane])
        mean = f32(tree(s) / f32(n))
        if two_pass:
            for lane, vals in enumerate(lanes):
                for v in vals:
                    d = f32(v - mean)
                    q[lane] = fma(d, d, q[lane])
            var = f32(tree(q) / f32(n))
        else:
            var = fma(-mean, mean, f32(tree(q) / f32(n)))
        with np.errstate(invalid="ignore"):
            rstd = f32(1.0) / np.sqrt(f32(var + f32(eps)))
        out[r] = (f - mean) * rstd * G + Bb
    return torch.from_numpy(out).to(R.BF16)


def test_one_pass_variance_fails_the_layernorm_bound():
    """The bound discriminates: the kernel's former one-pass variance, in its
    own reduction order, violates it on the (768, 1000, 0.05) rows; a
    two-pass form over the same lane partition meets it on every
    ill-conditioned row."""
    x, res, g, b = R.ln_ill_inputs(768, 1000.0, 0.05)
    ref, tol = R.layernorm_ref(x, res, g, b)
    assert R.exceeds(_wave_kernel_emulation(x, res, g, b, False), ref, tol)
    for c, s in R.LN_ILL:
        x, res, g, b = R.ln_ill_inputs(768, c, s)
        ref, tol = R.layernorm_ref(x, res, g, b)
        R.assert_within(_wave_kernel_emulation(x, res, g, b, True), ref, tol,
                        f"two-pass emulation c={c} s={s}")


# --------------------------------------------------------------------- softmax
def test_softmax_bound_holds_for_fp32_reference():
    shapes = [(rows, n) for n in R.SM_WIDTHS for rows in R.SM_ROWS]
    for rows, n in shapes + [R.SM_WRAP]:
        for scale in R.SM_SCALES:
            x, masked = R.softmax_inputs(rows, n, scale)
            ref, tol = R.softmax_ref(x, scale)
            assert bool(torch.isfinite(ref).all())
            got = torch.softmax(x.float() * scale, dim=-1).to(R.BF16)
            what = f"softmax {rows}x{n} scale={scale}"
            R.assert_within(got, ref, tol, what)
            assert float((got.double().sum(-1) - 1).abs().max()) <= \
                R.SM_ROWSUM_TOL, what
            if masked is not None:
                assert bool((ref[masked] == 0).all())
                assert bool((got[masked] == 0).all())


# ------------------------------------------------------------------- attention
def test_attention_bound_holds_for_bf16_p_emulation():
    cases = [(s, f) for s in R.ATTN_SHAPES for f in R.ATTN_FAMILIES]
    for shape, family in cases + [((2, 3, 128, 64), "randn")]:
        qkv, scale = R.attention_inputs(shape, family)
        q, k, v = R.split_qkv(qkv)
        ref, tol = R.attention_ref(q, k, v, scale)
        R.assert_within(R.attention_emulate(q, k, v, scale), ref, tol,
                        f"attn {shape} {family}", tile=(128, 64))


def test_attention_rescale_families_move_the_running_max():
    """kgrow must raise the row max in (nearly) every 64-column KV tile, and
    kshrink must put it in the first tile, or the families test nothing."""
    shape = R.ATTN_SHAPES[1]
    S = shape[2]
    for family, want_first in (("kgrow", False), ("kshrink", True)):
        qkv, scale = R.attention_inputs(shape, family)
        q, k, _ = R.split_qkv(qkv)
        s = (q.double() @ k.double().transpose(-1, -2)) * scale
        tile_max = s.reshape(*s.shape[:-1], S // 64, 64).amax(-1)
        run = tile_max.cummax(-1).values
        raised = (run[..., 1:] > run[..., :-1]).double().mean()
        if want_first:
            assert float((tile_max.argmax(-1) == 0).double().mean()) > 0.7
        else:
            assert float(raised) > 0.7


# -------------------------------------------------------------------- featpack
def test_featpack_reference_rounds_ties_to_even():
    for dtype in (torch.float32, torch.float64):
        cols = R.featpack_sources(1, len(R.FP_SPECIALS) + 1, dtype)
        ref = R.featpack_ref(cols, 32)[:, 0].float()
        assert ref[0] == 1.0 and ref[1] == 1.0 + 2.0 ** -6
        assert ref[2] == -1.0
        assert ref[3] == 0 and not torch.signbit(ref[3])
        assert ref[4] == 0 and torch.signbit(ref[4])
        assert 0 < ref[5] < 2.0 ** -126  # the denormal survives
        assert torch.isinf(ref[6]) and torch.isinf(ref[7])
        assert torch.isnan(ref[8]) and torch.isinf(ref[9])
        if dtype == torch.float64:
            assert ref[len(R.FP_SPECIALS)] == 1.0
    good = torch.tensor([0.0, float("nan")]).to(R.BF16)
    R.assert_bf16_identical(good, good.clone())
    with pytest.raises(AssertionError):
        R.assert_bf16_identical(good, torch.tensor(
            [-0.0, float("nan")]).to(R.BF16))
