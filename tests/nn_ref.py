"""fp64 references, per-element error bounds and shared inputs for the
inference kernels (GEMM family, row ops, gemv, featpack, attention).

Plain helpers, no fixtures: `tests/test_nn_kernels.py` runs the HIP kernels
against these on the GPU, `tests/test_nn_tolerances.py` proves on the CPU that
a correct implementation meets every bound on the very same inputs.

Every comparison is `|got - ref64| <= tol` element-wise (`assert_within`).
Bound ingredients:
  * half an ulp of bf16 is 2^-9 relative;
  * fp32 accumulation over K terms is bounded by K * 2^-24 * sum|a||b|;
  * every term carries a factor 2 of margin (the MFMA's internal rounding is
    not documented to be per-step IEEE).
"""
from __future__ import annotations

import math
from collections import namedtuple

import torch

BF16 = torch.bfloat16
F64 = torch.float64

ACT_NONE, ACT_RELU, ACT_GELU, ACT_SILU = 0, 1, 2, 3
ACT_NAMES = {0: "none", 1: "relu", 2: "gelu", 3: "silu"}
# bound on the activation's slope (how much it can amplify an error in z)
ACT_SLOPE = {ACT_NONE: 1.0, ACT_RELU: 1.0, ACT_GELU: 1.13, ACT_SILU: 1.1}

# Absolute error of the kernels' own activation formula (apply_act in
# csrc/gemm_common.h, the one copy every GEMM epilogue and bias_act_bf16 call:
# tanh-GELU through exp(2c) with c clamped to +-10, SiLU
# as x / (1 + exp(-x))) evaluated in fp32 torch against exact fp64 tanh-GELU
# and SiLU on a 2,400,001-point grid over [-12, 12]: the maximum absolute
# difference is 1.157e-6 (SiLU, the fp32 rounding of outputs near 12; GELU
# peaks at 4.33e-7), doubled and rounded up in the third digit.
# `measure_act_eps()` reproduces the measurement;
# test_nn_tolerances.py::test_act_eps_constant_matches_measurement pins it.
ACT_EPS = 2.32e-6

LN_EPS = 1e-5


def _gen(seed: int) -> torch.Generator:
    g = torch.Generator()
    g.manual_seed(seed)
    return g


# --------------------------------------------------------------- comparison
def assert_within(got, ref, tol, what="", tile=None):
    """|got - ref| <= tol element-wise (NaN/inf in `got` where `ref` is finite
    fails). On failure reports the worst element's index and, for 2-D outputs
    with `tile=(BM, BN)`, the tile it falls in and its offset inside it."""
    g = got.to(F64)
    assert g.shape == ref.shape, f"{what}: shape {tuple(g.shape)} vs " \
                                 f"{tuple(ref.shape)}"
    err = (g - ref).abs()
    bad = ~(err <= tol)  # NaN compares false -> bad
    nbad = int(bad.sum())
    if nbad == 0:
        return
    excess = torch.where(torch.isfinite(err), err - tol,
                         torch.full_like(err, float("inf")))
    excess = torch.where(bad, excess, torch.full_like(err, -float("inf")))
    flat = int(excess.reshape(-1).argmax())
    idx = []
    for d in reversed(ref.shape):
        idx.append(flat % d)
        flat //= d
    idx = tuple(reversed(idx))
    msg = (f"{what}: {nbad}/{err.numel()} elements out of bound; worst at "
           f"{idx}: got {float(g[idx])!r} ref {float(ref[idx])!r} "
           f"err {float(err[idx]):.3e} tol {float(tol[idx]):.3e}")
    if tile is not None and len(idx) >= 2:
        r, c = idx[-2], idx[-1]
        msg += (f"; tile ({r // tile[0]}, {c // tile[1]}) of "
                f"{tile[0]}x{tile[1]}, offset ({r % tile[0]}, {c % tile[1]})")
    raise AssertionError(msg)


def exceeds(got, ref, tol) -> bool:
    """True when `got` violates the bound anywhere (or is not finite)."""
    err = (got.to(F64) - ref).abs()
    return bool((~(err <= tol)).any())


# --------------------------------------------------------------- activations
def act64(z: torch.Tensor, act: int) -> torch.Tensor:
    """Exact activation in fp64 (tanh-GELU, SiLU, ReLU)."""
    if act == ACT_RELU:
        return torch.relu(z)
    if act == ACT_GELU:
        c = math.sqrt(2.0 / math.pi) * (z + 0.044715 * z * z * z)
        return 0.5 * z * (1.0 + torch.tanh(c))
    if act == ACT_SILU:
        return z * torch.sigmoid(z)
    return z


def kernel_act_f32(x: torch.Tensor, act: int) -> torch.Tensor:
    """The kernels' own activation formulas, evaluated in fp32 torch."""
    x = x.float()
    if act == ACT_RELU:
        return torch.relu(x)
    if act == ACT_GELU:
        c = 0.7978845608028654 * (x + 0.044715 * x * x * x)
        c = c.clamp(-10.0, 10.0)
        e = torch.exp(2.0 * c)
        return 0.5 * x * (1.0 + (e - 1.0) / (e + 1.0))
    if act == ACT_SILU:
        return x / (1.0 + torch.exp(-x))
    return x


def measure_act_eps() -> dict:
    """Max |kernel formula in fp32 - exact fp64| per activation on a dense
    grid over [-12, 12] (the raw figures; ACT_EPS is twice their maximum)."""
    x = torch.linspace(-12.0, 12.0, 2_400_001, dtype=F64).float()
    out = {}
    for act in (ACT_GELU, ACT_SILU):
        d = (kernel_act_f32(x, act).to(F64) - act64(x.to(F64), act)).abs()
        out[ACT_NAMES[act]] = float(d.max())
    return out


# ---------------------------------------------------------------------- GEMM
def gemm_ref(A, Bt, bias, act):
    """(ref, tol) for act(A @ Bt^T + bias) with bf16 output.
    tol = 2^-8 |ref| + L K 2^-23 (|A| @ |Bt|^T) + act_eps."""
    K = A.shape[1]
    a, b = A.to(F64), Bt.to(F64)
    z = a @ b.T
    if bias is not None:
        z = z + bias.to(F64)
    ref = act64(z, act)
    s = a.abs() @ b.abs().T
    tol = 2.0 ** -8 * ref.abs() + ACT_SLOPE[act] * K * 2.0 ** -23 * s + \
        (ACT_EPS if act in (ACT_GELU, ACT_SILU) else 0.0)
    return ref, tol


def gemm_emulate(A, Bt, bias, act):
    """A correct implementation: fp32 matmul + bias, the kernel's activation
    formula in fp32, rounded to bf16."""
    z = A.float() @ Bt.float().T
    if bias is not None:
        z = z + bias.float()
    return kernel_act_f32(z, act).to(BF16)


# variant id (GemmVariant in csrc/gemm_api.h) -> (BM, BN, K values): tile
# sizes read from the launch_tiles<BM, BN> calls in csrc/gemm_bf16.hip and
# csrc/gemm_8phase.hip; K values are multiples of the variant's BK from
# the launcher's minimum K-tile count upwards.
GEMM_VARIANTS = {
    0: (128, 128, (32, 64, 160)),        # 128^2 BK=32 (dispatcher fall-through)
    6: (64, 64, (32, 64, 160)),          # skinny 64^2 BK=32
    3: (128, 128, (64, 96, 160)),        # 2-phase BK=32, >= 2 K-tiles
    7: (128, 128, (64, 128, 320)),       # k64
    8: (128, 128, (64, 128, 320)),       # k64s
    9: (128, 128, (64, 128, 320)),       # k64d
    10: (128, 128, (64, 128, 320)),      # k64p
    11: (256, 256, (64, 128, 320)),      # k64w
    12: (128, 128, (64, 128, 320)),      # k64s3
    1: (256, 256, (192, 256, 320, 448)),  # 8-phase BM=256 linear, >= 3 K-tiles
    2: (256, 256, (192, 256, 320, 448)),  # 8-phase BM=256 swizzled
    4: (128, 256, (192, 256, 320, 448)),  # 8-phase BM=128 linear
    5: (128, 256, (192, 256, 320, 448)),  # 8-phase BM=128 swizzled
}
EPILOGUES = [(act, hb) for act in (ACT_NONE, ACT_RELU, ACT_GELU, ACT_SILU)
             for hb in (False, True)]

GemmCase = namedtuple("GemmCase", "id variant shape M N K act has_bias seed")


def _gemm_shapes(bm, bn):
    return {"a": (bm - 3, bn - 5), "b": (5 * bm - 7, 4 * bn - 1),
            "c": (1, bn + 1)}


def gemm_variant_cases():
    """Shapes (a) ragged single tile, (b) ragged 20-tile grid, (c) single row
    at every K of the variant, epilogues rotating through all eight
    combinations; at shape (b) and the variant's middle K the full cross of
    epilogues (flagged shape 'x')."""
    cases = []
    seed = 1000
    for v, (bm, bn, ks) in GEMM_VARIANTS.items():
        shapes = _gemm_shapes(bm, bn)
        kx = ks[1]
        rot = v  # start each variant at a different epilogue
        for K in ks:
            for sh in ("a", "b", "c"):
                if sh == "b" and K == kx:
                    continue  # covered by the full cross below
                act, hb = EPILOGUES[rot % 8]
                rot += 1
                M, N = shapes[sh]
                seed += 1
                cases.append(GemmCase(
                    f"v{v}-{sh}-{M}x{N}x{K}-{ACT_NAMES[act]}-"
                    f"{'bias' if hb else 'nobias'}", v, sh, M, N, K, act, hb,
                    seed))
        M, N = shapes["b"]
        for act, hb in EPILOGUES:
            seed += 1
            cases.append(GemmCase(
                f"v{v}-x-{M}x{N}x{kx}-{ACT_NAMES[act]}-"
                f"{'bias' if hb else 'nobias'}", v, "x", M, N, kx, act, hb,
                seed))
    return cases


# one shape per branch of the gemm_bf16 dispatcher, each with gelu + bias
GEMM_DISPATCH_CASES = [
    GemmCase("8phase-4000x2049x1536", None, "d", 4000, 2049, 1536, ACT_GELU,
             True, 501),
    GemmCase("bk32-2000x1700x96", None, "d", 2000, 1700, 96, ACT_GELU, True,
             502),
    GemmCase("k64s-2000x1700x128", None, "d", 2000, 1700, 128, ACT_GELU, True,
             503),
    GemmCase("skinny-300x257x96", None, "d", 300, 257, 96, ACT_GELU, True,
             504),
]
# the variant id each of those branches is documented to take (bindings.cpp
# gemm_bf16: GEMM_8P256S, GEMM_BK32, GEMM_K64S, GEMM_SKINNY)
GEMM_DISPATCH_VARIANTS = [2, 0, 8, 6]


def gemm_inputs(case):
    """Fresh random asymmetric A [M,K], Bt [N,K] bf16 and bias = 4 randn."""
    g = _gen(case.seed)
    A = torch.randn(case.M, case.K, generator=g).to(BF16)
    Bt = torch.randn(case.N, case.K, generator=g).to(BF16)
    bias = 4.0 * torch.randn(case.N, generator=g) if case.has_bias else None
    return A, Bt, bias


# ---------------------------------------------------------------------- gemv
GEMV_M = (1, 7, 8, 9, 4097)
GEMV_K = (1, 5, 8, 32, 256, 1000)
GEMV_BIAS = 0.375  # exactly representable: the binding casts it to fp32


def gemv_inputs(M, K):
    g = _gen(7000 + 31 * M + K)
    return (torch.randn(M, K, generator=g).to(BF16),
            torch.randn(K, generator=g).to(BF16))


def gemv_ref(x, w, bias):
    """tol = K 2^-23 sum|x||w| + 2^-23 |ref| (fp32 output)."""
    K = x.shape[1]
    ref = x.to(F64) @ w.to(F64) + bias
    s = x.to(F64).abs() @ w.to(F64).abs()
    return ref, K * 2.0 ** -23 * s + 2.0 ** -23 * ref.abs()


# ----------------------------------------------------------------- LayerNorm
LN_WIDTHS = (8, 64, 504, 512, 520, 768, 1024, 1032, 2048, 2056, 4096)
LN_ROWS = (1, 3, 5)
LN_WRAP = ((16388, 64), (2051, 2056))  # past the wave / block grid caps
LN_ILL = ((1000.0, 0.05), (256.0, 0.05), (100.0, 0.02), (1000.0, 0.5))
LN_ILL_WIDTHS = (256, 768, 1536, 4096)
LN_ILL_ROWS = 4


def ln_inputs(rows, n):
    """x, residual bf16 [rows, n]; gamma, beta fp32 [n] with both signs."""
    g = _gen(3000 + 17 * rows + n)
    x = (1.5 * torch.randn(rows, n, generator=g) + 0.3).to(BF16)
    res = torch.randn(rows, n, generator=g).to(BF16)
    gamma = torch.randn(n, generator=g)
    beta = torch.randn(n, generator=g)
    return x, res, gamma, beta


def ln_ill_inputs(n, c, sigma, rows=LN_ILL_ROWS):
    """x = bf16(c) everywhere, residual = bf16(sigma * randn): the row's mean
    dwarfs its spread, which a one-pass E[f^2] - mean^2 cannot resolve."""
    g = _gen(4000 + n + int(c) + int(sigma * 1000))
    x = torch.full((rows, n), c).to(BF16)
    res = (sigma * torch.randn(rows, n, generator=g)).to(BF16)
    gamma = torch.randn(n, generator=g)
    beta = torch.randn(n, generator=g)
    return x, res, gamma, beta


def layernorm_ref(x, res, gamma, beta, eps=LN_EPS):
    """tol = 2^-8 |ref| + 2^-18 ((1 + |mu|/s) |gamma| max(1, |xhat|) + |beta|)
    with mu, s = sqrt(var + eps) and xhat from the fp64 reference."""
    f = x.to(F64)
    if res is not None:
        f = f + res.to(F64)
    mu = f.mean(-1, keepdim=True)
    var = ((f - mu) ** 2).mean(-1, keepdim=True)
    s = torch.sqrt(var + eps)
    xhat = (f - mu) / s
    ga, be = gamma.to(F64), beta.to(F64)
    ref = xhat * ga + be
    tol = 2.0 ** -8 * ref.abs() + 2.0 ** -18 * (
        (1.0 + mu.abs() / s) * ga.abs() * xhat.abs().clamp(min=1.0) +
        be.abs())
    return ref, tol


def layernorm_emulate(x, res, gamma, beta, eps=LN_EPS):
    """A correct implementation: fp32 layer_norm of x + res, rounded to bf16."""
    f = x.float()
    if res is not None:
        f = f + res.float()
    return torch.nn.functional.layer_norm(
        f, (x.shape[-1],), gamma.float(), beta.float(), eps).to(BF16)


# ------------------------------------------------------------------- softmax
SM_WIDTHS = (8, 64, 128, 2040, 2048, 2056, 4096)
SM_ROWS = (1, 5)
SM_WRAP = (4099, 64)
SM_SCALES = (1.0, 0.125, -1.0)


def softmax_inputs(rows, n, scale):
    """4 randn logits. With >= 5 rows: row 1 has one dominant logit (+80),
    row 2 is all-equal, row 3 mixes finite entries with masked ones (-inf
    after scaling, so the entry is -inf * sign(scale)), row 4 holds +-3e4."""
    g = _gen(5000 + 13 * rows + n)
    x = 4.0 * torch.randn(rows, n, generator=g)
    masked = None
    if rows >= 5:
        x[1, (3 * n) // 7] = 80.0
        x[2, :] = 1.25
        masked = torch.zeros(rows, n, dtype=torch.bool)
        masked[3] = torch.rand(n, generator=g) < 0.4
        masked[3, n // 2] = False  # at least one finite entry
        masked[3, 0] = True
        x[masked] = -math.copysign(float("inf"), scale)
        x[4] = torch.where(torch.rand(n, generator=g) < 0.5, 3e4, -3e4)
        x[4, n - 1] = 3e4
    return x.to(BF16), masked


def softmax_ref(x, scale):
    """tol = 2^-8 ref + 2^-14 ref + 2^-126."""
    ref = torch.softmax(x.to(F64) * scale, dim=-1)
    return ref, (2.0 ** -8 + 2.0 ** -14) * ref + 2.0 ** -126


SM_ROWSUM_TOL = 2.0 ** -8


# ------------------------------------------------------------------ bias_act
BA_WIDTHS = (1, 7, 768)
BA_ROWS = 3
BA_WRAP = (700, 768)  # 537600 elements > 2048 blocks x 256 threads


def bias_act_inputs(rows, n):
    g = _gen(6000 + 7 * rows + n)
    return (3.0 * torch.randn(rows, n, generator=g)).to(BF16), \
        4.0 * torch.randn(n, generator=g)


def bias_act_ref(x, bias, act):
    """The GEMM bound with the single fp32 add in place of the K-term sum:
    tol = 2^-8 |ref| + L 2^-23 (|x| + |bias|) + act_eps."""
    z = x.to(F64)
    s = z.abs()
    if bias is not None:
        z = z + bias.to(F64)
        s = s + bias.to(F64).abs()
    ref = act64(z, act)
    tol = 2.0 ** -8 * ref.abs() + ACT_SLOPE[act] * 2.0 ** -23 * s + \
        (ACT_EPS if act in (ACT_GELU, ACT_SILU) else 0.0)
    return ref, tol


# ------------------------------------------------------------------ featpack
FP_SHAPES = ((1, 32), (9, 32), (32, 32), (3, 64))
FP_ROWS = (1, 255)
FP_WRAP = (524_300, 3, 32)  # n past 2048 blocks x 256 threads

# round-to-nearest-even ties of the bf16 cast (1 + 2^-8 -> 1, 1 + 3 2^-8 ->
# 1 + 2^-6), signed zeros, an fp32 denormal, overflow to inf, inf and NaN
FP_SPECIALS = (1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 0.0,
               -0.0, 1e-40, float("inf"), -float("inf"), float("nan"),
               3.4028234663852886e38, -1.0 - 2.0 ** -9, 2.0 ** -126)


def featpack_sources(nf, n, dtype):
    """nf source columns of length n: the special values rotated by column,
    then randn * 100. f64 sources add a value that rounds to an fp32 tie."""
    g = _gen(8000 + 3 * nf + n)
    sp = list(FP_SPECIALS)
    if dtype == F64:
        sp.append(1.0 + 2.0 ** -8 + 2.0 ** -40)
    cols = []
    for f in range(nf):
        c = (100.0 * torch.randn(n, generator=g)).to(dtype)
        m = min(n, len(sp))
        c[:m] = torch.tensor([sp[(i + f) % len(sp)] for i in range(m)],
                             dtype=dtype)
        cols.append(c)
    return cols


def featpack_ref(cols, kpad):
    """[n, kpad] bf16: src.float().to(bf16) per column, zero pad columns."""
    n = cols[0].shape[0]
    out = torch.zeros(n, kpad, dtype=BF16)
    for f, c in enumerate(cols):
        out[:, f] = c.float().to(BF16)
    return out


def assert_bf16_identical(got, ref, what=""):
    """Bitwise equality (so -0 != +0) except that any NaN matches any NaN."""
    g, r = got.cpu(), ref.cpu()
    gn, rn = torch.isnan(g), torch.isnan(r)
    assert torch.equal(gn, rn), f"{what}: NaN positions differ"
    gb = torch.where(gn, torch.zeros_like(g), g).view(torch.int16)
    rb = torch.where(rn, torch.zeros_like(r), r).view(torch.int16)
    if not torch.equal(gb, rb):
        i = torch.nonzero(gb != rb)[0].tolist()
        raise AssertionError(
            f"{what}: first mismatch at {tuple(i)}: got "
            f"{float(g[tuple(i)])!r} ref {float(r[tuple(i)])!r}")


# ----------------------------------------------------------------- attention
# S=64: the smallest flash shape, one KV tile, waves 2 and 3 entirely past S
# (the q-row clamp and the row < S store guard carry the result). Appended:
# test_nn_tolerances names ATTN_SHAPES[1].
ATTN_SHAPES = ((2, 3, 192, 64), (1, 2, 320, 64), (2, 2, 64, 64))
ATTN_FAMILIES = ("randn", "kgrow", "kshrink", "scale1")


def attention_inputs(shape, family):
    """qkv [B,S,3,H,D] bf16 and the softmax scale.
    kgrow: k[s] *= 1 + s/16 so the row max grows with every KV tile (the
    running-max rescale moves far); kshrink: the same reversed, max in the
    first tile; scale1: scale = 1 so scores reach tens."""
    B, H, S, D = shape
    g = _gen(9000 + S + 7 * ATTN_FAMILIES.index(family))
    qkv = torch.randn(B, S, 3, H, D, generator=g)
    ramp = 1.0 + torch.arange(S, dtype=torch.float32) / 16.0
    if family == "kgrow":
        qkv[:, :, 1] *= ramp.view(1, S, 1, 1)
    elif family == "kshrink":
        qkv[:, :, 1] *= ramp.flip(0).view(1, S, 1, 1)
    scale = 1.0 if family == "scale1" else D ** -0.5
    return qkv.to(BF16), scale


def split_qkv(qkv):
    """[B,S,3,H,D] -> q, k, v as contiguous [B,H,S,D]."""
    return tuple(qkv[:, :, i].permute(0, 2, 1, 3).contiguous()
                 for i in range(3))


def attention_ref(q, k, v, scale):
    """[B,H,S,D] in, (ref, tol) out: tol = 2^-7 (P @ |V|) + 2^-8 |ref|."""
    q64, k64, v64 = q.to(F64), k.to(F64), v.to(F64)
    p = torch.softmax(q64 @ k64.transpose(-1, -2) * scale, dim=-1)
    ref = p @ v64
    return ref, 2.0 ** -7 * (p @ v64.abs()) + 2.0 ** -8 * ref.abs()


def attention_emulate(q, k, v, scale):
    """A correct bf16-P implementation: fp32 softmax, P cast to bf16, P V in
    fp32, output cast to bf16."""
    p = torch.softmax(q.float() @ k.float().transpose(-1, -2) * scale, dim=-1)
    return (p.to(BF16).float() @ v.float()).to(BF16)


def heads_to_rows(o):
    """[B,H,S,D] -> [B,S,H*D], the layout attention_qkv_bf16 writes."""
    B, H, S, D = o.shape
    return o.permute(0, 2, 1, 3).reshape(B, S, H * D)
