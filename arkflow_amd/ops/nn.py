"""Neural-net ops for the inference processor: bf16 MFMA GEMM (fused
bias+activation), LayerNorm, softmax. GPU = hand-written gfx950 kernels
(csrc/gemm_bf16.hip, csrc/rowops.hip); CPU = fp32 torch reference (also the
numerics oracle in tests)."""
from __future__ import annotations

from typing import Optional

import torch

from . import require_native

ACT_NONE, ACT_RELU, ACT_GELU, ACT_SILU = 0, 1, 2, 3

try:
    from torch.utils.weak import WeakTensorKeyDictionary
    _bias_bf16_cache = WeakTensorKeyDictionary()
except ImportError:  # pragma: no cover
    _bias_bf16_cache = {}


def _bias_bf16(bias: torch.Tensor) -> torch.Tensor:
    """Cached fp32→bf16 bias cast: inference weights are static, and a
    per-call cast is a kernel that replays inside every captured graph."""
    c = _bias_bf16_cache.get(bias)
    if c is None:
        c = bias.to(torch.bfloat16)
        _bias_bf16_cache[bias] = c
    return c
_ACTS = {"none": ACT_NONE, "relu": ACT_RELU, "gelu": ACT_GELU,
         "silu": ACT_SILU}


def linear_bf16(x: torch.Tensor, weight: torch.Tensor,
                bias: Optional[torch.Tensor] = None,
                act: str = "none") -> torch.Tensor:
    """act(x @ weight.T + bias). x:[M,K] bf16, weight:[N,K] (torch Linear
    layout — consumed directly as the GEMM's B^T operand).

    FUSED linears (activation epilogues) run our gfx950 MFMA kernels;
    PLAIN linears (no activation) go to hipBLASLt via torch.addmm — the
    division of labor the design brief prescribes (hand-written kernels for
    fused hot ops, the vendor library for plain GEMMs).
    Env overrides: ARKFLOW_GEMM_VARIANT forces a specific native kernel;
    ARKFLOW_PLAIN_GEMM=native keeps plain linears on our kernel.
    """
    import os
    a = _ACTS[act]
    if x.is_cuda:
        nat = require_native()
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        force = os.environ.get("ARKFLOW_GEMM_VARIANT")
        if force is not None:
            out = nat.gemm_bf16_variant(x2, weight.contiguous(), bias, a,
                                        int(force))
        elif a == ACT_NONE and \
                os.environ.get("ARKFLOW_PLAIN_GEMM", "blaslt") != "native":
            out = torch.nn.functional.linear(
                x2, weight, _bias_bf16(bias) if bias is not None else None)
        elif a != ACT_NONE and \
                os.environ.get("ARKFLOW_FUSED_GEMM", "native") == "split":
            # A/B path: hipBLASLt GEMM + our activation kernel (measured
            # per-shape; see profiles r15)
            out = torch.nn.functional.linear(
                x2, weight, _bias_bf16(bias) if bias is not None else None)
            out = nat.bias_act_bf16(out, None, a)
        else:
            out = nat.gemm_bf16(x2, weight.contiguous(), bias, a)
        return out.reshape(*x.shape[:-1], weight.shape[0])
    y = torch.nn.functional.linear(x.float(), weight.float(),
                                   bias.float() if bias is not None else None)
    if act == "relu":
        y = torch.relu(y)
    elif act == "gelu":
        y = torch.nn.functional.gelu(y, approximate="tanh")
    elif act == "silu":
        y = torch.nn.functional.silu(y)
    return y.to(x.dtype)


def layernorm_bf16(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                   eps: float = 1e-5,
                   residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    if x.is_cuda:
        nat = require_native()
        return nat.layernorm_bf16(x.contiguous(), gamma, beta, eps,
                                  residual.contiguous()
                                  if residual is not None else None)
    xf = x.float()
    if residual is not None:
        xf = xf + residual.float()
    y = torch.nn.functional.layer_norm(
        xf, (x.shape[-1],), gamma.float(), beta.float(), eps)
    return y.to(x.dtype)


def softmax_bf16(x: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    if x.is_cuda:
        nat = require_native()
        return nat.softmax_bf16(x.contiguous(), scale)
    return torch.softmax(x.float() * scale, dim=-1).to(x.dtype)


def _lens_i32(lengths: torch.Tensor, device: torch.device) -> torch.Tensor:
    """Valid key counts as contiguous int32 on `device` (a no-op for a tensor
    that already is). Values are not read on the host; every consumer treats
    L < 0 as 0 and L > S as S."""
    return lengths.to(device=device, dtype=torch.int32).contiguous()


def _unfused_attention(q, k, v, lengths, softmax):
    """Attention out of whole-tensor ops; `softmax(scores)` returns the
    probabilities of the unscaled scores. With `lengths`, the variable-length
    contract: keys >= L are masked to -inf before the softmax, V rows >= L
    are replaced by 0 with a select (a NaN there must not meet a zero
    probability in the product) and output rows >= L are written as +0; rows
    with L == 0 come back NaN from the softmax and are selected away."""
    scores = torch.matmul(q, k.transpose(-1, -2))
    if lengths is None:
        return torch.matmul(softmax(scores), v)
    S = q.shape[-2]
    L = _lens_i32(lengths, q.device).view(-1, 1, 1, 1)
    pos = torch.arange(S, device=q.device, dtype=torch.int32)
    key_ok = pos.view(1, 1, 1, S) < L
    row_ok = pos.view(1, 1, S, 1) < L
    scores = torch.where(key_ok, scores,
                         torch.full_like(scores, float("-inf")))
    p = softmax(scores)
    p = torch.where(key_ok & row_ok, p, torch.zeros_like(p))
    out = torch.matmul(p, torch.where(row_ok, v, torch.zeros_like(v)))
    return torch.where(row_ok, out, torch.zeros_like(out))


def attention_bf16(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                   scale: float,
                   lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused attention for [B,H,S,D] bf16. GPU: one-workgroup-per-(b,h)
    MFMA kernel (csrc/attention.hip) for its supported tile (S=128, D=64 —
    the BERT-base shape); other shapes compose batched hipBLASLt GEMMs with
    our softmax kernel. CPU: fp32 reference.

    lengths: optional int [B] tensor of valid key counts, 0 <= L <= S. Row b
    then attends over its first L keys only, its output rows >= L are +0, and
    whatever q, k and v hold at rows >= L (NaN included) is ignored."""
    if q.is_cuda:
        nat = require_native()
        qc, kc, vc = q.contiguous(), k.contiguous(), v.contiguous()
        if lengths is not None:
            lengths = _lens_i32(lengths, q.device)
        try:
            return nat.attention_bf16(qc, kc, vc, scale, lens=lengths)
        except RuntimeError as e:
            if "unsupported shape" not in str(e):
                raise
        return _unfused_attention(
            qc, kc, vc, lengths,
            lambda sc: nat.softmax_bf16(
                sc.reshape(-1, sc.shape[-1]).contiguous(),
                scale).reshape(sc.shape))
    return _unfused_attention(
        q.float(), k.float(), v.float(), lengths,
        lambda sc: torch.softmax(sc * scale, dim=-1)).to(q.dtype)


def attention_qkv_bf16(qkv: torch.Tensor, scale: float,
                       lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Attention straight from the QKV projection: qkv [B,S,3,H,D] bf16 →
    [B,S,H*D]. GPU: strided-load kernel, zero transpose copies; shapes the
    kernel doesn't cover (or CPU) go through the permuted path. `lengths`
    as in attention_bf16."""
    B, S, three, H, D = qkv.shape
    if qkv.is_cuda:
        nat = require_native()
        try:
            return nat.attention_qkv_bf16(
                qkv.contiguous(), scale,
                lens=None if lengths is None
                else _lens_i32(lengths, qkv.device))
        except RuntimeError as e:
            if "unsupported shape" not in str(e):
                raise
    q = qkv[:, :, 0].permute(0, 2, 1, 3).contiguous()
    k = qkv[:, :, 1].permute(0, 2, 1, 3).contiguous()
    v = qkv[:, :, 2].permute(0, 2, 1, 3).contiguous()
    attn = attention_bf16(q, k, v, scale, lengths)
    return attn.permute(0, 2, 1, 3).reshape(B, S, H * D)
