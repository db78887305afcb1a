"""Shared inputs, fp64 reference and bound for variable-length attention
(per-sequence key-length masking), used by test_attention_varlen_cpu.py (CPU)
and test_attention_varlen.py (GPU kernels).

Contract under test, for batch row b with L = lens[b]:
  * output rows i < L are softmax(scale q_i K[:L]^T) V[:L];
  * output rows i >= L are exactly +0;
  * rows >= L of q, k, v may hold anything (NaN, +-Inf, 3e38).

Reference and tolerance are fp64 over inputs whose padded rows are replaced
by 0, with the project's attention bound applied to the MASKED P:
    tol = 2^-7 (P @ |V|) + 2^-8 |ref|
P is 0 at query rows >= L and key columns >= L, so both ref and tol are 0 at
output rows >= L: those rows must be exactly 0.
"""
from __future__ import annotations

import functools

import torch

from tests import nn_ref as R

BF16 = R.BF16
F64 = R.F64

# (B, H, S, D), lens. S=128: the full-S kernel at its 16-column fragment,
# 32-column K-step and 32-row wave edges. S=192/320: the flash kernel at its
# 64-column KV-tile and 128-row Q-block edges, partial last Q block included.
# S=64: the flash kernel's smallest shape, one KV tile, waves 2 and 3 past S.
VARLEN_CASES = (
    ((10, 2, 128, 64), (1, 15, 16, 17, 32, 33, 64, 96, 127, 128)),
    ((8, 2, 192, 64), (1, 63, 64, 65, 128, 129, 191, 192)),
    ((10, 1, 320, 64), (1, 64, 127, 128, 129, 200, 256, 257, 319, 320)),
    ((6, 2, 64, 64), (1, 31, 32, 33, 63, 64)),
)
VARLEN_FAMILIES = ("randn", "scale1", "lastkey", "poison")
POISON = (float("nan"), float("inf"), -float("inf"), 3e38)

CASE_PARAMS = [(ci, fam) for ci in range(len(VARLEN_CASES))
               for fam in VARLEN_FAMILIES]
CASE_IDS = [f"S{VARLEN_CASES[ci][0][2]}-{fam}" for ci, fam in CASE_PARAMS]


def row_valid(lens, S):
    """[B, S] bool: position s of batch row b is < lens[b]."""
    L = torch.as_tensor(lens, dtype=torch.int64).view(-1, 1)
    return torch.arange(S).view(1, S) < L


def poison_rows(qkv, lens):
    """Rows s >= L of q, k and v <- NaN, +Inf, -Inf, 3e38 cycling by s % 4."""
    B, S = qkv.shape[:2]
    fill = torch.tensor([POISON[s % 4] for s in range(S)],
                        dtype=qkv.dtype).view(1, S, 1, 1, 1)
    pad = ~row_valid(lens, S).view(B, S, 1, 1, 1)
    return torch.where(pad, fill.expand_as(qkv), qkv)


def varlen_inputs(shape, lens, family):
    """qkv [B,S,3,H,D] bf16 and the softmax scale, seeded in the style of
    nn_ref.attention_inputs.
    lastkey: k[b, L-1] *= 4, so a mask one key short moves the output;
    poison: padded rows hold NaN/+-Inf/3e38, so a mask one key long, or a
    0 * Inf in the P V product, shows as NaN; scale1: scale = 1."""
    B, H, S, D = shape
    g = R._gen(9500 + S + 7 * VARLEN_FAMILIES.index(family))
    qkv = torch.randn(B, S, 3, H, D, generator=g)
    if family == "lastkey":
        for b, L in enumerate(lens):
            if L > 0:
                qkv[b, L - 1, 1] *= 4.0
    elif family == "poison":
        qkv = poison_rows(qkv, lens)
    scale = 1.0 if family == "scale1" else D ** -0.5
    return qkv.to(BF16), scale


def _zero_padded(x, lens):
    """[B,H,S,D] with rows >= L replaced by 0 (a select: NaN-safe)."""
    ok = row_valid(lens, x.shape[2]).view(x.shape[0], 1, x.shape[2], 1)
    return torch.where(ok, x, torch.zeros_like(x))


def _masked_p(q, k, scale, lens):
    """softmax over keys < L, 0 at key columns >= L and query rows >= L."""
    B, _, S, _ = q.shape
    ok = row_valid(lens, S)
    key_ok = ok.view(B, 1, 1, S)
    both = key_ok & ok.view(B, 1, S, 1)
    s = q @ k.transpose(-1, -2) * scale
    s = torch.where(key_ok, s, torch.full_like(s, -float("inf")))
    p = torch.softmax(s, dim=-1)  # an L == 0 row is NaN here, selected away
    return torch.where(both, p, torch.zeros_like(p))


def varlen_ref(q, k, v, scale, lens):
    """[B,H,S,D] in, (ref, tol) fp64 out."""
    q64, k64, v64 = (_zero_padded(t.to(F64), lens) for t in (q, k, v))
    p = _masked_p(q64, k64, scale, lens)
    ref = p @ v64
    return ref, 2.0 ** -7 * (p @ v64.abs()) + 2.0 ** -8 * ref.abs()


def varlen_emulate(q, k, v, scale, lens):
    """A correct bf16-P implementation: fp32 masked softmax, P cast to bf16,
    fp32 P V, bf16 output, padded rows zero."""
    qf, kf, vf = (_zero_padded(t.float(), lens) for t in (q, k, v))
    p = _masked_p(qf, kf, scale, lens)
    return (p.to(BF16).float() @ vf).to(BF16)


@functools.lru_cache(maxsize=None)
def case(ci, family):
    """Inputs and reference of one shape x family, computed once and shared:
    dict(shape, lens, qkv, scale, q, k, v, ref, tol); treat as read-only."""
    shape, lens = VARLEN_CASES[ci]
    qkv, scale = varlen_inputs(shape, lens, family)
    q, k, v = R.split_qkv(qkv)
    ref, tol = varlen_ref(q, k, v, scale, lens)
    return dict(shape=shape, lens=lens, qkv=qkv, scale=scale, q=q, k=k, v=v,
                ref=ref, tol=tol)


def assert_padded_rows_zero(out, lens, what=""):
    """out [B,H,S,D]: rows >= L are +0 bit for bit (so -0 fails too)."""
    B, _, S, _ = out.shape
    pad = ~row_valid(lens, S).view(B, 1, S, 1).expand_as(out)
    bits = out.cpu().contiguous().view(torch.int16)
    assert not bool((bits[pad] != 0).any()), \
        f"{what}: a padded output row is not exactly +0"
