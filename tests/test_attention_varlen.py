"""Variable-length (key-length masked) attention on the GPU: both fused
kernels of csrc/attention.hip through both bindings, the unfused fallback,
BertEncoder's masked hipGraph path and the inference processor's
`sequence_column` mode. Inputs, reference and bound: tests/attn_varlen_ref.py
(tests/test_attention_varlen_cpu.py proves them on the CPU)."""
import pytest
import torch

from arkflow_amd.batch import MessageBatch
from tests import attn_varlen_ref as V
from tests import nn_ref as R

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


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
    freed to the next allocation of that size: fill it with NaN so a row the
    kernel fails to write cannot inherit a plausible value."""
    t = torch.full(shape, float("nan"), dtype=dtype, device=dev)
    del t


def _still_clean(dev):
    torch.cuda.synchronize()
    assert int((torch.arange(8, device=dev) * 2).sum()) == 56


def _lens(lens, dev):
    return torch.tensor(lens, dtype=torch.int32, device=dev)


def _rows_to_heads(o, H):
    """[B,S,H*D] (what attention_qkv_bf16 writes) -> [B,H,S,D]."""
    B, S, HD = o.shape
    return o.reshape(B, S, H, HD // H).permute(0, 2, 1, 3)


def _check(out, ref, tol, lens, what):
    out = out.cpu()
    assert torch.isfinite(out.float()).all(), f"{what}: non-finite output"
    R.assert_within(out, ref, tol, what)
    V.assert_padded_rows_zero(out, lens, what)


def _both_entry_points(nat, dev, qkv, scale, lens, ref, tol, what):
    B, S, _, H, D = qkv.shape
    q, k, v = (t.to(dev) for t in R.split_qkv(qkv))
    ld = _lens(lens, dev)
    _poison((B, H, S, D), BF16, dev)
    _check(nat.attention_bf16(q, k, v, scale, lens=ld), ref, tol, lens,
           f"attention_bf16 {what}")
    _poison((B, S, H * D), BF16, dev)
    out = nat.attention_qkv_bf16(qkv.to(dev), scale, lens=ld)
    _check(_rows_to_heads(out, H), ref, tol, lens,
           f"attention_qkv_bf16 {what}")


# ------------------------------------------------------------------- kernels
@pytest.mark.parametrize("ci,family", V.CASE_PARAMS, ids=V.CASE_IDS)
def test_varlen_kernels(nat, dev, ci, family):
    c = V.case(ci, family)
    _both_entry_points(nat, dev, c["qkv"], c["scale"], c["lens"], c["ref"],
                       c["tol"], f"S={c['shape'][2]} {family}")


@pytest.mark.parametrize("S", (128, 192))
def test_zero_length_row(nat, dev, S):
    lens = (S // 2 + 1, 0, S)
    qkv, scale = V.varlen_inputs((3, 2, S, 64), lens, "poison")
    ref, tol = V.varlen_ref(*R.split_qkv(qkv), scale, lens)
    assert not bool(ref[1].any()) and not bool(tol[1].any())
    _both_entry_points(nat, dev, qkv, scale, lens, ref, tol, f"S={S} L=0")


@pytest.mark.parametrize("ci", (0, 1))
def test_padding_invariance_bitwise(nat, dev, ci):
    """Same valid prefix, different finite padding: same bits out."""
    c = V.case(ci, "randn")
    B, H, S, D = c["shape"]
    other = torch.randn(B, S, 3, H, D, generator=R._gen(4242)).to(BF16)
    pad = ~V.row_valid(c["lens"], S).view(B, S, 1, 1, 1)
    qkv2 = torch.where(pad, other, c["qkv"])
    assert not torch.equal(qkv2, c["qkv"])
    ld = _lens(c["lens"], dev)
    a = nat.attention_qkv_bf16(c["qkv"].to(dev), c["scale"], lens=ld)
    b = nat.attention_qkv_bf16(qkv2.to(dev), c["scale"], lens=ld)
    assert torch.equal(a, b)
    qa, qb = R.split_qkv(c["qkv"]), R.split_qkv(qkv2)
    a = nat.attention_bf16(*(t.to(dev) for t in qa), c["scale"], lens=ld)
    b = nat.attention_bf16(*(t.to(dev) for t in qb), c["scale"], lens=ld)
    assert torch.equal(a, b)


@pytest.mark.parametrize("ci", (0, 1, 2))
def test_full_lens_equals_unmasked(nat, dev, ci):
    """lens = S everywhere against lens=None: both within the bound of the
    unmasked reference, and bit-identical (the masked form evaluates the
    same expressions in the same order on valid columns)."""
    c = V.case(ci, "randn")
    B, H, S, D = c["shape"]
    ref, tol = R.attention_ref(c["q"], c["k"], c["v"], c["scale"])
    qkv = c["qkv"].to(dev)
    full = _lens([S] * B, dev)
    _poison((B, S, H * D), BF16, dev)
    plain = nat.attention_qkv_bf16(qkv, c["scale"])
    masked = nat.attention_qkv_bf16(qkv, c["scale"], lens=full)
    R.assert_within(_rows_to_heads(plain.cpu(), H), ref, tol, "lens=None")
    R.assert_within(_rows_to_heads(masked.cpu(), H), ref, tol, "lens=S")
    if not torch.equal(plain, masked):
        i = tuple(torch.nonzero(plain != masked)[0].tolist())
        raise AssertionError(
            f"S={S}: lens=S differs from lens=None at {i}: "
            f"{float(masked[i])!r} vs {float(plain[i])!r} "
            f"({int((plain != masked).sum())} elements)")
    q, k, v = (t.to(dev) for t in (c["q"], c["k"], c["v"]))
    assert torch.equal(nat.attention_bf16(q, k, v, c["scale"]),
                       nat.attention_bf16(q, k, v, c["scale"], lens=full))


def test_pad_variants_with_lens(nat, dev):
    lens = (17, 128)
    qkv, scale = V.varlen_inputs((2, 3, 128, 64), lens, "randn")
    ref, tol = V.varlen_ref(*R.split_qkv(qkv), scale, lens)
    qkv, ld = qkv.to(dev), _lens(lens, dev)
    base = nat.attention_qkv_bf16(qkv, scale, 8, lens=ld)
    _check(_rows_to_heads(base, 3), ref, tol, lens, "pad 8")
    for pad in (4, 16, 20):
        _poison(tuple(base.shape), BF16, dev)
        assert torch.equal(nat.attention_qkv_bf16(qkv, scale, pad, lens=ld),
                           base), f"pad {pad}"


def test_bad_lens_raises_before_launch(nat, dev):
    qkv, scale = V.varlen_inputs((2, 2, 128, 64), (5, 9), "randn")
    q, k, v = (t.to(dev) for t in R.split_qkv(qkv))
    qkv = qkv.to(dev)
    bad = {
        "host": torch.tensor([5, 9], dtype=torch.int32),
        "int64": torch.tensor([5, 9], dtype=torch.int64, device=dev),
        "wrong length": _lens([5, 9, 3], dev),
        "2-D": _lens([[5, 9]], dev),
    }
    for name, lens in bad.items():
        with pytest.raises(RuntimeError):
            nat.attention_bf16(q, k, v, scale, lens=lens)
        with pytest.raises(RuntimeError):
            nat.attention_qkv_bf16(qkv, scale, lens=lens)
        _still_clean(dev)


# ------------------------------------------------------------------ fallback
@pytest.mark.parametrize("shape,lens", [((2, 4, 64, 32), (37, 64)),
                                        ((1, 2, 96, 128), (50,)),
                                        ((2, 4, 64, 32), (0, 1))])
def test_unfused_fallback_with_lengths(dev, shape, lens):
    """Shapes the kernels reject: batched GEMM + our softmax kernel, masked.
    0.05 is the figure test_attention_other_shapes holds this path to."""
    from arkflow_amd.ops.nn import attention_bf16
    B, H, S, D = shape
    g = R._gen(9700 + S + D)
    q, k, v = (torch.randn(B, H, S, D, generator=g).to(BF16)
               for _ in range(3))
    pad = ~V.row_valid(lens, S).view(B, 1, S, 1)
    q, k, v = (torch.where(pad, torch.full_like(t, float("nan")), t)
               for t in (q, k, v))
    lt = torch.tensor(lens, dtype=torch.int32)
    ref = attention_bf16(q, k, v, D ** -0.5, lengths=lt)
    got = attention_bf16(q.to(dev), k.to(dev), v.to(dev), D ** -0.5,
                         lengths=lt.to(dev)).cpu()
    assert torch.isfinite(got.float()).all()
    assert (got.float() - ref.float()).abs().max().item() < 0.05
    V.assert_padded_rows_zero(got, lens, "fallback")


# ------------------------------------------------------------------- encoder
def test_bert_masked_gpu(dev):
    from arkflow_amd.models.bert import BertConfig, BertEncoder
    enc = BertEncoder(BertConfig(layers=2), dev, seed=5)
    g = R._gen(13)
    lens = torch.tensor([128, 77, 16, 1])
    ids = torch.randint(0, 30000, (4, 128), generator=g)
    ids2 = torch.where(V.row_valid(lens.tolist(), 128), ids,
                       torch.randint(0, 30000, (4, 128), generator=g))
    logits = enc.forward(ids, lens).cpu()
    assert logits.shape == (4, 2) and torch.isfinite(logits).all()
    cpu = BertEncoder(BertConfig(layers=2), torch.device("cpu"), seed=5)
    want = cpu.forward(ids, lens)
    assert (logits - want).abs().max() < 0.35, (logits, want)
    assert torch.equal(enc.forward(ids2, lens).cpu(), logits)

    # B = 3 then B = 5 share the one graph captured at B rounded up to 8
    l3 = enc.forward(ids[:3], lens[:3]).cpu()
    ids5 = torch.cat([ids[1:2], ids, ])[:5]
    lens5 = torch.cat([lens[1:2], lens])[:5]
    l5 = enc.forward(ids5, lens5).cpu()
    masked = [k for k in enc._graphs if k[0] == "masked"]
    assert masked == [("masked", 8, 128)] and len(enc._graphs) == 1
    assert torch.equal(l3, logits[:3])
    assert torch.equal(l5[0], logits[1]) and torch.equal(l5[1:], logits[:4])

    # the unmasked path is untouched by all of the above
    plain = enc.forward(ids).clone()
    assert set(enc._graphs) == {("masked", 8, 128), (4, 128)}
    fresh = BertEncoder(BertConfig(layers=2), dev, seed=5)
    assert torch.equal(plain, fresh.forward(ids))


# ----------------------------------------------------------------- processor
def test_processor_sequence_column_gpu(run, dev):
    from arkflow_amd.processors.inference import InferenceProcessor
    p = InferenceProcessor({"model": "bert_base", "layers": 2,
                            "device": str(dev), "sequence_column": "doc"})
    runs = ((3, 20), (8, 128), (5, 140), (9, 1), (2, 77))
    g = R._gen(21)
    docs, toks = [], []
    for doc, n in runs:
        docs += [doc] * n
        toks.append(torch.randint(1, 30000, (n,), generator=g))
    out = run(p.process(MessageBatch.from_dict(
        {"token": torch.cat(toks).tolist(), "doc": docs})))[0]
    assert out.num_rows == 5
    assert out.column("doc").to_pylist() == [3, 8, 5, 9, 2]
    ids = torch.zeros(5, 128, dtype=torch.int64)
    for r, t in enumerate(toks):
        ids[r, :min(len(t), 128)] = t[:128]
    want = p.model.forward(ids, torch.tensor([20, 128, 128, 1, 77]))
    got = torch.stack([out.column("logit_0").data,
                       out.column("logit_1").data], dim=1)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)
