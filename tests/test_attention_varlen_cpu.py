"""Variable-length attention on the CPU: the bound of tests/attn_varlen_ref.py
is met by a correct bf16-P emulation and catches a mask that is one key off,
and the CPU paths of ops.nn, BertEncoder and the inference processor keep
the contract (rows >= L exactly zero, padding never read)."""
import pytest
import torch

from arkflow_amd.batch import MessageBatch
from tests import attn_varlen_ref as V
from tests import nn_ref as R

TINY = dict(layers=1, hidden=64, heads=2, ff=128, seq_len=8)


# ------------------------------------------------------------------ the bound
@pytest.mark.parametrize("ci,family", V.CASE_PARAMS, ids=V.CASE_IDS)
def test_emulation_meets_bound(ci, family):
    c = V.case(ci, family)
    got = V.varlen_emulate(c["q"], c["k"], c["v"], c["scale"], c["lens"])
    assert torch.isfinite(got.float()).all()
    R.assert_within(got, c["ref"], c["tol"], f"emulate {family}")
    V.assert_padded_rows_zero(got, c["lens"], f"emulate {family}")


@pytest.mark.parametrize("ci", range(len(V.VARLEN_CASES)))
@pytest.mark.parametrize("family,delta", [("lastkey", -1), ("randn", +1),
                                          ("poison", +1)])
def test_bound_catches_off_by_one(ci, family, delta):
    """An emulation masking at L + delta violates the bound in EVERY sequence
    whose length actually changed, on the rows both lengths call valid
    (rows < min(L, L + delta)). L = 1 with delta = -1 leaves no such row: the
    short emulation attends to nothing and writes 0 to row 0, so there the
    sequence's own valid rows (< L) are compared."""
    c = V.case(ci, family)
    S = c["shape"][2]
    off = tuple(min(max(L + delta, 0), S) for L in c["lens"])
    got = V.varlen_emulate(c["q"], c["k"], c["v"], c["scale"], off)
    for b, (L, Lo) in enumerate(zip(c["lens"], off)):
        if Lo == L:
            continue
        n = min(L, Lo) or L
        assert R.exceeds(got[b, :, :n], c["ref"][b, :, :n],
                         c["tol"][b, :, :n]), \
            f"{family} S={S}: L={L} masked at {Lo} stays within the bound"


# ------------------------------------------------------------- ops.nn on CPU
@pytest.mark.parametrize("ci,family", V.CASE_PARAMS, ids=V.CASE_IDS)
def test_ops_cpu_path(ci, family):
    from arkflow_amd.ops import nn as opsnn
    c = V.case(ci, family)
    lens = torch.tensor(c["lens"], dtype=torch.int32)
    got = opsnn.attention_bf16(c["q"], c["k"], c["v"], c["scale"],
                               lengths=lens)
    R.assert_within(got, c["ref"], c["tol"], f"ops cpu {family}")
    V.assert_padded_rows_zero(got, c["lens"], f"ops cpu {family}")
    got2 = opsnn.attention_qkv_bf16(c["qkv"], c["scale"], lengths=lens)
    assert torch.equal(got2, R.heads_to_rows(got))


def test_ops_cpu_zero_length_and_none():
    from arkflow_amd.ops import nn as opsnn
    lens = (17, 0, 128)
    qkv, scale = V.varlen_inputs((3, 2, 128, 64), lens, "poison")
    q, k, v = R.split_qkv(qkv)
    ref, tol = V.varlen_ref(q, k, v, scale, lens)
    got = opsnn.attention_bf16(q, k, v, scale,
                               lengths=torch.tensor(lens, dtype=torch.int64))
    R.assert_within(got, ref, tol, "L == 0 neighbours")
    V.assert_padded_rows_zero(got, lens, "L == 0")
    assert not bool(got[1].view(torch.int16).any())
    # lengths=None is the call that existed before
    c = V.case(1, "randn")
    old = opsnn.attention_bf16(c["q"], c["k"], c["v"], c["scale"])
    assert torch.equal(
        old, opsnn.attention_bf16(c["q"], c["k"], c["v"], c["scale"],
                                  lengths=None))
    p = torch.softmax(c["q"].float() @ c["k"].float().transpose(-1, -2) *
                      c["scale"], dim=-1)
    assert torch.equal(old, (p @ c["v"].float()).to(torch.bfloat16))
    assert torch.equal(
        opsnn.attention_qkv_bf16(c["qkv"], c["scale"]),
        opsnn.attention_qkv_bf16(c["qkv"], c["scale"], lengths=None))
    assert torch.equal(opsnn.attention_qkv_bf16(c["qkv"], c["scale"]),
                       R.heads_to_rows(old))


# ----------------------------------------------------------------- encoder
def test_bert_cpu_ignores_padding():
    from arkflow_amd.models.bert import BertConfig, BertEncoder
    enc = BertEncoder(BertConfig(**TINY), torch.device("cpu"), seed=3)
    g = R._gen(77)
    lens = torch.tensor([8, 5, 1, 3])
    a = torch.randint(1, 30000, (4, 8), generator=g)
    b = torch.where(V.row_valid(lens.tolist(), 8), a,
                    torch.randint(1, 30000, (4, 8), generator=g))
    assert not torch.equal(a[1:], b[1:])
    la, lb = enc.forward(a, lens), enc.forward(b, lens)
    assert la.shape == (4, 2) and torch.isfinite(la).all()
    assert torch.equal(la, lb)
    ua, ub = enc.forward(a), enc.forward(b)
    assert torch.equal(ua[0], ub[0])  # row 0 is full length: same ids
    for r in (1, 2, 3):
        assert not torch.equal(ua[r], ub[r])
    # a zero-length row: finite logits
    assert torch.isfinite(enc.forward(a, torch.tensor([8, 0, 1, 3]))).all()


# --------------------------------------------------------------- processor
def _tiny_proc(device="cpu", **extra):
    from arkflow_amd.processors.inference import InferenceProcessor
    return InferenceProcessor(dict(
        {"model": "bert_base", "layers": 1, "hidden_size": 64, "heads": 2,
         "ff": 128, "seq_len": 8, "device": device}, **extra))


def test_processor_sequence_column_cpu(run):
    runs = ((7, 3), (9, 8), (4, 11), (12, 1))  # (doc id, token count)
    docs, toks = [], []
    for doc, n in runs:
        docs += [doc] * n
        toks += [100 * doc + i for i in range(n)]
    p = _tiny_proc(sequence_column="doc")
    out = run(p.process(MessageBatch.from_dict({"token": toks,
                                                "doc": docs})))[0]
    assert out.num_rows == 4
    assert out.column("doc").to_pylist() == [7, 9, 4, 12]
    ids = torch.zeros(4, 8, dtype=torch.int64)
    for r, (doc, n) in enumerate(runs):
        m = min(n, 8)  # the 11-token run keeps its first 8
        ids[r, :m] = torch.tensor([100 * doc + i for i in range(m)])
    want = p.model.forward(ids, torch.tensor([3, 8, 8, 1], dtype=torch.int32))
    for i in range(2):
        assert torch.equal(out.column(f"logit_{i}").data, want[:, i])
    assert out.column("score").to_pylist() == \
        torch.argmax(want, dim=1).tolist()


def test_processor_without_sequence_column_unchanged(run):
    p = _tiny_proc()
    out = run(p.process(MessageBatch.from_dict(
        {"token": list(range(16)), "doc": [0] * 5 + [1] * 11})))[0]
    assert out.num_rows == 2  # 16 tokens / seq_len 8, the doc column ignored
    assert "logit_0" in out.columns and "score" in out.columns
    want = p.model.forward(torch.arange(16).reshape(2, 8))
    assert torch.equal(out.column("logit_0").data, want[:, 0])
