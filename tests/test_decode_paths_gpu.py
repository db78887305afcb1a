"""GPU tests of csrc/json_decode.hip and csrc/proto_decode.hip, every dispatch
of each. Whole columns are compared, exactly, against json.loads (with the
absent / wrong-type rule of JsonToArrowProcessor._decode_host_schema) and
against proto_wire.decode_message. The batch's own sizes select the kernel,
as in production; each test asserts the size precondition it relies on."""
import asyncio
import functools
import json
import struct

import numpy as np
import pytest
import torch

from arkflow_amd import ops
from arkflow_amd.batch import Column, MessageBatch
from arkflow_amd.errors import ProcessError
from arkflow_amd.processors.json_proc import JsonToArrowProcessor
from arkflow_amd.processors.proto_wire import (
    ProtoSchema, _write_varint, decode_message, encode_message)
from arkflow_amd.processors.protobuf_proc import ProtobufToArrowProcessor
from tests import test_decode_schema_limits as L

pytestmark = pytest.mark.gpu

LDS_BYTES = 48 * 1024       # document cache of the thread-per-doc parse
TILE = 128                  # documents per tile of the thread-per-doc parse
WAVE_PARSE_MEAN = 2048      # mean document bytes that select the wave parse
WAVE_COPY_MEAN = 32         # mean string bytes that select the wave copy
WAVE_GRID_DOCS = 8192 * 4   # documents one pass of either wave grid covers
PROTO_GRID_ROWS = 2048 * 256


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def nat():
    return ops.require_native()  # GPU present ⇒ extension must load


def _run(coro):
    return asyncio.new_event_loop().run_until_complete(coro)


# ======================================================================== JSON
J_SCHEMA = {"id": "int", "s": "str", "x": "float", "ok": "bool",
            "u.id": "int", "u.name": "str"}
ESCAPES = ['\\"', "\\\\", "\\u00e9", "\\u4e2d", "\\ud83d\\ude00"]


def _corpus():
    """Valid JSON documents, as text. `s` bodies are written by hand so that
    each escape sits where it is meant to, counted in raw bytes from the
    opening quote."""
    docs = []

    def doc(s_body=None, **kw):
        parts = [f'"id": {len(docs)}']
        parts += [f'"{k}": {v}' for k, v in kw.items()]
        if s_body is not None:
            parts.append(f'"s": "{s_body}"')
        parts.append(f'"x": {len(docs) * 0.25}')
        docs.append("{" + ", ".join(parts) + "}")

    for n in (0, 1, 7, 8, 9, 15, 16, 63, 64, 65, 511, 512, 513, 1025):
        doc("x" * n, ok="true")
    for esc in ESCAPES:
        for bound in (8, 512):
            # starts on, ends on, straddles a multiple of `bound`
            for lead in (bound, -len(esc) % bound, bound - len(esc) // 2):
                doc("a" * lead + esc + "bcd")
        doc("final" + esc)  # an escape as the last character
    doc("a\\n\\t\\r\\b\\f\\/z")
    # skipped values holding quotes and escapes, ahead of the wanted fields
    doc("after a string", skip='"a \\" b \\\\ c \\u00e9 } ] { \\\\"')
    doc("after an object",
        skip='{"k": "q\\"}", "m": {"z": ["]", "\\\\"]}, "s": "inner"}')
    doc("after an array", skip='["a\\"", "]", "}", "\\\\", "\\u4e2d"]')
    # null, wrong types, missing fields
    docs.append('{"id": 900, "s": null, "x": null, "ok": null}')
    docs.append('{"id": 901, "s": 5, "x": 1.5, "ok": false}')
    docs.append('{"id": "902", "s": "kept", "x": "str", "ok": true}')
    docs.append('{"id": 903}')
    docs.append('{ }')
    # one level of nesting; "v" and "w" hold the same keys but are no parents
    docs.append('{"v": {"id": 99, "name": "wrong"}, "id": 904, '
                '"u": {"id": 3, "name": "nm \\" \\u00e9", "s": "inner"}, '
                '"w": {"u": {"id": 98}}, "s": "outer", "x": -2.5e10}')
    docs.append('{"u": {"name": "only"}, "x": 123456.789, "id": 905}')
    docs.append('{"u": 7, "x": 1e-3, "id": -906}')
    return [d.encode() for d in docs]


CORPUS = _corpus()


def corpus_rows(n):
    return [CORPUS[i % len(CORPUS)] for i in range(n)]


@functools.lru_cache(maxsize=None)
def j_extract(payload):
    """Per schema field the value json.loads finds, None where the host rule
    calls it absent."""
    doc = json.loads(payload)
    row = []
    for name, t in J_SCHEMA.items():
        cur = doc
        for part in name.split("."):
            cur = cur.get(part) if isinstance(cur, dict) else None
            if cur is None:
                break
        if t == "str":
            ok = isinstance(cur, str)
        else:
            ok = not (cur is None or isinstance(cur, (str, dict, list)))
        row.append(cur if ok else None)
    return tuple(row)


def j_decode(payloads, dev, column=None):
    col = column if column is not None else \
        MessageBatch.from_binary(payloads).to(dev).column("__value__")
    out = _run(JsonToArrowProcessor({"schema": J_SCHEMA}, None).process(
        MessageBatch({"__value__": col})))[0]
    assert all(c.data.is_cuda for c in out.columns.values())
    return out


def assert_validity(col, valid, name):
    if all(valid):
        assert col.validity is None or bool(col.validity.all()), name
    else:
        assert col.validity is not None, name
        assert col.validity.cpu().tolist() == valid, name


def assert_binary(col, want, name):
    """Exact data and offsets, compared whole."""
    offs = col.offsets.cpu().tolist()
    assert offs[0] == 0 and len(offs) == len(want) + 1, name
    assert [b - a for a, b in zip(offs, offs[1:])] == \
        [len(w) for w in want], name
    assert bytes(col.data.cpu().numpy().tobytes()) == b"".join(want), name


def j_check(out, payloads):
    """Every column of `out` against the reference for `payloads`."""
    rows = [j_extract(p) for p in payloads]
    for f, (name, t) in enumerate(J_SCHEMA.items()):
        vals = [r[f] for r in rows]
        col = out.column(name)
        assert len(col) == len(payloads)
        assert_validity(col, [v is not None for v in vals], name)
        if t == "str":
            assert_binary(col, [(v or "").encode() for v in vals], name)
        elif t == "float":
            want = torch.tensor([float(v or 0.0) for v in vals],
                                dtype=torch.float64)
            got = col.data.cpu()
            print(name, "max |got - want|", (got - want).abs().max().item())
            assert bool(((got - want).abs() <= torch.clamp(
                1e-6 * want.abs(), min=1e-6)).all()), name
        elif t == "bool":
            assert col.data.cpu().tolist() == [bool(v) for v in vals], name
        else:
            assert col.data.dtype == torch.int64
            assert col.data.cpu().tolist() == [int(v or 0) for v in vals], name


def tile_bytes(payloads):
    return [sum(map(len, payloads[t:t + TILE]))
            for t in range(0, len(payloads), TILE)]


def mean_len(payloads):
    return sum(map(len, payloads)) // len(payloads)  # the binding's division


def mean_s(payloads):
    return sum(len((j_extract(p)[1] or "").encode())
               for p in payloads) // len(payloads)


@pytest.mark.parametrize("n", [1, 127, 128, 129])
def test_json_corpus_in_every_dispatch(dev, n):
    rows = corpus_rows(n)
    pad = "z" * 50_000
    batches = {}
    # (a) thread parse, every tile from the LDS cache
    batches["lds"] = (0, rows)
    assert max(tile_bytes(rows)) <= LDS_BYTES
    assert mean_len(rows) < WAVE_PARSE_MEAN
    # (b) thread parse: the first tile is over the cache and parses from
    # global memory, the later ones from LDS in the same launch
    b = [f'{{"id": -1, "pad": "{pad}", "s": "filler"}}'.encode()] + rows + \
        corpus_rows(TILE)
    tb = tile_bytes(b)
    assert tb[0] > LDS_BYTES and len(tb) >= 2 and max(tb[1:]) <= LDS_BYTES
    assert mean_len(b) < WAVE_PARSE_MEAN
    batches["global"] = (1, b)
    # (c) wave parse: an ignored key long enough to lift the batch mean
    big = "y" * (WAVE_PARSE_MEAN * (n + 2))
    c = [f'{{"id": -2, "pad": "{big}", "s": "filler"}}'.encode()] + rows
    assert mean_len(c) >= WAVE_PARSE_MEAN
    batches["wave"] = (1, c)
    # (d) mean extracted string on both sides of the copy threshold
    hi = rows + [f'{{"id": -3, "s": "{"w" * (64 * (n + 1))}"}}'.encode()]
    assert mean_s(hi) >= WAVE_COPY_MEAN and mean_len(hi) < WAVE_PARSE_MEAN
    batches["wave copy"] = (0, hi)
    lo = rows + [b'{"id": -4, "s": ""}'] * (1 + sum(
        len((j_extract(p)[1] or "").encode()) for p in rows) // 16)
    assert 0 <= mean_s(lo) < WAVE_COPY_MEAN
    batches["thread copy"] = (0, lo)

    x_bits = {}
    for label, (first, payloads) in batches.items():
        out = j_decode(payloads, dev)
        j_check(out, payloads)
        # the corpus rows of every dispatch, bit for bit (one parse_number)
        x_bits[label] = out.column("x").data[first:first + n].view(
            torch.int64).cpu().tolist()
    for label, bits in x_bits.items():
        assert bits == x_bits["lds"], label


def test_json_wave_copy_past_the_capped_grid(dev):
    n = WAVE_GRID_DOCS + 5  # the wave stride loop of the copy runs
    tail = "p" * 31
    payloads = [f'{{"id": {i}, "s": "{i:08d}-{tail}"}}'.encode()
                for i in range(n)]
    assert mean_len(payloads) < WAVE_PARSE_MEAN
    out = j_decode(payloads, dev)
    assert 40 >= WAVE_COPY_MEAN  # every string is 8 + 1 + 31 bytes
    assert out.column("id").data.cpu().tolist() == list(range(n))
    assert out.column("id").validity is None
    assert_binary(out.column("s"),
                  [f"{i:08d}-{tail}".encode() for i in range(n)], "s")
    assert out.column("s").validity is None
    assert not bool(out.column("x").validity.any())


def test_json_wave_parse_past_the_capped_grid(dev):
    """Documents of ~2.1 KB that differ in their id alone; what to expect is
    arithmetic, no per-document parse."""
    n = WAVE_GRID_DOCS + 3  # the wave stride loop of the parse runs
    body = ("lorem ipsum dolor sit amet " * 78)[:2100]
    head, tail = b'{"id": ', f', "s": "{body}", "x": 0.5}}'.encode()
    width = len(head) + 8 + len(tail)
    assert width >= WAVE_PARSE_MEAN
    ids = np.arange(n, dtype=np.int64) + 10_000_000  # always 8 digits
    data = np.empty((n, width), dtype=np.uint8)
    data[:, :len(head)] = np.frombuffer(head, dtype=np.uint8)
    data[:, len(head) + 8:] = np.frombuffer(tail, dtype=np.uint8)
    for k in range(8):
        data[:, len(head) + k] = ord("0") + (ids // 10 ** (7 - k)) % 10
    assert json.loads(data[n - 1].tobytes())["id"] == ids[-1]
    col = Column("binary", torch.from_numpy(data.reshape(-1)).to(dev),
                 (torch.arange(n + 1, dtype=torch.int64) * width).to(dev))
    out = j_decode(None, dev, column=col)
    assert torch.equal(out.column("id").data.cpu(), torch.from_numpy(ids))
    assert torch.equal(out.column("x").data.cpu(),
                       torch.full((n,), 0.5, dtype=torch.float64))
    s = out.column("s")
    assert torch.equal(s.offsets.cpu(),
                       torch.arange(n + 1, dtype=torch.int64) * len(body))
    assert torch.equal(
        s.data.cpu().reshape(n, len(body)),
        torch.from_numpy(np.frombuffer(body.encode(), dtype=np.uint8).copy()
                         ).expand(n, len(body)))
    for name in ("id", "x", "s"):
        assert out.column(name).validity is None
    assert not bool(out.column("ok").validity.any())


def test_json_17_fields_on_a_device_batch(dev, nat):
    schema, docs = L.json_rows(17, 300)
    batch = MessageBatch.from_binary(
        [json.dumps(d).encode() for d in docs]).to(dev)
    out = _run(JsonToArrowProcessor({"schema": schema},
                                    None).process(batch))[0]
    assert len(out.columns) == 17
    assert all(c.data.is_cuda for c in out.columns.values())
    L.check_json_columns(out, schema, docs)
    col = batch.column("__value__")
    with pytest.raises(RuntimeError, match="at most 16 fields"):
        nat.json_decode(col.data, col.offsets, list(schema), [0] * 17,
                        list(range(17)), 17, 0, 0)
    with pytest.raises(RuntimeError, match="too many nested parents"):
        nat.json_decode(col.data, col.offsets, [f"p{i}.x" for i in range(9)],
                        [0] * 9, list(range(9)), 9, 0, 0)


# ==================================================================== protobuf
P_SRC = """
message All {
  int64 a = 1; uint64 ub = 2; int32 c = 3; sint32 z32 = 4; sint64 z64 = 5;
  fixed32 f32 = 6; fixed64 f64 = 7; sfixed32 s32 = 8; sfixed64 s64 = 9;
  double d = 10; float f = 11; bool ok = 12; string s = 13; bytes b = 14;
}
"""
P_SCHEMA = ProtoSchema.parse(P_SRC)
P_WIDE = ProtoSchema.parse(P_SRC.replace(
    "}", "int64 x0 = 20; fixed64 x1 = 21; string x2 = 22; fixed32 x5 = 23; }"))
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
NAN64, NAN32 = 0x7FF8000000000000, 0x7FC00000


def field(no, wt, payload):
    return _write_varint((no << 3) | wt) + payload


def _messages():
    msgs = []
    # varints of every encoded length, 1 to 10 bytes
    edges = [0, 127, -1]
    for k in range(1, 10):
        edges += [(1 << (7 * k)) - 1, 1 << (7 * k)]
    edges.append(I64_MAX)
    for v in edges:
        msgs.append(encode_message(
            {"a": v, "ub": max(v, 0), "c": max(min(v, I32_MAX), -1),
             "ok": v % 2 == 1}, P_SCHEMA))
    assert sorted({len(_write_varint(v)) for v in edges}) == list(range(1, 11))
    for z32, z64 in [(I32_MIN, I64_MIN), (I32_MAX, I64_MAX), (-1, -1), (1, 1)]:
        msgs.append(encode_message({"z32": z32, "z64": z64}, P_SCHEMA))
    for f32, f64, s32, s64 in [(1, 1, -1, -1), ((1 << 32) - 1, I64_MAX,
                                                I32_MIN, I64_MIN),
                               (1 << 31, 1 << 62, I32_MAX, I64_MAX)]:
        msgs.append(encode_message(
            {"f32": f32, "f64": f64, "s32": s32, "s64": s64}, P_SCHEMA))
    # float specials, written by bit pattern
    for d64, f32 in [(NAN64, NAN32), (0x7FF0 << 48, 0x7F80 << 16),
                     (0xFFF0 << 48, 0xFF80 << 16), (1 << 63, 1 << 31),
                     (0x3FF8 << 48, 0x3FC0 << 16)]:
        msgs.append(field(10, 1, struct.pack("<Q", d64)) +
                    field(11, 5, struct.pack("<I", f32)))
    for n in (0, 1, 127, 128, 300):
        msgs.append(field(13, 2, _write_varint(n) + b"s" * n) +
                    field(14, 2, _write_varint(n) + bytes(range(256)) [:n]
                          + b"\xff" * max(0, n - 256)))
    full = {"a": -5, "ub": 6, "c": 7, "z32": -8, "z64": 9, "f32": 10,
            "f64": 11, "s32": -12, "s64": -13, "d": 1.5, "f": -0.25,
            "ok": True, "s": "text é", "b": b"\x00\x01"}
    one = encode_message(full, P_SCHEMA)
    msgs.append(one)
    # fields out of order: the same fields, last to first
    parts = [encode_message({k: v}, P_SCHEMA) for k, v in full.items()]
    assert b"".join(parts) == one
    msgs.append(b"".join(reversed(parts)))
    # a scalar field given three times: the last one counts
    msgs.append(field(1, 0, _write_varint(1)) + field(10, 1, struct.pack(
        "<d", 1.0)) + field(1, 0, _write_varint(2)) + field(10, 1, struct.pack(
            "<d", 2.0)) + field(1, 0, _write_varint(3)))
    # unknown fields of wire types 0, 1, 2 and 5 between known ones
    msgs.append(encode_message(dict(full, x0=77, x1=88, x2="skip me", x5=99),
                               P_WIDE))
    msgs.append(encode_message({"x0": 1, "x1": 2, "x2": "q", "x5": 3}, P_WIDE))
    msgs.append(b"")  # every field missing
    return msgs


P_MSGS = _messages()


def _bits64(v):
    return struct.unpack("<q", struct.pack("<d", v))[0]


def _wrap(v):
    """The int64 that holds the same 64 bits as the unsigned v."""
    return v - (1 << 64) if v > I64_MAX else v


@functools.lru_cache(maxsize=None)
def p_reference():
    """decode_message over P_MSGS: per field a list of int64-representable
    values (floats as their float64 bit pattern), or of bytes."""
    rows = [decode_message(m, P_SCHEMA) for m in P_MSGS]
    ref = {}
    for name, (_, t) in P_SCHEMA.by_name.items():
        vals = [r[name] for r in rows]
        if t in ("string", "bytes"):
            ref[name] = [v.encode() if isinstance(v, str) else v for v in vals]
        elif t in ("double", "float"):
            ref[name] = [_bits64(v) for v in vals]
        else:
            ref[name] = [_wrap(int(v)) for v in vals]
    return ref


def p_decode(payloads, dev, schema_src=P_SRC):
    out = _run(ProtobufToArrowProcessor({"proto": schema_src}, None).process(
        MessageBatch.from_binary(payloads).to(dev)))[0]
    assert all(c.data.is_cuda for c in out.columns.values())
    return out


def p_check(out, n):
    """Rows i of `out` are P_MSGS[i % len(P_MSGS)]."""
    ref = p_reference()
    idx = torch.arange(n) % len(P_MSGS)
    assert list(out.columns) == [P_SCHEMA.fields[no][0]
                                 for no in sorted(P_SCHEMA.fields)]
    for name, (_, t) in P_SCHEMA.by_name.items():
        col = out.column(name)
        if t in ("string", "bytes"):
            lens = torch.tensor([len(v) for v in ref[name]])[idx]
            want_offs = torch.cat([torch.zeros(1, dtype=torch.int64),
                                   lens.cumsum(0)])
            assert torch.equal(col.offsets.cpu(), want_offs), name
            want = (b"".join(ref[name]) * (n // len(P_MSGS)) +
                    b"".join(ref[name][:n % len(P_MSGS)]))
            assert bytes(col.data.cpu().numpy().tobytes()) == want, name
            continue
        want = torch.tensor(ref[name], dtype=torch.int64)[idx]
        got = col.data.cpu()
        if t in ("double", "float"):
            assert got.dtype == torch.float64
            got = got.view(torch.int64)
        elif t == "bool":
            assert got.dtype == torch.bool
            got = got.to(torch.int64)
        assert torch.equal(got, want), name


@pytest.mark.parametrize("n", [1, 255, 256, 257, PROTO_GRID_ROWS + 7])
def test_proto_decode_is_decode_message(dev, n):
    assert len(P_MSGS) < 255  # the small sizes hold every message
    p_check(p_decode([P_MSGS[i % len(P_MSGS)] for i in range(n)], dev), n)


MALFORMED = {
    "truncated fixed32": field(6, 5, b"\x01\x02"),
    "truncated fixed64": field(7, 1, b"\x01\x02\x03\x04\x05\x06\x07"),
    "length past the end": field(13, 2, _write_varint(10) + b"abc"),
    "wire type 3": field(1, 3, b""),
    "wire type 4": field(1, 4, b""),
    "wire type 6": field(1, 6, b"\x00"),
    "wire type 7": field(1, 7, b"\x00"),
    "11-byte tag": b"\x88" + b"\x80" * 9 + b"\x01" + b"\x05",
    "11-byte value": field(1, 0, b"\x80" * 10 + b"\x01"),
    "11-byte length": field(13, 2, b"\x80" * 10 + b"\x01" + b"abc"),
    "length 2^63": field(13, 2, b"\x80" * 9 + b"\x01" + b"abc"),
}


@pytest.mark.parametrize("case", list(MALFORMED))
def test_proto_malformed_message_is_an_error(dev, case):
    bad = MALFORMED[case]
    good = [m for m in P_MSGS[:6]]
    payloads = good[:3] + [bad] + good[3:]
    with pytest.raises(ValueError):  # the host codec, on the same bytes
        decode_message(bad, P_SCHEMA)
    with pytest.raises(ValueError):
        _run(ProtobufToArrowProcessor({"proto": P_SRC}, None).process(
            MessageBatch.from_binary(payloads)))
    with pytest.raises(ProcessError):
        p_decode(payloads, dev)
    p_decode(good, dev)  # the batch without it decodes


def test_proto_17_fields_on_a_device_batch(dev, nat):
    schema, rows = L.proto_rows(17, 300)
    out = p_decode([encode_message(r, schema) for r in rows], dev,
                   L.proto_src(17))
    assert len(out.columns) == 17
    L.check_proto_columns(out, schema, rows)
    data = torch.zeros(1, dtype=torch.uint8, device=dev)
    offs = torch.tensor([0, 0], device=dev)
    with pytest.raises(RuntimeError, match="at most 16 fields"):
        nat.proto_decode(data, offs, list(range(1, 18)), [0] * 17, [0] * 17,
                         list(range(17)), 17, 0, 0)
