"""GPU tests of csrc/proto_encode.hip. Every comparison is exact byte equality
against proto_wire.encode_message applied row by row to the same values on
the host; the shapes are the smallest at which each piece can go wrong."""
import asyncio
import struct

import pytest
import torch

from arkflow_amd import ops
from arkflow_amd.batch import Column, MessageBatch
from arkflow_amd.codecs.protobuf_codec import ProtobufCodec
from arkflow_amd.codecs.schema_registry import SchemaRegistryCodec
from arkflow_amd.errors import ProcessError
from arkflow_amd.processors.proto_wire import ProtoSchema, encode_message
from arkflow_amd.processors.protobuf_proc import (
    ArrowToProtobufProcessor, build_gpu_spec, encode_device)

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
F32_MAX = 3.4028234663852886e38
GRID_ROWS = 2048 * 256   # rows one pass of the size/write grids covers
COPY_ROWS = 2048 * 4     # rows (waves) one pass of the copy grid covers


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def nat():
    return ops.require_native()  # GPU present ⇒ extension must load


def _run(coro):
    return asyncio.new_event_loop().run_until_complete(coro)


def _want(batch, schema, prefix=b""):
    """encode_message over the rows of a host batch."""
    out = []
    for row in batch.to_rows():
        clean = {}
        for name, (_, t) in schema.by_name.items():
            v = row.get(name)
            if isinstance(v, bytes) and t == "string":
                v = v.decode("utf-8")
            clean[name] = v
        out.append(prefix + encode_message(clean, schema))
    return out


def _assert_column_is(col, want):
    """Exact bytes and offsets; compared whole, so a stray byte anywhere in
    the data shows."""
    offs = col.offsets.cpu().tolist()
    lens = [len(w) for w in want]
    assert len(offs) == len(want) + 1 and offs[0] == 0
    assert [b - a for a, b in zip(offs, offs[1:])] == lens
    assert bytes(col.data.cpu().numpy().tobytes()) == b"".join(want)


def _check(batch, schema, dev, prefix=b""):
    """Device encode of the host batch's device copy == host reference."""
    on_dev = batch.to(dev)
    assert encode_device(schema, on_dev.columns) is not None
    got = ops.proto_encode(on_dev, schema, prefix)
    assert got.kind == "binary" and got.data.is_cuda and got.offsets.is_cuda
    want = _want(batch, schema, prefix)
    _assert_column_is(got, want)
    return got, want


def _num(values, dtype=torch.int64, valid=None):
    return Column("numeric", torch.tensor(values, dtype=dtype),
                  validity=None if valid is None else torch.tensor(valid))


# ------------------------------------------------------------------ row counts
MIXED = ProtoSchema.parse(
    "message R { int64 a = 1; double b = 2; string s = 3; sint32 z = 4; }")


def _mixed_batch(n):
    return MessageBatch({
        "a": _num([(i * 37) % 301 - 3 for i in range(n)]),
        "b": _num([(i % 5) * 0.25 for i in range(n)], torch.float64),
        "s": Column.from_bytes([b"r%d" % i * (i % 4) for i in range(n)]),
        "z": _num([(-1) ** i * (i % 130) for i in range(n)]),
    })


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257])
def test_row_counts(dev, n):
    got, _ = _check(_mixed_batch(n), MIXED, dev)
    assert len(got) == n


def test_rows_past_the_capped_grid(dev):
    n = GRID_ROWS + 5  # the stride loop of the size and write kernels runs
    schema = ProtoSchema.parse("message G { int64 a = 1; double b = 2; }")
    a = torch.arange(n, dtype=torch.int64) * 2654435761 % 70001 - 7
    b = (torch.arange(n, dtype=torch.float64) % 11) * 0.5
    _check(MessageBatch({"a": Column("numeric", a),
                         "b": Column("numeric", b)}), schema, dev)


def test_rows_past_the_capped_copy_grid(dev):
    n = COPY_ROWS + 3  # the wave stride loop of the payload copy runs
    schema = ProtoSchema.parse("message C { string s = 1; bytes t = 2; }")
    _check(MessageBatch({
        "s": Column.from_bytes([b"%05d" % i * (i % 3) for i in range(n)]),
        "t": Column.from_bytes([bytes([i % 256]) * (i % 5)
                                for i in range(n)])}), schema, dev)


# ------------------------------------------------------------ varint boundaries
def _varint_values():
    vals = [0, -1, I64_MIN, I64_MAX, 1, -2]
    for k in range(1, 10):
        # 2^63 itself exists in an int64 column only as INT64_MIN (above),
        # which is also how the decoder stores it
        vals += [v for v in ((1 << 7 * k) - 1, 1 << 7 * k) if v <= I64_MAX]
        # the values whose zigzag form is 2^(7k) - 1 and 2^(7k)
        vals += [-(1 << 7 * k - 1), 1 << 7 * k - 1]
    return vals


def test_varint_boundaries(dev):
    types = ["int32", "int64", "uint32", "uint64", "bool", "sint32", "sint64"]
    schema = ProtoSchema.parse("message V { " + " ".join(
        f"{t} c{i} = {i + 1};" for i, t in enumerate(types)) + " }")
    vals = _varint_values()
    batch = MessageBatch({f"c{i}": _num(vals) for i in range(len(types))})
    _, want = _check(batch, schema, dev)
    assert want[0] == b""                      # 0 is elided in every field
    assert len(want[1]) == len(types) * 11 - 2 * 9  # -1: 10 bytes; zigzag 1
    assert max(len(w) for w in want) == len(types) * 11


def test_field_numbers_out_of_order(dev):
    schema = ProtoSchema.parse("""
        message F {
          sfixed32 e = 2048;
          int64 a = 1;
          string f = 536870911;
          double c = 16;
          sint64 b = 15;
          bytes d = 2047;
        }""")
    batch = MessageBatch({
        "a": _num([5, 0, -9]), "b": _num([-3, 4, 0]),
        "c": _num([1.5, 0.0, -2.5], torch.float64),
        "d": Column.from_bytes([b"\x00\xff", b"", b"dd"]),
        "e": _num([-7, 8, 0]), "f": Column.from_bytes(["é", "ff", ""])})
    _, want = _check(batch, schema, dev)
    # tags of 1, 1, 2, 2, 3 and 5 bytes, ascending
    assert want[0] == (b"\x08\x05" b"\x78\x05" b"\x81\x01" +
                       struct.pack("<d", 1.5) + b"\xfa\x7f\x02\x00\xff" +
                       b"\x85\x80\x01" + struct.pack("<i", -7) +
                       b"\xfa\xff\xff\xff\x0f\x02\xc3\xa9")


# ----------------------------------------------------------- every scalar type
ALL_TYPES = ["double", "float", "int32", "int64", "uint32", "uint64",
             "sint32", "sint64", "bool", "fixed64", "sfixed64", "fixed32",
             "sfixed32", "string", "bytes"]
ALL_SCHEMA = ProtoSchema.parse("message A { " + " ".join(
    f"{t} c_{t} = {i + 1};" for i, t in enumerate(ALL_TYPES)) + " }")

FLOATS = [0.0, -0.0, torch.nan, float("inf"), float("-inf"), 5e-324,
          -2.2250738585072014e-308, 1e-45, -1e-40, 1.1754943508222875e-38,
          1e-50, F32_MAX, -F32_MAX, 3.4028235e38, 1.0, -2.5, 0.1, 16777217.0]


def _all_types_batch(fixed64_max=I64_MAX):
    n = len(FLOATS)
    ints = [0, 1, -1, 127, 128, -128, 300, I64_MAX, I64_MIN, 1 << 31,
            -(1 << 31), (1 << 32) - 1, 1 << 32, 16383, 16384, -16384, 7, 0]
    u32 = [0, 1, (1 << 32) - 1, 1 << 31, 255, 256, 65535, 65536] + [9] * 10
    i32 = [0, -1, (1 << 31) - 1, -(1 << 31), 255, -256, 1, 2] + [-9] * 10
    u64 = [0, 1, fixed64_max, 1 << 62, 255, 256] + [3] * 12
    cols = {}
    for t in ALL_TYPES:
        name = f"c_{t}"
        if t in ("double", "float"):
            cols[name] = _num(FLOATS, torch.float64)
        elif t == "bool":
            cols[name] = _num([i % 3 == 0 for i in range(n)], torch.bool)
        elif t == "fixed32":
            cols[name] = _num(u32)
        elif t == "sfixed32":
            cols[name] = _num(i32)
        elif t == "fixed64":
            cols[name] = _num(u64)
        elif t == "string":
            cols[name] = Column.from_bytes(
                ["", "a", "žluťoučký kůň", "日本語", "🙂🙃"] + ["s"] * (n - 5))
        elif t == "bytes":
            cols[name] = Column.from_bytes(
                [b"", b"\x00", b"\xff", b"\x00\xff\x00\xff", bytes(range(256))]
                + [b"\xfe"] * (n - 5))
        else:
            cols[name] = _num(ints)
    return MessageBatch(cols)


def test_every_scalar_type(dev):
    _, want = _check(_all_types_batch(), ALL_SCHEMA, dev)
    # NaN is written, never elided, and narrows to the float32 quiet NaN
    assert struct.pack("<f", float("nan")) in want[2]
    assert b"\x15" + struct.pack("<f", F32_MAX) in want[13]


# ------------------------------------------------------------ strings and bytes
STR_SCHEMA = ProtoSchema.parse(
    "message S { string s = 1; bytes b = 2; string t = 3; }")
STR_LENS = [0, 1, 63, 64, 65, 127, 128, 129, 16383, 16384]


def test_string_length_boundaries(dev):
    s = [("x" * ln).encode() for ln in STR_LENS]
    b = [bytes([0x00, 0xFF]) * (ln // 2) + b"\x00" * (ln % 2)
         for ln in reversed(STR_LENS)]
    t = [("é" * (ln // 2) + "a" * (ln % 2)).encode() for ln in STR_LENS]
    assert [len(v) for v in t] == STR_LENS
    _check(MessageBatch({"s": Column.from_bytes(s), "b": Column.from_bytes(b),
                         "t": Column.from_bytes(t)}), STR_SCHEMA, dev)


def test_sliced_source_column(dev):
    rows = [("row-%d-" % i).encode() * (i % 6) for i in range(70)]
    whole = Column.from_bytes(rows)
    skip = 9
    assert int(whole.offsets[skip]) > 0
    # the same data tensor, offsets that start above 0
    sliced = Column("binary", whole.data, whole.offsets[skip:])
    assert sliced.to_pylist() == rows[skip:]
    schema = ProtoSchema.parse("message L { int64 a = 1; string s = 2; }")
    _check(MessageBatch({"a": _num(list(range(70 - skip))), "s": sliced}),
           schema, dev)


def test_payload_alignment_residues(dev):
    # payload lengths 1..48 with a varying row head: source and destination
    # starts run through every residue mod 16, in many combinations
    n = 96
    rows = [bytes([65 + i % 26]) * (1 + (i * 7) % 48) for i in range(n)]
    schema = ProtoSchema.parse("message P { int64 a = 1; string s = 2; }")
    batch = MessageBatch({"a": _num([(1 << (i % 9) * 7) - 1 for i in range(n)]),
                          "s": Column.from_bytes(rows)})
    got, want = _check(batch, schema, dev)
    src = batch.columns["s"].offsets[:-1].tolist()
    ends = got.offsets.cpu().tolist()[1:]
    dst = [e - len(r) for e, r in zip(ends, rows)]  # s is the last field
    assert {p % 16 for p in src} == set(range(16))
    assert {p % 16 for p in dst} == set(range(16))
    assert len({(p % 16, q % 16) for p, q in zip(src, dst)}) > 48


# --------------------------------------------------------------------- validity
def test_nulls_in_numeric_and_binary_columns(dev):
    n = 67
    valid_a = [i % 3 != 0 for i in range(n)]
    valid_s = [i % 4 != 1 for i in range(n)]
    s = Column.from_bytes([b"v%d" % i for i in range(n)])
    s.validity = torch.tensor(valid_s)
    batch = MessageBatch({
        "a": _num([i + 1 for i in range(n)], valid=valid_a),
        "b": _num([i + 0.5 for i in range(n)], torch.float64,
                  valid=[i % 5 != 2 for i in range(n)]),
        "s": s, "z": _num([-i - 1 for i in range(n)])})
    _, want = _check(batch, MIXED, dev)
    assert b"v1" not in want[1] and b"v2" in want[2]


def test_all_null_batch_is_zero_bytes(dev):
    n = 65
    none = [False] * n
    s = Column.from_bytes([b"payload"] * n)
    s.validity = torch.tensor(none)
    batch = MessageBatch({
        "a": _num([7] * n, valid=none),
        "b": _num([1.5] * n, torch.float64, valid=none),
        "s": s, "z": _num([-1] * n, valid=none)})
    got, want = _check(batch, MIXED, dev)
    assert want == [b""] * n and got.data.numel() == 0


def test_schema_field_without_a_column(dev):
    batch = _mixed_batch(70)
    del batch.columns["b"], batch.columns["s"]
    _check(batch, MIXED, dev)
    batch = _mixed_batch(70)
    del batch.columns["a"], batch.columns["z"], batch.columns["b"]
    _check(batch, MIXED, dev)


# ------------------------------------------------------------------------ casts
def test_column_dtypes_are_cast_like_the_host(dev):
    schema = ProtoSchema.parse(
        "message K { int64 a = 1; sint32 z = 2; double d = 3; double e = 4; "
        "float f = 5; double g = 6; uint32 u = 7; double h = 8; }")
    fl = [1.9, -1.9, 0.4, -0.4, 3e9, -3e9, 0.0, 127.99]
    n = len(fl)
    batch = MessageBatch({
        "a": _num(fl, torch.float64),             # truncates toward zero
        "z": _num(fl, torch.float32),
        "d": _num([1, -2, 0, 4, 5, 6, 7, 1 << 30], torch.int32),
        "e": _num([i % 2 == 0 for i in range(n)], torch.bool),
        "f": _num(fl, torch.bfloat16),            # through float32
        "g": _num(fl, torch.float16),
        "u": _num([0, 1, 200, 255, 7, 8, 9, 10], torch.uint8),
        "h": _num(fl, torch.float32)})
    _check(batch, schema, dev)


# ----------------------------------------------------------------------- errors
RANGE_SCHEMA = "message E { fixed32 u = 1; sfixed32 i = 2; float f = 3; }"


@pytest.mark.parametrize("col,value", [
    ("u", -1), ("u", 1 << 32), ("i", 1 << 31), ("i", -(1 << 31) - 1),
    ("f", 1e39), ("f", -1e39)])
def test_out_of_range_raises(dev, col, value):
    schema = ProtoSchema.parse(RANGE_SCHEMA)
    vals = [1] * 70
    vals[66] = value
    dtype = torch.float64 if col == "f" else torch.int64
    batch = MessageBatch({col: _num(vals, dtype)})
    with pytest.raises((struct.error, OverflowError)):
        _want(batch, schema)            # the host codec refuses it too
    on_dev = batch.to(dev)
    with pytest.raises(ProcessError):
        ops.proto_encode(on_dev, schema)
    with pytest.raises(ProcessError):
        _run(ArrowToProtobufProcessor({"proto": RANGE_SCHEMA})
             .process(on_dev))
    with pytest.raises(ProcessError):
        ProtobufCodec({"proto": RANGE_SCHEMA}).encode(on_dev)
    with pytest.raises(ProcessError):
        SchemaRegistryCodec({"schemas": {"1": RANGE_SCHEMA}}).encode(on_dev)


def test_range_limits_do_not_raise(dev):
    schema = ProtoSchema.parse(RANGE_SCHEMA)
    batch = MessageBatch({
        "u": _num([(1 << 32) - 1, 0, 1]),
        "i": _num([(1 << 31) - 1, -(1 << 31), 0]),
        "f": _num([F32_MAX, -F32_MAX, float("inf")], torch.float64)})
    _check(batch, schema, dev)


# ----------------------------------------------------------------------- prefix
def test_registry_header_prefix(dev):
    header = b"\x00" + struct.pack(">I", 0x01020304)
    got, want = _check(_mixed_batch(65), MIXED, dev, prefix=header)
    assert all(w.startswith(header) for w in want)
    # a row with nothing present is the prefix alone
    _, want = _check(MessageBatch({"a": _num([0, 5, 0])}), MIXED, dev, b"PREFIX08")
    assert want[0] == want[2] == b"PREFIX08"


def test_schema_registry_codec_matches_host(dev):
    src = "message R { int64 a = 1; double b = 2; string s = 3; sint32 z = 4; }"
    codec = SchemaRegistryCodec({"schemas": {"77": src},
                                 "default_schema_id": 77})
    batch = _mixed_batch(130)
    on_dev = batch.to(dev)
    assert encode_device(ProtoSchema.parse(src), on_dev.columns) is not None
    got = codec.encode(on_dev)
    assert got == codec.encode(on_dev.to("cpu"))
    assert got == _want(batch, MIXED, b"\x00\x00\x00\x00\x4d")


def test_protobuf_codec_matches_host(dev):
    batch = _all_types_batch()
    src = "message A { " + " ".join(
        f"{t} c_{t} = {i + 1};" for i, t in enumerate(ALL_TYPES)) + " }"
    got = ProtobufCodec({"proto": src}).encode(batch.to(dev))
    assert got == _want(batch, ALL_SCHEMA)
    assert got == ProtobufCodec({"proto": src, "encoder": "host"}).encode(
        batch.to(dev))


# ------------------------------------------------------------------- round trip
def test_decode_of_encode_gives_the_columns_back(dev, nat):
    # fixed64 up to 2^64 - 1: the decoder stores it as a negative int64 and
    # the encoder writes those 8 bytes back
    batch = _all_types_batch(fixed64_max=-1).to(dev)
    # a float field round-trips what float32 holds
    f32 = batch.columns["c_float"].data.to(torch.float32).to(torch.float64)
    batch.columns["c_float"] = Column("numeric", f32)
    enc = ops.proto_encode(batch, ALL_SCHEMA)
    fno, kind, isf, slot, int_f, float_f, str_f = build_gpu_spec(ALL_SCHEMA)
    assert len(fno) <= 16
    out_i, out_f, _, strings, summary = nat.proto_decode(
        enc.data.contiguous(), enc.offsets, fno, kind, isf, slot,
        len(int_f), len(float_f), len(str_f))
    assert int(summary[0]) == 0
    for i, name in enumerate(int_f):
        want = batch.columns[name].data.to(torch.int64)
        assert torch.equal(out_i[i], want), name
    for i, name in enumerate(float_f):
        want = batch.columns[name].data
        if name == "c_double":
            # bit-exact, -0.0 aside: it is elided and decodes as +0.0
            want = torch.where(want == 0, torch.zeros_like(want), want)
        same = (out_f[i].view(torch.int64) == want.view(torch.int64))
        if name == "c_float":
            want = torch.where(want == 0, torch.zeros_like(want), want)
            same = (out_f[i] == want) | (out_f[i].isnan() & want.isnan())
        assert bool(same.all()), name
    for i, name in enumerate(str_f):
        data, offs = strings[i]
        src = batch.columns[name]
        assert torch.equal(offs, src.offsets), name
        assert torch.equal(data, src.data), name


# -------------------------------------------------------------------- processor
def test_processor_keeps_value_on_the_device(dev):
    src = "message R { int64 a = 1; double b = 2; string s = 3; sint32 z = 4; }"
    batch = _mixed_batch(257)
    batch.input_name = "kafka-in"
    on_dev = batch.to(dev)
    out, = _run(ArrowToProtobufProcessor({"proto": src}).process(on_dev))
    value = out.columns["__value__"]
    assert list(out.columns) == ["__value__"]
    assert value.data.is_cuda and value.offsets.is_cuda
    assert out.input_name == "kafka-in"
    cpu_out, = _run(ArrowToProtobufProcessor({"proto": src}).process(batch))
    assert not cpu_out.columns["__value__"].data.is_cuda
    assert out.binary_values() == cpu_out.binary_values()
    assert out.binary_values() == _want(batch, MIXED)

    host, = _run(ArrowToProtobufProcessor(
        {"proto": src, "encoder": "host"}).process(on_dev))
    assert not host.columns["__value__"].data.is_cuda
    assert host.input_name == "kafka-in"
    assert host.binary_values() == out.binary_values()


def test_wide_schema_takes_the_host_path(dev):
    src = "message W { " + " ".join(
        f"int64 c{i} = {i + 1};" for i in range(33)) + " }"
    schema = ProtoSchema.parse(src)
    batch = MessageBatch({f"c{i}": _num([i, 0, -i, i * 1000])
                          for i in range(33)})
    on_dev = batch.to(dev)
    assert encode_device(schema, on_dev.columns) is None
    out, = _run(ArrowToProtobufProcessor({"proto": src}).process(on_dev))
    assert not out.columns["__value__"].data.is_cuda
    assert out.binary_values() == _want(batch, schema)
    # 32 fields still run on the device
    src32 = src.replace("int64 c32 = 33;", "")
    out32, = _run(ArrowToProtobufProcessor({"proto": src32}).process(on_dev))
    assert out32.columns["__value__"].data.is_cuda
    assert out32.binary_values() == _want(batch, ProtoSchema.parse(src32))


def test_field_limit_matches_the_extension(nat):
    from arkflow_amd.processors.protobuf_proc import PROTO_ENC_MAX_FIELDS
    assert nat.PROTO_ENC_MAX_FIELDS == PROTO_ENC_MAX_FIELDS == 32


def test_mixed_residency_takes_the_host_path(dev):
    batch = _mixed_batch(5)
    mixed = MessageBatch(dict(batch.columns))
    mixed.columns["a"] = mixed.columns["a"].to(dev)
    assert encode_device(MIXED, mixed.columns) is None
    src = "message R { int64 a = 1; double b = 2; string s = 3; sint32 z = 4; }"
    out, = _run(ArrowToProtobufProcessor({"proto": src}).process(mixed))
    assert out.binary_values() == _want(batch, MIXED)
