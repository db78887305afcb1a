"""CPU tests of the protobuf encode plan: the kernel field spec, the decisions
that send an input to the host codec, and ops.proto_encode on host batches."""
import asyncio

import pytest
import torch

from arkflow_amd import ops
from arkflow_amd.batch import Column, MessageBatch
from arkflow_amd.codecs.protobuf_codec import ProtobufCodec
from arkflow_amd.errors import ConfigError, ProcessError
from arkflow_amd.processors.proto_wire import ProtoSchema, encode_message
from arkflow_amd.processors.protobuf_proc import (
    PROTO_ENC_MAX_FIELDS, ArrowToProtobufProcessor, build_encode_spec,
    encode_device)

# declared out of field-number order on purpose
PROTO = """
message M {
  string name = 7;
  double d = 3;
  sint64 z = 1;
  float f = 12;
  bytes raw = 2;
  fixed32 u = 5;
  bool ok = 4;
  sfixed64 sf = 6;
}
"""


def _batch(n=3):
    return MessageBatch.from_dict({
        "name": ["a", "", "ccc"][:n], "d": [1.5, 0.0, -2.0][:n],
        "z": [-1, 0, 7][:n], "f": [0.5, 1e-3, 0.0][:n],
        "raw": [b"\x00\xff", b"", b"x"][:n], "u": [1, 2, 0][:n],
        "ok": [True, False, True][:n], "sf": [-5, 0, 9][:n]})


def test_spec_order_kinds_and_slots():
    schema = ProtoSchema.parse(PROTO)
    spec = build_encode_spec(schema, _batch().columns)
    assert spec.fno == [1, 2, 3, 4, 5, 6, 7, 12]
    assert spec.names == ["z", "raw", "d", "ok", "u", "sf", "name", "f"]
    # 0 varint, 1 zigzag, 2 f64, 3 f32, 4 fixed64, 6 fixed32, 9 bytes
    assert spec.kind == [1, 9, 2, 0, 6, 4, 9, 3]
    assert spec.int_fields == ["z", "ok", "u", "sf"]
    assert spec.float_fields == ["d", "f"]
    assert spec.str_fields == ["raw", "name"]
    assert spec.slot == [0, 0, 0, 1, 2, 3, 1, 1]


def test_spec_every_type_has_a_kind():
    types = ["double", "float", "int32", "int64", "uint32", "uint64",
             "sint32", "sint64", "bool", "fixed64", "sfixed64", "fixed32",
             "sfixed32", "string", "bytes"]
    src = "message A { " + " ".join(
        f"{t} c{i} = {i + 1};" for i, t in enumerate(types)) + " }"
    cols = {f"c{i}": (Column.from_bytes([b"x"]) if t in ("string", "bytes")
                      else Column.from_numeric([1]))
            for i, t in enumerate(types)}
    spec = build_encode_spec(ProtoSchema.parse(src), cols)
    assert spec.kind == [2, 3, 0, 0, 0, 0, 1, 1, 0, 4, 4, 6, 7, 9, 9]


def test_missing_column_is_left_out_of_the_spec():
    schema = ProtoSchema.parse(PROTO)
    cols = dict(_batch().columns)
    del cols["d"], cols["raw"]
    spec = build_encode_spec(schema, cols)
    assert spec is not None
    assert spec.names == ["z", "ok", "u", "sf", "name", "f"]
    assert spec.float_fields == ["f"] and spec.str_fields == ["name"]
    assert spec.slot == [0, 1, 2, 3, 0, 0]
    # columns that the schema does not name are ignored
    cols["extra"] = Column.from_numeric([1, 2, 3])
    assert build_encode_spec(schema, cols) == spec


def test_kind_mismatch_falls_back():
    schema = ProtoSchema.parse(PROTO)
    cols = dict(_batch().columns)
    cols["d"] = Column.from_bytes([b"1", b"2", b"3"])  # binary → double
    assert build_encode_spec(schema, cols) is None
    cols = dict(_batch().columns)
    cols["name"] = Column.from_numeric([1, 2, 3])      # numeric → string
    assert build_encode_spec(schema, cols) is None


def test_wide_schema_falls_back():
    def schema(nf):
        return ProtoSchema.parse("message W { " + " ".join(
            f"int64 c{i} = {i + 1};" for i in range(nf)) + " }")
    cols = {"c0": Column.from_numeric([1])}
    assert PROTO_ENC_MAX_FIELDS == 32
    assert build_encode_spec(schema(32), cols) is not None
    # the width of the schema decides, not how many columns match
    assert build_encode_spec(schema(33), cols) is None


def test_host_batch_never_takes_the_device_encoder():
    schema = ProtoSchema.parse(PROTO)
    assert encode_device(schema, _batch().columns) is None
    assert encode_device(schema, {}) is None


def test_ops_proto_encode_host_equals_encode_message():
    schema = ProtoSchema.parse(PROTO)
    batch = _batch()
    want = [encode_message(r, schema) for r in batch.to_rows()]
    col = ops.proto_encode(batch, schema)
    assert col.kind == "binary" and col.data.device.type == "cpu"
    assert col.to_pylist() == want
    # a dict of columns, and a prefix ahead of every row (empty rows too)
    col = ops.proto_encode(dict(batch.columns), schema, prefix=b"\x00\x01\x02")
    assert col.to_pylist() == [b"\x00\x01\x02" + w for w in want]
    nulls = MessageBatch({"z": Column(
        "numeric", torch.tensor([5, 6]),
        validity=torch.tensor([False, True]))})
    assert ops.proto_encode(nulls, schema, prefix=b"P").to_pylist() == \
        [b"P", b"P" + encode_message({"z": 6}, schema)]


def test_ops_proto_encode_host_out_of_range_raises():
    schema = ProtoSchema.parse(PROTO)
    with pytest.raises(ProcessError):
        ops.proto_encode(MessageBatch.from_dict({"u": [1 << 32]}), schema)
    with pytest.raises(ProcessError):
        ops.proto_encode(MessageBatch.from_dict({"f": [1e39]}), schema)


def test_long_prefix_is_rejected():
    schema = ProtoSchema.parse(PROTO)
    assert ops.proto_encode(_batch(), schema, prefix=b"12345678") is not None
    with pytest.raises(ValueError):
        ops.proto_encode(_batch(), schema, prefix=b"123456789")


def test_encoder_config_key():
    assert ArrowToProtobufProcessor({"proto": PROTO}).encoder == "auto"
    for choice in ("auto", "host"):
        cfg = {"proto": PROTO, "encoder": choice}
        assert ArrowToProtobufProcessor(cfg).encoder == choice
        assert ProtobufCodec(cfg).encoder == choice
    for bad in ("gpu", "", None, True):
        with pytest.raises(ConfigError):
            ArrowToProtobufProcessor({"proto": PROTO, "encoder": bad})
        with pytest.raises(ConfigError):
            ProtobufCodec({"proto": PROTO, "encoder": bad})


def test_host_processor_and_codec_unchanged():
    schema = ProtoSchema.parse(PROTO)
    batch = _batch()
    batch.input_name = "in0"
    want = [encode_message(r, schema) for r in batch.to_rows()]
    for choice in ("auto", "host"):
        cfg = {"proto": PROTO, "encoder": choice}
        out, = asyncio.new_event_loop().run_until_complete(
            ArrowToProtobufProcessor(cfg).process(batch))
        assert out.binary_values() == want and out.input_name == "in0"
        assert out.device.type == "cpu"
        assert ProtobufCodec(cfg).encode(batch) == want
