"""CPU tests of the decoders' schema limits: the two functions that decide
whether a schema goes to the device kernels, and the host decode that a
schema over the limits gets."""
import asyncio
import json

from arkflow_amd.batch import MessageBatch
from arkflow_amd.processors import json_proc, protobuf_proc
from arkflow_amd.processors.json_proc import JsonToArrowProcessor
from arkflow_amd.processors.proto_wire import ProtoSchema, encode_message
from arkflow_amd.processors.protobuf_proc import ProtobufToArrowProcessor


def _run(coro):
    return asyncio.new_event_loop().run_until_complete(coro)


def proto_src(nf):
    types = ["int64", "double", "string", "sint32", "bool", "fixed32"]
    return "message W { " + " ".join(
        f"{types[i % len(types)]} c{i} = {i + 1};" for i in range(nf)) + " }"


def proto_rows(nf, n):
    """Rows under proto_src(nf); no value is a proto3 default, so every field
    is on the wire."""
    make = {"int64": lambda r, i: r * 1000 + i + 1,
            "double": lambda r, i: r + i + 0.5,
            "string": lambda r, i: f"s{r}-{i}",
            "sint32": lambda r, i: -(r + i + 1),
            "bool": lambda r, i: True,
            "fixed32": lambda r, i: r * 7 + i + 1}
    schema = ProtoSchema.parse(proto_src(nf))
    return schema, [{name: make[t](r, no) for no, (name, t)
                     in schema.fields.items()} for r in range(n)]


def json_rows(nf, n):
    """(schema, docs): field c<i> is an int, float, str or bool by i % 4."""
    kinds = ["int", "float", "str", "bool"]
    make = {"int": lambda r, i: r * 100 + i, "float": lambda r, i: r + i / 4,
            "str": lambda r, i: f"v{r}.{i}",
            "bool": lambda r, i: (r + i) % 2 == 0}
    schema = {f"c{i}": kinds[i % 4] for i in range(nf)}
    return schema, [{f"c{i}": make[kinds[i % 4]](r, i) for i in range(nf)}
                    for r in range(n)]


def check_proto_columns(out, schema, rows):
    assert list(out.columns) == [schema.fields[no][0]
                                 for no in sorted(schema.fields)]
    for name, (_, t) in schema.by_name.items():
        want = [r[name] for r in rows]
        if t == "string":
            want = [w.encode() for w in want]
        assert out.column(name).to_pylist() == want, name


def check_json_columns(out, schema, docs):
    assert list(out.columns) == list(schema)
    for name, t in schema.items():
        want = [d[name] for d in docs]
        if t == "str":
            want = [w.encode() for w in want]
        assert out.column(name).to_pylist() == want, name
        assert out.column(name).validity is None


# ------------------------------------------------------------------- choosers
def test_proto_chooser_field_count():
    assert protobuf_proc.PROTO_MAX_FIELDS == 16
    assert protobuf_proc.decode_on_device(ProtoSchema.parse(proto_src(16)))
    assert not protobuf_proc.decode_on_device(ProtoSchema.parse(proto_src(17)))


def test_json_chooser_field_count():
    assert json_proc.decode_on_device({f"c{i}": "int" for i in range(16)})
    assert not json_proc.decode_on_device({f"c{i}": "int" for i in range(17)})


def test_json_chooser_parent_count():
    assert json_proc.decode_on_device({f"p{i}.x": "int" for i in range(8)})
    assert not json_proc.decode_on_device({f"p{i}.x": "int" for i in range(9)})
    # 16 fields under 8 parents: the parents are counted once each
    assert json_proc.decode_on_device(
        {f"p{i % 8}.x{i}": "int" for i in range(16)})


def test_json_chooser_name_length():
    ok, long = "n" * 23, "n" * 24
    assert json_proc.decode_on_device({ok: "int"})
    assert not json_proc.decode_on_device({long: "int"})
    assert json_proc.decode_on_device({f"{ok}.{ok}": "int"})
    assert not json_proc.decode_on_device({f"{long}.x": "int"})
    assert not json_proc.decode_on_device({f"x.{long}": "int"})
    # bytes count, not characters: 12 two-byte characters are 24 bytes
    assert json_proc.decode_on_device({"é" * 11: "int"})
    assert not json_proc.decode_on_device({"é" * 12: "int"})


def test_json_chooser_nesting_depth():
    assert json_proc.decode_on_device({"a.b": "int"})
    assert not json_proc.decode_on_device({"a.b.c": "int"})


# ------------------------------------------------- 17 fields on a host batch
def test_proto_17_fields_host_batch():
    schema, rows = proto_rows(17, 5)
    batch = MessageBatch.from_binary([encode_message(r, schema) for r in rows])
    out = _run(ProtobufToArrowProcessor(
        {"proto": proto_src(17)}, None).process(batch))[0]
    assert len(out.columns) == 17
    check_proto_columns(out, schema, rows)


def test_json_17_fields_host_batch():
    schema, docs = json_rows(17, 5)
    batch = MessageBatch.from_binary([json.dumps(d).encode() for d in docs])
    out = _run(JsonToArrowProcessor({"schema": schema},
                                    None).process(batch))[0]
    assert len(out.columns) == 17
    check_json_columns(out, schema, docs)
