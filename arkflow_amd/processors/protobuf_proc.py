"""`protobuf_to_arrow` / `arrow_to_protobuf` processors.

Mirrors reference crates/arkflow-plugin/src/processor/protobuf.rs +
component/protobuf.rs: dynamic decode/encode of scalar proto3 fields from a
.proto source (no nested/repeated/map/oneof — header :14-25). The decode hot
path is a GPU kernel parsing the device-resident binary column directly
(csrc/proto_decode.hip) — numeric fields into typed columns, string/bytes
fields via a two-pass span-record + copy-out into binary columns; a schema of
more than PROTO_MAX_FIELDS fields is decoded by the host codec instead. The
encode hot path is its inverse (csrc/proto_encode.hip, through
ops.proto_encode): a size pass, an offsets scan, a write pass and a
wave-per-row payload copy turn device-resident columns into a device-resident
``__value__`` column, byte for byte what the host codec
(proto_wire.encode_message) writes row by row.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

from ..batch import Column, DEFAULT_BINARY_VALUE_FIELD, MessageBatch
from ..errors import ConfigError, ProcessError
from ..registry import register
from ..spi import Processor
from .proto_wire import ProtoSchema, decode_message, encode_message

# ProtoKind of csrc/kernels_api.h by proto3 type: one table for the device
# decoder and the device encoder
KIND_BYTES = 9
_KIND = {
    "int32": 0, "int64": 0, "uint32": 0, "uint64": 0, "bool": 0,
    "sint32": 1, "sint64": 1, "double": 2, "float": 3,
    "fixed64": 4, "sfixed64": 4, "fixed32": 6, "sfixed32": 7,
    "string": KIND_BYTES, "bytes": KIND_BYTES,
}
_FLOAT_TYPES = {"double", "float"}
PROTO_MAX_FIELDS = 16      # the device decoder's limit (csrc/kernels_api.h)
PROTO_ENC_MAX_FIELDS = 32  # the device encoder's


def _load_schema(config: dict) -> ProtoSchema:
    src = config.get("proto")
    if not src and config.get("proto_path"):
        with open(config["proto_path"]) as f:
            src = f.read()
    if not src:
        raise ConfigError("protobuf processor requires 'proto' or 'proto_path'")
    return ProtoSchema.parse(src, config.get("message"))


def decode_on_device(schema: ProtoSchema) -> bool:
    """Whether the device decoder takes this schema: at most PROTO_MAX_FIELDS
    fields. A wider one is decoded by the host codec."""
    return len(schema.fields) <= PROTO_MAX_FIELDS


def build_gpu_spec(schema):
    """Kernel field spec from a ProtoSchema: (fno, kind, isf, slot,
    int_fields, float_fields, str_fields) — shared by the processor and the
    fused bench graph (ops/stepgraph.FusedProtoMlp)."""
    fno, kind, isf, slot = [], [], [], []
    int_fields, float_fields, str_fields = [], [], []
    for no in sorted(schema.fields):
        name, t = schema.fields[no]
        # uint32/uint64/fixed stay in int64 (values < 2^63 in practice);
        # only true floats go to the f64 output
        fields = str_fields if _KIND[t] == KIND_BYTES else \
            float_fields if t in _FLOAT_TYPES else int_fields
        fno.append(no)
        kind.append(_KIND[t])
        isf.append(int(t in _FLOAT_TYPES))
        slot.append(len(fields))
        fields.append(name)
    return fno, kind, isf, slot, int_fields, float_fields, str_fields


class EncodeSpec(NamedTuple):
    """Field spec of the device encoder, fields in ascending field number.
    ``slot[f]`` is field f's row in the int64 inputs (``int_fields``), the
    float64 inputs (``float_fields``) or its string slot (``str_fields``),
    whichever its kind reads."""
    fno: List[int]
    kind: List[int]
    slot: List[int]
    names: List[str]
    int_fields: List[str]
    float_fields: List[str]
    str_fields: List[str]


def build_encode_spec(schema: ProtoSchema, columns: Dict[str, Column]
                      ) -> Optional[EncodeSpec]:
    """Kernel field spec for encoding ``columns`` under ``schema``, or None
    when the device encoder does not take this input and the host codec must:
    a schema wider than PROTO_ENC_MAX_FIELDS, or a matched column of the
    wrong kind (scalar fields need numeric columns, string/bytes fields
    binary ones). A schema field with no column is absent from every row and
    therefore from the spec. Residency is the caller's check
    (``encode_device``)."""
    if len(schema.fields) > PROTO_ENC_MAX_FIELDS:
        return None
    spec = EncodeSpec([], [], [], [], [], [], [])
    for no in sorted(schema.fields):
        name, t = schema.fields[no]
        col = columns.get(name)
        if col is None:
            continue
        k = _KIND[t]
        if col.kind != ("binary" if k == KIND_BYTES else "numeric"):
            return None
        fields = spec.str_fields if k == KIND_BYTES else \
            spec.float_fields if t in _FLOAT_TYPES else spec.int_fields
        spec.fno.append(no)
        spec.kind.append(k)
        spec.slot.append(len(fields))
        spec.names.append(name)
        fields.append(name)
    return spec


def encode_device(schema: ProtoSchema, columns: Dict[str, Column]
                  ) -> Optional[Tuple[EncodeSpec, torch.device]]:
    """(spec, device) when the device encoder applies: the native extension
    is loaded, ``build_encode_spec`` accepts the input and every matched
    column is on the same GPU. None → host path."""
    from .. import ops
    spec = build_encode_spec(schema, columns)
    if spec is None or not spec.fno or not ops.native_available():
        return None
    devices = set()
    for name in spec.names:
        col = columns[name]
        devices.update(t.device for t in (col.data, col.offsets, col.validity)
                       if t is not None)
    if len(devices) != 1:
        return None
    device = devices.pop()
    return (spec, device) if device.type == "cuda" else None


def encode_rows_host(batch: MessageBatch, schema: ProtoSchema) -> List[bytes]:
    """The per-row host encode: every column to the host, one dict per row,
    ``encode_message`` on each."""
    payloads = []
    for r in batch.to_rows():
        clean = {}
        for name, (no, t) in schema.by_name.items():
            v = r.get(name)
            if isinstance(v, (bytes, bytearray)) and t == "string":
                v = v.decode("utf-8", "replace")
            clean[name] = v
        payloads.append(encode_message(clean, schema))
    return payloads


class ProtobufToArrowProcessor(Processor):
    def __init__(self, config: dict, resource=None):
        self.schema = _load_schema(config)
        self.value_field = config.get("value_field",
                                      DEFAULT_BINARY_VALUE_FIELD)
        self.device = getattr(resource, "device", None)

    async def process(self, batch: MessageBatch) -> List[MessageBatch]:
        if batch.num_rows == 0:
            return []
        col = batch.columns.get(self.value_field)
        if col is None or col.kind != "binary":
            raise ProcessError(
                f"protobuf_to_arrow: no binary column {self.value_field!r}")
        if not col.data.is_cuda:
            out = self._decode_cpu(col)
        elif decode_on_device(self.schema):
            out = self._decode_gpu(col)
        else:  # over the device decoder's limit: host codec, result returned
            out = self._decode_cpu(col).to(col.data.device)
        out.input_name = batch.input_name
        return [out]

    # ---------------------------------------------------------------- gpu path
    def _decode_gpu(self, col: Column) -> MessageBatch:
        from .. import ops
        nat = ops.require_native()
        (fno, kind, isf, slot,
         int_fields, float_fields, str_fields) = build_gpu_spec(self.schema)
        out_i, out_f, err, strings, summary = nat.proto_decode(
            col.data, col.offsets, fno, kind, isf, slot,
            len(int_fields), len(float_fields), len(str_fields))
        if int(summary[0]) != 0:  # err rode the one consolidated readback
            raise ProcessError("protobuf decode error (malformed message)")
        cols = {}
        for i, name in enumerate(int_fields):
            t = self.schema.by_name[name][1]
            data = out_i[i]
            if t == "bool":
                data = data.to(torch.bool)
            cols[name] = Column("numeric", data.contiguous())
        for i, name in enumerate(float_fields):
            cols[name] = Column("numeric", out_f[i].contiguous())
        for i, name in enumerate(str_fields):
            sdata, soffs = strings[i]
            cols[name] = Column("binary", sdata.contiguous(),
                                soffs.contiguous())
        # preserve declared field order
        ordered = {self.schema.fields[no][0]: cols[self.schema.fields[no][0]]
                   for no in sorted(self.schema.fields)
                   if self.schema.fields[no][0] in cols}
        return MessageBatch(ordered)

    # ---------------------------------------------------------------- cpu path
    def _decode_cpu(self, col: Column) -> MessageBatch:
        rows = [decode_message(p, self.schema) for p in col.to_pylist()]
        cols = {}
        for no in sorted(self.schema.fields):
            name, t = self.schema.fields[no]
            vals = [r[name] for r in rows]
            if t in ("string", "bytes"):
                cols[name] = Column.from_bytes(
                    [v.encode() if isinstance(v, str) else v for v in vals])
            elif t in _FLOAT_TYPES:
                cols[name] = Column.from_numeric(
                    torch.tensor(vals, dtype=torch.float64))
            elif t == "bool":
                cols[name] = Column.from_numeric(
                    torch.tensor(vals, dtype=torch.bool))
            else:
                cols[name] = Column.from_numeric(
                    torch.tensor(vals, dtype=torch.int64))
        out = MessageBatch(cols)
        if self.device is not None and self.device.type == "cuda":
            out = out.to(self.device)
        return out


def load_encoder_choice(config: dict) -> str:
    choice = config.get("encoder", "auto")
    if choice not in ("auto", "host"):
        raise ConfigError(
            f"protobuf 'encoder' must be 'auto' or 'host', got {choice!r}")
    return choice


class ArrowToProtobufProcessor(Processor):
    """Rows → one proto3 message each, in ``__value__``.

    ``encoder: auto`` (default) encodes on the GPU (csrc/proto_encode.hip)
    when the native extension is loaded, every schema-matched column is on
    one device with the kind its field needs (numeric for scalar fields,
    binary for string/bytes) and the schema has at most PROTO_ENC_MAX_FIELDS
    fields; ``__value__`` then stays on that device. Every other input — host
    batches, mixed residency, a kind mismatch, wider schemas — and
    ``encoder: host`` take the per-row host codec and give a host-resident
    ``__value__``. The bytes are the same either way, with one exception: the
    device copies a ``string`` field's bytes as they are, while the host path
    decodes them with ``errors="replace"`` and re-encodes, so input that is
    not valid UTF-8 comes out with U+FFFD substitutions on the host and
    untouched on the device. UTF-8 is not validated on the device.
    """

    def __init__(self, config: dict, resource=None):
        self.schema = _load_schema(config)
        self.encoder = load_encoder_choice(config)

    async def process(self, batch: MessageBatch) -> List[MessageBatch]:
        if batch.num_rows == 0:
            return []
        if self.encoder == "auto" and \
                encode_device(self.schema, batch.columns) is not None:
            from .. import ops
            value = ops.proto_encode(batch, self.schema)
            return [MessageBatch({DEFAULT_BINARY_VALUE_FIELD: value},
                                 batch.input_name)]
        payloads = encode_rows_host(batch, self.schema)
        return [MessageBatch.from_binary(payloads,
                                         input_name=batch.input_name)]


@register("processor", "protobuf_to_arrow",
          description="Decode scalar proto3 messages from __value__ into "
                      "typed columns (GPU varint kernel for numeric schemas)",
          example={"type": "protobuf_to_arrow",
                   "proto": "message M { double v = 1; }"})
def _build_p2a(config: dict, resource=None) -> ProtobufToArrowProcessor:
    return ProtobufToArrowProcessor(config, resource)


@register("processor", "arrow_to_protobuf",
          description="Encode rows as scalar proto3 messages into __value__ "
                      "(GPU encode kernel for device-resident batches; "
                      "encoder: auto | host)",
          example={"type": "arrow_to_protobuf",
                   "proto": "message M { double v = 1; }"})
def _build_a2p(config: dict, resource=None) -> ArrowToProtobufProcessor:
    return ArrowToProtobufProcessor(config, resource)
