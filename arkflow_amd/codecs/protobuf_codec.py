"""`protobuf` codec: batch ↔ scalar proto3 wire format
(reference codec/protobuf.rs)."""
from __future__ import annotations

from typing import List, Sequence

import torch

from ..batch import Column, MessageBatch
from ..processors.proto_wire import decode_message
from ..processors.protobuf_proc import (
    _load_schema, encode_device, encode_rows_host, load_encoder_choice)
from ..registry import register
from ..spi import Codec


class ProtobufCodec(Codec):
    def __init__(self, config: dict, resource=None):
        self.schema = _load_schema(config)
        self.encoder = load_encoder_choice(config)
        self.device = getattr(resource, "device", None)

    def encode(self, batch: MessageBatch) -> List[bytes]:
        """One message per row. A device-resident batch that the GPU encoder
        takes (protobuf_proc.encode_device) is encoded there and comes back
        in one device-to-host copy of data and offsets; anything else, or
        ``encoder: host``, is encoded row by row on the host."""
        if self.encoder == "auto" and batch.num_rows and \
                encode_device(self.schema, batch.columns) is not None:
            from .. import ops
            return ops.proto_encode(batch, self.schema).to_pylist()
        return encode_rows_host(batch, self.schema)

    def decode(self, payloads: Sequence[bytes]) -> MessageBatch:
        rows = [decode_message(p, self.schema) for p in payloads]
        cols = {}
        for no in sorted(self.schema.fields):
            name, t = self.schema.fields[no]
            vals = [r[name] for r in rows]
            if t in ("string", "bytes"):
                cols[name] = Column.from_bytes(
                    [v.encode() if isinstance(v, str) else v for v in vals])
            elif t in ("double", "float"):
                cols[name] = Column.from_numeric(
                    torch.tensor(vals, dtype=torch.float64))
            elif t == "bool":
                cols[name] = Column.from_numeric(
                    torch.tensor(vals, dtype=torch.bool))
            else:
                cols[name] = Column.from_numeric(
                    torch.tensor(vals, dtype=torch.int64))
        return MessageBatch(cols)


@register("codec", "protobuf",
          description="batch ↔ scalar proto3 wire format (device-resident "
                      "batches encode on the GPU, host batches on the host)",
          example={"type": "protobuf",
                   "proto": "message M { double v = 1; }"})
def _build_protobuf_codec(config: dict, resource=None) -> ProtobufCodec:
    return ProtobufCodec(config, resource)
