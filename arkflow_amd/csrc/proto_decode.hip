// GPU protobuf scalar decode: one thread per message, parsing varint /
// fixed-width fields straight out of the device-resident binary column
// (data + offsets) into columnar outputs — the survey's "warp-per-message
// varint decode kernel writing columnar" mapping for the reference's
// protobuf_to_arrow processor (crates/arkflow-plugin/src/processor/
// protobuf.rs — scalar proto3 only). Numeric fields land in typed columns;
// string/bytes fields record their span here and proto_copy_bytes_kernel
// copies them out into a binary column, so every schema of at most
// PROTO_MAX_FIELDS fields stays fully on-device.
#include "common.h"
#include "kernels_api.h"
#include "proto_wire.h"

__global__ void proto_decode_kernel(const uint8_t* __restrict__ data,
                                    const int64_t* __restrict__ offsets,
                                    int64_t n_msgs, ProtoSpec spec,
                                    int64_t* __restrict__ out_i64,  // [ni][n]
                                    double* __restrict__ out_f64,   // [nd][n]
                                    int64_t* __restrict__ str_start,  // [ns][n]
                                    int32_t* __restrict__ str_len,
                                    int32_t* __restrict__ err_flags) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n_msgs; i += stride) {
    int64_t pos = offsets[i];
    const int64_t end = offsets[i + 1];
    // proto3 defaults: the outputs start zeroed
    while (pos < end) {
      uint64_t tag;
      if (!proto_read_varint(data, &pos, end, &tag)) {
        err_flags[0] = 1;
        return;
      }
      int fno = (int)(tag >> 3);
      int wt = (int)(tag & 7);
      // find field slot
      int fi = -1;
#pragma unroll
      for (int f = 0; f < PROTO_MAX_FIELDS; ++f)
        if (f < spec.nf && spec.fno[f] == fno) fi = f;
      uint64_t raw = 0;
      if (wt == 0) {
        if (!proto_read_varint(data, &pos, end, &raw)) {
          err_flags[0] = 1;
          return;
        }
      } else if (wt == 1) {
        if (pos + 8 > end) { err_flags[0] = 1; return; }
        raw = proto_load_le<8>(data, pos);
        pos += 8;
      } else if (wt == 5) {
        if (pos + 4 > end) { err_flags[0] = 1; return; }
        raw = proto_load_le<4>(data, pos);
        pos += 4;
      } else if (wt == 2) {
        // length-delimited: string/bytes fields record their span for the
        // copy-out pass; other wt==2 payloads are skipped. Compared unsigned:
        // a length of 2^63 or more must not turn negative and pass.
        uint64_t ln;
        if (!proto_read_varint(data, &pos, end, &ln) ||
            ln > (uint64_t)(end - pos)) {
          err_flags[0] = 1;
          return;
        }
        if (fi >= 0 && spec.kind[fi] == PROTO_BYTES) {
          str_start[(int64_t)spec.slot[fi] * n_msgs + i] = pos;
          str_len[(int64_t)spec.slot[fi] * n_msgs + i] = (int32_t)ln;
        }
        pos += (int64_t)ln;
        continue;
      } else {
        err_flags[0] = 1;
        return;
      }
      if (fi < 0) continue;
      const int64_t o = (int64_t)spec.slot[fi] * n_msgs + i;
      switch (spec.kind[fi]) {
        case PROTO_F64:
          out_f64[o] = __longlong_as_double((long long)raw);
          break;
        case PROTO_F32:
          out_f64[o] = (double)__uint_as_float((uint32_t)raw);
          break;
        case PROTO_ZIGZAG:
          out_i64[o] = (int64_t)((raw >> 1) ^ (~(raw & 1) + 1));
          break;
        case PROTO_SFIXED32:
          out_i64[o] = (int64_t)(int32_t)(uint32_t)raw;
          break;
        case PROTO_BYTES:  // a string field sent with a scalar wire type
          break;
        default:  // PROTO_VARINT, PROTO_FIXED64, PROTO_FIXED32
          out_i64[o] = (int64_t)raw;
          break;
      }
    }
  }
}

// copy-out pass for ONE string/bytes field: raw span copy, no transform
__global__ void proto_copy_bytes_kernel(const uint8_t* __restrict__ data,
                                        const int64_t* __restrict__ start,
                                        const int64_t* __restrict__ out_offs,
                                        int64_t n_msgs,
                                        uint8_t* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n_msgs; i += stride) {
    int64_t w = out_offs[i];
    const int64_t wend = out_offs[i + 1];
    int64_t p = start[i];
    for (; w < wend; ++w, ++p) out[w] = data[p];
  }
}

extern "C" {

void launch_proto_copy_bytes(const uint8_t* data, const int64_t* start,
                             const int64_t* out_offs, int64_t n_msgs,
                             uint8_t* out, hipStream_t st) {
  if (n_msgs < 1) return;
  proto_copy_bytes_kernel<<<capped_grid(n_msgs), 256, 0, st>>>(
      data, start, out_offs, n_msgs, out);
}

void launch_proto_decode(const ProtoSpec* spec, const uint8_t* data,
                         const int64_t* offsets, int64_t n_msgs,
                         int64_t* out_i64, double* out_f64,
                         int64_t* str_start, int32_t* str_len,
                         int32_t* err_flags, hipStream_t st) {
  if (n_msgs < 1) return;
  proto_decode_kernel<<<capped_grid(n_msgs), 256, 0, st>>>(
      data, offsets, n_msgs, *spec, out_i64, out_f64, str_start, str_len,
      err_flags);
}

}  // extern "C"
