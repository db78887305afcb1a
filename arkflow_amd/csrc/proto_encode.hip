// GPU protobuf scalar encode: the inverse of proto_decode.hip for the
// reference's arrow_to_protobuf processor (crates/arkflow-plugin/src/
// processor/protobuf.rs — scalar proto3 only). Columnar inputs go to one
// binary column of messages in two passes over the rows, one thread per row:
// a size pass (encoded length of each row → int32, scanned to offsets by the
// caller) and a write pass (prefix, tags, varints, fixed-width values, length
// prefixes). String/bytes payloads are not written by the row thread: the
// write pass records where each one goes and a third kernel copies them, one
// wave per row, lanes on consecutive bytes. Size and write run the same row
// body, so the bytes written are the bytes counted.
//
// The output equals processors/proto_wire.encode_message byte for byte:
// proto3 default elision (0, ±0.0, empty), NULL → absent, negatives as 10-byte
// two's-complement varints, fields in ascending field number.
#include "common.h"
#include "kernels_api.h"

namespace {

// Counts (WRITE = false) or stores (WRITE = true) the bytes of one row. A
// store past `end` — possible only if the inputs changed between the two
// passes — is dropped, never written.
template <bool WRITE>
struct RowSink {
  uint8_t* __restrict__ out;
  int64_t pos;
  int64_t end;

  DEV_INLINE void byte(uint8_t b) {
    if (WRITE && pos < end) out[pos] = b;
    ++pos;
  }
  DEV_INLINE void varint(uint64_t v) {
    if (WRITE) {
      while (v >= 0x80) {
        byte((uint8_t)(v | 0x80));
        v >>= 7;
      }
      byte((uint8_t)v);
    } else {
      pos += (70 - __clzll((long long)(v | 1))) / 7;  // ceil(bits / 7)
    }
  }
  DEV_INLINE void fixed(uint64_t v, int nbytes) {
    if (WRITE) {
      for (int b = 0; b < nbytes; ++b) byte((uint8_t)(v >> (8 * b)));
    } else {
      pos += nbytes;
    }
  }
};

// Source span of row i in string slot sl; a span outside the column's data
// flags an error and reads as empty.
DEV_INLINE int64_t str_span(const ProtoEncSpec& spec, int sl, int64_t i,
                            int64_t* start, int32_t* err) {
  const int64_t b = spec.soffs[sl][i];
  const int64_t e = spec.soffs[sl][i + 1];
  if (b < 0 || e < b || e > spec.sdata_len[sl]) {
    err[0] = 1;
    return 0;
  }
  *start = b;
  return e - b;
}

template <bool WRITE>
DEV_INLINE int64_t encode_row(const ProtoEncSpec& spec,
                              const int64_t* __restrict__ in_i64,
                              const double* __restrict__ in_f64, int64_t n,
                              int64_t i, uint8_t* __restrict__ out,
                              int64_t pos, int64_t end,
                              int64_t* __restrict__ str_dst,
                              int32_t* __restrict__ err) {
  RowSink<WRITE> sink{out, pos, end};
  for (int b = 0; b < spec.prefix_len; ++b) sink.byte(spec.prefix[b]);
  for (int f = 0; f < spec.nf; ++f) {
    const int kind = spec.kind[f];
    const int sl = spec.slot[f];
    const uint8_t* valid = spec.valid[f];
    const bool present = !valid || valid[i];
    if (kind == PROTO_BYTES) {
      int64_t start = 0;
      const int64_t len = present ? str_span(spec, sl, i, &start, err) : 0;
      if (len == 0) {
        if (WRITE) str_dst[(int64_t)sl * n + i] = -1;
        continue;
      }
      sink.varint(spec.tag[f]);
      sink.varint((uint64_t)len);
      if (WRITE) str_dst[(int64_t)sl * n + i] = sink.pos;
      sink.pos += len;
      continue;
    }
    if (!present) continue;
    if (kind == PROTO_F64 || kind == PROTO_F32) {
      const double v = in_f64[(int64_t)sl * n + i];
      if (v == 0.0) continue;  // ±0.0; NaN compares unequal and is written
      sink.varint(spec.tag[f]);
      if (kind == PROTO_F64) {
        sink.fixed((uint64_t)__double_as_longlong(v), 8);
      } else {
        const float fv = (float)v;  // round to nearest even
        if (isinf(fv) && !isinf(v)) err[0] = 1;
        sink.fixed(__float_as_uint(fv), 4);
      }
      continue;
    }
    const int64_t v = in_i64[(int64_t)sl * n + i];
    if (v == 0) continue;
    sink.varint(spec.tag[f]);
    switch (kind) {
      case PROTO_ZIGZAG:
        sink.varint(((uint64_t)v << 1) ^ (uint64_t)(v >> 63));
        break;
      case PROTO_FIXED64:
        sink.fixed((uint64_t)v, 8);
        break;
      case PROTO_FIXED32:
        if (v < 0 || v > 0xFFFFFFFFll) err[0] = 1;
        sink.fixed((uint64_t)v, 4);
        break;
      case PROTO_SFIXED32:
        if (v < -2147483648ll || v > 2147483647ll) err[0] = 1;
        sink.fixed((uint64_t)v, 4);
        break;
      case PROTO_VARINT:
      default:
        sink.varint((uint64_t)v);
        break;
    }
  }
  return sink.pos;
}

__global__ void proto_encode_size_kernel(ProtoEncSpec spec,
                                         const int64_t* __restrict__ in_i64,
                                         const double* __restrict__ in_f64,
                                         int64_t n, int32_t* __restrict__ lens,
                                         int32_t* __restrict__ err) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    int64_t len = encode_row<false>(spec, in_i64, in_f64, n, i, nullptr, 0, 0,
                                    nullptr, err);
    if (len > 2147483647ll) {
      err[0] = 1;
      len = 0;
    }
    lens[i] = (int32_t)len;
  }
}

__global__ void proto_encode_write_kernel(ProtoEncSpec spec,
                                          const int64_t* __restrict__ in_i64,
                                          const double* __restrict__ in_f64,
                                          int64_t n,
                                          const int64_t* __restrict__ out_offs,
                                          uint8_t* __restrict__ out,
                                          int64_t* __restrict__ str_dst,
                                          int32_t* __restrict__ err) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride)
    encode_row<true>(spec, in_i64, in_f64, n, i, out, out_offs[i],
                     out_offs[i + 1], str_dst, err);
}

// One wave per row, lanes on consecutive bytes of each string/bytes payload
// of the row. str_dst[s][i] < 0: the field is absent from row i.
__global__ void proto_encode_copy_kernel(ProtoEncSpec spec, int64_t n,
                                         const int64_t* __restrict__ str_dst,
                                         uint8_t* __restrict__ out,
                                         int64_t out_len) {
  const int64_t wave =
      ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t wstride = ((int64_t)gridDim.x * blockDim.x) / WAVE;
  for (int64_t i = wave; i < n; i += wstride) {
    for (int s = 0; s < spec.ns; ++s) {
      const int64_t dst = str_dst[(int64_t)s * n + i];
      if (dst < 0) continue;
      const int64_t src = spec.soffs[s][i];
      const int64_t len = spec.soffs[s][i + 1] - src;
      const uint8_t* __restrict__ data = spec.sdata[s];
      for (int64_t off = lane; off < len; off += WAVE)
        if (dst + off < out_len) out[dst + off] = data[src + off];
    }
  }
}

}  // namespace

extern "C" {

void launch_proto_encode_size(const ProtoEncSpec* spec, const int64_t* in_i64,
                              const double* in_f64, int64_t n, int32_t* lens,
                              int32_t* err, hipStream_t st) {
  if (n < 1) return;
  proto_encode_size_kernel<<<capped_grid(n), 256, 0, st>>>(
      *spec, in_i64, in_f64, n, lens, err);
}

void launch_proto_encode_write(const ProtoEncSpec* spec, const int64_t* in_i64,
                               const double* in_f64, int64_t n,
                               const int64_t* out_offs, uint8_t* out,
                               int64_t* str_dst, int32_t* err,
                               hipStream_t st) {
  if (n < 1) return;
  proto_encode_write_kernel<<<capped_grid(n), 256, 0, st>>>(
      *spec, in_i64, in_f64, n, out_offs, out, str_dst, err);
}

void launch_proto_encode_copy(const ProtoEncSpec* spec, int64_t n,
                              const int64_t* str_dst, uint8_t* out,
                              int64_t out_len, hipStream_t st) {
  if (n < 1 || spec->ns < 1) return;
  // 256 threads = 4 waves = 4 rows per block per pass of the stride loop
  proto_encode_copy_kernel<<<capped_grid(n, 256 / WAVE), 256, 0, st>>>(
      *spec, n, str_dst, out, out_len);
}

}  // extern "C"
