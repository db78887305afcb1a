// Protobuf wire primitives of the decoder. __host__ __device__, so the same
// code that runs in proto_decode_kernel can be walked over malformed input on
// the CPU under a sanitizer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Base-128 varint at d[*pos .. end): the tag, a value or a length. Returns
// false when the continuation bit is still set after 10 bytes. A varint cut
// off by `end` yields the bits read so far; the field that follows it then
// fails its own bound check or the message simply ends.
__host__ __device__ inline bool proto_read_varint(const uint8_t* d,
                                                  int64_t* pos, int64_t end,
                                                  uint64_t* out) {
  uint64_t v = 0;
  int64_t p = *pos;
  int shift = 0;
  while (p < end) {
    const uint8_t b = d[p++];
    v |= (uint64_t)(b & 0x7F) << shift;
    if (!(b & 0x80)) break;
    shift += 7;
    if (shift > 63) return false;
  }
  *pos = p;
  *out = v;
  return true;
}

// Little-endian fixed32 (NB = 4) or fixed64 (NB = 8); the caller has checked
// pos + NB <= end.
template <int NB>
__host__ __device__ inline uint64_t proto_load_le(const uint8_t* d,
                                                  int64_t pos) {
  uint64_t v = 0;
#pragma unroll
  for (int b = 0; b < NB; ++b) v |= (uint64_t)d[pos + b] << (8 * b);
  return v;
}
