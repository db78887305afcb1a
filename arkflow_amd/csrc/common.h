// Shared device helpers for arkflow_amd gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

#define WAVE 64
#define DEV_INLINE __device__ __forceinline__

DEV_INLINE uint64_t lanemask_lt() {
  return (1ull << (threadIdx.x & 63)) - 1ull;
}

// 64-bit splittable mix (Stafford variant 13) — key hashing.
DEV_INLINE uint64_t mix64(uint64_t z) {
  z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ull;
  z ^= z >> 27; z *= 0x94d049bb133111ebull;
  z ^= z >> 31;
  return z;
}

// wave-wide sum reduce (f32)
DEV_INLINE float wave_reduce_sum(float v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
DEV_INLINE float wave_reduce_max(float v) {
  for (int off = 32; off > 0; off >>= 1)
    v = fmaxf(v, __shfl_down(v, off, 64));
  return v;
}

// atomic float max/min via monotone flip to UNSIGNED int order
// (the flipped values must be compared unsigned — top-bit-set patterns)
DEV_INLINE uint32_t float_flip_bits(uint32_t u) {
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
DEV_INLINE uint32_t float_flip(float f) {
  return float_flip_bits((uint32_t)__float_as_int(f));
}
DEV_INLINE bool f32_bits_nan(uint32_t u) {
  return (u & 0x7fffffffu) > 0x7f800000u;
}
DEV_INLINE float float_unflip(uint32_t u) {
  return __int_as_float(
      (int32_t)((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u));
}

constexpr int cdiv(int a, int b) { return (a + b - 1) / b; }

// Free-slot marker of the open-addressing tables (GROUP BY and join). It is
// INT64_MIN, which is also a legal key, so a row with that key never probes:
// it owns the one extra slot at index table_size, which `& table_mask` cannot
// reach. The per-slot int32 arrays (group ids, chain heads) are therefore
// table_size + 1 long; the key array stays at table_size.
#define EMPTY_KEY 0x8000000000000000ll

// Where a kernel's row count comes from. The sync form of an operator knows
// it on the host; the capture form reads what an earlier kernel of the same
// hipGraph wrote to device memory. Kernels take the type as a template
// parameter, so both forms are instantiations of one body.
struct HostCount {
  int64_t n;
  DEV_INLINE int64_t get() const { return n; }
};
struct DevCount {
  const int32_t* __restrict__ n;
  DEV_INLINE int64_t get() const { return *n; }
};

// Blocks of `block` threads covering n items, clamped to [1, cap]; kernels
// launched with it are grid-stride.
inline int capped_grid(int64_t n, int block = 256, int cap = 2048) {
  int64_t g = (n + block - 1) / block;
  return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

template <typename T>
__global__ void fill_kernel(T* p, T v, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) p[i] = v;
}
