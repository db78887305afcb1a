// Host-side interface of the bf16 GEMM family, shared by bindings.cpp and
// the GEMM .hip files: the variant ids, the argument block and the single
// launch entry.
#pragma once
#include <hip/hip_runtime.h>

// Values are the public `gemm_bf16_variant` ids (tests, tools/ and the
// ARKFLOW_GEMM_VARIANT override use the numbers) — never renumber.
enum GemmVariant {
  GEMM_BK32 = 0,     // direct-to-LDS 128² tile, BK=32
  GEMM_8P256 = 1,    // 8-phase BM=256, linear LDS
  GEMM_8P256S = 2,   // 8-phase BM=256 + XOR swizzle
  GEMM_2P = 3,       // 2-phase double-buffered 128², BK=32
  GEMM_8P128 = 4,    // 8-phase BM=128, linear LDS
  GEMM_8P128S = 5,   // 8-phase BM=128 + XOR swizzle
  GEMM_SKINNY = 6,   // direct-to-LDS 64² tile, BK=32
  GEMM_K64 = 7,      // direct-to-LDS 128² tile, BK=64
  GEMM_K64S = 8,     // register-staged swizzled 128², BK=64
  GEMM_K64D = 9,     // K64S with two LDS buffers
  GEMM_K64P = 10,    // K64S with register prefetch
  GEMM_K64W = 11,    // register-staged swizzled 256², 8 waves
  GEMM_K64S3 = 12,   // K64S at launch-bounds occupancy 3
};

enum GemmStatus {
  GEMM_OK = 0,
  GEMM_BAD_SHAPE = 1,    // K not a multiple of / too few of the variant's BK
  GEMM_BAD_VARIANT = 2,  // id is not a GemmVariant; nothing was launched
};

struct GemmArgs {
  const void* A;      // [M,K] bf16
  const void* Bt;     // [N,K] bf16 (torch Linear weight layout)
  const float* bias;  // [N] or null
  void* C;            // [M,N] bf16
  int M, N, K;
  int act;            // Act (gemm_common.h): 0 none, 1 relu, 2 gelu, 3 silu
  hipStream_t stream;
};

extern "C" int launch_gemm_bf16(int variant, const GemmArgs* args);
