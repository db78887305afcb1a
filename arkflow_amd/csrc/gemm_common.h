// Building blocks shared by the bf16 MFMA GEMM kernels (gemm_bf16.hip,
// gemm_8phase.hip): block remap, operand staging, fragment read + MFMA,
// the fused epilogue and the host-side epilogue dispatch. A kernel body is
// then only what is different about it: its staging and its loop schedule.
//
// Conventions: B is supplied transposed ([N,K] row-major — the torch Linear
// weight layout), so both A and B^T fragments read LDS with the same
// contiguous-16B pattern (ds_read_b128). Waves tile the block 2-wide in N;
// each wave owns FM×FN fragments of mfma_f32_16x16x32_bf16.
//
// C/D fragment mapping (gfx950, 16x16x32): col = lane&15,
// row = (lane>>4)*4 + reg. Verified against torch.matmul in
// tests/test_gpu_kernels.py with random asymmetric inputs (transpose-detecting).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "common.h"
#include "gemm_api.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

// ---- activation ---------------------------------------------------------------
// The one formula every fused epilogue and rowops' bias_act_bf16_kernel use;
// tests/nn_ref.py derives ACT_EPS from it.
enum Act { ACT_NONE = 0, ACT_RELU = 1, ACT_GELU = 2, ACT_SILU = 3 };

DEV_INLINE float apply_act(float x, int act) {
  switch (act) {
    case ACT_RELU: return fmaxf(x, 0.f);
    case ACT_GELU: {
      // tanh approximation (matches torch.nn.GELU(approximate="tanh")).
      // tanh via the hardware exp (v_exp_f32) — libm tanhf is a software
      // routine that costs ~100 TF on the fc1 epilogue (profiles r18).
      float c = 0.7978845608028654f * (x + 0.044715f * x * x * x);
      c = fminf(fmaxf(c, -10.f), 10.f);  // saturate: no overflow in expf
      float e = __expf(2.f * c);
      return 0.5f * x * (1.f + (e - 1.f) / (e + 1.f));
    }
    case ACT_SILU: return x / (1.f + __expf(-x));
    default: return x;
  }
}

// ---- block remap --------------------------------------------------------------
// XCD-aware bijective block swizzle (8 XCDs; guide §5 m204 variant): blocks
// that the hardware round-robins onto one XCD get consecutive tile ids.
DEV_INLINE int xcd_block_id() {
  int nwg = gridDim.x;
  int bid = blockIdx.x;
  if (nwg >= 16) {
    int q = nwg / 8, r = nwg % 8;
    int xcd = bid % 8, off = bid / 8;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + off;
  }
  return bid;
}

// ---- staging ------------------------------------------------------------------
// Both forms move a TILE-row × BKT-col slice of A and of Bt at column k0 into
// LDS, 16 B per lane per step, wave w covering bytes [w*1024, w*1024+1024) of
// every THREADS*16-byte step. Source rows are clamped: out-of-range rows
// produce garbage that only lands in out-of-range C rows/cols, which the
// epilogue never writes.

// Direct global→LDS via __builtin_amdgcn_global_load_lds width=16 (the CDNA4
// cp.async analog). A wave's 1 KiB lands LINEARLY from a scalar LDS base, so
// the layout is row-major [TILE][BKT]; completion is tracked by vmcnt.
template <int TILE, int BKT, int THREADS>
DEV_INLINE void stage_direct(const __bf16* __restrict__ A,
                             const __bf16* __restrict__ Bt, int row0, int col0,
                             int M, int N, int K, int k0, __bf16* Asm,
                             __bf16* Bsm) {
  constexpr int ROW_BYTES = BKT * 2;
  constexpr int STEPS = TILE * ROW_BYTES / (THREADS * 16);
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
#pragma unroll
  for (int it = 0; it < STEPS; ++it) {
    int wbase = wid * 1024 + it * THREADS * 16;  // wave-uniform LDS offset
    int lin = wbase + lane * 16;
    int trow = lin / ROW_BYTES;
    int tcol = lin % ROW_BYTES;
    int ga_row = min(row0 + trow, M - 1);
    const char* a_src = (const char*)(A + (int64_t)ga_row * K + k0) + tcol;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) uint32_t*)a_src,
        (__attribute__((address_space(3))) uint32_t*)((char*)Asm + wbase),
        16, 0, 0);
    int gb_row = min(col0 + trow, N - 1);
    const char* b_src = (const char*)(Bt + (int64_t)gb_row * K + k0) + tcol;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) uint32_t*)b_src,
        (__attribute__((address_space(3))) uint32_t*)((char*)Bsm + wbase),
        16, 0, 0);
  }
}

// Register staging for the XOR-swizzled [TILE][64] layout. The linear layout
// has a 128 B row stride = exactly one bank period: the 16 fragment rows a
// quarter-wave reads per ds_read_b128 alias onto the SAME banks (PMC r2:
// 4.4e5 conflicts/dispatch on the linear BK=64 kernel). XOR-swizzling the
// 16 B chunk index by (row & 7) spreads them: chunk' = chunk ^ (row & 7).
// global_load_lds cannot express a per-lane destination, so the slice goes
// global → 4+4 VGPR quads (swz_load) → per-lane ds_write_b128 (swz_write).
// Splitting the two lets a kernel issue the next slice's loads early.
constexpr int SWZ_BK = 64;
constexpr int SWZ_STEPS = 4;  // TILE*128 B / (2*TILE threads * 16 B)

template <int TILE>
DEV_INLINE void swz_load(const __bf16* __restrict__ A,
                         const __bf16* __restrict__ Bt, int row0, int col0,
                         int M, int N, int K, int k0, u32x4 (&va)[SWZ_STEPS],
                         u32x4 (&vb)[SWZ_STEPS]) {
  const int lin0 = (threadIdx.x >> 6) * 1024 + (threadIdx.x & 63) * 16;
#pragma unroll
  for (int it = 0; it < SWZ_STEPS; ++it) {
    int lin = lin0 + it * (2 * TILE * 16);
    int trow = lin >> 7;   // 128 B per row
    int tcol = lin & 127;  // multiple of 16
    int ga_row = min(row0 + trow, M - 1);
    va[it] = *(const u32x4*)((const char*)(A + (int64_t)ga_row * K + k0) +
                             tcol);
    int gb_row = min(col0 + trow, N - 1);
    vb[it] = *(const u32x4*)((const char*)(Bt + (int64_t)gb_row * K + k0) +
                             tcol);
  }
}

template <int TILE>
DEV_INLINE void swz_write(__bf16* Asm, __bf16* Bsm,
                          const u32x4 (&va)[SWZ_STEPS],
                          const u32x4 (&vb)[SWZ_STEPS]) {
  const int lin0 = (threadIdx.x >> 6) * 1024 + (threadIdx.x & 63) * 16;
#pragma unroll
  for (int it = 0; it < SWZ_STEPS; ++it) {
    int lin = lin0 + it * (2 * TILE * 16);
    int trow = lin >> 7;
    int tcol = lin & 127;
    int dst = (trow << 7) + (((tcol >> 4) ^ (trow & 7)) << 4);
    *(u32x4*)((char*)Asm + dst) = va[it];
    *(u32x4*)((char*)Bsm + dst) = vb[it];
  }
}

// ---- fragment read + MFMA over one staged K slice -----------------------------
// The lane holds 8 contiguous bf16 of row (frag*16 + (lane&15)) at 16 B chunk
// ks*4 + (lane>>4) of the BKT-wide LDS row; SWZ applies the staging swizzle.
template <int FM, int FN, int BKT, bool SWZ>
DEV_INLINE void load_frags(const __bf16* Asm, const __bf16* Bsm, int wm,
                           int wn, int ks, bf16x8 (&a_frag)[FM],
                           bf16x8 (&b_frag)[FN]) {
  const int lane = threadIdx.x & 63;
  const int fr = lane & 15;
  const int chunk = ks * 4 + (lane >> 4);
#pragma unroll
  for (int m = 0; m < FM; ++m) {
    int row = wm + m * 16 + fr;
    a_frag[m] =
        *(const bf16x8*)&Asm[row * BKT + (SWZ ? chunk ^ (row & 7) : chunk) * 8];
  }
#pragma unroll
  for (int n = 0; n < FN; ++n) {
    int row = wn + n * 16 + fr;
    b_frag[n] =
        *(const bf16x8*)&Bsm[row * BKT + (SWZ ? chunk ^ (row & 7) : chunk) * 8];
  }
}

template <int FM, int FN>
DEV_INLINE void mma_frags(const bf16x8 (&a_frag)[FM],
                          const bf16x8 (&b_frag)[FN], f32x4 (&acc)[FM][FN]) {
#pragma unroll
  for (int m = 0; m < FM; ++m)
#pragma unroll
    for (int n = 0; n < FN; ++n)
      acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          a_frag[m], b_frag[n], acc[m][n], 0, 0, 0);
}

template <int FM, int FN, int BKT, bool SWZ>
DEV_INLINE void mma_slice(const __bf16* Asm, const __bf16* Bsm, int wm, int wn,
                          f32x4 (&acc)[FM][FN]) {
#pragma unroll
  for (int ks = 0; ks < BKT / 32; ++ks) {
    bf16x8 a_frag[FM], b_frag[FN];
    load_frags<FM, FN, BKT, SWZ>(Asm, Bsm, wm, wn, ks, a_frag, b_frag);
    mma_frags<FM, FN>(a_frag, b_frag, acc);
  }
}

// ---- epilogue -----------------------------------------------------------------
// bias + activation, bf16 store with bounds check, over an FM×FN grid of
// 16×16 accumulator fragments. frag_row(m) / frag_col(n) give the C row / col
// of fragment (m, n)'s top-left element, so one body serves both the plain
// contiguous wave tile (store_tile) and the 8-phase kernel's interleaved
// fragments. (Kept as one loop nest, not a per-fragment function: the latter
// makes the compiler hoist the row math across n, which changes the epilogue's
// block layout and wait counts for no gain.)
template <int ACT, bool HAS_BIAS, int FM, int FN, class RowOf, class ColOf>
DEV_INLINE void store_frags(const f32x4 (&acc)[FM][FN],
                            const float* __restrict__ bias,
                            __bf16* __restrict__ C, int M, int N,
                            RowOf frag_row, ColOf frag_col) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int m = 0; m < FM; ++m) {
#pragma unroll
    for (int n = 0; n < FN; ++n) {
      int col = frag_col(n) + (lane & 15);
      if (col >= N) continue;
      float b = HAS_BIAS ? bias[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = frag_row(m) + (lane >> 4) * 4 + r;
        if (row >= M) continue;
        C[(int64_t)row * N + col] = (__bf16)apply_act(acc[m][n][r] + b, ACT);
      }
    }
  }
}

// A wave's contiguous FM×FN fragment grid whose top-left is C[wrow][wcol].
template <int ACT, bool HAS_BIAS, int FM, int FN>
DEV_INLINE void store_tile(const f32x4 (&acc)[FM][FN],
                           const float* __restrict__ bias,
                           __bf16* __restrict__ C, int M, int N, int wrow,
                           int wcol) {
  store_frags<ACT, HAS_BIAS>(
      acc, bias, C, M, N, [&](int m) { return wrow + m * 16; },
      [&](int n) { return wcol + n * 16; });
}

// ---- host side ----------------------------------------------------------------
// Turns the runtime (act, bias != null) into template arguments:
// f(std::integral_constant<int, ACT>, std::bool_constant<HAS_BIAS>).
template <class F>
static void dispatch_epilogue(int act, bool has_bias, F&& f) {
  auto with_act = [&](auto a) {
    if (has_bias) f(a, std::true_type{});
    else f(a, std::false_type{});
  };
  switch (act) {
    case ACT_RELU: with_act(std::integral_constant<int, ACT_RELU>{}); break;
    case ACT_GELU: with_act(std::integral_constant<int, ACT_GELU>{}); break;
    case ACT_SILU: with_act(std::integral_constant<int, ACT_SILU>{}); break;
    default: with_act(std::integral_constant<int, ACT_NONE>{}); break;
  }
}

// One block per BMT×BNT output tile; every GEMM kernel takes the same
// (A, Bt, bias, C, M, N, K, tiles_n) and derives its tile from xcd_block_id().
template <int BMT, int BNT, class Kernel>
static void launch_tiles(Kernel kernel, int threads, size_t lds_bytes,
                         const GemmArgs& g) {
  int tiles_n = cdiv(g.N, BNT);
  hipLaunchKernelGGL(kernel, dim3(cdiv(g.M, BMT) * tiles_n), dim3(threads),
                     lds_bytes, g.stream, (const __bf16*)g.A,
                     (const __bf16*)g.Bt, g.bias, (__bf16*)g.C, g.M, g.N, g.K,
                     tiles_n);
}

// gemm_8phase.hip; bm is 256 or 128. Returns a GemmStatus.
int launch_gemm_bf16_8p(const GemmArgs& g, int bm, bool swz);
