// bf16 MFMA GEMM with fused bias+activation epilogue — the inference
// processor's matmul (replaces the reference's python-processor escape hatch
// for ML, reference processor/python.rs:47-98, with a native CDNA4 path).
//
// Five kernel bodies on the building blocks of gemm_common.h; each is its
// staging form and its loop schedule, nothing else:
//   gemm_direct_kernel  direct-to-LDS, single buffer     (variants 0, 7, 6)
//   gemm_swz_kernel     register-staged, XOR-swizzled    (variants 8, 12, 11)
//   gemm_k64p_kernel    swizzled + register prefetch     (variant 10)
//   gemm_k64d_kernel    swizzled + two LDS buffers       (variant 9)
//   gemm_2p_kernel      direct-to-LDS, two LDS buffers   (variant 3)
// The 256²-tile 8-phase pipeline (variants 1, 2, 4, 5) is gemm_8phase.hip.
#include "gemm_common.h"

#define GEMM_THREADS 256

// This block's tile origin and this wave's origin inside it (waves 2-wide in
// N, each owning FM×FN fragments).
template <int BMT, int BNT, int FM, int FN>
struct TilePos {
  int row0, col0, wm, wn;
  DEV_INLINE explicit TilePos(int tiles_n) {
    const int bid = xcd_block_id();
    row0 = (bid / tiles_n) * BMT;
    col0 = (bid % tiles_n) * BNT;
    const int wid = threadIdx.x >> 6;
    wm = (wid >> 1) * (FM * 16);
    wn = (wid & 1) * (FN * 16);
  }
};

// ---- direct-to-LDS, single buffer ---------------------------------------------
// TILE×TILE output, 4 waves in 2×2, global_load_lds staging into linear
// [TILE][BKT] LDS, two barriers per K slice. Instantiations:
//  <128, 32, 2>  the baseline tile (8 KiB/operand, 2 stage steps per wave).
//  <128, 64, 2>  a 64-deep K slice: halves the K-loop trip count (and the
//                __syncthreads per K) for the K=768-class BERT shapes where
//                BK=32 leaves ~300 TF on the table vs hipBLASLt (profiles
//                r06/r17). LDS 16 KiB/operand (32 KiB total → still 2
//                blocks/CU). Its 128 B row stride bank-aliases — see
//                gemm_swz_kernel.
//  <64, 32, 4>   "skinny": for narrow outputs (N ≤ a few hundred: the MLP
//                anomaly scorer's 32→256→256 chain) the 128² tile yields only
//                tiles_m×⌈N/128⌉ workgroups — 128 blocks at [8192,256], half
//                the 256 CUs idle. The 64² tile quadruples the grid so the
//                chip fills; LDS is 8 KiB → high occupancy hides the short K
//                loop. Each wave owns a 32×32 quadrant = 2×2 fragments.
template <int TILE, int BKT, int OCC, int ACT, bool HAS_BIAS>
__global__ __launch_bounds__(GEMM_THREADS, OCC)
void gemm_direct_kernel(const __bf16* __restrict__ A,   // [M,K]
                        const __bf16* __restrict__ Bt,  // [N,K]
                        const float* __restrict__ bias, // [N] or null
                        __bf16* __restrict__ C,         // [M,N]
                        int M, int N, int K, int tiles_n) {
  constexpr int F = TILE / 32;
  const TilePos<TILE, TILE, F, F> t(tiles_n);
  __shared__ __bf16 Asm[TILE * BKT];
  __shared__ __bf16 Bsm[TILE * BKT];
  f32x4 acc[F][F] = {};

  for (int k0 = 0; k0 < K; k0 += BKT) {
    stage_direct<TILE, BKT, GEMM_THREADS>(A, Bt, t.row0, t.col0, M, N, K, k0,
                                          Asm, Bsm);
    __syncthreads();  // drains vmcnt → LDS tiles ready
    mma_slice<F, F, BKT, false>(Asm, Bsm, t.wm, t.wn, acc);
    __syncthreads();
  }
  store_tile<ACT, HAS_BIAS>(acc, bias, C, M, N, t.row0 + t.wm, t.col0 + t.wn);
}

// ---- register-staged, XOR-swizzled BK=64 --------------------------------------
// The BK=64 tile with the bank-conflict-free layout (see swz_load). TILE=128:
// 4 waves, the dispatched K%64==0 kernel; OCC=3 is the occupancy-3 A/B of the
// same kernel (more inter-block latency overlap if the register allocator
// fits 3 blocks; measured identical — the allocator is already there).
// TILE=256 ("k64w"): 8 waves each owning a 64×128 fragment grid, one block
// per CU, 64 KB LDS. Quadruple the MFLOP-per-byte of the 128×128 tile: A
// re-read N/256 times and B re-read M/256 times, which at short-K fc shapes
// (fc1: M8192 N3072 K768) halves the L2/MALL traffic that bounds the 128×128
// kernel — but nothing overlaps the barriers at occupancy 1 (profiles r2-17).
template <int TILE, int OCC, int ACT, bool HAS_BIAS>
__global__ __launch_bounds__(2 * TILE, OCC)
void gemm_swz_kernel(const __bf16* __restrict__ A,
                     const __bf16* __restrict__ Bt,
                     const float* __restrict__ bias,
                     __bf16* __restrict__ C,
                     int M, int N, int K, int tiles_n) {
  constexpr int FN = TILE / 32;
  const TilePos<TILE, TILE, 4, FN> t(tiles_n);
  __shared__ __bf16 Asm[TILE * SWZ_BK];
  __shared__ __bf16 Bsm[TILE * SWZ_BK];
  f32x4 acc[4][FN] = {};

  for (int k0 = 0; k0 < K; k0 += SWZ_BK) {
    u32x4 va[SWZ_STEPS], vb[SWZ_STEPS];
    swz_load<TILE>(A, Bt, t.row0, t.col0, M, N, K, k0, va, vb);
    swz_write<TILE>(Asm, Bsm, va, vb);
    __syncthreads();
    mma_slice<4, FN, SWZ_BK, true>(Asm, Bsm, t.wm, t.wn, acc);
    __syncthreads();
  }
  store_tile<ACT, HAS_BIAS>(acc, bias, C, M, N, t.row0 + t.wm, t.col0 + t.wn);
}

// ---- register-prefetch swizzled BK=64 -----------------------------------------
// gemm_swz_kernel<128> with the NEXT k-slice's global loads issued right after
// the LDS-write barrier, so their (L2/MALL) latency overlaps the MFMA block.
// Unlike the double-buffered k64d (two LDS buffers: register pressure killed
// it) this keeps ONE LDS buffer and double-buffers only the 16 staging VGPRs.
// Measured 68 µs vs 64 at fc1: occupancy 2 already overlaps another block's
// loads across the barrier (profiles r2-17).
template <int ACT, bool HAS_BIAS>
__global__ __launch_bounds__(GEMM_THREADS, 2)
void gemm_k64p_kernel(const __bf16* __restrict__ A,
                      const __bf16* __restrict__ Bt,
                      const float* __restrict__ bias,
                      __bf16* __restrict__ C,
                      int M, int N, int K, int tiles_n) {
  const TilePos<128, 128, 4, 4> t(tiles_n);
  __shared__ __bf16 Asm[128 * SWZ_BK];
  __shared__ __bf16 Bsm[128 * SWZ_BK];
  f32x4 acc[4][4] = {};

  u32x4 va[SWZ_STEPS], vb[SWZ_STEPS];
  swz_load<128>(A, Bt, t.row0, t.col0, M, N, K, 0, va, vb);
  for (int k0 = 0; k0 < K; k0 += SWZ_BK) {
    swz_write<128>(Asm, Bsm, va, vb);
    __syncthreads();
    const int k1 = k0 + SWZ_BK;
    if (k1 < K)  // prefetch next slice; latency hides under the MFMAs
      swz_load<128>(A, Bt, t.row0, t.col0, M, N, K, k1, va, vb);
    mma_slice<4, 4, SWZ_BK, true>(Asm, Bsm, t.wm, t.wn, acc);
    __syncthreads();
  }
  store_tile<ACT, HAS_BIAS>(acc, bias, C, M, N, t.row0 + t.wm, t.col0 + t.wn);
}

// ---- double-buffered swizzled BK=64 -------------------------------------------
// Same tile/swizzle as gemm_swz_kernel<128> but two LDS buffers: the NEXT
// K-slice's global loads are issued before the current slice's MFMAs so HBM
// latency hides under compute, and the loop needs ONE __syncthreads per slice
// instead of two. LDS 2×32 KiB — still 2 blocks/CU. NEGATIVE result: holding
// the next slice in registers under the MFMAs costs enough VGPRs to lose the
// gain (fc1 GELU 456 TF vs 584 single-buffered; profiles r2-12).
template <int ACT, bool HAS_BIAS>
__global__ __launch_bounds__(GEMM_THREADS, 2)
void gemm_k64d_kernel(const __bf16* __restrict__ A,
                      const __bf16* __restrict__ Bt,
                      const float* __restrict__ bias,
                      __bf16* __restrict__ C,
                      int M, int N, int K, int tiles_n) {
  const TilePos<128, 128, 4, 4> t(tiles_n);
  __shared__ __bf16 Asm[2][128 * SWZ_BK];
  __shared__ __bf16 Bsm[2][128 * SWZ_BK];
  f32x4 acc[4][4] = {};

  u32x4 va[SWZ_STEPS], vb[SWZ_STEPS];
  swz_load<128>(A, Bt, t.row0, t.col0, M, N, K, 0, va, vb);
  swz_write<128>(Asm[0], Bsm[0], va, vb);
  __syncthreads();

  int buf = 0;
  for (int k0 = 0; k0 < K; k0 += SWZ_BK) {
    const bool has_next = k0 + SWZ_BK < K;
    if (has_next)  // hides under the MFMAs
      swz_load<128>(A, Bt, t.row0, t.col0, M, N, K, k0 + SWZ_BK, va, vb);
    mma_slice<4, 4, SWZ_BK, true>(Asm[buf], Bsm[buf], t.wm, t.wn, acc);
    if (has_next) swz_write<128>(Asm[buf ^ 1], Bsm[buf ^ 1], va, vb);
    buf ^= 1;
    __syncthreads();
  }
  store_tile<ACT, HAS_BIAS>(acc, bias, C, M, N, t.row0 + t.wm, t.col0 + t.wn);
}

// ---- 2-phase double-buffered BK=32 --------------------------------------------
// T3-minimal prefetch (guide §5.5): stage K-tile t+1 into the other LDS
// buffer while computing tile t; ONE vmcnt(0)+barrier per K-tile AFTER the
// MFMAs so the staging loads overlap compute. Pays at short-K / latency-bound
// shapes (BERT: K=768) where block occupancy can't hide the HBM latency.
template <int ACT, bool HAS_BIAS>
__global__ __launch_bounds__(GEMM_THREADS, 2)
void gemm_2p_kernel(const __bf16* __restrict__ A,
                    const __bf16* __restrict__ Bt,
                    const float* __restrict__ bias,
                    __bf16* __restrict__ C,
                    int M, int N, int K, int tiles_n) {
  constexpr int BK = 32;
  const TilePos<128, 128, 4, 4> t(tiles_n);
  __shared__ __bf16 Asm[2][128 * BK];
  __shared__ __bf16 Bsm[2][128 * BK];
  const int NT = K / BK;

  auto stage = [&](int buf, int kt) {
    stage_direct<128, BK, GEMM_THREADS>(A, Bt, t.row0, t.col0, M, N, K,
                                        kt * BK, Asm[buf], Bsm[buf]);
  };

  f32x4 acc[4][4] = {};

  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)");
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();

  int cur = 0;
  for (int kt = 0; kt < NT; ++kt) {
    if (kt + 1 < NT) stage(cur ^ 1, kt + 1);  // prefetch next tile
    bf16x8 a_frag[4], b_frag[4];
    load_frags<4, 4, BK, false>(Asm[cur], Bsm[cur], t.wm, t.wn, 0, a_frag,
                                b_frag);
    asm volatile("s_waitcnt lgkmcnt(0)");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    mma_frags<4, 4>(a_frag, b_frag, acc);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    // next tile must be resident before anyone reads buf cur^1
    asm volatile("s_waitcnt vmcnt(0)");
    __builtin_amdgcn_s_barrier();
    cur ^= 1;
  }
  store_tile<ACT, HAS_BIAS>(acc, bias, C, M, N, t.row0 + t.wm, t.col0 + t.wn);
}

// ---- the one launch entry -----------------------------------------------------
// Each variant's kernel reads whole BK-wide K slices: K must be a multiple of
// its BK (the pipelined ones also need a minimum slice count).
extern "C" int launch_gemm_bf16(int variant, const GemmArgs* args) {
  const GemmArgs& g = *args;
  switch (variant) {
    case GEMM_8P256: return launch_gemm_bf16_8p(g, 256, false);
    case GEMM_8P256S: return launch_gemm_bf16_8p(g, 256, true);
    case GEMM_8P128: return launch_gemm_bf16_8p(g, 128, false);
    case GEMM_8P128S: return launch_gemm_bf16_8p(g, 128, true);
    case GEMM_BK32: case GEMM_SKINNY:  // K % 32: the bindings' argument check
      break;
    case GEMM_2P:
      if (g.K % 32 != 0 || g.K / 32 < 2) return GEMM_BAD_SHAPE;
      break;
    case GEMM_K64: case GEMM_K64S: case GEMM_K64D: case GEMM_K64P:
    case GEMM_K64W: case GEMM_K64S3:
      if (g.K % 64 != 0) return GEMM_BAD_SHAPE;
      break;
    default: return GEMM_BAD_VARIANT;
  }
  dispatch_epilogue(g.act, g.bias != nullptr, [&](auto act, auto has_bias) {
    constexpr int ACT = decltype(act)::value;
    constexpr bool HB = decltype(has_bias)::value;
    constexpr int T = GEMM_THREADS;
    switch (variant) {
      case GEMM_BK32:
        launch_tiles<128, 128>(gemm_direct_kernel<128, 32, 2, ACT, HB>, T, 0, g);
        break;
      case GEMM_K64:
        launch_tiles<128, 128>(gemm_direct_kernel<128, 64, 2, ACT, HB>, T, 0, g);
        break;
      case GEMM_SKINNY:
        launch_tiles<64, 64>(gemm_direct_kernel<64, 32, 4, ACT, HB>, T, 0, g);
        break;
      case GEMM_K64S:
        launch_tiles<128, 128>(gemm_swz_kernel<128, 2, ACT, HB>, T, 0, g);
        break;
      case GEMM_K64S3:
        launch_tiles<128, 128>(gemm_swz_kernel<128, 3, ACT, HB>, T, 0, g);
        break;
      case GEMM_K64W:
        launch_tiles<256, 256>(gemm_swz_kernel<256, 1, ACT, HB>, 512, 0, g);
        break;
      case GEMM_K64P:
        launch_tiles<128, 128>(gemm_k64p_kernel<ACT, HB>, T, 0, g);
        break;
      case GEMM_K64D:
        launch_tiles<128, 128>(gemm_k64d_kernel<ACT, HB>, T, 0, g);
        break;
      case GEMM_2P:
        launch_tiles<128, 128>(gemm_2p_kernel<ACT, HB>, T, 0, g);
        break;
    }
  });
  return GEMM_OK;
}
