// Fused bf16 attention for the BERT inference processor: softmax(Q·K^T)·V
// in ONE kernel, one workgroup per (batch, head). Sized for encoder shapes
// (S=128, D=64: BERT-base). MFMA 16x16x32 for both QK^T and P·V; the softmax
// runs entirely in registers (row max/sum via quarter-wave shfl_xor over the
// MFMA C-fragment layout: col=lane&15, row=(lane>>4)*4+reg).
//
// LDS: K [S][D+4] + V^T [D][S+4] staged once (padded rows: +4 bf16 = 2-bank
// row stride → conflict-free ds_read_b128), P bf16 [32][S+4] per wave.
#include "common.h"
#include "kernels_api.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define ATTN_THREADS 256

// Variable-length form (MASKED = true): `lens[b]` (clamped to [0, S]) is the
// number of valid keys AND valid query rows of batch row b. It is uniform per
// workgroup and held in an SGPR, so the decisions on it are scalar branches:
// score fragments, P·V K-steps, KV tiles, staging chunks and whole waves /
// Q blocks past L are skipped, not predicated. Only the fragment that
// straddles L selects per lane (score → -inf, P → 0). A staged K / Vᵗ row
// ≥ L is written to the LDS as 0 by a select (whatever was loaded for it is
// dropped), so what rows ≥ L hold in memory, NaN included, meets no multiply. Output rows ≥ L are written as +0.
// MASKED = false compiles to the code this file had before lens existed.
__device__ __forceinline__ int clamp_len(const int* __restrict__ lens, int b,
                                         int S) {
  int l = lens[b];
  // readfirstlane: keep the clamped value in an SGPR (the compiler clamps
  // with a vector med3 otherwise, and every branch on L turns into a
  // v_cmp + vcc branch)
  return __builtin_amdgcn_readfirstlane(l < 0 ? 0 : (l > S ? S : l));
}

// +0 to rows [row0, row0+32) ∩ [0, S) of one head's D=64 output columns:
// one wave, 16-byte stores (8 rows × 8 lanes per pass).
__device__ __forceinline__ void zero_rows32(__bf16* __restrict__ Ob, int ldo,
                                            int row0, int S, int lane) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int row = row0 + j * 8 + (lane >> 3);
    if (row < S)
      *(uint4*)(Ob + (int64_t)row * ldo + (lane & 7) * 8) =
          make_uint4(0u, 0u, 0u, 0u);
  }
}

// Strided layout: row s of head h in batch b lives at
// base + ((int64_t)b*S + s)*ld + h*D. With Hd=1/ld=D this is the packed
// [BH, S, D] layout; with Hd=H/ld=3*H*D the kernel reads q/k/v DIRECTLY out
// of the [B,S,3,H,D] QKV-projection tensor (no transpose copies), and with
// ldo=H*D writes O back in [B,S,H*D] so the next linear consumes it as-is.
template <int S, int D, int PAD = 4, bool MASKED = false>
__global__ __launch_bounds__(ATTN_THREADS, 1)
void attention_kernel(const __bf16* __restrict__ Q,
                      const __bf16* __restrict__ K,
                      const __bf16* __restrict__ V,
                      __bf16* __restrict__ O, float scale,
                      int ldq, int ldo, int Hd,
                      const int* __restrict__ lens) {
  constexpr int DP = D + PAD;  // padded row strides (bank spread)
  constexpr int SP = S + PAD;
  constexpr int QROWS = 32;   // q rows per wave
  constexpr int NWAVE = ATTN_THREADS / WAVE;
  static_assert(S == NWAVE * QROWS, "one block covers all S rows");
  static_assert(!MASKED || D == 64, "zero_rows32 writes 64 columns");

  extern __shared__ char smem[];
  __bf16* K_lds = (__bf16*)smem;                       // [S][DP]
  __bf16* Vt_lds = K_lds + S * DP;                     // [D][SP]
  __bf16* P_lds = Vt_lds + D * SP;                     // [NWAVE][QROWS][SP]

  const int bh = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  // the masked form branches on the wave's rows: make the wave id provably
  // uniform there (the unmasked form keeps the plain shift)
  const int wid =
      MASKED ? __builtin_amdgcn_readfirstlane(tid >> 6) : (tid >> 6);
  const int b = bh / Hd, h = bh % Hd;
  const __bf16* Qb = Q + (int64_t)b * S * ldq + h * D;
  const __bf16* Kb = K + (int64_t)b * S * ldq + h * D;
  const __bf16* Vb = V + (int64_t)b * S * ldq + h * D;
  __bf16* Ob = O + (int64_t)b * S * ldo + h * D;

  // ---- stage K and V^T (coalesced global reads) -----------------------------
  // Masked: 64-row chunks, a chunk past L skipped on a scalar branch; all
  // loads are issued before the first LDS write (a loop bounded by L would
  // wait for each pair in turn), and chunk 0's before L itself is read, so
  // the lens load hides behind them. Every row < S is valid memory, so a
  // row ≥ L is loaded like any other and replaced by 0 with a select before
  // it reaches the LDS.
  // L valid keys/rows; K-step granularity: rows [L, L32) are the last P·V
  // K-step's tail (staged as 0, P stored as 0), rows ≥ L32 are never read.
  int L = S;
  if constexpr (MASKED) {
    constexpr int CH = 64, NCH = S / CH, NIT = CH * D / 2 / ATTN_THREADS;
    uint32_t kv[NCH][NIT], vv[NCH][NIT];
    auto load_chunk = [&](int c) {
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        int i = c * CH * D / 2 + it * ATTN_THREADS + tid;
        int s = (i * 2) / D, d = (i * 2) % D;
        kv[c][it] = *(const uint32_t*)(Kb + (int64_t)s * ldq + d);
        vv[c][it] = *(const uint32_t*)(Vb + (int64_t)s * ldq + d);
      }
    };
    load_chunk(0);
    L = clamp_len(lens, b, S);
    if (L == 0) {  // whole block: nothing to attend to
      zero_rows32(Ob, ldo, wid * QROWS, S, lane);
      return;
    }
#pragma unroll
    for (int c = 1; c < NCH; ++c)
      if (c * CH < L) load_chunk(c);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (c * CH >= L) break;
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        int i = c * CH * D / 2 + it * ATTN_THREADS + tid;
        int s = (i * 2) / D, d = (i * 2) % D;
        *(uint32_t*)(&K_lds[s * DP + d]) = s < L ? kv[c][it] : 0u;
        uint32_t vz = s < L ? vv[c][it] : 0u;
        Vt_lds[d * SP + s] = ((const __bf16*)&vz)[0];
        Vt_lds[(d + 1) * SP + s] = ((const __bf16*)&vz)[1];
      }
    }
  } else {
    for (int i = tid; i < S * D / 2; i += ATTN_THREADS) {
      // 2 elements per thread via 32-bit loads
      int s = (i * 2) / D, d = (i * 2) % D;
      uint32_t kv = *(const uint32_t*)(Kb + (int64_t)s * ldq + d);
      *(uint32_t*)(&K_lds[s * DP + d]) = kv;
      uint32_t vv = *(const uint32_t*)(Vb + (int64_t)s * ldq + d);
      __bf16 v0 = ((const __bf16*)&vv)[0], v1 = ((const __bf16*)&vv)[1];
      Vt_lds[d * SP + s] = v0;
      Vt_lds[(d + 1) * SP + s] = v1;
    }
  }
  const int L32 = MASKED ? ((L + 31) & ~31) : S;

  // ---- Q fragments (held in registers for the whole kernel) ----------------
  const int q0 = wid * QROWS;
  const int fr = lane & 15;
  const int fk = (lane >> 4) * 8;
  bf16x8 q_frag[2][D / 32];
#pragma unroll
  for (int am = 0; am < 2; ++am)
#pragma unroll
    for (int ks = 0; ks < D / 32; ++ks)
      q_frag[am][ks] = *(const bf16x8*)(
          Qb + (int64_t)(q0 + am * 16 + fr) * ldq + ks * 32 + fk);

  __syncthreads();  // K/Vt staged

  if constexpr (MASKED) {
    if (q0 >= L) {  // all 32 query rows of this wave are padding
      zero_rows32(Ob, ldo, q0, S, lane);
      return;
    }
  }

  // ---- scores = Q·K^T : acc[am][nf] covers rows 32 × cols S -----------------
  constexpr int NF = S / 16;
  f32x4 acc[2][NF] = {};
#pragma unroll
  for (int nf = 0; nf < NF; ++nf) {
    if (MASKED && nf * 16 >= L) continue;  // scalar: fragment past L
#pragma unroll
    for (int ks = 0; ks < D / 32; ++ks) {
      bf16x8 b_frag =
          *(const bf16x8*)(&K_lds[(nf * 16 + fr) * DP + ks * 32 + fk]);
#pragma unroll
      for (int am = 0; am < 2; ++am)
        acc[am][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            q_frag[am][ks], b_frag, acc[am][nf], 0, 0, 0);
    }
  }

  // ---- in-register softmax over each score row ------------------------------
  // lane holds, for fixed (am, r), one value per nf → row = quarter-wave's
  // 16 lanes × NF regs. reduce: per-lane over nf, then shfl_xor {1,2,4,8}.
  __bf16* Pw = P_lds + wid * QROWS * SP;
#pragma unroll
  for (int am = 0; am < 2; ++am) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      // masked: a column ≥ L is -inf by SELECT (its score is 0 from the
      // zero fill, or the untouched 0 of a skipped fragment; never
      // arithmetic on what memory held). Column 0 is valid (L ≥ 1), so a
      // valid row's rmax is finite.
      float rmax = -INFINITY;
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) {
        float sc = acc[am][nf][r] * scale;
        rmax = fmaxf(rmax, (!MASKED || nf * 16 + fr < L) ? sc : -INFINITY);
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1)
        rmax = fmaxf(rmax, __shfl_xor(rmax, off, 64));
      float rsum = 0.f;
      float p[NF];
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) {
        if (MASKED && nf * 16 >= L) {  // scalar: no exp for a skipped fragment
          p[nf] = 0.f;
          continue;
        }
        // the valid lanes evaluate the very expression of the unmasked form
        float e = __expf(acc[am][nf][r] * scale - rmax);
        p[nf] = (!MASKED || nf * 16 + fr < L) ? e : 0.f;
        rsum += p[nf];
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1)
        rsum += __shfl_xor(rsum, off, 64);
      float inv = 1.f / rsum;
      int prow = am * 16 + (lane >> 4) * 4 + r;
#pragma unroll
      for (int nf = 0; nf < NF; ++nf)
        if (!MASKED || nf * 16 < L32)  // P columns [L, L32) are stored as 0
          Pw[prow * SP + nf * 16 + fr] = (__bf16)(p[nf] * inv);
    }
  }
  // P is consumed only by this wave; compiler orders the LDS ops.

  // ---- out = P·V ------------------------------------------------------------
  constexpr int ND = D / 16;
  f32x4 acc2[2][ND] = {};
#pragma unroll
  for (int ks = 0; ks < S / 32; ++ks) {
    if (MASKED && ks * 32 >= L) continue;  // scalar: K-step past L
    bf16x8 a_frag[2];
#pragma unroll
    for (int am = 0; am < 2; ++am)
      a_frag[am] = *(const bf16x8*)(&Pw[(am * 16 + fr) * SP + ks * 32 + fk]);
#pragma unroll
    for (int nd = 0; nd < ND; ++nd) {
      bf16x8 b_frag =
          *(const bf16x8*)(&Vt_lds[(nd * 16 + fr) * SP + ks * 32 + fk]);
#pragma unroll
      for (int am = 0; am < 2; ++am)
        acc2[am][nd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a_frag[am], b_frag, acc2[am][nd], 0, 0, 0);
    }
  }

  // ---- write O --------------------------------------------------------------
#pragma unroll
  for (int am = 0; am < 2; ++am)
#pragma unroll
    for (int nd = 0; nd < ND; ++nd)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = q0 + am * 16 + (lane >> 4) * 4 + r;
        int col = nd * 16 + fr;
        // a padded row inside a partly valid wave: +0 by select (its
        // accumulator may hold NaN from its own garbage q row)
        Ob[(int64_t)row * ldo + col] =
            (!MASKED || row < L) ? (__bf16)acc2[am][nd][r] : (__bf16)0.f;
      }
}

// ---- flash-tiled attention: S > 128 (KV streamed in 64-col tiles) ----------
// One workgroup per (batch·head, 128-row Q block); 4 waves × 32 q rows each
// (same fragment layout as the full-S kernel). KV tiles of 64 columns are
// staged in LDS; softmax is the running-rescale form (m/l state per row in
// registers): o ← o·e^{m−m'} + P·Vᵗ, l ← l·e^{m−m'} + Σp. Covers any
// S % 64 == 0 at D=64; the S=128 full-S kernel stays the BERT fast path.
#define FA_QROWS 32
#define FA_KT 64   // kv tile columns
#define FA_PAD 8

template <int D, bool MASKED = false>
__global__ __launch_bounds__(ATTN_THREADS, 2)
void attention_flash_kernel(const __bf16* __restrict__ Q,
                            const __bf16* __restrict__ K,
                            const __bf16* __restrict__ V,
                            __bf16* __restrict__ O, float scale, int S,
                            int ldq, int ldo, int Hd, int qblocks,
                            const int* __restrict__ lens) {
  static_assert(!MASKED || D == 64, "zero_rows32 writes 64 columns");
  constexpr int DP = D + FA_PAD;
  constexpr int KTP = FA_KT + FA_PAD;
  __shared__ __bf16 K_lds[FA_KT * DP];        // kv tile, row-major [64][DP]
  __shared__ __bf16 Vt_lds[D * KTP];          // tile of Vᵗ [D][64+pad]
  __shared__ __bf16 P_lds[4][FA_QROWS * KTP]; // per-wave P [32][64+pad]

  const int bh = blockIdx.x / qblocks;
  const int qb = blockIdx.x % qblocks;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid =
      MASKED ? __builtin_amdgcn_readfirstlane(tid >> 6) : (tid >> 6);
  const int b = bh / Hd, h = bh % Hd;
  const __bf16* Qb = Q + (int64_t)b * S * ldq + h * D;
  const __bf16* Kb = K + (int64_t)b * S * ldq + h * D;
  const __bf16* Vb = V + (int64_t)b * S * ldq + h * D;
  __bf16* Ob = O + (int64_t)b * S * ldo + h * D;

  const int q0 = qb * 128 + wid * FA_QROWS;   // this wave's first q row
  const int fr = lane & 15;
  const int fk = (lane >> 4) * 8;

  // L valid keys/rows. The KV loop ends at the tile that holds key L-1, so
  // every processed tile has a valid first column and the running max of a
  // valid row is finite from the first tile on.
  int L = S;
  if constexpr (MASKED) {
    L = clamp_len(lens, b, S);
    if (qb * 128 >= L) {  // whole Q block is padding (block-uniform: no
      zero_rows32(Ob, ldo, q0, S, lane);  // barrier has been reached yet)
      return;
    }
  }
  const int kv_end = MASKED ? ((L + FA_KT - 1) / FA_KT) * FA_KT : S;
  // a wave whose 32 rows are all padding keeps staging and the barriers of
  // its block but does no MFMA and no softmax
  const bool wave_live = !MASKED || q0 < L;

  // Q fragments in registers for the wave's 32 rows (rows ≥ S clamp to S-1;
  // their outputs are never stored)
  bf16x8 q_frag[2][D / 32];
#pragma unroll
  for (int am = 0; am < 2; ++am)
#pragma unroll
    for (int ks = 0; ks < D / 32; ++ks) {
      int row = q0 + am * 16 + fr;
      row = row < S ? row : S - 1;
      q_frag[am][ks] =
          *(const bf16x8*)(Qb + (int64_t)row * ldq + ks * 32 + fk);
    }

  // running state: per (am, r) row of this lane's quarter
  float m_run[2][4], l_run[2][4];
  f32x4 o_acc[2][D / 16] = {};
#pragma unroll
  for (int am = 0; am < 2; ++am)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      m_run[am][r] = -INFINITY;
      l_run[am][r] = 0.f;
    }

  for (int kt = 0; kt < kv_end; kt += FA_KT) {
    // stage K tile + Vᵗ tile (cooperative, 2 bf16 per thread per step);
    // masked: a row ≥ L of the last tile loads row L-1 (valid memory; the
    // loads stay unconditional and issue back to back) and is replaced by 0
    // with a select before it reaches the LDS
    for (int i = tid; i < FA_KT * D / 2; i += ATTN_THREADS) {
      int s = (i * 2) / D, d = (i * 2) % D;
      const bool live = !MASKED || kt + s < L;
      const int sl = live ? kt + s : L - 1;
      uint32_t kv = *(const uint32_t*)(Kb + (int64_t)sl * ldq + d);
      kv = live ? kv : 0u;
      *(uint32_t*)(&K_lds[s * DP + d]) = kv;
      uint32_t vv = *(const uint32_t*)(Vb + (int64_t)sl * ldq + d);
      vv = live ? vv : 0u;
      __bf16 v0 = ((const __bf16*)&vv)[0], v1 = ((const __bf16*)&vv)[1];
      Vt_lds[d * KTP + s] = v0;
      Vt_lds[(d + 1) * KTP + s] = v1;
    }
    __syncthreads();

    if (wave_live) {
      // scores tile: [32 q rows][64 kv cols] per wave = acc[2][4] frags
      f32x4 acc[2][FA_KT / 16] = {};
#pragma unroll
      for (int nf = 0; nf < FA_KT / 16; ++nf) {
        if (MASKED && kt + nf * 16 >= L) continue;  // scalar: fragment past L
#pragma unroll
        for (int ks = 0; ks < D / 32; ++ks) {
          bf16x8 b_frag =
              *(const bf16x8*)(&K_lds[(nf * 16 + fr) * DP + ks * 32 + fk]);
#pragma unroll
          for (int am = 0; am < 2; ++am)
            acc[am][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                q_frag[am][ks], b_frag, acc[am][nf], 0, 0, 0);
        }
      }

      // running softmax + stage P
      __bf16* Pw = P_lds[wid];
#pragma unroll
      for (int am = 0; am < 2; ++am) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float tmax = -INFINITY;
#pragma unroll
          for (int nf = 0; nf < FA_KT / 16; ++nf) {
            // masked: a column ≥ L is -inf by SELECT, never by arithmetic
            // (per-lane selects only here: a scalar branch per row and
            // fragment costs more than the exp it would save)
            float sc = acc[am][nf][r] * scale;
            tmax = fmaxf(tmax, (!MASKED || kt + nf * 16 + fr < L) ? sc
                                                                  : -INFINITY);
          }
#pragma unroll
          for (int off = 1; off < 16; off <<= 1)
            tmax = fmaxf(tmax, __shfl_xor(tmax, off, 64));
          float m_new = fmaxf(m_run[am][r], tmax);
          float rescale = __expf(m_run[am][r] - m_new);
          float psum = 0.f;
          float p[FA_KT / 16];
#pragma unroll
          for (int nf = 0; nf < FA_KT / 16; ++nf) {
            // the valid lanes evaluate the very expression of the unmasked form
            float e = __expf(acc[am][nf][r] * scale - m_new);
            p[nf] = (!MASKED || kt + nf * 16 + fr < L) ? e : 0.f;
            psum += p[nf];
          }
#pragma unroll
          for (int off = 1; off < 16; off <<= 1)
            psum += __shfl_xor(psum, off, 64);
          l_run[am][r] = l_run[am][r] * rescale + psum;
          m_run[am][r] = m_new;
          // rescale accumulated output for this row
#pragma unroll
          for (int nd = 0; nd < D / 16; ++nd) o_acc[am][nd][r] *= rescale;
          int prow = am * 16 + (lane >> 4) * 4 + r;
#pragma unroll
          for (int nf = 0; nf < FA_KT / 16; ++nf)
            Pw[prow * KTP + nf * 16 + fr] = (__bf16)p[nf];
        }
      }
      // o += P·Vᵗ over this tile
#pragma unroll
      for (int ks = 0; ks < FA_KT / 32; ++ks) {
        if (MASKED && kt + ks * 32 >= L) continue;  // scalar: K-step past L
        bf16x8 a_frag[2];
#pragma unroll
        for (int am = 0; am < 2; ++am)
          a_frag[am] =
              *(const bf16x8*)(&Pw[(am * 16 + fr) * KTP + ks * 32 + fk]);
#pragma unroll
        for (int nd = 0; nd < D / 16; ++nd) {
          bf16x8 b_frag =
              *(const bf16x8*)(&Vt_lds[(nd * 16 + fr) * KTP + ks * 32 + fk]);
#pragma unroll
          for (int am = 0; am < 2; ++am)
            o_acc[am][nd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a_frag[am], b_frag, o_acc[am][nd], 0, 0, 0);
        }
      }
    }  // wave_live
    __syncthreads();  // K/Vt tiles reused next iteration
  }

  // epilogue: O = o / l
  const int c_col = lane & 15;
  const int c_row_base = (lane >> 4) * 4;
#pragma unroll
  for (int am = 0; am < 2; ++am)
#pragma unroll
    for (int nd = 0; nd < D / 16; ++nd)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = q0 + am * 16 + c_row_base + r;
        if (row >= S) continue;
        float inv = l_run[am][r] > 0.f ? 1.f / l_run[am][r] : 0.f;
        // a padded row (its own garbage q may have made it NaN) is +0 by
        // select
        Ob[(int64_t)row * ldo + nd * 16 + c_col] =
            (!MASKED || row < L) ? (__bf16)(o_acc[am][nd][r] * inv)
                                 : (__bf16)0.f;
      }
}

// ---- launchers --------------------------------------------------------------
// lens == nullptr picks the unmasked instantiations: the kernels every call
// without lengths has always run. lens is an int32 [B] device array whose
// values the host never reads (capturable; the kernels clamp to [0, S]).

// Full-S kernel at S=128, D=64 over the strided layout of attention_kernel.
template <int PAD, bool MASKED>
static void launch_full_s(const __bf16* Q, const __bf16* K, const __bf16* V,
                          __bf16* O, int BH, float scale, int ldq, int ldo,
                          int Hd, const int* lens, hipStream_t st) {
  constexpr int SS = 128, DD = 64;
  size_t lds = (SS * (DD + PAD) + DD * (SS + PAD) + 4 * 32 * (SS + PAD)) *
               sizeof(__bf16);
  static bool attr_set = false;  // one per instantiation
  if (!attr_set) {
    (void)hipFuncSetAttribute(
        (const void*)attention_kernel<SS, DD, PAD, MASKED>,
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr_set = true;
  }
  attention_kernel<SS, DD, PAD, MASKED><<<BH, ATTN_THREADS, lds, st>>>(
      Q, K, V, O, scale, ldq, ldo, Hd, lens);
}

template <int PAD>
static void launch_full_s(const __bf16* Q, const __bf16* K, const __bf16* V,
                          __bf16* O, int BH, float scale, int ldq, int ldo,
                          int Hd, const int* lens, hipStream_t st) {
  if (lens)
    launch_full_s<PAD, true>(Q, K, V, O, BH, scale, ldq, ldo, Hd, lens, st);
  else
    launch_full_s<PAD, false>(Q, K, V, O, BH, scale, ldq, ldo, Hd, nullptr,
                              st);
}

extern "C" int launch_attention_flash(const void* Q, const void* K,
                                      const void* V, void* O, int BH, int S,
                                      int D, float scale, int ldq, int ldo,
                                      int Hd, const int32_t* lens,
                                      hipStream_t st) {
  if (D != 64 || S % FA_KT != 0) return -1;
  int qblocks = (S + 127) / 128;
  if (lens)
    attention_flash_kernel<64, true><<<BH * qblocks, ATTN_THREADS, 0, st>>>(
        (const __bf16*)Q, (const __bf16*)K, (const __bf16*)V, (__bf16*)O,
        scale, S, ldq, ldo, Hd, qblocks, lens);
  else
    attention_flash_kernel<64, false><<<BH * qblocks, ATTN_THREADS, 0, st>>>(
        (const __bf16*)Q, (const __bf16*)K, (const __bf16*)V, (__bf16*)O,
        scale, S, ldq, ldo, Hd, qblocks, nullptr);
  return 0;
}

// Packed [B,H,S,D] q, k, v: BH independent (batch, head) rows, one head
// each (Hd = 1), so a masked call takes one length per ROW: lens has BH
// entries (the binding repeats each batch row's length H times).
extern "C" int launch_attention_bf16(const void* Q, const void* K,
                                     const void* V, void* O, int BH, int S,
                                     int D, float scale, const int32_t* lens,
                                     hipStream_t st) {
  if (S == 128 && D == 64) {
    // PAD=8: the +4 row pad measured ~590K LDS bank conflicts/dispatch;
    // +8 runs 28.8→19.8 µs at BERT shape (pad sweep, profiles r2)
    launch_full_s<8>((const __bf16*)Q, (const __bf16*)K, (const __bf16*)V,
                     (__bf16*)O, BH, scale, D, D, 1, lens, st);
    return 0;
  }
  // longer sequences (S % 64 == 0, D=64): flash-tiled kernel
  return launch_attention_flash(Q, K, V, O, BH, S, D, scale, D, D, 1, lens,
                                st);
}

// qkv: [B, S, 3, H, D] contiguous (the QKV linear's natural output);
// O: [B, S, H*D]. No transpose copies on either side. lens: B entries.
// pad: LDS row-padding in bf16 elements (pad sweep — NOTES r2: the +4
// layout still measured ~590K bank conflicts/dispatch).
extern "C" int launch_attention_qkv_bf16_pad(const void* QKV, void* O,
                                             int B, int H, int S, int D,
                                             float scale, int pad,
                                             const int32_t* lens,
                                             hipStream_t st) {
  const __bf16* base = (const __bf16*)QKV;
  const __bf16* kb = base + (int64_t)H * D;
  const __bf16* vb = base + (int64_t)2 * H * D;
  const int ld = 3 * H * D;
  if (!(S == 128 && D == 64))
    // longer sequences: flash-tiled kernel, same strided-QKV layout
    return launch_attention_flash(base, kb, vb, O, B * H, S, D, scale, ld,
                                  H * D, H, lens, st);
  __bf16* o = (__bf16*)O;
  switch (pad) {
    case 4:
      launch_full_s<4>(base, kb, vb, o, B * H, scale, ld, H * D, H, lens, st);
      break;
    case 16:
      launch_full_s<16>(base, kb, vb, o, B * H, scale, ld, H * D, H, lens, st);
      break;
    case 20:
      launch_full_s<20>(base, kb, vb, o, B * H, scale, ld, H * D, H, lens, st);
      break;
    default:
      launch_full_s<8>(base, kb, vb, o, B * H, scale, ld, H * D, H, lens, st);
  }
  return 0;
}

extern "C" int launch_attention_qkv_bf16(const void* QKV, void* O, int B,
                                         int H, int S, int D, float scale,
                                         hipStream_t st) {
  return launch_attention_qkv_bf16_pad(QKV, O, B, H, S, D, scale, 8, nullptr,
                                       st);
}
