// Fused bf16 attention for the BERT inference processor: softmax(Q·K^T)·V
// in ONE kernel. Two kernels, built from one set of device pieces:
//   attention_kernel        S=128, D=64 (BERT-base): one workgroup per
//                           (batch, head), K and Vᵗ staged once, P normalised
//                           before P·V;
//   attention_flash_kernel  S % 64 == 0, D=64: one workgroup per (batch·head,
//                           128-row Q block), KV streamed in 64-column tiles,
//                           running-rescale softmax.
// Both: 4 waves × 32 q rows, MFMA 16x16x32 for QK^T and P·V, the softmax
// entirely in registers (row max/sum via quarter-wave shfl_xor over the MFMA
// C-fragment layout: col=lane&15, row=(lane>>4)*4+reg), K [rows][D+pad] and
// V^T [D][rows+pad] in LDS (padded rows spread the banks for ds_read_b128),
// P bf16 [32][rows+pad] per wave.
//
// Strided layout: row s of head h in batch b lives at
// base + ((int64_t)b*S + s)*ld + h*D. With Hd=1/ld=D this is the packed
// [BH, S, D] layout; with Hd=H/ld=3*H*D the kernels read q/k/v DIRECTLY out
// of the [B,S,3,H,D] QKV-projection tensor (no transpose copies), and with
// ldo=H*D write O back in [B,S,H*D] so the next linear consumes it as-is.
//
// Variable-length form (MASKED = true): `lens[b]` (clamped to [0, S]) is the
// number of valid keys AND valid query rows of batch row b. It is uniform per
// workgroup and held in an SGPR, so the decisions on it are scalar branches:
// score fragments, P·V K-steps, KV tiles, staging chunks and whole waves /
// Q blocks past L are skipped, not predicated. Only the fragment that
// straddles L selects per lane (keep_valid: score → -inf, P → 0). A staged
// K / Vᵗ row ≥ L is written to the LDS as 0 by a select (whatever was loaded
// for it is dropped), so what rows ≥ L hold in memory, NaN included, meets no
// multiply. Output rows ≥ L are written as +0.
// MASKED = false compiles every masking decision out.
#include "common.h"
#include "kernels_api.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define ATTN_THREADS 256
#define ATTN_QROWS 32  // q rows per wave: two 16-row MFMA fragments (am)

// ---- shared device pieces ---------------------------------------------------

// A lane's coordinates in the 16x16x32 MFMA fragments: A/B operand row `fr`
// and first k element `fk`; C-fragment column `fr`, rows `cr + reg`.
struct FragLane {
  int fr, fk, cr;
  DEV_INLINE explicit FragLane(int lane)
      : fr(lane & 15), fk((lane >> 4) * 8), cr((lane >> 4) * 4) {}
};

// One (batch, head)'s q/k/v/o bases in the strided layout.
struct HeadPtrs {
  const __bf16 *Qb, *Kb, *Vb;
  __bf16* Ob;
  int b;
};
DEV_INLINE HeadPtrs head_ptrs(const __bf16* Q, const __bf16* K,
                              const __bf16* V, __bf16* O, int bh, int Hd,
                              int S, int D, int ldq, int ldo) {
  const int b = bh / Hd, h = bh % Hd;
  const int64_t in = (int64_t)b * S * ldq + h * D;
  return {Q + in, K + in, V + in, O + (int64_t)b * S * ldo + h * D, b};
}

// the masked form branches on the wave's rows: make the wave id provably
// uniform there (the unmasked form keeps the plain shift)
template <bool MASKED>
DEV_INLINE int wave_id(int tid) {
  return MASKED ? __builtin_amdgcn_readfirstlane(tid >> 6) : (tid >> 6);
}

DEV_INLINE int clamp_len(const int* __restrict__ lens, int b, int S) {
  int l = lens[b];
  // readfirstlane: keep the clamped value in an SGPR (the compiler clamps
  // with a vector med3 otherwise, and every branch on L turns into a
  // v_cmp + vcc branch)
  return __builtin_amdgcn_readfirstlane(l < 0 ? 0 : (l > S ? S : l));
}

// +0 to rows [row0, row0+32) ∩ [0, S) of one head's D=64 output columns:
// one wave, 16-byte stores (8 rows × 8 lanes per pass).
DEV_INLINE void zero_rows32(__bf16* __restrict__ Ob, int ldo, int row0, int S,
                            int lane) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int row = row0 + j * 8 + (lane >> 3);
    if (row < S)
      *(uint4*)(Ob + (int64_t)row * ldo + (lane & 7) * 8) =
          make_uint4(0u, 0u, 0u, 0u);
  }
}

// The wave's 32 q rows from q0 as MFMA A fragments, held in registers for
// the whole kernel. CLAMP: a row ≥ S loads row S-1 instead (its output is
// never stored); needed wherever q0 + 31 can reach S.
template <int D, bool CLAMP>
DEV_INLINE void load_q(bf16x8 (&q_frag)[2][D / 32], const __bf16* Qb, int ldq,
                       int q0, int S, FragLane ln) {
#pragma unroll
  for (int am = 0; am < 2; ++am)
#pragma unroll
    for (int ks = 0; ks < D / 32; ++ks) {
      int row = q0 + am * 16 + ln.fr;
      if (CLAMP) row = row < S ? row : S - 1;
      q_frag[am][ks] =
          *(const bf16x8*)(Qb + (int64_t)row * ldq + ks * 32 + ln.fk);
    }
}

// scores = Q·K^T: acc[am][nf] covers 32 q rows × the NF·16 staged key
// columns, which are keys col0 .. col0 + NF·16 - 1. Masked: a fragment whose
// 16 columns are all ≥ L is skipped on a scalar branch and stays 0.
template <int NF, int D, int KP, bool MASKED>
DEV_INLINE void qk_scores(f32x4 (&acc)[2][NF],
                          const bf16x8 (&q_frag)[2][D / 32],
                          const __bf16* K_lds, int col0, int L, FragLane ln) {
#pragma unroll
  for (int nf = 0; nf < NF; ++nf) {
    if (MASKED && col0 + nf * 16 >= L) continue;
#pragma unroll
    for (int ks = 0; ks < D / 32; ++ks) {
      bf16x8 b_frag =
          *(const bf16x8*)(&K_lds[(nf * 16 + ln.fr) * KP + ks * 32 + ln.fk]);
#pragma unroll
      for (int am = 0; am < 2; ++am)
        acc[am][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            q_frag[am][ks], b_frag, acc[am][nf], 0, 0, 0);
    }
  }
}

// THE masking rule: what belongs to key column `col` ≥ L is replaced by
// `fill` with a SELECT, never by arithmetic on it (the value is 0 from the
// zero fill or the untouched 0 of a skipped fragment, but it may be anything
// in a row whose own q is padding).
template <bool MASKED>
DEV_INLINE float keep_valid(float x, int col, int L, float fill) {
  return (!MASKED || col < L) ? x : fill;
}

// Reductions over a score row: the 16 lanes of a quarter wave.
DEV_INLINE float quarter_max(float x) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) x = fmaxf(x, __shfl_xor(x, off, 64));
  return x;
}
DEV_INLINE float quarter_sum(float x) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// One step of a lane's row max of scale·score; a column ≥ L counts as -inf.
// (Per element, like masked_exp: a helper that takes the accumulator row
// by reference changed the masked flash kernel's register allocation.)
template <bool MASKED>
DEV_INLINE float masked_max(float mx, float score, float scale, int col,
                            int L) {
  float sc = score * scale;
  return fmaxf(mx, keep_valid<MASKED>(sc, col, L, -INFINITY));
}

// e^(scale·score − mx), 0 at a column ≥ L: the valid lanes evaluate the very
// expression of the unmasked form.
template <bool MASKED>
DEV_INLINE float masked_exp(float score, float scale, float mx, int col,
                            int L) {
  float e = __expf(score * scale - mx);
  return keep_valid<MASKED>(e, col, L, 0.f);
}

// o += P·Vᵗ over KSTEPS 32-key steps, the first at key col0; P [32][LD] is
// this wave's, Vt [D][LD]. Masked: a step whose 32 keys are all ≥ L is
// skipped on a scalar branch.
template <int KSTEPS, int D, int LD, bool MASKED>
DEV_INLINE void pv_accumulate(f32x4 (&o_acc)[2][D / 16], const __bf16* Pw,
                              const __bf16* Vt_lds, int col0, int L,
                              FragLane ln) {
#pragma unroll
  for (int ks = 0; ks < KSTEPS; ++ks) {
    if (MASKED && col0 + ks * 32 >= L) continue;
    bf16x8 a_frag[2];
#pragma unroll
    for (int am = 0; am < 2; ++am)
      a_frag[am] =
          *(const bf16x8*)(&Pw[(am * 16 + ln.fr) * LD + ks * 32 + ln.fk]);
#pragma unroll
    for (int nd = 0; nd < D / 16; ++nd) {
      bf16x8 b_frag =
          *(const bf16x8*)(&Vt_lds[(nd * 16 + ln.fr) * LD + ks * 32 + ln.fk]);
#pragma unroll
      for (int am = 0; am < 2; ++am)
        o_acc[am][nd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a_frag[am], b_frag, o_acc[am][nd], 0, 0, 0);
    }
  }
}

// ---- full-S kernel ----------------------------------------------------------

// Softmax over whole score rows, P normalised and stored as bf16 [32][SP].
// L32 = L rounded up to the P·V K-step: P columns [L, L32) are stored as 0,
// columns ≥ L32 are never read. Column 0 is valid (L ≥ 1), so a valid row's
// max is finite.
template <int NF, int SP, bool MASKED>
DEV_INLINE void softmax_rows(const f32x4 (&acc)[2][NF], __bf16* Pw,
                             float scale, int L, int L32, FragLane ln) {
#pragma unroll
  for (int am = 0; am < 2; ++am) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float rmax = -INFINITY;
#pragma unroll
      for (int nf = 0; nf < NF; ++nf)
        rmax = masked_max<MASKED>(rmax, acc[am][nf][r], scale,
                                  nf * 16 + ln.fr, L);
      rmax = quarter_max(rmax);
      float rsum = 0.f;
      float p[NF];
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) {
        if (MASKED && nf * 16 >= L) {  // scalar: no exp for a skipped fragment
          p[nf] = 0.f;
          continue;
        }
        p[nf] = masked_exp<MASKED>(acc[am][nf][r], scale, rmax,
                                   nf * 16 + ln.fr, L);
        rsum += p[nf];
      }
      rsum = quarter_sum(rsum);
      float inv = 1.f / rsum;
      int prow = am * 16 + ln.cr + r;
#pragma unroll
      for (int nf = 0; nf < NF; ++nf)
        if (!MASKED || nf * 16 < L32)
          Pw[prow * SP + nf * 16 + ln.fr] = (__bf16)(p[nf] * inv);
    }
  }
  // P is consumed only by this wave; compiler orders the LDS ops.
}

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
  constexpr int NWAVE = ATTN_THREADS / WAVE;
  static_assert(S == NWAVE * ATTN_QROWS, "one block covers all S rows");
  static_assert(!MASKED || D == 64, "zero_rows32 writes 64 columns");

  extern __shared__ char smem[];
  __bf16* K_lds = (__bf16*)smem;                       // [S][DP]
  __bf16* Vt_lds = K_lds + S * DP;                     // [D][SP]
  __bf16* P_lds = Vt_lds + D * SP;                     // [NWAVE][32][SP]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = wave_id<MASKED>(tid);
  const FragLane ln(lane);
  const HeadPtrs hp = head_ptrs(Q, K, V, O, blockIdx.x, Hd, S, D, ldq, ldo);
  const int q0 = wid * ATTN_QROWS;

  // ---- stage K and V^T (coalesced global reads, 2 bf16 per thread per step).
  // The three staging forms (this kernel masked and unmasked, the flash
  // tile) stay written out in their kernels: each measured faster that way
  // than through a shared routine (NOTES.md).
  // Masked: 64-row chunks, a chunk past L skipped on a scalar branch; all
  // loads are issued before the first LDS write (a loop bounded by L would
  // wait for each pair in turn), and chunk 0's before L itself is read, so
  // the lens load hides behind them. Every row < S is valid memory, so a
  // row ≥ L is loaded like any other and replaced by 0 with a select before
  // it reaches the LDS.
  int L = S;  // valid keys / rows
  if constexpr (MASKED) {
    constexpr int CH = 64, NCH = S / CH, NIT = CH * D / 2 / ATTN_THREADS;
    uint32_t kv[NCH][NIT], vv[NCH][NIT];
    auto load_chunk = [&](int c) {
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        int i = c * CH * D / 2 + it * ATTN_THREADS + tid;
        int s = (i * 2) / D, d = (i * 2) % D;
        kv[c][it] = *(const uint32_t*)(hp.Kb + (int64_t)s * ldq + d);
        vv[c][it] = *(const uint32_t*)(hp.Vb + (int64_t)s * ldq + d);
      }
    };
    load_chunk(0);
    L = clamp_len(lens, hp.b, S);
    if (L == 0) {  // whole block: nothing to attend to
      zero_rows32(hp.Ob, ldo, q0, S, lane);
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
      uint32_t kv = *(const uint32_t*)(hp.Kb + (int64_t)s * ldq + d);
      *(uint32_t*)(&K_lds[s * DP + d]) = kv;
      uint32_t vv = *(const uint32_t*)(hp.Vb + (int64_t)s * ldq + d);
      __bf16 v0 = ((const __bf16*)&vv)[0], v1 = ((const __bf16*)&vv)[1];
      Vt_lds[d * SP + s] = v0;
      Vt_lds[(d + 1) * SP + s] = v1;
    }
  }
  const int L32 = MASKED ? ((L + 31) & ~31) : S;

  // no row clamp: the block's rows are exactly the S rows
  bf16x8 q_frag[2][D / 32];
  load_q<D, false>(q_frag, hp.Qb, ldq, q0, S, ln);

  __syncthreads();  // K/Vt staged

  if constexpr (MASKED) {
    if (q0 >= L) {  // all 32 query rows of this wave are padding
      zero_rows32(hp.Ob, ldo, q0, S, lane);
      return;
    }
  }

  f32x4 acc[2][S / 16] = {};
  qk_scores<S / 16, D, DP, MASKED>(acc, q_frag, K_lds, 0, L, ln);

  __bf16* Pw = P_lds + wid * ATTN_QROWS * SP;
  softmax_rows<S / 16, SP, MASKED>(acc, Pw, scale, L, L32, ln);

  f32x4 o_acc[2][D / 16] = {};
  pv_accumulate<S / 32, D, SP, MASKED>(o_acc, Pw, Vt_lds, 0, L, ln);

#pragma unroll
  for (int am = 0; am < 2; ++am)
#pragma unroll
    for (int nd = 0; nd < D / 16; ++nd)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = q0 + am * 16 + ln.cr + r;
        // a padded row inside a partly valid wave: +0 by select (its
        // accumulator may hold NaN from its own garbage q row)
        hp.Ob[(int64_t)row * ldo + nd * 16 + ln.fr] =
            (!MASKED || row < L) ? (__bf16)o_acc[am][nd][r] : (__bf16)0.f;
      }
}

// ---- flash-tiled kernel -----------------------------------------------------
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
  __shared__ __bf16 K_lds[FA_KT * DP];          // kv tile, row-major [64][DP]
  __shared__ __bf16 Vt_lds[D * KTP];            // tile of Vᵗ [D][64+pad]
  __shared__ __bf16 P_lds[4][ATTN_QROWS * KTP]; // per-wave P [32][64+pad]

  const int qb = blockIdx.x % qblocks;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = wave_id<MASKED>(tid);
  const FragLane ln(lane);
  const HeadPtrs hp =
      head_ptrs(Q, K, V, O, blockIdx.x / qblocks, Hd, S, D, ldq, ldo);
  const int q0 = qb * 128 + wid * ATTN_QROWS;  // this wave's first q row

  // L valid keys/rows. The KV loop ends at the tile that holds key L-1, so
  // every processed tile has a valid first column and the running max of a
  // valid row is finite from the first tile on.
  int L = S;
  if constexpr (MASKED) {
    L = clamp_len(lens, hp.b, S);
    if (qb * 128 >= L) {  // whole Q block is padding (block-uniform: no
      zero_rows32(hp.Ob, ldo, q0, S, lane);  // barrier has been reached yet)
      return;
    }
  }
  const int kv_end = MASKED ? ((L + FA_KT - 1) / FA_KT) * FA_KT : S;
  // a wave whose 32 rows are all padding keeps staging and the barriers of
  // its block but does no MFMA and no softmax
  const bool wave_live = !MASKED || q0 < L;

  // row clamp: at S % 128 == 64 the last block's waves 2 and 3 lie past S
  bf16x8 q_frag[2][D / 32];
  load_q<D, true>(q_frag, hp.Qb, ldq, q0, S, ln);

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
      uint32_t kv = *(const uint32_t*)(hp.Kb + (int64_t)sl * ldq + d);
      kv = live ? kv : 0u;
      *(uint32_t*)(&K_lds[s * DP + d]) = kv;
      uint32_t vv = *(const uint32_t*)(hp.Vb + (int64_t)sl * ldq + d);
      vv = live ? vv : 0u;
      __bf16 v0 = ((const __bf16*)&vv)[0], v1 = ((const __bf16*)&vv)[1];
      Vt_lds[d * KTP + s] = v0;
      Vt_lds[(d + 1) * KTP + s] = v1;
    }
    __syncthreads();

    if (wave_live) {
      f32x4 acc[2][FA_KT / 16] = {};
      qk_scores<FA_KT / 16, D, DP, MASKED>(acc, q_frag, K_lds, kt, L, ln);
      // running-rescale softmax over this tile's rows (m/l state per row in
      // registers): o ← o·e^{m−m'}, l ← l·e^{m−m'} + Σp, P staged
      // unnormalised. Per-lane selects only here: a scalar branch per row and
      // fragment costs more than the exp it would save. (Kept in the kernel
      // body: as a function the same text compiled to ~50 more moves per
      // tile in the masked kernel.)
      __bf16* Pw = P_lds[wid];
      constexpr int NF = FA_KT / 16;
#pragma unroll
      for (int am = 0; am < 2; ++am) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float tmax = -INFINITY;
#pragma unroll
          for (int nf = 0; nf < NF; ++nf)
            tmax = masked_max<MASKED>(tmax, acc[am][nf][r], scale,
                                      kt + nf * 16 + ln.fr, L);
          tmax = quarter_max(tmax);
          float m_new = fmaxf(m_run[am][r], tmax);
          float rescale = __expf(m_run[am][r] - m_new);
          float psum = 0.f;
          float p[NF];
#pragma unroll
          for (int nf = 0; nf < NF; ++nf) {
            p[nf] = masked_exp<MASKED>(acc[am][nf][r], scale, m_new,
                                       kt + nf * 16 + ln.fr, L);
            psum += p[nf];
          }
          psum = quarter_sum(psum);
          l_run[am][r] = l_run[am][r] * rescale + psum;
          m_run[am][r] = m_new;
#pragma unroll
          for (int nd = 0; nd < D / 16; ++nd) o_acc[am][nd][r] *= rescale;
          int prow = am * 16 + ln.cr + r;
#pragma unroll
          for (int nf = 0; nf < NF; ++nf)
            Pw[prow * KTP + nf * 16 + ln.fr] = (__bf16)p[nf];
        }
      }
      pv_accumulate<FA_KT / 32, D, KTP, MASKED>(o_acc, Pw, Vt_lds, kt, L, ln);
    }
    __syncthreads();  // K/Vt tiles reused next iteration
  }

  // epilogue: O = o / l; rows ≥ S (a partial last Q block) do not exist.
  // A padded row is +0 by select, as in the full-S kernel; the select is
  // written in both epilogues because a shared store helper made this one
  // slower (NOTES.md).
#pragma unroll
  for (int am = 0; am < 2; ++am)
#pragma unroll
    for (int nd = 0; nd < D / 16; ++nd)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = q0 + am * 16 + ln.cr + r;
        if (row >= S) continue;
        float inv = l_run[am][r] > 0.f ? 1.f / l_run[am][r] : 0.f;
        hp.Ob[(int64_t)row * ldo + nd * 16 + ln.fr] =
            (!MASKED || row < L) ? (__bf16)(o_acc[am][nd][r] * inv)
                                 : (__bf16)0.f;
      }
}

// ---- launcher ---------------------------------------------------------------
// lens == nullptr picks the unmasked instantiations: the kernels every call
// without lengths has always run.

template <bool MASKED, int PAD>
static void launch_full_s(const AttnArgs& a) {
  constexpr int S = 128, D = 64;
  constexpr size_t lds =
      (S * (D + PAD) + D * (S + PAD) + 4 * ATTN_QROWS * (S + PAD)) *
      sizeof(__bf16);
  static bool attr_set = false;  // one per instantiation
  if (!attr_set) {
    (void)hipFuncSetAttribute(
        (const void*)attention_kernel<S, D, PAD, MASKED>,
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr_set = true;
  }
  attention_kernel<S, D, PAD, MASKED>
      <<<a.B * a.Hd, ATTN_THREADS, lds, a.stream>>>(
          (const __bf16*)a.q, (const __bf16*)a.k, (const __bf16*)a.v,
          (__bf16*)a.o, a.scale, a.ldq, a.ldo, a.Hd, a.lens);
}

template <bool MASKED>
static int launch_attention(const AttnArgs& a) {
  if (a.S == 128 && a.D == 64) {
    // pad 8 is the production value: the +4 row pad measured ~590K LDS bank
    // conflicts/dispatch; +8 runs 28.8→19.8 µs at BERT shape (pad sweep,
    // profiles r2). The others are kept for that sweep.
    switch (a.pad) {
      case 4: launch_full_s<MASKED, 4>(a); break;
      case 16: launch_full_s<MASKED, 16>(a); break;
      case 20: launch_full_s<MASKED, 20>(a); break;
      default: launch_full_s<MASKED, 8>(a);
    }
    return 0;
  }
  if (a.D != 64 || a.S % FA_KT != 0) return -1;
  const int qblocks = (a.S + 127) / 128;
  attention_flash_kernel<64, MASKED>
      <<<a.B * a.Hd * qblocks, ATTN_THREADS, 0, a.stream>>>(
          (const __bf16*)a.q, (const __bf16*)a.k, (const __bf16*)a.v,
          (__bf16*)a.o, a.scale, a.S, a.ldq, a.ldo, a.Hd, qblocks, a.lens);
  return 0;
}

extern "C" int launch_attention_bf16(const AttnArgs* a) {
  return a->lens ? launch_attention<true>(*a) : launch_attention<false>(*a);
}
