// Row-wise bf16 ops for the inference processor: LayerNorm (with optional
// fused residual add) and row softmax. Memory-bound → vectorized short4/short8
// loads per guide Guideline 13; one block per row, wave+LDS reductions.
#include "gemm_common.h"  // Act / apply_act: the GEMM epilogues' formula
#include "kernels_api.h"

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(8))) __bf16 vbf16x8;

#define ROW_THREADS 256

DEV_INLINE float block_reduce_sum(float v, float* lds) {
  v = wave_reduce_sum(v);
  const int wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds[wid] = v;
  __syncthreads();
  float total = 0.f;
#pragma unroll
  for (int w = 0; w < ROW_THREADS / WAVE; ++w) total += lds[w];
  __syncthreads();
  return total;
}

// All-lanes wave sum for the wave-per-row LayerNorm, whose two reductions
// are serial (the mean feeds the squared deviations): four DPP row rotations
// sum each 16-lane row in the VALU, then two xor shuffles combine the four
// rows — 2 LDS-crossbar round trips instead of the 7 of shfl_down +
// broadcast. Each step adds the same pair of values in both partner lanes, so
// every lane ends with the same bits.
template <int N>
DEV_INLINE float row_ror_add(float v) {
  int r = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x120 + N, 0xf,
                                      0xf, false);  // row_ror:N
  return v + __int_as_float(r);
}
DEV_INLINE float wave_allreduce_sum(float v) {
  v = row_ror_add<8>(v);
  v = row_ror_add<4>(v);
  v = row_ror_add<2>(v);
  v = row_ror_add<1>(v);
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

DEV_INLINE float block_reduce_max(float v, float* lds) {
  v = wave_reduce_max(v);
  const int wid = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds[wid] = v;
  __syncthreads();
  float total = -INFINITY;
#pragma unroll
  for (int w = 0; w < ROW_THREADS / WAVE; ++w) total = fmaxf(total, lds[w]);
  __syncthreads();
  return total;
}

// ---- LayerNorm ---------------------------------------------------------------
// x:[rows,n] bf16 (+ optional residual), gamma/beta:[n] f32 → out bf16.
// n must be a multiple of 8 (bf16x8 vector path).
template <bool ADD_RESIDUAL>
__global__ __launch_bounds__(ROW_THREADS)
void layernorm_bf16_kernel(const __bf16* __restrict__ x,
                           const __bf16* __restrict__ residual,
                           const float* __restrict__ gamma,
                           const float* __restrict__ beta,
                           __bf16* __restrict__ out,
                           __bf16* __restrict__ resid_out,  // optional x+res
                           int64_t rows, int n, float eps) {
  __shared__ float red[ROW_THREADS / WAVE];
  const int nv = n / 8;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const vbf16x8* xr = (const vbf16x8*)(x + row * n);
    const vbf16x8* rr =
        ADD_RESIDUAL ? (const vbf16x8*)(residual + row * n) : nullptr;
    // two-pass variance: E[f^2] - mean^2 cancels catastrophically in fp32
    // once |mean| >> stddev (x + residual rows); sum((f - mean)^2) is >= 0
    // by construction. The second pass re-reads the row (L2-resident).
    float sum = 0.f;
    for (int i = threadIdx.x; i < nv; i += ROW_THREADS) {
      vbf16x8 v = xr[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = (float)v[j];
        if (ADD_RESIDUAL) f += (float)rr[i][j];
        sum += f;
      }
    }
    float mean = block_reduce_sum(sum, red) / n;
    float sq = 0.f;
    for (int i = threadIdx.x; i < nv; i += ROW_THREADS) {
      vbf16x8 v = xr[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = (float)v[j];
        if (ADD_RESIDUAL) f += (float)rr[i][j];
        float d = f - mean;
        sq += d * d;
      }
    }
    float var = block_reduce_sum(sq, red) / n;
    float rstd = rsqrtf(var + eps);
    vbf16x8* orow = (vbf16x8*)(out + row * n);
    vbf16x8* resrow =
        (ADD_RESIDUAL && resid_out) ? (vbf16x8*)(resid_out + row * n) : nullptr;
    for (int i = threadIdx.x; i < nv; i += ROW_THREADS) {
      vbf16x8 v = xr[i];
      vbf16x8 o, rsum;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = (float)v[j];
        if (ADD_RESIDUAL) f += (float)rr[i][j];
        if (ADD_RESIDUAL && resrow) rsum[j] = (__bf16)f;
        int c = i * 8 + j;
        o[j] = (__bf16)((f - mean) * rstd * gamma[c] + beta[c]);
      }
      orow[i] = o;
      if (ADD_RESIDUAL && resrow) resrow[i] = rsum;
    }
    __syncthreads();
  }
}

// wave-per-row LayerNorm: at BERT width (n=768 → 96 bf16x8 vectors) the
// block-per-row kernel leaves 160 of 256 threads idle and pays two block
// barriers per row; a wave per row uses shuffle-only reductions and packs
// 4 rows per block (measured ~2× at 8192×768 — profiles r2).
template <bool ADD_RESIDUAL>
__global__ __launch_bounds__(ROW_THREADS)
void layernorm_bf16_wave_kernel(const __bf16* __restrict__ x,
                                const __bf16* __restrict__ residual,
                                const float* __restrict__ gamma,
                                const float* __restrict__ beta,
                                __bf16* __restrict__ out,
                                __bf16* __restrict__ resid_out,
                                int64_t rows, int n, float eps) {
  const int nv = n / 8;
  const int lane = threadIdx.x & 63;
  int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  int64_t wstride = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const bool cached = nv <= 2 * WAVE;  // lane holds <=2 vectors in regs
  const float inv_n = 1.f / n;  // once per wave, off the per-row chain
  for (int64_t row = wave; row < rows; row += wstride) {
    const vbf16x8* xr = (const vbf16x8*)(x + row * n);
    const vbf16x8* rr =
        ADD_RESIDUAL ? (const vbf16x8*)(residual + row * n) : nullptr;
    vbf16x8* orow = (vbf16x8*)(out + row * n);
    vbf16x8* resrow = (ADD_RESIDUAL && resid_out)
                          ? (vbf16x8*)(resid_out + row * n)
                          : nullptr;
    // two-pass variance (see layernorm_bf16_kernel): mean first, then
    // sum((f - mean)^2) from the register cache, or from a re-read of the
    // row when it is streamed.
    float sum = 0.f, sq = 0.f;
    float c0[16];  // row cache: the (x+residual) floats, read-once
    if (cached) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        int i = lane + t * WAVE;
        if (i < nv) {
          vbf16x8 v = xr[i];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float f = (float)v[j];
            if (ADD_RESIDUAL) f += (float)rr[i][j];
            c0[t * 8 + j] = f;
            sum += f;
          }
        }
      }
    } else {
      for (int i = lane; i < nv; i += WAVE) {
        vbf16x8 v = xr[i];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float f = (float)v[j];
          if (ADD_RESIDUAL) f += (float)rr[i][j];
          sum += f;
        }
      }
    }
    float mean = wave_allreduce_sum(sum) * inv_n;
    if (cached) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (lane + t * WAVE < nv) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float d = c0[t * 8 + j] - mean;
            sq += d * d;
          }
        }
      }
    } else {
      for (int i = lane; i < nv; i += WAVE) {
        vbf16x8 v = xr[i];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float f = (float)v[j];
          if (ADD_RESIDUAL) f += (float)rr[i][j];
          float d = f - mean;
          sq += d * d;
        }
      }
    }
    float var = wave_allreduce_sum(sq) * inv_n;
    float rstd = rsqrtf(var + eps);
    if (cached) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        int i = lane + t * WAVE;
        if (i < nv) {
          vbf16x8 o, rsum;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float f = c0[t * 8 + j];
            if (ADD_RESIDUAL && resrow) rsum[j] = (__bf16)f;
            int c = i * 8 + j;
            o[j] = (__bf16)((f - mean) * rstd * gamma[c] + beta[c]);
          }
          orow[i] = o;
          if (ADD_RESIDUAL && resrow) resrow[i] = rsum;
        }
      }
    } else {
      for (int i = lane; i < nv; i += WAVE) {
        vbf16x8 v = xr[i];
        vbf16x8 o, rsum;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float f = (float)v[j];
          if (ADD_RESIDUAL) f += (float)rr[i][j];
          if (ADD_RESIDUAL && resrow) rsum[j] = (__bf16)f;
          int c = i * 8 + j;
          o[j] = (__bf16)((f - mean) * rstd * gamma[c] + beta[c]);
        }
        orow[i] = o;
        if (ADD_RESIDUAL && resrow) resrow[i] = rsum;
      }
    }
  }
}

// ---- Softmax -----------------------------------------------------------------
// Row softmax over the last dim (n multiple of 8), numerically stable.
__global__ __launch_bounds__(ROW_THREADS)
void softmax_bf16_kernel(const __bf16* __restrict__ x, __bf16* __restrict__ out,
                         int64_t rows, int n, float scale) {
  __shared__ float red[ROW_THREADS / WAVE];
  const int nv = n / 8;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const vbf16x8* xr = (const vbf16x8*)(x + row * n);
    float m = -INFINITY;
    for (int i = threadIdx.x; i < nv; i += ROW_THREADS) {
      vbf16x8 v = xr[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) m = fmaxf(m, (float)v[j] * scale);
    }
    m = block_reduce_max(m, red);
    float sum = 0.f;
    for (int i = threadIdx.x; i < nv; i += ROW_THREADS) {
      vbf16x8 v = xr[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += __expf((float)v[j] * scale - m);
    }
    sum = block_reduce_sum(sum, red);
    float inv = 1.f / sum;
    vbf16x8* orow = (vbf16x8*)(out + row * n);
    for (int i = threadIdx.x; i < nv; i += ROW_THREADS) {
      vbf16x8 v = xr[i];
      vbf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        o[j] = (__bf16)(__expf((float)v[j] * scale - m) * inv);
      orow[i] = o;
    }
    __syncthreads();
  }
}

// ---- elementwise bias+activation (fallback when not fused into GEMM) ---------
__global__ void bias_act_bf16_kernel(const __bf16* __restrict__ x,
                                     const float* __restrict__ bias,
                                     __bf16* __restrict__ out, int64_t rows,
                                     int n, int act) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t total = rows * n;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    float v = (float)x[i] + (bias ? bias[i % n] : 0.f);
    out[i] = (__bf16)apply_act(v, act);
  }
}

extern "C" {

void launch_layernorm_bf16(const void* x, const void* residual,
                           const float* gamma, const float* beta, void* out,
                           void* resid_out, int64_t rows, int n, float eps,
                           hipStream_t st) {
  if (rows < 1) return;
  if (n <= 2048) {  // wave-per-row: shuffle-only reductions, 4 rows/block
    int64_t waves = rows;
    int grid = (int)((waves * 64 + ROW_THREADS - 1) / ROW_THREADS);
    if (grid > 4096) grid = 4096;
    if (residual)
      layernorm_bf16_wave_kernel<true><<<grid, ROW_THREADS, 0, st>>>(
          (const __bf16*)x, (const __bf16*)residual, gamma, beta,
          (__bf16*)out, (__bf16*)resid_out, rows, n, eps);
    else
      layernorm_bf16_wave_kernel<false><<<grid, ROW_THREADS, 0, st>>>(
          (const __bf16*)x, nullptr, gamma, beta, (__bf16*)out, nullptr,
          rows, n, eps);
    return;
  }
  int grid = rows < 2048 ? (int)rows : 2048;
  if (grid < 1) return;
  if (residual)
    layernorm_bf16_kernel<true><<<grid, ROW_THREADS, 0, st>>>(
        (const __bf16*)x, (const __bf16*)residual, gamma, beta, (__bf16*)out,
        (__bf16*)resid_out, rows, n, eps);
  else
    layernorm_bf16_kernel<false><<<grid, ROW_THREADS, 0, st>>>(
        (const __bf16*)x, nullptr, gamma, beta, (__bf16*)out, nullptr, rows,
        n, eps);
}

void launch_softmax_bf16(const void* x, void* out, int64_t rows, int n,
                         float scale, hipStream_t st) {
  int grid = rows < 4096 ? (int)rows : 4096;
  if (grid < 1) return;
  softmax_bf16_kernel<<<grid, ROW_THREADS, 0, st>>>(
      (const __bf16*)x, (__bf16*)out, rows, n, scale);
}

void launch_bias_act_bf16(const void* x, const float* bias, void* out,
                          int64_t rows, int n, int act, hipStream_t st) {
  int64_t total = rows * n;
  int grid = (int)((total + 255) / 256);
  if (grid > 2048) grid = 2048;
  if (grid < 1) return;
  bias_act_bf16_kernel<<<grid, 256, 0, st>>>(
      (const __bf16*)x, bias, (__bf16*)out, rows, n, act);
}

}  // extern "C"
