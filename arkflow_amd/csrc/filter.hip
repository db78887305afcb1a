// Order-preserving stream compaction + fused compare-and-compact + gather.
//
// MI355X-native replacement for DataFusion's FilterExec on the `sql`
// processor's hot path (reference processor/sql.rs:107-146). Two-pass
// block-count → scan → scatter keeps row order without global atomics;
// the scan between passes is one tiny device cumsum done by the caller.
#include "common.h"
#include "relational_api.h"

// items per block: 256 threads × 4 = 1024 rows — small batches (8192 rows)
// still fill ≥8 blocks; big batches scale to thousands of workgroups.
#define FILTER_BLOCK 256
#define FILTER_IPT 4
#define FILTER_TILE (FILTER_BLOCK * FILTER_IPT)

enum CmpOp { LT = 0, LE = 1, GT = 2, GE = 3, EQ = 4, NE = 5 };

template <typename T>
DEV_INLINE bool cmp_apply(T v, int op, T s) {
  switch (op) {
    case LT: return v < s;
    case LE: return v <= s;
    case GT: return v > s;
    case GE: return v >= s;
    case EQ: return v == s;
    default: return v != s;
  }
}

// ---- row predicates: does row i survive? ------------------------------------
template <typename T>
struct CmpPred {
  const T* __restrict__ col;
  int op;
  T scalar;
  DEV_INLINE bool operator()(int64_t i) const {
    return cmp_apply(col[i], op, scalar);
  }
};
struct MaskPred {
  const bool* __restrict__ mask;
  DEV_INLINE bool operator()(int64_t i) const { return mask[i]; }
};

// ---- pass 1: per-block count of matching rows -------------------------------
template <typename Pred>
__global__ void compact_count_kernel(Pred pred, int64_t n,
                                     int32_t* __restrict__ block_counts) {
  int64_t base = (int64_t)blockIdx.x * FILTER_TILE;
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < FILTER_IPT; ++i) {
    int64_t idx = base + threadIdx.x + i * FILTER_BLOCK;
    if (idx < n && pred(idx)) ++cnt;
  }
  // wave reduce then LDS across the 4 waves
  __shared__ int wsum[FILTER_BLOCK / WAVE];
  int v = cnt;
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
#pragma unroll
    for (int w = 0; w < FILTER_BLOCK / WAVE; ++w) total += wsum[w];
    block_counts[blockIdx.x] = total;
  }
}

// ---- pass 2: scatter matching row indices at block offsets ------------------
template <typename Pred>
__global__ void compact_scatter_kernel(
    Pred pred, int64_t n, const int32_t* __restrict__ block_offsets,
    int32_t* __restrict__ out_idx) {
  int64_t base = (int64_t)blockIdx.x * FILTER_TILE;
  __shared__ int wave_base[FILTER_BLOCK / WAVE + 1];
  int write = block_offsets[blockIdx.x];
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  // process the tile in FILTER_IPT ordered strips so output stays row-ordered
#pragma unroll
  for (int i = 0; i < FILTER_IPT; ++i) {
    int64_t idx = base + i * FILTER_BLOCK + threadIdx.x;
    bool keep = (idx < n) && pred(idx);
    uint64_t ballot = __ballot(keep);
    int rank = __popcll(ballot & lanemask_lt());
    int wave_total = __popcll(ballot);
    if (lane == 0) wave_base[wid + 1] = wave_total;
    __syncthreads();
    if (threadIdx.x == 0) {
      wave_base[0] = write;
      for (int w = 1; w <= FILTER_BLOCK / WAVE; ++w)
        wave_base[w] += wave_base[w - 1];
    }
    __syncthreads();
    if (keep) out_idx[wave_base[wid] + rank] = (int32_t)idx;
    write = wave_base[FILTER_BLOCK / WAVE];
    __syncthreads();
  }
}

// Calls f with the device functor for a host-side Predicate.
template <typename F>
static void with_pred(const Predicate& p, F&& f) {
  switch (p.kind) {
    case PRED_MASK: f(MaskPred{(const bool*)p.data}); break;
    case PRED_F32:
      f(CmpPred<float>{(const float*)p.data, p.op, (float)p.scalar}); break;
    case PRED_I64:
      f(CmpPred<int64_t>{(const int64_t*)p.data, p.op, (int64_t)p.scalar});
      break;
  }
}

extern "C" int filter_grid(int64_t n) {
  return (int)((n + FILTER_TILE - 1) / FILTER_TILE);
}

extern "C" void launch_compact_count(const Predicate* pred, int64_t n,
                                     int32_t* counts, hipStream_t st) {
  with_pred(*pred, [&](auto p) {
    compact_count_kernel<<<filter_grid(n), FILTER_BLOCK, 0, st>>>(p, n, counts);
  });
}
extern "C" void launch_compact_scatter(const Predicate* pred, int64_t n,
                                       const int32_t* offs, int32_t* out_idx,
                                       hipStream_t st) {
  with_pred(*pred, [&](auto p) {
    compact_scatter_kernel<<<filter_grid(n), FILTER_BLOCK, 0, st>>>(
        p, n, offs, out_idx);
  });
}

// ---- gather -----------------------------------------------------------------
// Columns are gathered as opaque 1/2/4/8-byte elements: calls f with a zero
// of the unsigned type of that width.
template <typename F>
__host__ __device__ __forceinline__ void with_elem_type(int esz, F&& f) {
  switch (esz) {
    case 1: f(uint8_t{}); break;
    case 2: f(uint16_t{}); break;
    case 4: f(uint32_t{}); break;
    default: f(uint64_t{}); break;
  }
}

// Coalesced row gather by element size; one thread per output row × chunk.
template <typename T>
__global__ void gather_kernel(const T* __restrict__ src,
                              const int32_t* __restrict__ idx, int64_t m,
                              T* __restrict__ dst) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < m; i += stride) dst[i] = src[idx[i]];
}

extern "C" void launch_gather(const void* src, const int32_t* idx, int64_t m,
                              void* dst, int elem_size, hipStream_t st) {
  if (m < 1) return;
  with_elem_type(elem_size, [&](auto t) {
    using T = decltype(t);
    gather_kernel<T><<<capped_grid(m), 256, 0, st>>>((const T*)src, idx, m,
                                                     (T*)dst);
  });
}

// ---- multi-column gather: one launch for a whole batch ----------------------
#define GATHER_MAX_COLS 32
struct GatherSpec {
  int ncols;
  const void* src[GATHER_MAX_COLS];
  void* dst[GATHER_MAX_COLS];
  int esz[GATHER_MAX_COLS];
};

// Count = HostCount: m rows. Count = DevCount: the row count lives in DEVICE
// memory (written by the scan), so the whole filter→gather chain captures
// into a hipGraph with no host sync; the grid is sized for the batch cap and
// threads past the count exit.
template <typename Count>
__global__ void gather_multi_kernel(GatherSpec spec,
                                    const int32_t* __restrict__ idx,
                                    Count count) {
  int64_t m = count.get();
  int64_t total = (int64_t)spec.ncols * m;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    int c = (int)(i / m);
    int64_t j = i - (int64_t)c * m;
    int64_t s = idx[j];
    with_elem_type(spec.esz[c], [&](auto t) {
      using T = decltype(t);
      ((T*)spec.dst[c])[j] = ((const T*)spec.src[c])[s];
    });
  }
}

extern "C" void launch_gather_multi(int ncols, const void* const* src,
                                    void* const* dst, const int* esz,
                                    const int32_t* idx, int64_t m,
                                    const int32_t* count_dev, hipStream_t st) {
  GatherSpec spec{};
  spec.ncols = ncols;
  for (int c = 0; c < ncols; ++c) {
    spec.src[c] = src[c];
    spec.dst[c] = dst[c];
    spec.esz[c] = esz[c];
  }
  int64_t total = (int64_t)ncols * m;
  if (total < 1) return;
  int grid = capped_grid(total, 256, 4096);
  if (count_dev)
    gather_multi_kernel<<<grid, 256, 0, st>>>(spec, idx, DevCount{count_dev});
  else
    gather_multi_kernel<<<grid, 256, 0, st>>>(spec, idx, HostCount{m});
}

// ---- per-row bytes hash (binary columns: group-by / repartition keys) -------
// 64-bit FNV-1a over each row's byte slice; one thread per row. Used to
// dictionary-encode string keys on-device (collision probability ~n²/2^65 —
// negligible at stream batch sizes; exact verification is the CPU path).
__global__ void bytes_hash_kernel(const uint8_t* __restrict__ data,
                                  const int64_t* __restrict__ offsets,
                                  int64_t n, int64_t* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (int64_t p = offsets[i]; p < offsets[i + 1]; ++p) {
      h ^= data[p];
      h *= 0x100000001b3ull;
    }
    out[i] = (int64_t)h;
  }
}

extern "C" void launch_bytes_hash(const uint8_t* data, const int64_t* offsets,
                                  int64_t n, int64_t* out, hipStream_t st) {
  if (n < 1) return;
  bytes_hash_kernel<<<capped_grid(n), 256, 0, st>>>(data, offsets, n, out);
}

// ------------------------------------------------------------------ prefix sum
// Exclusive prefix sum of an int32 array into int64 offsets — the device-side
// cumsum for string-column copy-out (json/proto decoders) and any
// offsets-from-lengths step. Two passes: per-block sums, then (after a tiny
// torch cumsum over <=2048 block sums) an in-block scan + add. Replaces
// torch's innermost-dim scan kernel, which is ~600 µs at n=262K vs ~15 µs
// for this pair.
#define SCAN_BLOCK 256
#define SCAN_IPT 8
#define SCAN_TILE (SCAN_BLOCK * SCAN_IPT)

__global__ void scan_partials_kernel(const int32_t* __restrict__ in, int64_t n,
                                     int64_t* __restrict__ partials) {
  int64_t base = (int64_t)blockIdx.x * SCAN_TILE;
  int64_t local = 0;
#pragma unroll
  for (int k = 0; k < SCAN_IPT; ++k) {
    int64_t i = base + threadIdx.x * SCAN_IPT + k;
    if (i < n) local += in[i];
  }
  __shared__ int64_t lds[SCAN_BLOCK];
  lds[threadIdx.x] = local;
  __syncthreads();
  // tree reduce
  for (int s = SCAN_BLOCK / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partials[blockIdx.x] = lds[0];
}

__global__ void scan_write_kernel(const int32_t* __restrict__ in, int64_t n,
                                  const int64_t* __restrict__ block_offs,
                                  int64_t* __restrict__ out) {
  int64_t base = (int64_t)blockIdx.x * SCAN_TILE;
  int32_t vals[SCAN_IPT];
  int64_t local = 0;
#pragma unroll
  for (int k = 0; k < SCAN_IPT; ++k) {
    int64_t i = base + threadIdx.x * SCAN_IPT + k;
    vals[k] = i < n ? in[i] : 0;
    local += vals[k];
  }
  __shared__ int64_t lds[SCAN_BLOCK];
  lds[threadIdx.x] = local;
  __syncthreads();
  // Hillis-Steele inclusive scan over per-thread sums
  for (int s = 1; s < SCAN_BLOCK; s <<= 1) {
    int64_t add = threadIdx.x >= s ? lds[threadIdx.x - s] : 0;
    __syncthreads();
    lds[threadIdx.x] += add;
    __syncthreads();
  }
  int64_t run = block_offs[blockIdx.x] +
                (threadIdx.x ? lds[threadIdx.x - 1] : 0);
#pragma unroll
  for (int k = 0; k < SCAN_IPT; ++k) {
    int64_t i = base + threadIdx.x * SCAN_IPT + k;
    if (i < n) {
      out[i] = run;  // exclusive
      run += vals[k];
    }
  }
}

// single-block exclusive scan of ≤1024 int64 block sums → block offsets +
// grand total (replaces the torch cumsum + sub + copy chain between the
// two scan passes — 3-4 launches → 1)
__global__ void scan_boffs64_kernel(const int64_t* __restrict__ partials,
                                    int nb, int64_t* __restrict__ boffs,
                                    int64_t* __restrict__ total_out) {
  __shared__ int64_t lds[1024];
  int tid = threadIdx.x;
  int64_t v = tid < nb ? partials[tid] : 0;
  lds[tid] = v;
  __syncthreads();
  for (int s = 1; s < 1024; s <<= 1) {
    int64_t add = tid >= s ? lds[tid - s] : 0;
    __syncthreads();
    lds[tid] += add;
    __syncthreads();
  }
  if (tid < nb) boffs[tid] = lds[tid] - v;
  if (tid == nb - 1) *total_out = lds[tid];
}

extern "C" void launch_scan_boffs64(const int64_t* partials, int nb,
                                    int64_t* boffs, int64_t* total_out,
                                    hipStream_t st) {
  scan_boffs64_kernel<<<1, 1024, 0, st>>>(partials, nb, boffs, total_out);
}

extern "C" int scan_grid(int64_t n) {
  return (int)((n + SCAN_TILE - 1) / SCAN_TILE);
}

extern "C" void launch_scan_partials(const int32_t* in, int64_t n,
                                     int64_t* partials, hipStream_t st) {
  scan_partials_kernel<<<scan_grid(n), SCAN_BLOCK, 0, st>>>(in, n, partials);
}

extern "C" void launch_scan_write(const int32_t* in, int64_t n,
                                  const int64_t* block_offs, int64_t* out,
                                  hipStream_t st) {
  scan_write_kernel<<<scan_grid(n), SCAN_BLOCK, 0, st>>>(in, n, block_offs,
                                                         out);
}

// ------------------------------------------------------------------ LIKE match
// SQL LIKE on a binary column entirely on-device: mode 0 = contains (%x%),
// 1 = prefix (x%), 2 = suffix (%x), 3 = equals. Needle passed by value in
// the kernarg segment (bounded, like JsonSpec).
#define MATCH_MAX_NEEDLE 64

struct MatchNeedle {
  uint8_t bytes[MATCH_MAX_NEEDLE];
  int len;
  int mode;
};

__global__ void bytes_match_kernel(const uint8_t* __restrict__ data,
                                   const int64_t* __restrict__ offsets,
                                   int64_t n, MatchNeedle nd,
                                   bool* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int64_t s = offsets[i], e = offsets[i + 1];
    const int64_t len = e - s;
    bool m = false;
    if (nd.len == 0) {
      m = (nd.mode == 3) ? (len == 0) : true;
    } else if (len >= nd.len) {
      if (nd.mode == 1 || nd.mode == 3) {        // prefix / equals
        m = (nd.mode == 1 || len == nd.len);
        for (int k = 0; m && k < nd.len; ++k)
          m = data[s + k] == nd.bytes[k];
      } else if (nd.mode == 2) {                 // suffix
        m = true;
        for (int k = 0; m && k < nd.len; ++k)
          m = data[e - nd.len + k] == nd.bytes[k];
      } else {                                   // contains
        for (int64_t p = s; !m && p + nd.len <= e; ++p) {
          bool eq = true;
          for (int k = 0; eq && k < nd.len; ++k)
            eq = data[p + k] == nd.bytes[k];
          m = eq;
        }
      }
    }
    out[i] = m;
  }
}

extern "C" void launch_bytes_match(const uint8_t* data, const int64_t* offsets,
                                   int64_t n, const uint8_t* needle, int nl,
                                   int mode, bool* out, hipStream_t st) {
  MatchNeedle nd{};
  nd.len = nl > MATCH_MAX_NEEDLE ? MATCH_MAX_NEEDLE : nl;
  nd.mode = mode;
  for (int k = 0; k < nd.len; ++k) nd.bytes[k] = needle[k];
  if (n < 1) return;
  bytes_match_kernel<<<capped_grid(n), 256, 0, st>>>(data, offsets, n, nd,
                                                     out);
}
