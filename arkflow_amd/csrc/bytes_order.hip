// Order of binary (string) columns on the device — ORDER BY / MIN / MAX /
// < <= > >= / BETWEEN / window ORDER BY on string keys.
//
// Order is bytewise, unsigned, a proper prefix first (Python bytes order,
// SQLite BINARY, UTF-8 code-point order). Row i is
// data[offsets[i] .. offsets[i+1]).
//
// bytes_compare: one thread per row, three-way compare against a second
// column or one literal.
//
// bytes_rank (dense rank) is a most-significant-chunk-first refinement built
// on the radix argsort. Rows are kept in their current order (`perm`) with a
// dense segment id per position: rows of one segment agree on all bytes seen
// so far. Round d gives a row the 64-bit key
//     b[7d] << 56 | ... | b[7d+6] << 8 | nvalid,   nvalid = clamp(len-7d,0,7)
// with bytes past the end read as 0. Unsigned order of the keys is the order
// of the chunks: a padded 0 ties only with a real 0 byte, and then the
// smaller nvalid — the proper prefix — wins. The host sorts the round's rows
// by key, then stably by segment, and the kernels below write the rows back,
// mark a head wherever segment or key changes, and flag the rows that stay
// open: nvalid == 7 in a segment of more than one row. Only open rows take
// part in the next round; the count of them is the one value read back.
#include "common.h"
#include "relational_api.h"

namespace {

// ---- three-way compare ------------------------------------------------------
// a and b address bytes at equal positions of the two strings. Words are
// loaded only from 8-byte-aligned addresses, so both sides must share their
// alignment mod 8; otherwise every byte is loaded on its own.
DEV_INLINE int compare_bytes(const uint8_t* __restrict__ a, int64_t la,
                             const uint8_t* __restrict__ b, int64_t lb) {
  const int64_t m = la < lb ? la : lb;
  int64_t k = 0;
  if ((((uintptr_t)a ^ (uintptr_t)b) & 7) == 0) {
    for (; k < m && (((uintptr_t)(a + k)) & 7); ++k)
      if (a[k] != b[k]) return a[k] < b[k] ? -1 : 1;
    for (; k + 8 <= m; k += 8) {
      uint64_t wa = *(const uint64_t*)(a + k);
      uint64_t wb = *(const uint64_t*)(b + k);
      if (wa != wb) {
        // little-endian words: the first differing byte is the lowest
        int sh = (__ffsll((long long)(wa ^ wb)) - 1) & ~7;
        return ((wa >> sh) & 0xFF) < ((wb >> sh) & 0xFF) ? -1 : 1;
      }
    }
  }
  for (; k < m; ++k)
    if (a[k] != b[k]) return a[k] < b[k] ? -1 : 1;
  return la < lb ? -1 : (la > lb ? 1 : 0);
}

__global__ void bytes_compare_cols_kernel(
    const uint8_t* __restrict__ da, const int64_t* __restrict__ oa,
    const uint8_t* __restrict__ db, const int64_t* __restrict__ ob, int64_t n,
    int8_t* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    int64_t sa = oa[i], sb = ob[i];
    out[i] = (int8_t)compare_bytes(da + sa, oa[i + 1] - sa, db + sb,
                                   ob[i + 1] - sb);
  }
}

// lit8 holds 8 copies of the literal, copy s starting s bytes into its own
// 8-byte-aligned slab of `slab` bytes: a row picks the copy that shares its
// alignment, so the word loop runs for every row.
__global__ void bytes_compare_lit_kernel(
    const uint8_t* __restrict__ da, const int64_t* __restrict__ oa, int64_t n,
    const uint8_t* __restrict__ lit8, int64_t slab, int64_t nl,
    int8_t* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    int64_t sa = oa[i];
    const uint8_t* a = da + sa;
    int s = (int)((uintptr_t)a & 7);
    out[i] = (int8_t)compare_bytes(a, oa[i + 1] - sa, lit8 + s * slab + s, nl);
  }
}

// ---- rank: round keys -------------------------------------------------------
// Position pos[j] holds row perm[pos[j]]; its key of round d goes to key[j],
// its row and segment to row_o[j] / seg_o[j].
__global__ void bo_chunk_keys_kernel(
    const uint8_t* __restrict__ data, const int64_t* __restrict__ offsets,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ seg,
    const int32_t* __restrict__ pos, int64_t m, int64_t d,
    uint64_t* __restrict__ key, int32_t* __restrict__ row_o,
    int32_t* __restrict__ seg_o) {
  int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; j < m; j += stride) {
    int32_t p = pos[j];
    int32_t r = perm[p];
    int64_t s = offsets[r] + 7 * d;
    int64_t left = offsets[r + 1] - s;
    int nvalid = left < 0 ? 0 : (left > 7 ? 7 : (int)left);
    uint64_t k = 0;
#pragma unroll
    for (int b = 0; b < 7; ++b)
      k = (k << 8) | (b < nvalid ? (uint64_t)data[s + b] : 0ull);
    key[j] = (k << 8) | (uint64_t)nvalid;
    row_o[j] = r;
    seg_o[j] = seg[p];
  }
}

// ---- rank: write a sorted round back ----------------------------------------
// Sorted slot j holds what slot src = idx_a[idx_b[j]] of the round's input
// held (idx_a: sort by key, idx_b: stable sort of that by segment); key_a /
// seg_b are the keys after the first sort and the segments after the second.
// The open rows of one segment sit at consecutive positions, so slot j goes
// back to position pos[j]. head: first position of a (segment, key) run;
// open: the run has more than one row and its chunk was a full 7 bytes.
__global__ void bo_apply_round_kernel(
    const int32_t* __restrict__ idx_a, const int32_t* __restrict__ idx_b,
    const uint64_t* __restrict__ key_a, const int32_t* __restrict__ seg_b,
    const int32_t* __restrict__ row_o, const int32_t* __restrict__ pos,
    int64_t m, int32_t* __restrict__ perm, int32_t* __restrict__ head,
    bool* __restrict__ open) {
  int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; j < m; j += stride) {
    int32_t b = idx_b[j];
    uint64_t k = key_a[b];
    int32_t sg = seg_b[j];
    bool is_head = j == 0 || seg_b[j - 1] != sg || key_a[idx_b[j - 1]] != k;
    bool next_head =
        j + 1 == m || seg_b[j + 1] != sg || key_a[idx_b[j + 1]] != k;
    int32_t p = pos[j];
    perm[p] = row_o[idx_a[b]];
    head[p] = is_head ? 1 : 0;
    open[p] = (k & 0xFF) == 7 && !(is_head && next_head);
  }
}

// offs = exclusive scan of the head flags (n + 1 entries): the segment of
// position p is the number of heads up to and including p, less one.
__global__ void bo_segments_kernel(const int64_t* __restrict__ offs, int64_t n,
                                   int32_t* __restrict__ seg) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; p < n; p += stride) seg[p] = (int32_t)(offs[p + 1] - 1);
}

__global__ void bo_scatter_rank_kernel(const int32_t* __restrict__ perm,
                                       const int32_t* __restrict__ seg,
                                       int64_t n, int64_t* __restrict__ rank) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; p < n; p += stride) rank[perm[p]] = seg[p];
}

}  // namespace

extern "C" {

void launch_bytes_compare_cols(const uint8_t* da, const int64_t* oa,
                               const uint8_t* db, const int64_t* ob, int64_t n,
                               int8_t* out, hipStream_t st) {
  if (n < 1) return;
  bytes_compare_cols_kernel<<<capped_grid(n), 256, 0, st>>>(da, oa, db, ob, n,
                                                            out);
}

void launch_bytes_compare_lit(const uint8_t* da, const int64_t* oa, int64_t n,
                              const uint8_t* lit8, int64_t slab, int64_t nl,
                              int8_t* out, hipStream_t st) {
  if (n < 1) return;
  bytes_compare_lit_kernel<<<capped_grid(n), 256, 0, st>>>(da, oa, n, lit8,
                                                           slab, nl, out);
}

void launch_bo_chunk_keys(const uint8_t* data, const int64_t* offsets,
                          const int32_t* perm, const int32_t* seg,
                          const int32_t* pos, int64_t m, int64_t d,
                          uint64_t* key, int32_t* row_o, int32_t* seg_o,
                          hipStream_t st) {
  if (m < 1) return;
  bo_chunk_keys_kernel<<<capped_grid(m), 256, 0, st>>>(
      data, offsets, perm, seg, pos, m, d, key, row_o, seg_o);
}

void launch_bo_apply_round(const int32_t* idx_a, const int32_t* idx_b,
                           const uint64_t* key_a, const int32_t* seg_b,
                           const int32_t* row_o, const int32_t* pos, int64_t m,
                           int32_t* perm, int32_t* head, bool* open,
                           hipStream_t st) {
  if (m < 1) return;
  bo_apply_round_kernel<<<capped_grid(m), 256, 0, st>>>(
      idx_a, idx_b, key_a, seg_b, row_o, pos, m, perm, head, open);
}

void launch_bo_segments(const int64_t* offs, int64_t n, int32_t* seg,
                        hipStream_t st) {
  if (n < 1) return;
  bo_segments_kernel<<<capped_grid(n), 256, 0, st>>>(offs, n, seg);
}

void launch_bo_scatter_rank(const int32_t* perm, const int32_t* seg, int64_t n,
                            int64_t* rank, hipStream_t st) {
  if (n < 1) return;
  bo_scatter_rank_kernel<<<capped_grid(n), 256, 0, st>>>(perm, seg, n, rank);
}

}  // extern "C"
