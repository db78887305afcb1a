// Host-side interface of the relational kernels (WHERE, gather, GROUP BY,
// join, ORDER BY, window frames, string order and the scans between their
// passes). Included by the .hip file that defines each launcher and by
// bindings.cpp, so a declaration that drifts from its definition is a compile
// error.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Row predicate of a stream compaction: a bool mask, or `col OP scalar` on an
// f32 / i64 column. op: 0 < 1 <= 2 > 3 >= 4 == 5 != ; scalar is cast to the
// column's type.
enum PredKind { PRED_MASK = 0, PRED_F32 = 1, PRED_I64 = 2 };
struct Predicate {
  PredKind kind;
  const void* data;  // bool[n], float[n] or int64_t[n]
  int op;
  double scalar;
};

// Segmented-scan operator and window function of a framed evaluation.
enum ScanOpKind { SCAN_SUM = 0, SCAN_MIN = 1, SCAN_MAX = 2 };
enum WindowFunc {
  WF_SUM = 0, WF_COUNT = 1, WF_AVG = 2, WF_MIN = 3, WF_MAX = 4,
  WF_FIRST = 5, WF_LAST = 6, WF_COUNT_STAR = 7
};
// Inputs of the frame kernel, all in sorted (partition, order) row order.
// Row i's frame is [max(start, i+lo), min(end, i+hi)] clipped to its
// partition; an unbounded side ignores lo / hi.
struct FrameArgs {
  const double* start;    // first row of the row's partition
  const double* end;      // last row of the row's partition
  const double* vals;     // raw values (first/last_value), else unused
  const uint8_t* valid;   // null: no NULL input
  const double* prefix;   // forward scan: sums, or min/max
  const double* suffix;   // backward min/max scan
  const double* count;    // forward scan of valid rows; null: no NULL input
  const int64_t* perm;    // null: results stay in sorted order
  int64_t lo, hi;
  int lo_unbounded, hi_unbounded;
  int func;               // WindowFunc
  int64_t n;
  double* out;            // out[perm[i]]
  uint8_t* out_valid;     // 0 = NULL result
};

extern "C" {

// ---- window.hip: segmented scan, window frames ------------------------------
int seg_scan_tiles(int64_t n);  // entries of tile_v / tile_f / carry
int seg_scan_tile_rows();
// Inclusive scan of vals restarting at every row whose head flag is set; in
// reverse the scan runs from row n-1 down. op is a ScanOpKind.
void launch_segmented_scan(const double* vals, const uint8_t* head, int64_t n,
                           int op, int reverse, double* tile_v,
                           uint8_t* tile_f, double* carry, double* out,
                           hipStream_t st);
void launch_win_bounds(const int64_t* part, int64_t n, uint8_t* head,
                       uint8_t* tail, double* head_idx, double* tail_idx,
                       hipStream_t st);
void launch_win_inputs(const double* vals, const uint8_t* valid,
                       const double* start, const double* end, int64_t n,
                       double fill, int64_t width, double* masked,
                       double* ones, uint8_t* chunk_head, uint8_t* chunk_tail,
                       hipStream_t st);
void launch_win_frame(const FrameArgs* args, hipStream_t st);

// ---- filter.hip: compaction, gather -----------------------------------------
int filter_grid(int64_t n);  // blocks (= entries of counts / offs) for n rows
void launch_compact_count(const Predicate* pred, int64_t n, int32_t* counts,
                          hipStream_t st);
void launch_compact_scatter(const Predicate* pred, int64_t n,
                            const int32_t* offs, int32_t* out_idx,
                            hipStream_t st);
void launch_gather(const void* src, const int32_t* idx, int64_t m, void* dst,
                   int elem_size, hipStream_t st);
// Up to 32 columns in one launch. count_dev null: m rows. Otherwise the row
// count is read from *count_dev on the device and m only sizes the grid.
void launch_gather_multi(int ncols, const void* const* src, void* const* dst,
                         const int* esz, const int32_t* idx, int64_t m,
                         const int32_t* count_dev, hipStream_t st);

// ---- filter.hip: binary columns, prefix sum ---------------------------------
void launch_bytes_hash(const uint8_t* data, const int64_t* offsets, int64_t n,
                       int64_t* out, hipStream_t st);
void launch_bytes_match(const uint8_t* data, const int64_t* offsets, int64_t n,
                        const uint8_t* needle, int nl, int mode, bool* out,
                        hipStream_t st);
int scan_grid(int64_t n);
void launch_scan_partials(const int32_t* in, int64_t n, int64_t* partials,
                          hipStream_t st);
void launch_scan_boffs64(const int64_t* partials, int nb, int64_t* boffs,
                         int64_t* total_out, hipStream_t st);
void launch_scan_write(const int32_t* in, int64_t n, const int64_t* block_offs,
                       int64_t* out, hipStream_t st);

// ---- hash_agg.hip -----------------------------------------------------------
// table_size is a power of two. table_keys has table_size entries, table_gids
// table_size + 1: the last belongs to the key equal to the free-slot marker.
void launch_hash_build(const int64_t* keys, int64_t n, int64_t* table_keys,
                       int32_t* table_gids, uint32_t table_size,
                       int32_t* counter, int32_t* gids_out, hipStream_t st);
void launch_hash_export(const int64_t* table_keys, const int32_t* table_gids,
                        uint32_t table_size, int64_t* uniq, hipStream_t st);
void launch_segment_reduce_f32(const float* vals, const int32_t* gids,
                               int64_t n, int g, int op, float* out,
                               int32_t* scratch_flipped, hipStream_t st);
void launch_hash_agg_capture(const int64_t* keys, const int32_t* nrow,
                             int64_t n_cap, int64_t* table_keys,
                             int32_t* table_gids, uint32_t table_size,
                             int32_t* counter, int32_t* gids, float* counts,
                             int g_cap, const float* const* vals,
                             const int* ops, float* const* red_out,
                             int32_t* const* mm_scratch, int nv,
                             int64_t* uniq, int64_t* counts_i64,
                             int32_t* gcount_out, hipStream_t st);

// ---- hash_join.hip ----------------------------------------------------------
// Likewise table_head has table_size + 1 entries.
void launch_join_build(const int64_t* rkeys, int64_t n_right,
                       int64_t* table_keys, int32_t* table_head, int32_t* next,
                       uint32_t table_size, hipStream_t st);
void launch_join_probe_count(const int64_t* lkeys, int64_t n_left,
                             const int64_t* table_keys,
                             const int32_t* table_head, const int32_t* next,
                             const int64_t* rkeys, uint32_t table_size,
                             int32_t* counts, hipStream_t st);
void launch_join_probe_emit(const int64_t* lkeys, int64_t n_left,
                            const int64_t* table_keys,
                            const int32_t* table_head, const int32_t* next,
                            const int64_t* rkeys, uint32_t table_size,
                            const int32_t* offsets, int64_t* l_out,
                            int64_t* r_out, hipStream_t st);

// ---- radix_sort.hip ---------------------------------------------------------
void launch_f32_to_ordered(const float* in, uint32_t* out, int64_t n,
                           int descending, hipStream_t st);
void launch_i32_to_ordered(const int32_t* in, uint32_t* out, int64_t n,
                           int descending, hipStream_t st);
void launch_i64_to_ordered(const int64_t* in, uint64_t* out, int64_t n,
                           int descending, hipStream_t st);
int onesweep_nblocks(int64_t n);
void launch_os_hist256_u32(const uint32_t* keys, int64_t n, int shift,
                           int32_t* hist, int nblocks, hipStream_t st);
void launch_os_hist256_u64(const uint64_t* keys, int64_t n, int shift,
                           int32_t* hist, int nblocks, hipStream_t st);
void launch_onesweep_pass_u32(const uint32_t* keys_in, const int32_t* idx_in,
                              uint32_t* keys_out, int32_t* idx_out, int64_t n,
                              int shift, const int32_t* block_offsets,
                              int nblocks, hipStream_t st);
void launch_onesweep_pass_u64(const uint64_t* keys_in, const int32_t* idx_in,
                              uint64_t* keys_out, int32_t* idx_out, int64_t n,
                              int shift, const int32_t* block_offsets,
                              int nblocks, hipStream_t st);

// ---- bytes_order.hip: three-way compare and dense rank of binary columns ----
// out[i] = -1 / 0 / +1: row i of a against row i of b, bytewise unsigned, a
// proper prefix first.
void launch_bytes_compare_cols(const uint8_t* da, const int64_t* oa,
                               const uint8_t* db, const int64_t* ob, int64_t n,
                               int8_t* out, hipStream_t st);
// Against one literal of nl bytes. lit8: 8 slabs of `slab` bytes (a multiple
// of 8, at least nl + 8), slab s holding the literal from its byte s on.
void launch_bytes_compare_lit(const uint8_t* da, const int64_t* oa, int64_t n,
                              const uint8_t* lit8, int64_t slab, int64_t nl,
                              int8_t* out, hipStream_t st);
// One refinement round of the rank over the m open positions pos[0..m): keys
// of byte chunk d, then (after the two sorts) rows, heads and open flags
// written back. See the head of bytes_order.hip.
void launch_bo_chunk_keys(const uint8_t* data, const int64_t* offsets,
                          const int32_t* perm, const int32_t* seg,
                          const int32_t* pos, int64_t m, int64_t d,
                          uint64_t* key, int32_t* row_o, int32_t* seg_o,
                          hipStream_t st);
void launch_bo_apply_round(const int32_t* idx_a, const int32_t* idx_b,
                           const uint64_t* key_a, const int32_t* seg_b,
                           const int32_t* row_o, const int32_t* pos, int64_t m,
                           int32_t* perm, int32_t* head, bool* open,
                           hipStream_t st);
void launch_bo_segments(const int64_t* offs, int64_t n, int32_t* seg,
                        hipStream_t st);
void launch_bo_scatter_rank(const int32_t* perm, const int32_t* seg, int64_t n,
                            int64_t* rank, hipStream_t st);

}  // extern "C"
