// Segmented scan + SQL window-frame evaluation (ROWS BETWEEN ...).
//
// MI355X-native replacement for DataFusion's BoundedWindowAggExec on the
// `sql` processor's path. Everything a frame needs is a segmented inclusive
// scan over double[n] steered by one head flag per row: partition bounds,
// prefix sums and counts, and the two scans of the van Herk/Gil-Werman
// sliding min/max. The scan is three passes like the prefix sum in
// filter.hip (tile aggregates → one-block carry scan → write), but carries
// the pair (value, seen-a-head) so a segment can span any number of tiles.
// One kernel then turns the scans into per-row results.
#include "common.h"
#include "relational_api.h"

#define WIN_BLOCK 256
#define WIN_IPT 4
#define WIN_TILE (WIN_BLOCK * WIN_IPT)
#define WIN_WAVES (WIN_BLOCK / WAVE)

// ---- scan operators ---------------------------------------------------------
// identity() is neutral on the left: apply(identity(), x) == x bit for bit
// (SUM: up to the sign of zero). MIN/MAX propagate NaN like torch.minimum.
template <int OP> struct ScanOp;
template <> struct ScanOp<SCAN_SUM> {
  static DEV_INLINE double identity() { return 0.0; }
  static DEV_INLINE double apply(double a, double b) { return a + b; }
};
template <> struct ScanOp<SCAN_MIN> {
  static DEV_INLINE double identity() { return __builtin_huge_val(); }
  static DEV_INLINE double apply(double a, double b) {
    return (a < b || a != a) ? a : b;
  }
};
template <> struct ScanOp<SCAN_MAX> {
  static DEV_INLINE double identity() { return -__builtin_huge_val(); }
  static DEV_INLINE double apply(double a, double b) {
    return (a > b || a != a) ? a : b;
  }
};

// Scan value of a run of rows and whether the run holds a head.
struct SegPair {
  double v;
  int f;
};

// a = the earlier run, b = the later one: a head in b cuts a off.
template <typename Op>
DEV_INLINE SegPair seg_combine(SegPair a, SegPair b) {
  return SegPair{b.f ? b.v : Op::apply(a.v, b.v), a.f | b.f};
}

// Block-wide segmented scan of one pair per thread (WIN_BLOCK threads, all
// must call). excl = everything before this thread, total = the whole block.
// wagg is WIN_WAVES pairs of LDS; the trailing barrier lets callers loop.
template <typename Op>
DEV_INLINE void block_seg_scan(SegPair x, SegPair* wagg, SegPair& excl,
                               SegPair& total) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    SegPair p{__shfl_up(x.v, off, WAVE), __shfl_up(x.f, off, WAVE)};
    if (lane >= off) x = seg_combine<Op>(p, x);
  }
  SegPair prev{__shfl_up(x.v, 1, WAVE), __shfl_up(x.f, 1, WAVE)};
  if (lane == 0) prev = SegPair{Op::identity(), 0};
  if (lane == WAVE - 1) wagg[wid] = x;
  __syncthreads();
  SegPair before{Op::identity(), 0};
  total = before;
#pragma unroll
  for (int w = 0; w < WIN_WAVES; ++w) {
    if (w == wid) before = total;
    total = seg_combine<Op>(total, wagg[w]);
  }
  excl = seg_combine<Op>(before, prev);
  __syncthreads();
}

// ---- passes 1 and 3: per-tile scan ------------------------------------------
// Row j of the scan order is row j of the array, or row n-1-j when REV.
// WRITE = false: tile aggregate pair → tile_v/tile_f. WRITE = true: the scan
// itself, with carry[tile] folded into the rows before the tile's first head.
template <int OP, bool REV, bool WRITE>
__global__ __launch_bounds__(WIN_BLOCK) void seg_scan_tile_kernel(
    const double* __restrict__ vals, const uint8_t* __restrict__ head,
    int64_t n, double* __restrict__ tile_v, uint8_t* __restrict__ tile_f,
    const double* __restrict__ carry, double* __restrict__ out) {
  using Op = ScanOp<OP>;
  __shared__ SegPair wagg[WIN_WAVES];
  const int64_t base =
      (int64_t)blockIdx.x * WIN_TILE + (int64_t)threadIdx.x * WIN_IPT;
  double v[WIN_IPT];
  int f[WIN_IPT];
  SegPair mine{Op::identity(), 0};
#pragma unroll
  for (int k = 0; k < WIN_IPT; ++k) {
    const int64_t j = base + k;
    const int64_t p = REV ? n - 1 - j : j;
    v[k] = j < n ? vals[p] : Op::identity();
    f[k] = j < n ? (head[p] != 0) : 0;
    mine = seg_combine<Op>(mine, SegPair{v[k], f[k]});
  }
  SegPair excl, total;
  block_seg_scan<Op>(mine, wagg, excl, total);
  if (!WRITE) {
    if (threadIdx.x == 0) {
      tile_v[blockIdx.x] = total.v;
      tile_f[blockIdx.x] = (uint8_t)total.f;
    }
    return;
  }
  double run = excl.f ? excl.v : Op::apply(carry[blockIdx.x], excl.v);
#pragma unroll
  for (int k = 0; k < WIN_IPT; ++k) {
    const int64_t j = base + k;
    run = f[k] ? v[k] : Op::apply(run, v[k]);
    if (j < n) out[REV ? n - 1 - j : j] = run;
  }
}

// ---- pass 2: segmented scan of the tile pairs, one block --------------------
// carry[t] = scan value entering tile t (identity for tile 0). Loops over
// WIN_BLOCK tiles at a time, so any tile count works.
template <int OP>
__global__ __launch_bounds__(WIN_BLOCK) void seg_scan_carry_kernel(
    const double* __restrict__ tile_v, const uint8_t* __restrict__ tile_f,
    int nt, double* __restrict__ carry) {
  using Op = ScanOp<OP>;
  __shared__ SegPair wagg[WIN_WAVES];
  SegPair run{Op::identity(), 0};
  for (int base = 0; base < nt; base += WIN_BLOCK) {
    const int t = base + threadIdx.x;
    SegPair x{Op::identity(), 0};
    if (t < nt) x = SegPair{tile_v[t], tile_f[t]};
    SegPair excl, total;
    block_seg_scan<Op>(x, wagg, excl, total);
    if (t < nt) carry[t] = seg_combine<Op>(run, excl).v;
    run = seg_combine<Op>(run, total);
  }
}

template <int OP, bool REV>
static void seg_scan_launch(const double* vals, const uint8_t* head, int64_t n,
                            double* tile_v, uint8_t* tile_f, double* carry,
                            double* out, hipStream_t st) {
  const int nt = seg_scan_tiles(n);
  seg_scan_tile_kernel<OP, REV, false><<<nt, WIN_BLOCK, 0, st>>>(
      vals, head, n, tile_v, tile_f, nullptr, nullptr);
  seg_scan_carry_kernel<OP><<<1, WIN_BLOCK, 0, st>>>(tile_v, tile_f, nt, carry);
  seg_scan_tile_kernel<OP, REV, true><<<nt, WIN_BLOCK, 0, st>>>(
      vals, head, n, nullptr, nullptr, carry, out);
}

extern "C" int seg_scan_tiles(int64_t n) {
  return (int)((n + WIN_TILE - 1) / WIN_TILE);
}
extern "C" int seg_scan_tile_rows() { return WIN_TILE; }

extern "C" void launch_segmented_scan(const double* vals, const uint8_t* head,
                                      int64_t n, int op, int reverse,
                                      double* tile_v, uint8_t* tile_f,
                                      double* carry, double* out,
                                      hipStream_t st) {
  if (n < 1) return;
#define SEG_SCAN_CASE(OP)                                                     \
  case OP:                                                                    \
    if (reverse)                                                              \
      seg_scan_launch<OP, true>(vals, head, n, tile_v, tile_f, carry, out,    \
                                st);                                          \
    else                                                                      \
      seg_scan_launch<OP, false>(vals, head, n, tile_v, tile_f, carry, out,   \
                                 st);                                         \
    break;
  switch (op) {
    SEG_SCAN_CASE(SCAN_SUM)
    SEG_SCAN_CASE(SCAN_MIN)
    SEG_SCAN_CASE(SCAN_MAX)
  }
#undef SEG_SCAN_CASE
}

// ---- scan inputs ------------------------------------------------------------
// Partition heads/tails of the sorted partition ids, and the values whose
// forward MAX / backward MIN scans give every row its partition's first and
// last row index.
__global__ void win_bounds_kernel(const int64_t* __restrict__ part, int64_t n,
                                  uint8_t* __restrict__ head,
                                  uint8_t* __restrict__ tail,
                                  double* __restrict__ head_idx,
                                  double* __restrict__ tail_idx) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const bool h = i == 0 || part[i] != part[i - 1];
    const bool t = i == n - 1 || part[i] != part[i + 1];
    head[i] = h;
    tail[i] = t;
    head_idx[i] = h ? (double)i : 0.0;
    tail_idx[i] = t ? (double)i : __builtin_huge_val();
  }
}

extern "C" void launch_win_bounds(const int64_t* part, int64_t n,
                                  uint8_t* head, uint8_t* tail,
                                  double* head_idx, double* tail_idx,
                                  hipStream_t st) {
  if (n < 1) return;
  win_bounds_kernel<<<capped_grid(n), 256, 0, st>>>(part, n, head, tail,
                                                    head_idx, tail_idx);
}

// Per-row inputs of the value scans; a null output is skipped.
//   masked[i] = valid[i] ? vals[i] : fill      (NULL contributes `fill`)
//   ones[i]   = valid[i] ? 1 : 0
//   chunk_head / chunk_tail: sliding min/max heads every `width` rows counted
//   from the partition start (tails also at the partition end)
__global__ void win_inputs_kernel(const double* __restrict__ vals,
                                  const uint8_t* __restrict__ valid,
                                  const double* __restrict__ start,
                                  const double* __restrict__ end, int64_t n,
                                  double fill, int64_t width,
                                  double* __restrict__ masked,
                                  double* __restrict__ ones,
                                  uint8_t* __restrict__ chunk_head,
                                  uint8_t* __restrict__ chunk_tail) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const bool ok = !valid || valid[i];
    if (masked) masked[i] = ok ? vals[i] : fill;
    if (ones) ones[i] = ok ? 1.0 : 0.0;
    if (chunk_head) {
      const int64_t pos = (i - (int64_t)start[i]) % width;
      chunk_head[i] = pos == 0;
      chunk_tail[i] = pos == width - 1 || i == (int64_t)end[i];
    }
  }
}

extern "C" void launch_win_inputs(const double* vals, const uint8_t* valid,
                                  const double* start, const double* end,
                                  int64_t n, double fill, int64_t width,
                                  double* masked, double* ones,
                                  uint8_t* chunk_head, uint8_t* chunk_tail,
                                  hipStream_t st) {
  if (n < 1) return;
  win_inputs_kernel<<<capped_grid(n), 256, 0, st>>>(
      vals, valid, start, end, n, fill, width, masked, ones, chunk_head,
      chunk_tail);
}

// ---- frame evaluation -------------------------------------------------------
// Row i of the sorted order has partition [s, e] and frame
// [l, r] = [max(s, i+lo), min(e, i+hi)], empty when l > r.
__global__ void win_frame_kernel(FrameArgs a) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < a.n; i += stride) {
    const int64_t s = (int64_t)a.start[i], e = (int64_t)a.end[i];
    int64_t l = s, r = e;
    if (!a.lo_unbounded && i + a.lo > l) l = i + a.lo;
    if (!a.hi_unbounded && i + a.hi < r) r = i + a.hi;
    const bool empty = l > r;
    // valid rows in the frame; every row counts when there is no NULL input
    double cnt = 0.0;
    if (!empty)
      cnt = a.count ? a.count[r] - (l == s ? 0.0 : a.count[l - 1])
                    : (double)(r - l + 1);
    double res = 0.0;
    bool ok = cnt > 0.0;
    switch (a.func) {
      case WF_COUNT_STAR:
        res = empty ? 0.0 : (double)(r - l + 1);
        ok = true;
        break;
      case WF_COUNT:
        res = cnt;
        ok = true;
        break;
      case WF_SUM:
      case WF_AVG:
        if (ok) {
          res = a.prefix[r] - (l == s ? 0.0 : a.prefix[l - 1]);
          if (a.func == WF_AVG) res /= cnt;
        }
        break;
      case WF_MIN:
      case WF_MAX:
        if (ok) {
          if (a.lo_unbounded) {
            res = a.prefix[r];
          } else if (a.hi_unbounded) {
            res = a.suffix[l];
          } else {
            // sliding: chunks of W = hi-lo+1 rows from the partition start;
            // a frame spans at most two of them
            const int64_t w = a.hi - a.lo + 1;
            const int64_t cl = (l - s) / w, cr = (r - s) / w;
            if (cl == cr) {
              res = (l - s) % w == 0 ? a.prefix[r] : a.suffix[l];
            } else {
              const double x = a.suffix[l], y = a.prefix[r];
              res = a.func == WF_MIN ? ScanOp<SCAN_MIN>::apply(x, y)
                                     : ScanOp<SCAN_MAX>::apply(x, y);
            }
          }
        }
        break;
      default: {  // WF_FIRST / WF_LAST: NULL rows are not skipped
        const int64_t at = a.func == WF_FIRST ? l : r;
        ok = !empty && (!a.valid || a.valid[at]);
        if (ok) res = a.vals[at];
      }
    }
    const int64_t o = a.perm ? a.perm[i] : i;
    a.out[o] = res;
    a.out_valid[o] = ok;
  }
}

extern "C" void launch_win_frame(const FrameArgs* args, hipStream_t st) {
  if (args->n < 1) return;
  win_frame_kernel<<<capped_grid(args->n), 256, 0, st>>>(*args);
}
