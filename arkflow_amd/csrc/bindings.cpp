// Torch extension bindings: arkflow_amd._native.
// Thin host layer over the gfx950 kernels in *.hip — tensor checks, workspace
// allocation, the tiny device cumsum between two-pass kernels, pybind exports.
#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>
#include <cstdint>
#include <limits>
#include <tuple>
#include <vector>

// kernel launchers, each declared in the header its defining .hip includes
#include "gemm_api.h"        // GemmVariant, GemmArgs, launch_gemm_bf16
#include "kernels_api.h"     // inference, decode, fused step
#include "relational_api.h"  // filter, gather, group-by, join, sort, scans

namespace {

hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

void check_cuda(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

uint32_t next_pow2(uint32_t v) {
  v--;
  v |= v >> 1; v |= v >> 2; v |= v >> 4; v |= v >> 8; v |= v >> 16;
  return v + 1;
}

// exclusive prefix-sum of int32 lengths → int64 offsets [n+1] (offsets[n] =
// total), all on device — csrc/filter.hip scan kernels (torch's innermost
// cumsum is ~40x slower at n~262K)
torch::Tensor exclusive_offsets(torch::Tensor lens) {
  int64_t n = lens.numel();
  auto out = torch::empty({n + 1}, lens.options().dtype(torch::kInt64));
  if (n == 0) return out.zero_();
  auto st = cur_stream();
  int grid = scan_grid(n);
  auto partials = torch::empty({grid}, lens.options().dtype(torch::kInt64));
  launch_scan_partials(lens.data_ptr<int32_t>(), n,
                       partials.data_ptr<int64_t>(), st);
  torch::Tensor boffs;
  if (grid <= 1024) {
    // single-block scan writes offsets AND the total slot in one launch
    boffs = torch::empty({grid}, partials.options());
    launch_scan_boffs64(partials.data_ptr<int64_t>(), grid,
                        boffs.data_ptr<int64_t>(),
                        out.data_ptr<int64_t>() + n, st);
  } else {
    auto inc = partials.cumsum(0);
    boffs = inc - partials;
    out.narrow(0, n, 1).copy_(inc.narrow(0, grid - 1, 1));
  }
  launch_scan_write(lens.data_ptr<int32_t>(), n, boffs.data_ptr<int64_t>(),
                    out.data_ptr<int64_t>(), st);
  return out;
}

// exclusive scan of int32 block counts → (offsets, total tensor on device)
std::tuple<torch::Tensor, torch::Tensor> exscan(const torch::Tensor& counts) {
  auto inc = counts.cumsum(0, torch::kInt32);
  auto offs = inc - counts;
  auto total = inc.numel() > 0
                   ? inc.slice(0, inc.numel() - 1, inc.numel())
                   : torch::zeros({1}, counts.options());
  return {offs, total};
}

// ---------------------------------------------------------------------- filter
// `col OP scalar` over an f32 or i64 column (callers widen or reject the rest)
Predicate cmp_predicate(const torch::Tensor& col, int64_t op, double scalar) {
  bool is_f32 = col.scalar_type() == torch::kFloat32;
  return {is_f32 ? PRED_F32 : PRED_I64, col.data_ptr(), (int)op, scalar};
}

// Order-preserving compaction of the n > 0 rows that satisfy pred: block
// counts → scan → scatter of row indices (int32).
// count_out null — sync form: the total is read back (the one host sync) and
// the index tensor has exactly `total` entries.
// count_out set — capture form: the total goes to *count_out on the device,
// the index tensor has n entries of which the first *count_out are valid, and
// the returned total is -1.
std::tuple<torch::Tensor, int64_t> compact(const Predicate& pred, int64_t n,
                                           const torch::TensorOptions& opts32,
                                           torch::Tensor* count_out) {
  auto st = cur_stream();
  int nblocks = filter_grid(n);
  auto counts = torch::empty({nblocks}, opts32);
  launch_compact_count(&pred, n, counts.data_ptr<int32_t>(), st);
  torch::Tensor offs;
  int64_t total = -1;
  if (count_out && nblocks <= 1024) {
    // single-block scan writes offsets AND the device total in one launch
    // (replaces torch cumsum + sub + copy_ — 3 kernels → 1 in the graph)
    offs = torch::empty({nblocks}, opts32);
    launch_scan_counts(counts.data_ptr<int32_t>(), nblocks,
                       offs.data_ptr<int32_t>(),
                       count_out->data_ptr<int32_t>(), st);
  } else {
    auto [offs2, total_t] = exscan(counts);
    offs = offs2;
    if (count_out)
      count_out->copy_(total_t, /*non_blocking=*/true);
    else
      total = total_t.item<int32_t>();
  }
  auto idx = torch::empty({count_out ? n : total}, opts32);
  if (count_out || total > 0)
    launch_compact_scatter(&pred, n, offs.data_ptr<int32_t>(),
                           idx.data_ptr<int32_t>(), st);
  return {idx, total};
}

// Rows idx[0..m) of every column, 32 columns per launch, into `outs` — or,
// where `outs` is empty, into fresh m-row tensors. With count_dev the row
// count is read on the device (capture form) and m is its upper bound.
std::vector<torch::Tensor> gather_multi(const std::vector<torch::Tensor>& cols,
                                        const torch::Tensor& idx, int64_t m,
                                        const int32_t* count_dev,
                                        std::vector<torch::Tensor> outs) {
  bool fresh = outs.empty();
  if (fresh) outs.reserve(cols.size());
  std::vector<const void*> src;
  std::vector<void*> dst;
  std::vector<int> esz;
  auto flush = [&]() {
    if (!src.empty() && m > 0)
      launch_gather_multi((int)src.size(), src.data(), dst.data(), esz.data(),
                          idx.data_ptr<int32_t>(), m, count_dev, cur_stream());
    src.clear(); dst.clear(); esz.clear();
  };
  for (size_t c = 0; c < cols.size(); ++c) {
    if (fresh) outs.push_back(torch::empty({m}, cols[c].options()));
    src.push_back(cols[c].data_ptr());
    dst.push_back(outs[c].data_ptr());
    esz.push_back((int)cols[c].element_size());
    if ((int)src.size() == 32) flush();
  }
  flush();
  return outs;
}

torch::Tensor mask_to_indices(torch::Tensor mask) {
  check_cuda(mask, "mask");
  TORCH_CHECK(mask.scalar_type() == torch::kBool, "mask must be bool");
  int64_t n = mask.numel();
  auto opts32 = mask.options().dtype(torch::kInt32);
  if (n == 0) return torch::empty({0}, opts32);
  Predicate pred{PRED_MASK, mask.data_ptr(), 0, 0.0};
  return std::get<0>(compact(pred, n, opts32, nullptr));
}

torch::Tensor filter_cmp_scalar(torch::Tensor col, int64_t op, double scalar) {
  check_cuda(col, "col");
  int64_t n = col.numel();
  auto opts32 = col.options().dtype(torch::kInt32);
  if (n == 0) return torch::empty({0}, opts32);
  if (col.scalar_type() == torch::kInt32) col = col.to(torch::kInt64);
  TORCH_CHECK(col.scalar_type() == torch::kFloat32 ||
                  col.scalar_type() == torch::kInt64,
              "filter_cmp_scalar supports f32/i64/i32 cols");
  return std::get<0>(
      compact(cmp_predicate(col, op, scalar), n, opts32, nullptr));
}

torch::Tensor gather(torch::Tensor col, torch::Tensor idx) {
  check_cuda(col, "col");
  check_cuda(idx, "idx");
  auto idx32 = idx.scalar_type() == torch::kInt32 ? idx
                                                  : idx.to(torch::kInt32);
  int64_t m = idx32.numel();
  auto out = torch::empty({m}, col.options());
  int esz = (int)col.element_size();
  TORCH_CHECK(esz == 1 || esz == 2 || esz == 4 || esz == 8,
              "unsupported element size");
  if (m)
    launch_gather(col.data_ptr(), idx32.data_ptr<int32_t>(), m,
                  out.data_ptr(), esz, cur_stream());
  return out;
}

// ------------------------------------------------------------------- group-by
std::tuple<torch::Tensor, torch::Tensor> hash_group_i64(torch::Tensor keys) {
  check_cuda(keys, "keys");
  TORCH_CHECK(keys.scalar_type() == torch::kInt64, "keys must be int64");
  int64_t n = keys.numel();
  auto opts32 = keys.options().dtype(torch::kInt32);
  if (n == 0)
    return {torch::empty({0}, opts32), torch::empty({0}, keys.options())};
  uint32_t tsize = next_pow2((uint32_t)std::max<int64_t>(n * 2, 64));
  auto table_keys = torch::empty({(int64_t)tsize}, keys.options());
  auto table_gids = torch::empty({(int64_t)tsize + 1}, opts32);
  auto counter = torch::zeros({1}, opts32);
  auto gids = torch::empty({n}, opts32);
  auto st = cur_stream();
  launch_hash_build(keys.data_ptr<int64_t>(), n,
                    table_keys.data_ptr<int64_t>(),
                    table_gids.data_ptr<int32_t>(), tsize,
                    counter.data_ptr<int32_t>(), gids.data_ptr<int32_t>(), st);
  int64_t g = counter.item<int32_t>();  // sync to size the uniq output
  auto uniq = torch::empty({g}, keys.options());
  launch_hash_export(table_keys.data_ptr<int64_t>(),
                     table_gids.data_ptr<int32_t>(), tsize,
                     uniq.data_ptr<int64_t>(), st);
  return {gids, uniq};
}

torch::Tensor segment_reduce_f32(torch::Tensor vals, torch::Tensor gids,
                                 int64_t g, int64_t op) {
  check_cuda(vals, "vals");
  check_cuda(gids, "gids");
  TORCH_CHECK(vals.scalar_type() == torch::kFloat32, "vals must be f32");
  auto g32 = gids.scalar_type() == torch::kInt32 ? gids
                                                 : gids.to(torch::kInt32);
  auto out = torch::zeros({g}, vals.options());
  if (vals.numel() == 0) return out;
  torch::Tensor scratch;
  int32_t* scratch_ptr = nullptr;
  if (op != 0) {
    scratch = torch::empty({g}, vals.options().dtype(torch::kInt32));
    scratch_ptr = scratch.data_ptr<int32_t>();
  }
  launch_segment_reduce_f32(vals.data_ptr<float>(), g32.data_ptr<int32_t>(),
                            vals.numel(), (int)g, (int)op,
                            out.data_ptr<float>(), scratch_ptr, cur_stream());
  return out;
}

// ----------------------------------------------------------------------- join
std::tuple<torch::Tensor, torch::Tensor> join_inner_i64(torch::Tensor lk,
                                                        torch::Tensor rk) {
  check_cuda(lk, "left_keys");
  check_cuda(rk, "right_keys");
  TORCH_CHECK(lk.scalar_type() == torch::kInt64 &&
                  rk.scalar_type() == torch::kInt64,
              "join keys must be int64");
  int64_t nl = lk.numel(), nr = rk.numel();
  auto opts64 = lk.options();
  auto opts32 = lk.options().dtype(torch::kInt32);
  if (nl == 0 || nr == 0)
    return {torch::empty({0}, opts64), torch::empty({0}, opts64)};
  uint32_t tsize = next_pow2((uint32_t)std::max<int64_t>(nr * 2, 64));
  auto table_keys = torch::empty({(int64_t)tsize}, opts64);
  auto table_head = torch::empty({(int64_t)tsize + 1}, opts32);
  auto next = torch::empty({nr}, opts32);
  auto st = cur_stream();
  launch_join_build(rk.data_ptr<int64_t>(), nr, table_keys.data_ptr<int64_t>(),
                    table_head.data_ptr<int32_t>(), next.data_ptr<int32_t>(),
                    tsize, st);
  auto counts = torch::empty({nl}, opts32);
  launch_join_probe_count(lk.data_ptr<int64_t>(), nl,
                          table_keys.data_ptr<int64_t>(),
                          table_head.data_ptr<int32_t>(),
                          next.data_ptr<int32_t>(), rk.data_ptr<int64_t>(),
                          tsize, counts.data_ptr<int32_t>(), st);
  auto [offs, total_t] = exscan(counts);
  int64_t total = total_t.item<int32_t>();
  auto l_out = torch::empty({total}, opts64);
  auto r_out = torch::empty({total}, opts64);
  if (total)
    launch_join_probe_emit(lk.data_ptr<int64_t>(), nl,
                           table_keys.data_ptr<int64_t>(),
                           table_head.data_ptr<int32_t>(),
                           next.data_ptr<int32_t>(), rk.data_ptr<int64_t>(),
                           tsize, offs.data_ptr<int32_t>(),
                           l_out.data_ptr<int64_t>(),
                           r_out.data_ptr<int64_t>(), st);
  return {l_out, r_out};
}

// ------------------------------------------------------------------ inference
// optional device vector → contiguous fp32 (undefined tensor when absent);
// the kernels read it through a raw pointer, so device and length are checked
torch::Tensor device_vec_f32(const c10::optional<torch::Tensor>& v,
                             int64_t numel, const char* name) {
  if (!v.has_value() || !v->defined()) return torch::Tensor();
  TORCH_CHECK(v->is_cuda(), name, " must be on GPU");
  TORCH_CHECK(v->numel() == numel, name, " must have ", numel, " elements");
  return v->scalar_type() == torch::kFloat32
             ? v->contiguous()
             : v->to(torch::kFloat32).contiguous();
}

// argument checks shared by gemm_bf16 and gemm_bf16_variant; returns the
// fp32 bias (undefined when absent)
torch::Tensor check_gemm_args(const torch::Tensor& A, const torch::Tensor& Bt,
                              const c10::optional<torch::Tensor>& bias) {
  check_cuda(A, "A");
  check_cuda(Bt, "Bt");
  TORCH_CHECK(A.scalar_type() == torch::kBFloat16 &&
                  Bt.scalar_type() == torch::kBFloat16,
              "gemm_bf16 requires bf16 inputs");
  TORCH_CHECK(A.dim() == 2 && Bt.dim() == 2, "A [M,K], Bt [N,K]");
  int64_t K = A.size(1);
  TORCH_CHECK(Bt.size(1) == K, "K mismatch");
  TORCH_CHECK(K % 32 == 0 && K >= 32, "K must be a multiple of 32");
  return device_vec_f32(bias, Bt.size(0), "bias");
}

GemmArgs gemm_args(const torch::Tensor& A, const torch::Tensor& Bt,
                   const torch::Tensor& bias_f, torch::Tensor& C,
                   int64_t act) {
  return GemmArgs{A.data_ptr(), Bt.data_ptr(),
                  bias_f.defined() ? bias_f.data_ptr<float>() : nullptr,
                  C.data_ptr(), (int)A.size(0), (int)Bt.size(0),
                  (int)A.size(1), (int)act, cur_stream()};
}

torch::Tensor gemm_bf16(torch::Tensor A, torch::Tensor Bt,
                        c10::optional<torch::Tensor> bias, int64_t act) {
  auto bias_f = check_gemm_args(A, Bt, bias);
  int64_t M = A.size(0), K = A.size(1), N = Bt.size(0);
  auto C = torch::empty({M, N}, A.options());
  if (M == 0 || N == 0) return C;  // a zero-size grid is a launch error
  GemmArgs g = gemm_args(A, Bt, bias_f, C, act);
  // measured dispatch (profiles/ r02/r06 GEMM tables): big square shapes →
  // 8-phase BM=256+swizzle; everything else → the 128² / 64² tile family.
  // NOTE: 8-phase BM128+swz wins STANDALONE at BERT shapes (+8-16%) but
  // measured ~2% slower in-context (L2-warm inputs; see profiles/ r06) — so
  // only the big-shape case dispatches to the pipelined kernel.
  int64_t t256 = ((M + 255) / 256) * ((N + 255) / 256);
  int rc = (t256 >= 128 && K >= 1536 && N >= 2048)
               ? launch_gemm_bf16(GEMM_8P256S, &g)
               : GEMM_BAD_SHAPE;
  if (rc != GEMM_OK) {
    // narrow outputs: the 128² grid can't fill 256 CUs (e.g. [8192,256] →
    // 128 blocks); the 64² tile quadruples the grid (profiles r2)
    int64_t t128grid = ((M + 127) / 128) * ((N + 127) / 128);
    if (t128grid < 208) {
      rc = launch_gemm_bf16(GEMM_SKINNY, &g);
    } else {
      // K%64==0 (BERT fc1/QKV/fc2 class): the swizzled BK=64 tile wins
      // 6-21% over BK=32 at every such shape measured (profiles r2
      // bench_gemm_k64; register staging + XOR chunk swizzle — the linear
      // layout's 128B-period LDS alias cost ~4e5 bank conflicts/dispatch).
      // Big squares already went to the 8-phase kernel above.
      rc = (K % 64 == 0) ? launch_gemm_bf16(GEMM_K64S, &g) : GEMM_BAD_SHAPE;
      if (rc != GEMM_OK) rc = launch_gemm_bf16(GEMM_BK32, &g);
    }
  }
  TORCH_CHECK(rc == GEMM_OK, "gemm_bf16: no kernel for this shape");
  return C;
}

// scores = x[M,K]·w[K] + bias → f32 (the MLP head: N=1 GEMM + downcast in
// one launch instead of a hipBLASLt GEMV + copy kernel)
torch::Tensor gemv_bf16_f32(torch::Tensor x, torch::Tensor w, double bias) {
  check_cuda(x, "x");
  check_cuda(w, "w");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 &&
              w.scalar_type() == torch::kBFloat16, "bf16 required");
  TORCH_CHECK(x.dim() == 2 && w.numel() == x.size(1), "x [M,K], w [K]");
  auto out = torch::empty({x.size(0)}, x.options().dtype(torch::kFloat32));
  if (x.size(0) == 0) return out;
  launch_gemv_bf16_f32(x.data_ptr(), w.data_ptr(), (float)bias, x.size(0),
                       (int)x.size(1), out.data_ptr<float>(), cur_stream());
  return out;
}

// one fused launch generating every float column + the int64 key column of
// a synthetic batch; ctr[0] advances on-device so graph replays
// re-randomize (ops/stepgraph.py)
void gen_fields(torch::Tensor block, c10::optional<torch::Tensor> key,
                std::vector<double> lo, std::vector<double> width,
                int64_t key_lo, int64_t key_range, torch::Tensor ctr) {
  check_cuda(block, "block");
  TORCH_CHECK(block.dim() == 2 && block.scalar_type() == torch::kFloat32,
              "block must be [nf, n] f32");
  TORCH_CHECK(ctr.scalar_type() == torch::kInt64 && ctr.numel() == 2,
              "ctr must be int64[2] on device");
  int nf = (int)block.size(0);
  int64_t n = block.size(1);
  TORCH_CHECK((int)lo.size() == nf && (int)width.size() == nf);
  std::vector<float> lof(nf), wf(nf);
  for (int f = 0; f < nf; ++f) { lof[f] = (float)lo[f]; wf[f] = (float)width[f]; }
  int64_t* key_ptr = nullptr;
  if (key.has_value() && key->defined()) {
    check_cuda(*key, "key");
    TORCH_CHECK(key->numel() == n && key->scalar_type() == torch::kInt64);
    key_ptr = key->data_ptr<int64_t>();
  } else {
    key_range = 0;
  }
  launch_gen_fields(block.data_ptr<float>(), key_ptr, n, lof.data(),
                    wf.data(), nf, key_lo, key_range,
                    (unsigned long long*)ctr.data_ptr<int64_t>(),
                    cur_stream());
}

// One-launch generate+filter+compact(+featpack): see stepfused.hip
// genfiltpack_kernel. outs = compacted float columns; key_out optional;
// feats optional [cap, dpad] bf16. counts_ws int32[>=256] and bar int64[1]
// are persistent workspaces (the barrier counter is monotonic across graph
// replays — never reset them between steps).
void genfiltpack(std::vector<double> lo, std::vector<double> width,
                 int64_t key_lo, int64_t key_range, int64_t n, int64_t fidx,
                 int64_t op, double scalar,
                 std::vector<torch::Tensor> outs,
                 c10::optional<torch::Tensor> key_out,
                 c10::optional<torch::Tensor> feats,
                 torch::Tensor count_out, torch::Tensor counts_ws,
                 torch::Tensor bar, torch::Tensor ctr) {
  int nf = (int)outs.size();
  TORCH_CHECK(nf >= 1 && nf <= 32, "1..32 float columns");
  TORCH_CHECK((int)lo.size() == nf && (int)width.size() == nf);
  TORCH_CHECK(fidx >= 0 && fidx < nf, "fidx out of range");
  TORCH_CHECK(count_out.scalar_type() == torch::kInt32 &&
              count_out.numel() == 1);
  TORCH_CHECK(counts_ws.scalar_type() == torch::kInt32 &&
              counts_ws.numel() >= (n + 1023) / 1024);
  TORCH_CHECK(bar.scalar_type() == torch::kInt64 && bar.numel() >= 1);
  TORCH_CHECK(ctr.scalar_type() == torch::kInt64 && ctr.numel() == 2);
  std::vector<float> lof(nf), wf(nf);
  std::vector<float*> optr(nf);
  for (int f = 0; f < nf; ++f) {
    lof[f] = (float)lo[f];
    wf[f] = (float)width[f];
    check_cuda(outs[f], "out col");
    TORCH_CHECK(outs[f].numel() >= n &&
                outs[f].scalar_type() == torch::kFloat32);
    optr[f] = outs[f].data_ptr<float>();
  }
  int64_t* kptr = nullptr;
  if (key_out.has_value() && key_out->defined()) {
    TORCH_CHECK(key_out->numel() >= n &&
                key_out->scalar_type() == torch::kInt64);
    kptr = key_out->data_ptr<int64_t>();
  } else {
    key_range = 0;
  }
  void* fptr = nullptr;
  int dpad = 0;
  if (feats.has_value() && feats->defined()) {
    TORCH_CHECK(feats->dim() == 2 &&
                feats->scalar_type() == torch::kBFloat16 &&
                feats->size(0) >= n && feats->size(1) >= nf);
    fptr = feats->data_ptr();
    dpad = (int)feats->size(1);
  }
  int rc = launch_genfiltpack(
      lof.data(), wf.data(), nf, key_lo, key_range, n, (int)fidx, (int)op,
      (float)scalar, optr.data(), kptr, fptr, dpad,
      count_out.data_ptr<int32_t>(), counts_ws.data_ptr<int32_t>(),
      (unsigned long long*)bar.data_ptr<int64_t>(),
      (unsigned long long*)ctr.data_ptr<int64_t>(), cur_stream());
  TORCH_CHECK(rc == 0, "genfiltpack: batch too large for the in-kernel "
              "barrier (max 256K rows) — use the multi-kernel chain");
}

// gathered f32 feature columns → [n, kpad] bf16 MFMA operand in one launch
void featpack(std::vector<torch::Tensor> srcs, torch::Tensor out) {
  TORCH_CHECK(!srcs.empty() && srcs.size() <= 32, "1..32 feature columns");
  check_cuda(out, "out");
  TORCH_CHECK(out.dim() == 2 && out.scalar_type() == torch::kBFloat16,
              "out must be [n, kpad] bf16");
  int64_t n = out.size(0);
  int kpad = (int)out.size(1);
  TORCH_CHECK((int64_t)srcs.size() <= out.size(1),
              "out has fewer columns than sources");
  if (n == 0) return;
  bool f64 = srcs[0].scalar_type() == torch::kFloat64;
  if (f64) {
    std::vector<const double*> ptrs;
    for (auto& s : srcs) {
      check_cuda(s, "src");
      TORCH_CHECK(s.numel() >= n && s.scalar_type() == torch::kFloat64);
      ptrs.push_back(s.data_ptr<double>());
    }
    launch_featpack64(ptrs.data(), (int)ptrs.size(), kpad, n,
                      out.data_ptr(), cur_stream());
    return;
  }
  std::vector<const float*> ptrs;
  for (auto& s : srcs) {
    check_cuda(s, "src");
    TORCH_CHECK(s.numel() >= n && s.scalar_type() == torch::kFloat32);
    ptrs.push_back(s.data_ptr<float>());
  }
  launch_featpack(ptrs.data(), (int)ptrs.size(), kpad, n, out.data_ptr(),
                  cur_stream());
}

// one named kernel of the family (GemmVariant, gemm_api.h) — the A/B hook
// for tests, tools/ and the ARKFLOW_GEMM_VARIANT override
torch::Tensor gemm_bf16_variant(torch::Tensor A, torch::Tensor Bt,
                                c10::optional<torch::Tensor> bias,
                                int64_t act, int64_t variant) {
  auto bias_f = check_gemm_args(A, Bt, bias);
  auto C = torch::empty({A.size(0), Bt.size(0)}, A.options());
  if (C.numel() == 0) return C;
  GemmArgs g = gemm_args(A, Bt, bias_f, C, act);
  int rc = variant == (int)variant ? launch_gemm_bf16((int)variant, &g)
                                   : (int)GEMM_BAD_VARIANT;
  TORCH_CHECK(rc != GEMM_BAD_VARIANT, "unknown gemm variant ", variant);
  TORCH_CHECK(rc == GEMM_OK, "K = ", g.K,
              " not supported by gemm variant ", variant);
  return C;
}

torch::Tensor layernorm_bf16(torch::Tensor x, torch::Tensor gamma,
                             torch::Tensor beta, double eps,
                             c10::optional<torch::Tensor> residual) {
  check_cuda(x, "x");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, "x must be bf16");
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) > 0, "x must be [..., n], n > 0");
  int64_t n = x.size(-1);
  TORCH_CHECK(n % 8 == 0, "inner dim must be a multiple of 8");
  int64_t rows = x.numel() / n;
  TORCH_CHECK(gamma.defined() && beta.defined(), "gamma and beta required");
  auto g = device_vec_f32(gamma, n, "gamma");
  auto b = device_vec_f32(beta, n, "beta");
  auto out = torch::empty_like(x);
  const void* res_ptr = nullptr;
  if (residual.has_value() && residual->defined()) {
    check_cuda(*residual, "residual");
    TORCH_CHECK(residual->scalar_type() == torch::kBFloat16,
                "residual must be bf16");
    TORCH_CHECK(residual->sizes() == x.sizes(),
                "residual must have x's shape");
    res_ptr = residual->data_ptr();
  }
  if (rows == 0) return out;
  launch_layernorm_bf16(x.data_ptr(), res_ptr, g.data_ptr<float>(),
                        b.data_ptr<float>(), out.data_ptr(), nullptr, rows,
                        (int)n, (float)eps, cur_stream());
  return out;
}

torch::Tensor softmax_bf16(torch::Tensor x, double scale) {
  check_cuda(x, "x");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, "x must be bf16");
  int64_t n = x.size(-1);
  TORCH_CHECK(n % 8 == 0, "inner dim must be a multiple of 8");
  int64_t rows = x.numel() / n;
  auto out = torch::empty_like(x);
  launch_softmax_bf16(x.data_ptr(), out.data_ptr(), rows, (int)n,
                      (float)scale, cur_stream());
  return out;
}

// Host-mapped (pinned, device-visible) int32 buffer: the capture-safe filter
// writes its surviving-row count HERE over PCIe, so consuming a fused step is
// a stream sync + CPU load instead of a hipMemcpyDtoH launch + sync
// (flagship step is ~0.1 ms; the D2H readback was ~10 us of it).
// Returns (host_view, device_view) over the same allocation — keep both
// alive; freeing follows the host view.
std::vector<torch::Tensor> mapped_int32(int64_t n) {
  TORCH_CHECK(n > 0, "n must be positive");
  void* hp = nullptr;
  auto err = hipHostMalloc(&hp, n * sizeof(int32_t), hipHostMallocMapped);
  TORCH_CHECK(err == hipSuccess, "hipHostMalloc failed: ",
              hipGetErrorString(err));
  memset(hp, 0, n * sizeof(int32_t));
  void* dp = nullptr;
  err = hipHostGetDevicePointer(&dp, hp, 0);
  if (err != hipSuccess) {
    hipHostFree(hp);
    TORCH_CHECK(false, "hipHostGetDevicePointer failed: ",
                hipGetErrorString(err));
  }
  auto host = torch::from_blob(
      hp, {n}, [](void* p) { hipHostFree(p); },
      torch::TensorOptions().dtype(torch::kInt32));
  auto dev = torch::from_blob(
      dp, {n},
      torch::TensorOptions().dtype(torch::kInt32).device(torch::kCUDA));
  return {host, dev};
}

torch::Tensor bias_act_bf16(torch::Tensor x,
                            c10::optional<torch::Tensor> bias, int64_t act) {
  check_cuda(x, "x");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, "x must be bf16");
  auto out = torch::empty_like(x);
  if (x.numel() == 0) return out;
  TORCH_CHECK(x.dim() >= 1, "x must be [..., n]");
  int64_t n = x.size(-1);
  int64_t rows = x.numel() / n;
  auto bias_f = device_vec_f32(bias, n, "bias");
  const float* bias_ptr =
      bias_f.defined() ? bias_f.data_ptr<float>() : nullptr;
  launch_bias_act_bf16(x.data_ptr(), bias_ptr, out.data_ptr(), rows, (int)n,
                       (int)act, cur_stream());
  return out;
}

// Valid-length argument of the attention bindings: absent (an undefined
// tensor is returned: the unmasked kernels), or an int32 [B] contiguous
// device tensor. Checked before any launch; its VALUES are never read on the
// host (no sync, capturable) — the kernels clamp them to [0, S].
static torch::Tensor check_lens(const c10::optional<torch::Tensor>& lens,
                                int64_t B, const torch::Tensor& like) {
  if (!lens.has_value() || !lens->defined()) return {};
  TORCH_CHECK(lens->is_cuda() && lens->device() == like.device(),
              "lens must be on the inputs' device");
  TORCH_CHECK(lens->scalar_type() == torch::kInt32, "lens must be int32");
  TORCH_CHECK(lens->dim() == 1 && lens->size(0) == B,
              "lens must be 1-D of length B=", B);
  TORCH_CHECK(lens->is_contiguous(), "lens must be contiguous");
  return *lens;
}

// What both attention bindings do once their layout is in `a`: `lens` is
// check_lens' result with a.B entries.
static void run_attention(const char* name, AttnArgs a,
                          const torch::Tensor& lens) {
  a.lens = lens.defined() ? lens.data_ptr<int32_t>() : nullptr;
  a.stream = cur_stream();
  int rc = launch_attention_bf16(&a);
  TORCH_CHECK(rc == 0, name, ": unsupported shape S=", a.S, " D=", a.D);
}

torch::Tensor attention_bf16(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                             double scale,
                             c10::optional<torch::Tensor> lens) {
  check_cuda(q, "q");
  check_cuda(k, "k");
  check_cuda(v, "v");
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16, "attention requires bf16");
  TORCH_CHECK(q.dim() == 4, "q must be [B,H,S,D]");
  TORCH_CHECK(k.scalar_type() == q.scalar_type() &&
                  v.scalar_type() == q.scalar_type(),
              "k and v must match q's dtype");
  TORCH_CHECK(k.sizes() == q.sizes() && v.sizes() == q.sizes(),
              "k and v must match q's shape");
  int64_t B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3);
  // the packed layout is BH independent rows: one length per (b, h)
  torch::Tensor lens_bh = check_lens(lens, B, q);
  if (lens_bh.defined() && H != 1)
    lens_bh = lens_bh.repeat_interleave(H).contiguous();
  auto out = torch::empty_like(q);
  run_attention("attention_bf16",
                {q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(),
                 (int)(B * H), 1, (int)S, (int)D, (int)D, (int)D, (float)scale,
                 8},
                lens_bh);
  return out;
}

// qkv [B,S,3,H,D] (the QKV linear's output reshaped) → O [B,S,H*D];
// the kernel reads strided rows directly — no permute/contiguous copies.
torch::Tensor attention_qkv_bf16(torch::Tensor qkv, double scale,
                                 int64_t pad,
                                 c10::optional<torch::Tensor> lens) {
  check_cuda(qkv, "qkv");
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16, "qkv must be bf16");
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(2) == 3, "qkv must be [B,S,3,H,D]");
  int64_t B = qkv.size(0), S = qkv.size(1), H = qkv.size(3), D = qkv.size(4);
  torch::Tensor lens_b = check_lens(lens, B, qkv);
  auto out = torch::empty({B, S, H * D}, qkv.options());
  const at::BFloat16* base = qkv.data_ptr<at::BFloat16>();
  run_attention("attention_qkv_bf16",
                {base, base + H * D, base + 2 * H * D, out.data_ptr(), (int)B,
                 (int)H, (int)S, (int)D, (int)(3 * H * D), (int)(H * D),
                 (float)scale, (int)pad},
                lens_b);
  return out;
}

std::vector<torch::Tensor> gather_columns(std::vector<torch::Tensor> cols,
                                          torch::Tensor idx) {
  check_cuda(idx, "idx");
  for (auto& c : cols) check_cuda(c, "col");
  auto idx32 = idx.scalar_type() == torch::kInt32 ? idx : idx.to(torch::kInt32);
  return gather_multi(cols, idx32, idx32.numel(), nullptr, {});
}

// Stable LSD radix sort of n > 0 unsigned keys by their low `npasses` bytes:
// uint32 bits in an int32 tensor, or (wide) uint64 bits in an int64 tensor.
// Returns (permutation, sorted keys).
std::tuple<torch::Tensor, torch::Tensor> radix_sort_passes(torch::Tensor ka,
                                                           bool wide,
                                                           int npasses) {
  int64_t n = ka.numel();
  auto opts32 = ka.options().dtype(torch::kInt32);
  auto st = cur_stream();
  int nblocks = onesweep_nblocks(n);
  auto hist = torch::empty({(int64_t)256 * nblocks}, opts32);
  auto kb = torch::empty_like(ka);
  auto idx_a = torch::arange(n, opts32);
  auto idx_b = torch::empty({n}, opts32);
  for (int p = 0; p < npasses; ++p) {
    if (wide)
      launch_os_hist256_u64((const uint64_t*)ka.data_ptr<int64_t>(), n,
                            8 * p, hist.data_ptr<int32_t>(), nblocks, st);
    else
      launch_os_hist256_u32((const uint32_t*)ka.data_ptr<int32_t>(), n,
                            8 * p, hist.data_ptr<int32_t>(), nblocks, st);
    // one device scan turns bin-major block counts into global offsets
    auto inc = hist.cumsum(0, torch::kInt32);
    auto offs = (inc - hist).contiguous();
    if (wide)
      launch_onesweep_pass_u64((const uint64_t*)ka.data_ptr<int64_t>(),
                               idx_a.data_ptr<int32_t>(),
                               (uint64_t*)kb.data_ptr<int64_t>(),
                               idx_b.data_ptr<int32_t>(), n, 8 * p,
                               offs.data_ptr<int32_t>(), nblocks, st);
    else
      launch_onesweep_pass_u32((const uint32_t*)ka.data_ptr<int32_t>(),
                               idx_a.data_ptr<int32_t>(),
                               (uint32_t*)kb.data_ptr<int32_t>(),
                               idx_b.data_ptr<int32_t>(), n, 8 * p,
                               offs.data_ptr<int32_t>(), nblocks, st);
    std::swap(ka, kb);
    std::swap(idx_a, idx_b);
  }
  return {idx_a, ka};
}

torch::Tensor radix_argsort(torch::Tensor keys, bool descending) {
  // Onesweep: 8-bit digits + decoupled lookback, keys ping-ponged alongside
  // the permutation (radix_sort.hip onesweep_* kernels). f32/i32 → 4 chained
  // passes, i64 → 8. The 4-bit two-kernel LSD this replaces measured ~6× off
  // rocPRIM at 10M keys (profiles r04 / VERDICT weak #7).
  check_cuda(keys, "keys");
  int64_t n = keys.numel();
  auto opts32 = keys.options().dtype(torch::kInt32);
  if (n == 0) return torch::empty({0}, opts32);
  TORCH_CHECK(n < (int64_t)1 << 30, "radix_argsort caps at 2^30 rows");
  auto st = cur_stream();
  bool wide;  // 64-bit key path
  torch::Tensor ka;
  if (keys.scalar_type() == torch::kFloat32) {
    wide = false;
    ka = torch::empty({n}, opts32);  // uint32 bits in an int32 tensor
    launch_f32_to_ordered(keys.data_ptr<float>(),
                          (uint32_t*)ka.data_ptr<int32_t>(), n,
                          descending ? 1 : 0, st);
  } else if (keys.scalar_type() == torch::kInt32) {
    wide = false;
    ka = torch::empty({n}, opts32);
    launch_i32_to_ordered(keys.data_ptr<int32_t>(),
                          (uint32_t*)ka.data_ptr<int32_t>(), n,
                          descending ? 1 : 0, st);
  } else if (keys.scalar_type() == torch::kInt64) {
    wide = true;
    ka = torch::empty({n}, keys.options().dtype(torch::kInt64));
    launch_i64_to_ordered(keys.data_ptr<int64_t>(),
                          (uint64_t*)ka.data_ptr<int64_t>(), n,
                          descending ? 1 : 0, st);
  } else {
    TORCH_CHECK(false, "radix_argsort supports f32/i64/i32 keys");
  }
  return std::get<0>(radix_sort_passes(ka, wide, wide ? 8 : 4));
}

// ---------------------------------------------------------------- string order
void check_binary(const torch::Tensor& data, const torch::Tensor& offsets) {
  check_cuda(data, "data");
  check_cuda(offsets, "offsets");
  TORCH_CHECK(data.scalar_type() == torch::kUInt8, "data must be uint8");
  TORCH_CHECK(offsets.scalar_type() == torch::kInt64 && offsets.numel() >= 1,
              "offsets must be int64 with rows + 1 entries");
}

torch::Tensor bytes_compare_cols(torch::Tensor data_a, torch::Tensor offsets_a,
                                 torch::Tensor data_b,
                                 torch::Tensor offsets_b) {
  check_binary(data_a, offsets_a);
  check_binary(data_b, offsets_b);
  int64_t n = offsets_a.numel() - 1;
  TORCH_CHECK(offsets_b.numel() - 1 == n,
              "bytes_compare: columns differ in row count");
  auto out = torch::empty({n}, data_a.options().dtype(torch::kInt8));
  launch_bytes_compare_cols(data_a.data_ptr<uint8_t>(),
                            offsets_a.data_ptr<int64_t>(),
                            data_b.data_ptr<uint8_t>(),
                            offsets_b.data_ptr<int64_t>(), n,
                            out.data_ptr<int8_t>(), cur_stream());
  return out;
}

torch::Tensor bytes_compare_lit(torch::Tensor data, torch::Tensor offsets,
                                std::string lit) {
  check_binary(data, offsets);
  int64_t n = offsets.numel() - 1;
  auto out = torch::empty({n}, data.options().dtype(torch::kInt8));
  if (n == 0) return out;
  // 8 copies of the literal, copy s shifted s bytes into its 8-byte-aligned
  // slab, so a row of any alignment has a copy it can compare by words
  int64_t nl = (int64_t)lit.size();
  int64_t slab = (nl + 8 + 7) / 8 * 8;
  std::vector<uint8_t> host((size_t)(8 * slab), 0);
  for (int s = 0; s < 8; ++s)
    std::copy(lit.begin(), lit.end(), host.begin() + s * slab + s);
  auto lit8 = torch::from_blob(host.data(), {8 * slab}, torch::kUInt8)
                  .to(data.device());  // blocking: host outlives the copy
  launch_bytes_compare_lit(data.data_ptr<uint8_t>(),
                           offsets.data_ptr<int64_t>(), n,
                           lit8.data_ptr<uint8_t>(), slab, nl,
                           out.data_ptr<int8_t>(), cur_stream());
  return out;
}

// Dense rank of the rows of a binary column: rank[i] = number of distinct
// strings smaller than row i. Chunk-at-a-time refinement (bytes_order.hip):
// per round two radix sorts over the open rows, a head-flag scan for the new
// segment ids, and ONE scalar readback — the number of rows still open
// (mask_to_indices sizes the next round with it).
torch::Tensor bytes_rank(torch::Tensor data, torch::Tensor offsets) {
  check_binary(data, offsets);
  int64_t n = offsets.numel() - 1;
  auto opts32 = offsets.options().dtype(torch::kInt32);
  auto rank = torch::zeros({n}, offsets.options());
  if (n <= 1) return rank;
  TORCH_CHECK(n < (int64_t)1 << 30, "bytes_rank caps at 2^30 rows");
  auto st = cur_stream();
  auto perm = torch::arange(n, opts32);  // position -> row
  auto seg = torch::zeros({n}, opts32);  // position -> dense segment id
  auto head = torch::empty({n}, opts32);
  auto pos = perm.clone();               // open positions, ascending
  int seg_passes = 1;                    // radix bytes that hold an id < n
  while (seg_passes < 4 && ((n - 1) >> (8 * seg_passes)) != 0) ++seg_passes;
  const uint8_t* dptr = data.data_ptr<uint8_t>();
  const int64_t* optr = offsets.data_ptr<int64_t>();
  for (int64_t d = 0;; ++d) {
    int64_t m = pos.numel();
    auto key = torch::empty({m}, offsets.options());
    auto row_o = torch::empty({m}, opts32);
    auto seg_o = torch::empty({m}, opts32);
    launch_bo_chunk_keys(dptr, optr, perm.data_ptr<int32_t>(),
                         seg.data_ptr<int32_t>(), pos.data_ptr<int32_t>(), m,
                         d, (uint64_t*)key.data_ptr<int64_t>(),
                         row_o.data_ptr<int32_t>(), seg_o.data_ptr<int32_t>(),
                         st);
    // stable sort by key, then by segment: segments keep their places and
    // are ordered by key inside
    auto [idx_a, key_a] = radix_sort_passes(key, /*wide=*/true, 8);
    auto seg_a = torch::empty({m}, opts32);
    launch_gather(seg_o.data_ptr(), idx_a.data_ptr<int32_t>(), m,
                  seg_a.data_ptr(), 4, st);
    auto [idx_b, seg_b] = radix_sort_passes(seg_a, /*wide=*/false, seg_passes);
    auto open = torch::zeros({n}, offsets.options().dtype(torch::kBool));
    launch_bo_apply_round(idx_a.data_ptr<int32_t>(), idx_b.data_ptr<int32_t>(),
                          (const uint64_t*)key_a.data_ptr<int64_t>(),
                          seg_b.data_ptr<int32_t>(), row_o.data_ptr<int32_t>(),
                          pos.data_ptr<int32_t>(), m, perm.data_ptr<int32_t>(),
                          head.data_ptr<int32_t>(), open.data_ptr<bool>(), st);
    auto offs = exclusive_offsets(head);
    launch_bo_segments(offs.data_ptr<int64_t>(), n, seg.data_ptr<int32_t>(),
                       st);
    pos = mask_to_indices(open);
    if (pos.numel() == 0) break;
  }
  launch_bo_scatter_rank(perm.data_ptr<int32_t>(), seg.data_ptr<int32_t>(), n,
                         rank.data_ptr<int64_t>(), st);
  return rank;
}

// one-call C++ execution of `SELECT * FROM flow WHERE col OP literal`:
// fused compare+compact then one multi-column gather — a single host→device
// round trip instead of per-op Python dispatch (the native pipeline-executor
// path; reference's Pipeline is compiled Rust end to end).
std::tuple<std::vector<torch::Tensor>, int64_t> fused_filter_gather(
    std::vector<torch::Tensor> cols, int64_t filter_idx, int64_t op,
    double scalar) {
  TORCH_CHECK(filter_idx >= 0 && filter_idx < (int64_t)cols.size());
  auto col = cols[filter_idx];
  check_cuda(col, "filter col");
  int64_t n = col.numel();
  torch::Tensor idx;
  int64_t total = 0;
  if (n > 0) {
    if (col.scalar_type() != torch::kFloat32 &&
        col.scalar_type() != torch::kInt64)
      col = col.to(torch::kInt64);
    std::tie(idx, total) =
        compact(cmp_predicate(col, op, scalar), n,
                col.options().dtype(torch::kInt32), nullptr);
  }
  return {gather_multi(cols, idx, total, nullptr, {}), total};
}

// hipGraph-capturable variant of fused_filter_gather: writes compacted rows
// into PREALLOCATED padded outputs and the row count into a device int32 —
// zero host syncs, so generate→filter→infer captures as ONE graph
// (the flagship step was host-dispatch-bound at batch 8192).
void filter_gather_capture(std::vector<torch::Tensor> cols,
                           int64_t filter_idx, int64_t op, double scalar,
                           std::vector<torch::Tensor> outs,
                           torch::Tensor count_out) {
  TORCH_CHECK(filter_idx >= 0 && filter_idx < (int64_t)cols.size());
  TORCH_CHECK(outs.size() == cols.size(), "outs must match cols");
  TORCH_CHECK(count_out.scalar_type() == torch::kInt32 &&
              count_out.numel() == 1, "count_out must be int32[1] on device");
  auto col = cols[filter_idx];
  check_cuda(col, "filter col");
  int64_t n = col.numel();
  TORCH_CHECK(n > 0, "capture path requires a non-empty static batch");
  TORCH_CHECK(col.scalar_type() == torch::kFloat32 ||
                  col.scalar_type() == torch::kInt64,
              "capture filter col must be f32 or i64");
  for (size_t c = 0; c < cols.size(); ++c)
    TORCH_CHECK(outs[c].numel() >= n &&
                outs[c].element_size() == cols[c].element_size(),
                "out buffer too small or wrong dtype");
  auto idx = std::get<0>(compact(cmp_predicate(col, op, scalar), n,
                                 col.options().dtype(torch::kInt32),
                                 &count_out));
  gather_multi(cols, idx, n, count_out.data_ptr<int32_t>(), outs);
}

// one-call `SELECT key, count(*), AGG(col)… FROM flow WHERE fcol OP lit
// GROUP BY key`: fused filter → key/value gather → LDS hash group →
// segment reductions, chained in C++ with exactly TWO host syncs (surviving
// row count, group count). The Python-op version of this chain is
// host-dispatch-bound at stream batch sizes (BASELINE config 2 @8192).
// val_ops: 0=sum 1=min 2=max per value column. Returns
// (unique_keys, group_counts_f32, [reduced…]).
std::tuple<torch::Tensor, torch::Tensor, std::vector<torch::Tensor>>
fused_filter_agg(torch::Tensor key, torch::Tensor filter_col, int64_t op,
                 double scalar, std::vector<torch::Tensor> val_cols,
                 std::vector<int64_t> val_ops) {
  check_cuda(key, "key");
  check_cuda(filter_col, "filter_col");
  TORCH_CHECK(key.scalar_type() == torch::kInt64, "key must be int64");
  TORCH_CHECK(filter_col.scalar_type() == torch::kFloat32,
              "filter col must be f32");
  TORCH_CHECK(val_cols.size() == val_ops.size());
  int64_t n = key.numel();
  auto st = cur_stream();
  auto opts32 = key.options().dtype(torch::kInt32);
  std::vector<torch::Tensor> cols = {key, filter_col};
  for (auto& v : val_cols) {
    check_cuda(v, "val col");
    TORCH_CHECK(v.scalar_type() == torch::kFloat32, "val cols must be f32");
    cols.push_back(v);
  }
  auto [outs, total] = fused_filter_gather(cols, 1, op, scalar);
  auto gkey = outs[0];
  if (total == 0) {
    std::vector<torch::Tensor> empt;
    for (size_t i = 0; i < val_cols.size(); ++i)
      empt.push_back(torch::empty({0}, filter_col.options()));
    return {torch::empty({0}, key.options()),
            torch::empty({0}, filter_col.options()), empt};
  }
  auto [gids, uniq] = hash_group_i64(gkey);
  int64_t g = uniq.numel();
  // counts via the f32 LDS-buffered segment sum (exact < 2^24 per group)
  auto ones = torch::ones({total}, filter_col.options());
  auto counts = segment_reduce_f32(ones, gids, g, 0);
  std::vector<torch::Tensor> reduced;
  for (size_t i = 0; i < val_cols.size(); ++i)
    reduced.push_back(segment_reduce_f32(outs[2 + i], gids, g,
                                         val_ops[i]));
  return {uniq, counts, reduced};
}

// Capture-safe GROUP BY: padded key/value columns + the filter's device row
// count in, padded (g_cap) group table out, group count written to
// gcount_out (host-mapped int32 — ONE CPU read per step, zero D2H copies).
// Records into a hipGraph: static grids, no host syncs; all workspaces are
// allocated here (graph-pool when called during capture). Reference analog:
// DataFusion AggregateExec (processor/sql.rs execute_query) as a replayable
// device-side program.
std::tuple<torch::Tensor, torch::Tensor, std::vector<torch::Tensor>>
hash_agg_capture(torch::Tensor keys, torch::Tensor nrow,
                 std::vector<torch::Tensor> vals, std::vector<int64_t> ops,
                 int64_t table_size, int64_t g_cap,
                 c10::optional<torch::Tensor> gcount_out) {
  check_cuda(keys, "keys");
  check_cuda(nrow, "nrow");
  TORCH_CHECK(keys.scalar_type() == torch::kInt64, "keys must be int64");
  TORCH_CHECK(nrow.scalar_type() == torch::kInt32 && nrow.numel() == 1,
              "nrow must be device int32[1]");
  TORCH_CHECK((table_size & (table_size - 1)) == 0, "table_size pow2");
  TORCH_CHECK(g_cap >= 1 && g_cap <= 2048, "g_cap must be in [1, 2048]");
  TORCH_CHECK(vals.size() == ops.size());
  TORCH_CHECK(vals.size() <= 4, "hash_agg_capture supports up to 4 "
              "reduction columns");
  int64_t n_cap = keys.numel();
  auto st = cur_stream();
  auto opts32 = keys.options().dtype(torch::kInt32);
  auto optsf = keys.options().dtype(torch::kFloat32);
  auto table_keys = torch::empty({table_size}, keys.options());
  auto table_gids = torch::empty({table_size + 1}, opts32);
  auto counter = torch::empty({1}, opts32);
  auto gids = torch::empty({std::max<int64_t>(n_cap, 1)}, opts32);
  auto counts = torch::empty({g_cap}, optsf);
  auto counts_i64 = torch::empty({g_cap}, keys.options());
  auto uniq = torch::zeros({g_cap}, keys.options());
  int nv = (int)vals.size();
  std::vector<torch::Tensor> red;
  std::vector<const float*> vptr;
  std::vector<float*> rptr;
  std::vector<int32_t*> mptr;
  std::vector<int> opsi;
  std::vector<torch::Tensor> scratch_keep;
  for (int i = 0; i < nv; ++i) {
    check_cuda(vals[i], "val");
    TORCH_CHECK(vals[i].scalar_type() == torch::kFloat32,
                "val cols must be f32");
    red.push_back(torch::empty({g_cap}, optsf));
    vptr.push_back(vals[i].data_ptr<float>());
    rptr.push_back(red.back().data_ptr<float>());
    if (ops[i] != 0) {
      scratch_keep.push_back(torch::empty({g_cap}, opts32));
      mptr.push_back(scratch_keep.back().data_ptr<int32_t>());
    } else {
      mptr.push_back(nullptr);
    }
    opsi.push_back((int)ops[i]);
  }
  int32_t* gout = nullptr;
  if (gcount_out.has_value() && gcount_out->defined()) {
    TORCH_CHECK(gcount_out->scalar_type() == torch::kInt32 &&
                gcount_out->numel() == 1);
    gout = gcount_out->data_ptr<int32_t>();
  }
  launch_hash_agg_capture(
      keys.data_ptr<int64_t>(), nrow.data_ptr<int32_t>(), n_cap,
      table_keys.data_ptr<int64_t>(), table_gids.data_ptr<int32_t>(),
      (uint32_t)table_size, counter.data_ptr<int32_t>(),
      gids.data_ptr<int32_t>(), counts.data_ptr<float>(), (int)g_cap,
      vptr.data(), opsi.data(), rptr.data(), mptr.data(), nv,
      uniq.data_ptr<int64_t>(), counts_i64.data_ptr<int64_t>(), gout, st);
  return {uniq, counts_i64, red};
}

using StringColumns = std::vector<std::tuple<torch::Tensor, torch::Tensor>>;

// String copy-out of a decoder. lens is the int32 [ns][n] lengths tensor its
// parse kernel filled; per slot, offsets = exclusive cumsum of the lengths
// (an absent value has length 0 → empty string). `head` holds the decoder's
// own leading summary entries (int64, on the device): they and the slot
// totals ride ONE concatenated readback, the batch's only device sync — the
// earlier shape (err.item + validity .cpu + totals .to(CPU)) cost three
// stream drains per batch and floored small-batch decode at ~0.2 ms. Then
// launch(s, offs, out) fills slot s's `out` where its total is > 0.
// Returns (per slot (data, offsets), summary = [head..., totals...] on host).
template <typename Launch>
std::tuple<StringColumns, torch::Tensor> copy_out_strings(
    const torch::Tensor& lens, int64_t ns, int64_t n,
    std::vector<torch::Tensor> head, Launch launch) {
  if (n == 0) ns = 0;
  int64_t lead = 0;
  for (const auto& h : head) lead += h.numel();
  std::vector<torch::Tensor> offs(std::max<int64_t>(ns, 0));
  for (int64_t s = 0; s < ns; ++s) {
    offs[s] = exclusive_offsets(lens[s].contiguous());
    head.push_back(offs[s].narrow(0, n, 1));
  }
  auto summary = torch::cat(head).cpu();  // the one device sync
  const int64_t* tot = summary.data_ptr<int64_t>() + lead;
  StringColumns strings;
  for (int64_t s = 0; s < ns; ++s) {
    auto out = torch::empty({std::max<int64_t>(tot[s], 1)},
                            lens.options().dtype(torch::kUInt8));
    if (tot[s] > 0) launch(s, offs[s], out);
    strings.emplace_back(out.slice(0, 0, tot[s]), offs[s]);
  }
  return {strings, summary};
}

// (out_f64, out_i64, found, err, strings, summary); summary = [err,
// all_valid × max(nf, 1), string totals × n_str] on the host.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           StringColumns, torch::Tensor>
json_decode(torch::Tensor data, torch::Tensor offsets,
            std::vector<std::string> names, std::vector<int64_t> kind,
            std::vector<int64_t> slot, int64_t n_int, int64_t n_float,
            int64_t n_str) {
  check_cuda(data, "data");
  check_cuda(offsets, "offsets");
  int64_t n = offsets.numel() - 1;
  TORCH_CHECK(names.size() <= JSON_MAX_FIELDS, "json_decode takes at most ",
              JSON_MAX_FIELDS, " fields, got ", names.size());
  TORCH_CHECK(kind.size() == names.size() && slot.size() == names.size());
  const int nf = (int)names.size();
  JsonSpec spec{};
  spec.nf = nf;
  // dotted names ("user.id") address one level of nesting: collect the
  // distinct parent segments, scope each field to its parent index
  std::vector<std::string> parents;
  for (int f = 0; f < nf; ++f) {
    std::string leaf = names[f];
    spec.parent[f] = -1;
    auto dot = leaf.find('.');
    if (dot != std::string::npos) {
      std::string parent = leaf.substr(0, dot);
      leaf = leaf.substr(dot + 1);
      TORCH_CHECK(leaf.find('.') == std::string::npos,
                  "json paths support one nesting level: ", names[f]);
      int pi = -1;
      for (size_t q = 0; q < parents.size(); ++q)
        if (parents[q] == parent) pi = (int)q;
      if (pi < 0) {
        TORCH_CHECK(parents.size() < JSON_MAX_PARENTS,
                    "too many nested parents (max ", JSON_MAX_PARENTS, ")");
        TORCH_CHECK(parent.size() < JSON_MAX_NAME,
                    "json parent name too long");
        pi = (int)parents.size();
        parents.push_back(parent);
        memcpy(spec.parents[pi], parent.data(), parent.size());
        spec.parent_len[pi] = (int)parent.size();
      }
      spec.parent[f] = pi;
    }
    TORCH_CHECK(leaf.size() < JSON_MAX_NAME, "json field name too long");
    memcpy(spec.names[f], leaf.data(), leaf.size());
    spec.name_len[f] = (int)leaf.size();
    const int64_t slots = kind[f] == 2 ? n_str : kind[f] == 1 ? n_float : n_int;
    TORCH_CHECK(kind[f] >= 0 && kind[f] <= 2 && slot[f] >= 0 &&
                    slot[f] < slots, "json field kind or slot out of range");
    spec.kind[f] = (int)kind[f];
    spec.slot[f] = (int)slot[f];
  }
  spec.np = (int)parents.size();
  auto rows = [&](int64_t r, torch::ScalarType t) {
    return torch::zeros({std::max<int64_t>(r, 1), std::max<int64_t>(n, 1)},
                        data.options().dtype(t));
  };
  auto out_f = rows(n_float, torch::kFloat64);
  auto out_i = rows(n_int, torch::kInt64);
  auto str_start = rows(n_str, torch::kInt64);
  auto str_ulen = rows(n_str, torch::kInt32);
  auto found = rows(nf, torch::kUInt8);
  auto err = torch::zeros({1}, data.options().dtype(torch::kInt32));
  auto found_count = torch::zeros({std::max(nf, 1)},
                                  data.options().dtype(torch::kInt32));
  if (n > 0)
    launch_json_decode(&spec, data.data_ptr<uint8_t>(),
                       offsets.data_ptr<int64_t>(), n,
                       out_f.data_ptr<double>(), out_i.data_ptr<int64_t>(),
                       str_start.data_ptr<int64_t>(),
                       str_ulen.data_ptr<int32_t>(),
                       found.data_ptr<uint8_t>(), err.data_ptr<int32_t>(),
                       found_count.data_ptr<int32_t>(),
                       // wave-per-doc parse pays off only when string
                       // scans dwarf the per-doc state machine (which the
                       // thread-per-doc kernel amortizes 64 docs/wave):
                       // measured crossover is in the multi-KB range
                       (int)(data.numel() / n >= 2048), cur_stream());
  // all_valid[f] ⇔ found_count[f] == n (counts accumulated in-kernel — a
  // found.min(dim=1) reduce cost ~40 µs/batch); validity = found
  auto all_valid = (found_count.to(torch::kInt64) ==
                    torch::full({std::max(nf, 1)}, n,
                                torch::dtype(torch::kInt64)
                                    .device(data.device())))
                       .to(torch::kInt64);
  auto [strings, summary] = copy_out_strings(
      str_ulen, n_str, n, {err.to(torch::kInt64), all_valid},
      [&](int64_t s, const torch::Tensor& offs, torch::Tensor& out) {
        // found row for this slot: the field index with this slot
        int frow = 0;
        for (int f = 0; f < nf; ++f)
          if (spec.kind[f] == 2 && spec.slot[f] == (int)s) frow = f;
        // wave-per-doc for long strings (coalesced fast path); the
        // thread-per-doc kernel stays ahead when strings are tiny
        auto* copy = out.numel() / n >= 32  // out holds the slot's total
                         ? launch_json_copy_strings_wave
                         : launch_json_copy_strings;
        copy(data.data_ptr<uint8_t>(), str_start[s].data_ptr<int64_t>(),
             offs.data_ptr<int64_t>(), found[frow].data_ptr<uint8_t>(), n,
             data.numel(), out.data_ptr<uint8_t>(), cur_stream());
      });
  return {out_f, out_i, found, err, strings, summary};
}

// gather rows of a binary column: (data, offsets, idx) -> (out_data,
// out_offsets). Device prefix-sum for the new offsets + span-copy kernel;
// ONE host sync (the total, needed for allocation).
std::tuple<torch::Tensor, torch::Tensor> take_binary(torch::Tensor data,
                                                     torch::Tensor offsets,
                                                     torch::Tensor idx) {
  check_cuda(data, "data");
  check_cuda(offsets, "offsets");
  check_cuda(idx, "idx");
  int64_t n = offsets.numel() - 1;
  auto idx64 = idx.scalar_type() == torch::kInt64 ? idx : idx.to(torch::kInt64);
  int64_t m = idx64.numel();
  auto lens_all = offsets.slice(0, 1, n + 1) - offsets.slice(0, 0, n);
  auto lens = lens_all.index_select(0, idx64).to(torch::kInt32);
  auto starts = offsets.slice(0, 0, n).index_select(0, idx64).contiguous();
  auto new_off = exclusive_offsets(lens.contiguous());
  int64_t total = m ? new_off.narrow(0, m, 1).item<int64_t>() : 0;
  auto out = torch::empty({std::max<int64_t>(total, 1)},
                          data.options().dtype(torch::kUInt8));
  if (total > 0)
    launch_proto_copy_bytes(data.data_ptr<uint8_t>(),
                            starts.data_ptr<int64_t>(),
                            new_off.data_ptr<int64_t>(), m,
                            out.data_ptr<uint8_t>(), cur_stream());
  return {out.slice(0, 0, total), new_off};
}

torch::Tensor bytes_match(torch::Tensor data, torch::Tensor offsets,
                          std::string needle, int64_t mode) {
  check_cuda(data, "data");
  check_cuda(offsets, "offsets");
  TORCH_CHECK(needle.size() <= 64, "LIKE needle too long for device match");
  int64_t n = offsets.numel() - 1;
  auto out = torch::empty({n}, data.options().dtype(torch::kBool));
  if (n > 0)
    launch_bytes_match(data.data_ptr<uint8_t>(), offsets.data_ptr<int64_t>(),
                       n, (const uint8_t*)needle.data(), (int)needle.size(),
                       (int)mode, out.data_ptr<bool>(), cur_stream());
  return out;
}

torch::Tensor bytes_hash(torch::Tensor data, torch::Tensor offsets) {
  check_cuda(data, "data");
  check_cuda(offsets, "offsets");
  int64_t n = offsets.numel() - 1;
  auto out = torch::empty({n}, offsets.options().dtype(torch::kInt64));
  if (n > 0)
    launch_bytes_hash(data.data_ptr<uint8_t>(), offsets.data_ptr<int64_t>(),
                      n, out.data_ptr<int64_t>(), cur_stream());
  return out;
}

// (out_i64, out_f64, err, strings, summary); summary = [err, string totals ×
// n_str] on the host, empty in capture mode. is_float[f] repeats what kind[f]
// says (F64/F32 → the float64 outputs) and is only checked against it.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, StringColumns,
           torch::Tensor>
proto_decode(
    torch::Tensor data, torch::Tensor offsets,
    std::vector<int64_t> fno, std::vector<int64_t> kind,
    std::vector<int64_t> is_float, std::vector<int64_t> slot,
    int64_t n_int, int64_t n_float, int64_t n_str, bool capture) {
  check_cuda(data, "data");
  check_cuda(offsets, "offsets");
  TORCH_CHECK(data.scalar_type() == torch::kUInt8);
  TORCH_CHECK(offsets.scalar_type() == torch::kInt64);
  int64_t n = offsets.numel() - 1;
  const size_t nf = fno.size();
  TORCH_CHECK(nf <= PROTO_MAX_FIELDS, "proto_decode takes at most ",
              PROTO_MAX_FIELDS, " fields, got ", nf);
  TORCH_CHECK(kind.size() == nf && is_float.size() == nf && slot.size() == nf);
  ProtoSpec spec{};
  spec.nf = (int)nf;
  for (size_t f = 0; f < nf; ++f) {
    const int64_t k = kind[f];
    const bool flt = k == PROTO_F64 || k == PROTO_F32;
    int64_t slots;
    switch (k) {
      case PROTO_VARINT: case PROTO_ZIGZAG: case PROTO_FIXED64:
      case PROTO_FIXED32: case PROTO_SFIXED32: slots = n_int; break;
      case PROTO_F64: case PROTO_F32: slots = n_float; break;
      case PROTO_BYTES: slots = n_str; break;
      default: TORCH_CHECK(false, "unknown proto_decode kind ", k);
    }
    TORCH_CHECK((is_float[f] != 0) == flt, "is_float disagrees with kind");
    TORCH_CHECK(slot[f] >= 0 && slot[f] < slots, "field slot out of range");
    spec.fno[f] = (int)fno[f];
    spec.kind[f] = (int)k;
    spec.slot[f] = (int)slot[f];
  }
  auto rows = [&](int64_t r, torch::ScalarType t) {
    return torch::zeros({std::max<int64_t>(r, 1), std::max<int64_t>(n, 1)},
                        data.options().dtype(t));
  };
  auto out_i = rows(n_int, torch::kInt64);
  auto out_f = rows(n_float, torch::kFloat64);
  auto str_start = rows(n_str, torch::kInt64);
  auto str_len = rows(n_str, torch::kInt32);
  auto err = torch::zeros({1}, data.options().dtype(torch::kInt32));
  if (n > 0)
    launch_proto_decode(&spec, data.data_ptr<uint8_t>(),
                        offsets.data_ptr<int64_t>(), n,
                        out_i.data_ptr<int64_t>(), out_f.data_ptr<double>(),
                        str_start.data_ptr<int64_t>(),
                        str_len.data_ptr<int32_t>(), err.data_ptr<int32_t>(),
                        cur_stream());
  if (capture) {
    // hipGraph capture: no host syncs allowed — string fields (which need
    // a totals readback for allocation) are unsupported; the caller
    // validates err outside the capture
    TORCH_CHECK(n_str == 0, "capture-mode proto decode cannot have strings");
    return {out_i, out_f, err, StringColumns{}, torch::empty({0})};
  }
  // proto3 missing field → len 0 → empty value
  auto [strings, summary] = copy_out_strings(
      str_len, n_str, n, {err.to(torch::kInt64)},
      [&](int64_t s, const torch::Tensor& offs, torch::Tensor& out) {
        launch_proto_copy_bytes(data.data_ptr<uint8_t>(),
                                str_start[s].data_ptr<int64_t>(),
                                offs.data_ptr<int64_t>(), n,
                                out.data_ptr<uint8_t>(), cur_stream());
      });
  return {out_i, out_f, err, strings, summary};
}

// Columns → one binary column of proto3 messages (csrc/proto_encode.hip):
// size pass → offsets scan → ONE host readback [total_bytes, error] (the
// total sizes the output) → write pass → wave-per-row payload copy.
// Field f (ascending field number) reads row slot[f] of in_i64 / in_f64, or
// string column slot[f]; valid_idx[f] indexes `valids` (uint8[n]) or is -1.
// Returns (data, offsets, summary); on error (summary[1] != 0) data is empty.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> proto_encode(
    torch::Tensor in_i64, torch::Tensor in_f64,
    std::vector<std::tuple<torch::Tensor, torch::Tensor>> strings,
    std::vector<int64_t> fno, std::vector<int64_t> kind,
    std::vector<int64_t> slot, std::vector<torch::Tensor> valids,
    std::vector<int64_t> valid_idx, std::string prefix) {
  check_cuda(in_i64, "in_i64");
  check_cuda(in_f64, "in_f64");
  TORCH_CHECK(in_i64.scalar_type() == torch::kInt64 && in_i64.dim() == 2);
  TORCH_CHECK(in_f64.scalar_type() == torch::kFloat64 && in_f64.dim() == 2);
  const int64_t n = in_i64.size(1);
  TORCH_CHECK(in_f64.size(1) == n, "in_f64 must have one column per row");
  const size_t nf = fno.size();
  TORCH_CHECK(nf <= PROTO_ENC_MAX_FIELDS, "too many fields for proto_encode");
  TORCH_CHECK(kind.size() == nf && slot.size() == nf && valid_idx.size() == nf);
  TORCH_CHECK(prefix.size() <= 8, "prefix is at most 8 bytes");
  TORCH_CHECK(strings.size() <= PROTO_ENC_MAX_FIELDS);

  ProtoEncSpec spec{};
  spec.nf = (int)nf;
  spec.ns = (int)strings.size();
  spec.prefix_len = (int)prefix.size();
  std::copy(prefix.begin(), prefix.end(), spec.prefix);
  for (size_t s = 0; s < strings.size(); ++s) {
    const auto& data = std::get<0>(strings[s]);
    const auto& offs = std::get<1>(strings[s]);
    check_cuda(data, "string data");
    check_cuda(offs, "string offsets");
    TORCH_CHECK(data.scalar_type() == torch::kUInt8);
    TORCH_CHECK(offs.scalar_type() == torch::kInt64 && offs.numel() == n + 1,
                "string offsets must be int64[n + 1]");
    spec.sdata[s] = data.data_ptr<uint8_t>();
    spec.soffs[s] = offs.data_ptr<int64_t>();
    spec.sdata_len[s] = data.numel();
  }
  int64_t prev_fno = 0;
  for (size_t f = 0; f < nf; ++f) {
    TORCH_CHECK(fno[f] > prev_fno && fno[f] < (1ll << 29),
                "field numbers must ascend within [1, 2^29)");
    prev_fno = fno[f];
    const int64_t k = kind[f];
    int wire;
    int64_t slots;
    switch (k) {
      case PROTO_VARINT: case PROTO_ZIGZAG:
        wire = 0; slots = in_i64.size(0); break;
      case PROTO_FIXED64: wire = 1; slots = in_i64.size(0); break;
      case PROTO_FIXED32: case PROTO_SFIXED32:
        wire = 5; slots = in_i64.size(0); break;
      case PROTO_F64: wire = 1; slots = in_f64.size(0); break;
      case PROTO_F32: wire = 5; slots = in_f64.size(0); break;
      case PROTO_BYTES: wire = 2; slots = (int64_t)strings.size(); break;
      default: TORCH_CHECK(false, "unknown proto_encode kind ", k);
    }
    TORCH_CHECK(slot[f] >= 0 && slot[f] < slots, "field slot out of range");
    spec.tag[f] = (uint32_t)((fno[f] << 3) | wire);
    spec.kind[f] = (uint8_t)k;
    spec.slot[f] = (uint8_t)slot[f];
    if (valid_idx[f] >= 0) {
      TORCH_CHECK(valid_idx[f] < (int64_t)valids.size());
      const auto& v = valids[valid_idx[f]];
      check_cuda(v, "validity");
      TORCH_CHECK(v.scalar_type() == torch::kUInt8 && v.dim() == 1 &&
                      v.numel() == n,
                  "validity must be uint8[n]");
      spec.valid[f] = v.data_ptr<uint8_t>();
    }
  }

  auto bytes_opt = in_i64.options().dtype(torch::kUInt8);
  auto i64_opt = in_i64.options();
  auto st = cur_stream();
  if (n == 0)
    return {torch::empty({0}, bytes_opt), torch::zeros({1}, i64_opt),
            torch::zeros({2}, torch::kInt64)};
  auto lens = torch::empty({n}, i64_opt.dtype(torch::kInt32));
  auto err = torch::zeros({1}, i64_opt.dtype(torch::kInt32));
  launch_proto_encode_size(&spec, in_i64.data_ptr<int64_t>(),
                           in_f64.data_ptr<double>(), n,
                           lens.data_ptr<int32_t>(), err.data_ptr<int32_t>(),
                           st);
  auto offs = exclusive_offsets(lens);
  auto summary =
      torch::cat({offs.narrow(0, n, 1), err.to(torch::kInt64)}).cpu();
  const int64_t total = summary.data_ptr<int64_t>()[0];
  if (summary.data_ptr<int64_t>()[1] != 0)
    return {torch::empty({0}, bytes_opt), offs, summary};
  auto out = torch::empty({std::max<int64_t>(total, 1)}, bytes_opt);
  auto str_dst = torch::empty({std::max<int64_t>(spec.ns, 1), n}, i64_opt);
  if (total > 0) {
    launch_proto_encode_write(&spec, in_i64.data_ptr<int64_t>(),
                              in_f64.data_ptr<double>(), n,
                              offs.data_ptr<int64_t>(),
                              out.data_ptr<uint8_t>(),
                              str_dst.data_ptr<int64_t>(),
                              err.data_ptr<int32_t>(), st);
    launch_proto_encode_copy(&spec, n, str_dst.data_ptr<int64_t>(),
                             out.data_ptr<uint8_t>(), total, st);
  }
  return {out.slice(0, 0, total), offs, summary};
}

// ---------------------------------------------------------------------- window
// Segmented inclusive scan of double[n] under uint8 head flags
// (csrc/window.hip): tile aggregates → one-block carry scan → write.
torch::Tensor seg_scan(const torch::Tensor& vals, const torch::Tensor& head,
                       int op, bool reverse) {
  int64_t n = vals.numel();
  auto out = torch::empty_like(vals);
  if (n == 0) return out;
  int nt = seg_scan_tiles(n);
  auto tile_v = torch::empty({nt}, vals.options());
  auto carry = torch::empty({nt}, vals.options());
  auto tile_f = torch::empty({nt}, head.options());
  launch_segmented_scan(vals.data_ptr<double>(), head.data_ptr<uint8_t>(), n,
                        op, reverse, tile_v.data_ptr<double>(),
                        tile_f.data_ptr<uint8_t>(), carry.data_ptr<double>(),
                        out.data_ptr<double>(), cur_stream());
  return out;
}

void check_rows(const torch::Tensor& t, const char* name,
                torch::ScalarType ty, int64_t n) {
  check_cuda(t, name);
  TORCH_CHECK(t.scalar_type() == ty, name, " has the wrong dtype");
  TORCH_CHECK(t.dim() == 1 && t.numel() == n, name, " must have one entry ",
              "per row");
}

torch::Tensor segmented_scan(torch::Tensor vals, torch::Tensor head,
                             int64_t op, bool reverse) {
  int64_t n = vals.numel();
  TORCH_CHECK(n < (int64_t(1) << 31), "row indices are int32");
  TORCH_CHECK(op >= SCAN_SUM && op <= SCAN_MAX, "unknown scan op ", op);
  check_rows(vals, "values", torch::kFloat64, n);
  check_rows(head, "head", torch::kUInt8, n);
  return seg_scan(vals, head, (int)op, reverse);
}

// One window function over ROWS frames. Inputs are in sorted (partition,
// order key) row order; row i's frame is rows [i+lo, i+hi] of its partition
// (lo / hi absent: unbounded). Returns (result f64[n], valid u8[n]) scattered
// through perm when given. Nothing here reads device memory on the host.
std::tuple<torch::Tensor, torch::Tensor> window_frame(
    torch::Tensor vals, c10::optional<torch::Tensor> valid,
    torch::Tensor part, c10::optional<int64_t> lo, c10::optional<int64_t> hi,
    int64_t func, c10::optional<torch::Tensor> perm) {
  int64_t n = part.numel();
  TORCH_CHECK(n < (int64_t(1) << 31), "row indices are int32");
  TORCH_CHECK(func >= WF_SUM && func <= WF_COUNT_STAR,
              "unknown window function ", func);
  TORCH_CHECK(!lo || !hi || *lo <= *hi, "frame start is after frame end");
  check_rows(part, "partition ids", torch::kInt64, n);
  check_rows(vals, "values", torch::kFloat64, n);
  if (valid) check_rows(*valid, "validity", torch::kUInt8, n);
  if (perm) check_rows(*perm, "perm", torch::kInt64, n);
  auto f64 = vals.options();
  auto u8 = vals.options().dtype(torch::kUInt8);
  auto out = torch::empty({n}, f64);
  auto out_valid = torch::empty({n}, u8);
  if (n == 0) return {out, out_valid};
  auto st = cur_stream();
  // an offset of n rows already leaves every partition: clamping keeps
  // i + lo and hi - lo + 1 far from overflow without changing any frame
  if (lo) lo = std::max(-n, std::min(n, *lo));
  if (hi) hi = std::max(-n, std::min(n, *hi));

  // partition bounds per row
  auto head = torch::empty({n}, u8), tail = torch::empty({n}, u8);
  auto head_idx = torch::empty({n}, f64), tail_idx = torch::empty({n}, f64);
  launch_win_bounds(part.data_ptr<int64_t>(), n, head.data_ptr<uint8_t>(),
                    tail.data_ptr<uint8_t>(), head_idx.data_ptr<double>(),
                    tail_idx.data_ptr<double>(), st);
  auto start = seg_scan(head_idx, head, SCAN_MAX, false);
  auto end = seg_scan(tail_idx, tail, SCAN_MIN, true);

  const bool is_sum = func == WF_SUM || func == WF_AVG;
  const bool is_minmax = func == WF_MIN || func == WF_MAX;
  const bool sliding = is_minmax && lo && hi;
  const bool need_count = valid && (is_sum || is_minmax || func == WF_COUNT);
  const int64_t width = sliding ? *hi - *lo + 1 : 1;
  const double inf = std::numeric_limits<double>::infinity();
  const double fill = func == WF_MIN ? inf : func == WF_MAX ? -inf : 0.0;

  torch::Tensor masked, ones, chunk_head, chunk_tail, prefix, suffix, count;
  if (is_sum || is_minmax) masked = torch::empty({n}, f64);
  if (need_count) ones = torch::empty({n}, f64);
  if (sliding) {
    chunk_head = torch::empty({n}, u8);
    chunk_tail = torch::empty({n}, u8);
  }
  auto ptr_f64 = [](const torch::Tensor& t) {
    return t.defined() ? t.data_ptr<double>() : nullptr;
  };
  auto ptr_u8 = [](const torch::Tensor& t) {
    return t.defined() ? t.data_ptr<uint8_t>() : nullptr;
  };
  const uint8_t* valid_p = valid ? valid->data_ptr<uint8_t>() : nullptr;
  if (masked.defined() || ones.defined())
    launch_win_inputs(vals.data_ptr<double>(), valid_p,
                      start.data_ptr<double>(), end.data_ptr<double>(), n,
                      fill, width, ptr_f64(masked), ptr_f64(ones),
                      ptr_u8(chunk_head), ptr_u8(chunk_tail), st);
  if (need_count) count = seg_scan(ones, head, SCAN_SUM, false);
  if (is_sum) prefix = seg_scan(masked, head, SCAN_SUM, false);
  if (is_minmax) {
    const int op = func == WF_MIN ? SCAN_MIN : SCAN_MAX;
    if (sliding || !lo)
      prefix = seg_scan(masked, sliding ? chunk_head : head, op, false);
    if (sliding || lo)
      suffix = seg_scan(masked, sliding ? chunk_tail : tail, op, true);
  }

  FrameArgs a{};
  a.start = start.data_ptr<double>();
  a.end = end.data_ptr<double>();
  a.vals = vals.data_ptr<double>();
  a.valid = valid_p;
  a.prefix = ptr_f64(prefix);
  a.suffix = ptr_f64(suffix);
  a.count = ptr_f64(count);
  a.perm = perm ? perm->data_ptr<int64_t>() : nullptr;
  a.lo = lo.value_or(0);
  a.hi = hi.value_or(0);
  a.lo_unbounded = !lo;
  a.hi_unbounded = !hi;
  a.func = (int)func;
  a.n = n;
  a.out = out.data_ptr<double>();
  a.out_valid = out_valid.data_ptr<uint8_t>();
  launch_win_frame(&a, st);
  return {out, out_valid};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "arkflow_amd gfx950 native kernels";
  m.def("exclusive_offsets", &exclusive_offsets);
  m.def("take_binary", &take_binary);
  m.def("bytes_match", &bytes_match);
  m.def("attention_qkv_bf16", &attention_qkv_bf16, py::arg("qkv"),
        py::arg("scale"), py::arg("pad") = 8, py::arg("lens") = py::none());
  m.def("mask_to_indices", &mask_to_indices);
  m.def("filter_cmp_scalar", &filter_cmp_scalar);
  m.def("gather", &gather);
  m.def("hash_group_i64", &hash_group_i64);
  m.def("segment_reduce_f32", &segment_reduce_f32);
  m.def("join_inner_i64", &join_inner_i64);
  m.def("gemm_bf16", &gemm_bf16, py::arg("A"), py::arg("Bt"),
        py::arg("bias") = py::none(), py::arg("act") = 0);
  m.def("layernorm_bf16", &layernorm_bf16, py::arg("x"), py::arg("gamma"),
        py::arg("beta"), py::arg("eps") = 1e-5,
        py::arg("residual") = py::none());
  m.def("softmax_bf16", &softmax_bf16, py::arg("x"), py::arg("scale") = 1.0);
  m.def("mapped_int32", &mapped_int32, py::arg("n"));
  m.def("bias_act_bf16", &bias_act_bf16, py::arg("x"),
        py::arg("bias") = py::none(), py::arg("act") = 0);
  m.def("attention_bf16", &attention_bf16, py::arg("q"), py::arg("k"),
        py::arg("v"), py::arg("scale"), py::arg("lens") = py::none());
  m.def("proto_decode", &proto_decode, py::arg("data"),
        py::arg("offsets"), py::arg("fno"), py::arg("kind"),
        py::arg("is_float"), py::arg("slot"), py::arg("n_int"),
        py::arg("n_float"), py::arg("n_str"), py::arg("capture") = false);
  m.def("proto_encode", &proto_encode, py::arg("in_i64"), py::arg("in_f64"),
        py::arg("strings"), py::arg("fno"), py::arg("kind"), py::arg("slot"),
        py::arg("valids"), py::arg("valid_idx"), py::arg("prefix") = "");
  m.attr("PROTO_ENC_MAX_FIELDS") = PROTO_ENC_MAX_FIELDS;
  m.def("gather_columns", &gather_columns);
  m.def("gemm_bf16_variant", &gemm_bf16_variant);
  m.def("bytes_hash", &bytes_hash);
  m.def("bytes_rank", &bytes_rank);
  m.def("bytes_compare_cols", &bytes_compare_cols);
  // Python bytes convert to std::string raw, as for bytes_match
  m.def("bytes_compare_lit", &bytes_compare_lit);
  m.def("json_decode", &json_decode);
  m.def("fused_filter_gather", &fused_filter_gather);
  m.def("genfiltpack", &genfiltpack, py::arg("lo"), py::arg("width"),
        py::arg("key_lo"), py::arg("key_range"), py::arg("n"),
        py::arg("fidx"), py::arg("op"), py::arg("scalar"), py::arg("outs"),
        py::arg("key_out"), py::arg("feats"), py::arg("count_out"),
        py::arg("counts_ws"), py::arg("bar"), py::arg("ctr"));
  m.def("fused_filter_agg", &fused_filter_agg);
  m.def("hash_agg_capture", &hash_agg_capture, py::arg("keys"),
        py::arg("nrow"), py::arg("vals"), py::arg("ops"),
        py::arg("table_size"), py::arg("g_cap"),
        py::arg("gcount_out") = c10::nullopt);
  m.def("filter_gather_capture", &filter_gather_capture);
  m.def("gemv_bf16_f32", &gemv_bf16_f32);
  m.def("gen_fields", &gen_fields);
  m.def("featpack", &featpack);
  m.def("radix_argsort", &radix_argsort, py::arg("keys"), py::arg("descending") = false);
  m.def("segmented_scan", &segmented_scan, py::arg("values"), py::arg("head"),
        py::arg("op"), py::arg("reverse") = false);
  m.def("seg_scan_tile_rows", &seg_scan_tile_rows);
  m.def("window_frame", &window_frame, py::arg("values"), py::arg("valid"),
        py::arg("part"), py::arg("lo"), py::arg("hi"), py::arg("func"),
        py::arg("perm") = py::none());
}
