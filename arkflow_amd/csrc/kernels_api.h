// Host-side interface of the inference, decode and fused-step kernels.
// Included by the .hip file that defines each launcher and by bindings.cpp,
// so a declaration that drifts from its definition is a compile error. (The
// relational kernels are in relational_api.h, the GEMMs in gemm_api.h.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {

// ---- rowops.hip -------------------------------------------------------------
void launch_layernorm_bf16(const void* x, const void* residual,
                           const float* gamma, const float* beta, void* out,
                           void* resid_out, int64_t rows, int n, float eps,
                           hipStream_t st);
void launch_softmax_bf16(const void* x, void* out, int64_t rows, int n,
                         float scale, hipStream_t st);
void launch_bias_act_bf16(const void* x, const float* bias, void* out,
                          int64_t rows, int n, int act, hipStream_t st);

// ---- attention.hip ----------------------------------------------------------
// Fused attention over B·Hd (batch, head) pairs. Row s of head h in batch b
// is at base + ((int64_t)b*S + s)*ld + h*D, ld = ldq for q/k/v, ldo for o:
//   packed [B,H,S,D]:  B = B·H, Hd = 1, ldq = ldo = D (one head per "batch"
//                      row, so one length per (b, h));
//   [B,S,3,H,D] → [B,S,H·D]:  Hd = H, q/k/v = base + {0,1,2}·H·D,
//                      ldq = 3·H·D, ldo = H·D (no transpose copies).
struct AttnArgs {
  const void *q, *k, *v;  // bf16
  void* o;                // bf16
  int B;                  // batch rows = entries of lens
  int Hd;                 // heads per batch row
  int S, D;
  int ldq, ldo;
  float scale;
  int pad;  // LDS row padding of the S=128 kernel in bf16 elements: 4, 8
            // (production), 16 or 20; anything else runs as 8
  // nullptr (every key of every sequence is valid: the unmasked kernels), or
  // a device array of B valid lengths that the kernels clamp to [0, S] and
  // the host never reads (capturable)
  const int32_t* lens;
  hipStream_t stream;
};
// S=128, D=64: the full-S kernel; else D=64, S%64==0: the flash-tiled
// kernel; else nothing is launched and -1 is returned. 0 otherwise.
int launch_attention_bf16(const AttnArgs* args);

// ---- proto_decode.hip -------------------------------------------------------
void launch_proto_copy_bytes(const uint8_t* data, const int64_t* start,
                             const int64_t* out_offs, int64_t n_msgs,
                             uint8_t* out, hipStream_t st);
void launch_proto_decode(const uint8_t* data, const int64_t* offsets,
                         int64_t n_msgs, int nf, const int* fno,
                         const int* kind, const int* is_float,
                         const int* slot, int64_t* out_i64, double* out_f64,
                         int64_t* str_start, int32_t* str_len,
                         int32_t* err_flags, hipStream_t st);

// ---- json_decode.hip --------------------------------------------------------
void launch_json_decode(const uint8_t* data, const int64_t* offsets,
                        int64_t n_docs, int nf, const char* names,
                        const int* name_len, const int* kind, const int* slot,
                        const int* parent, int np, const char* parents,
                        const int* parent_len, double* out_f64,
                        int64_t* out_i64, int64_t* str_start,
                        int32_t* str_ulen, uint8_t* found, int32_t* err,
                        int32_t* found_count, int use_wave, hipStream_t st);
void launch_json_copy_strings(const uint8_t* data, const int64_t* start,
                              const int64_t* out_offs, const uint8_t* found,
                              int64_t n_docs, int64_t data_len, uint8_t* out,
                              hipStream_t st);
void launch_json_copy_strings_wave(const uint8_t* data, const int64_t* start,
                                   const int64_t* out_offs,
                                   const uint8_t* found, int64_t n_docs,
                                   int64_t data_len, uint8_t* out,
                                   hipStream_t st);

// ---- stepfused.hip ----------------------------------------------------------
void launch_gen_fields(float* block, int64_t* key, int64_t n, const float* lo,
                       const float* width, int nf, int64_t key_lo,
                       int64_t key_range, unsigned long long* ctr,
                       hipStream_t st);
// single-block exclusive scan of <= 1024 block counts; *total = their sum
void launch_scan_counts(const int32_t* counts, int nb, int32_t* offs,
                        int32_t* total, hipStream_t st);
int launch_genfiltpack(const float* lo, const float* width, int nf,
                       int64_t key_lo, int64_t key_range, int64_t n, int fidx,
                       int op, float scalar, float* const* outs,
                       int64_t* key_out, void* feats, int dpad,
                       int32_t* count_out, int32_t* counts_ws,
                       unsigned long long* bar, unsigned long long* ctr,
                       hipStream_t st);
void launch_featpack(const float** src, int nf, int kpad, int64_t n, void* out,
                     hipStream_t st);
void launch_featpack64(const double** src, int nf, int kpad, int64_t n,
                       void* out, hipStream_t st);
void launch_gemv_bf16_f32(const void* x, const void* w, float bias, int64_t M,
                          int K, float* out, hipStream_t st);

}  // extern "C"
