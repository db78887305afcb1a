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

// ---- attention.hip: each returns 0, or -1 for an unsupported (S, D) ---------
// lens: nullptr (every key of every sequence is valid: the unmasked kernels),
// or a device array of valid lengths that the kernels clamp to [0, S] and
// the host never reads. It has one entry per kernel "batch" row: B for the
// [B,S,3,H,D] layout (index bh / Hd), BH for packed [B,H,S,D] (Hd = 1).
int launch_attention_bf16(const void* Q, const void* K, const void* V,
                          void* O, int BH, int S, int D, float scale,
                          const int32_t* lens, hipStream_t st);
int launch_attention_flash(const void* Q, const void* K, const void* V,
                           void* O, int BH, int S, int D, float scale,
                           int ldq, int ldo, int Hd, const int32_t* lens,
                           hipStream_t st);
int launch_attention_qkv_bf16(const void* QKV, void* O, int B, int H, int S,
                              int D, float scale, hipStream_t st);
int launch_attention_qkv_bf16_pad(const void* QKV, void* O, int B, int H,
                                  int S, int D, float scale, int pad,
                                  const int32_t* lens, hipStream_t st);

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
