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

// ---- proto_decode.hip, proto_encode.hip ------------------------------------
// Wire form of a scalar proto3 field, for the decoder and the encoder alike.
// Integer kinds live in int64 columns, F64/F32 in float64 columns.
enum ProtoKind {
  PROTO_VARINT = 0,    // int32/int64/uint32/uint64/bool
  PROTO_ZIGZAG = 1,    // sint32/sint64
  PROTO_F64 = 2,       // double
  PROTO_F32 = 3,       // float: encode rounds the float64 input to float32
  PROTO_FIXED64 = 4,   // fixed64/sfixed64: the int64's 8 bytes
  PROTO_FIXED32 = 6,   // fixed32: zero-extended; errors outside [0, 2^32)
  PROTO_SFIXED32 = 7,  // sfixed32: sign-extended; errors outside [-2^31, 2^31)
  PROTO_BYTES = 9,     // string/bytes
};

// ---- proto_decode.hip -------------------------------------------------------
#define PROTO_MAX_FIELDS 16
// Filled by the binding, passed to the kernel by value.
struct ProtoSpec {
  int nf;                      // <= PROTO_MAX_FIELDS
  int fno[PROTO_MAX_FIELDS];   // field number
  int kind[PROTO_MAX_FIELDS];  // ProtoKind
  // row of out_f64 (F64, F32) / out_i64 (integer kinds), or the string slot
  int slot[PROTO_MAX_FIELDS];
};
void launch_proto_copy_bytes(const uint8_t* data, const int64_t* start,
                             const int64_t* out_offs, int64_t n_msgs,
                             uint8_t* out, hipStream_t st);
// err_flags[0] is set to 1 for a varint longer than 10 bytes, a fixed or
// length-delimited field running past its message, or wire type 3/4/6/7.
void launch_proto_decode(const ProtoSpec* spec, const uint8_t* data,
                         const int64_t* offsets, int64_t n_msgs,
                         int64_t* out_i64, double* out_f64,
                         int64_t* str_start, int32_t* str_len,
                         int32_t* err_flags, hipStream_t st);

// ---- proto_encode.hip -------------------------------------------------------
#define PROTO_ENC_MAX_FIELDS 32
// Fields in ascending field number; a schema field with no input column is
// simply not listed. Passed to the kernels by value.
struct ProtoEncSpec {
  int nf;                                  // fields listed
  int ns;                                  // string/bytes slots in use
  int prefix_len;                          // <= 8
  uint8_t prefix[8];                       // written at the start of each row
  uint32_t tag[PROTO_ENC_MAX_FIELDS];      // (field number << 3) | wire type
  uint8_t kind[PROTO_ENC_MAX_FIELDS];      // ProtoKind
  // row of in_i64 (integer kinds) / in_f64 (F64, F32), or the string slot
  uint8_t slot[PROTO_ENC_MAX_FIELDS];
  const uint8_t* valid[PROTO_ENC_MAX_FIELDS];  // uint8[n], or null: no NULLs
  // per string slot: the source column. Its offsets need not start at 0.
  const uint8_t* sdata[PROTO_ENC_MAX_FIELDS];
  const int64_t* soffs[PROTO_ENC_MAX_FIELDS];  // int64[n + 1]
  int64_t sdata_len[PROTO_ENC_MAX_FIELDS];     // bytes behind sdata
};
// Size pass: lens[i] = encoded bytes of row i. err[0] is set to 1 for a
// fixed32/sfixed32 value out of range, a finite value that overflows float32,
// a source span outside its column, or a row longer than INT32_MAX.
void launch_proto_encode_size(const ProtoEncSpec* spec, const int64_t* in_i64,
                              const double* in_f64, int64_t n, int32_t* lens,
                              int32_t* err, hipStream_t st);
// Write pass: everything but the string/bytes payloads into out[out_offs[i]..
// out_offs[i+1]); str_dst[s][i] = where the payload of slot s goes, or -1.
void launch_proto_encode_write(const ProtoEncSpec* spec, const int64_t* in_i64,
                               const double* in_f64, int64_t n,
                               const int64_t* out_offs, uint8_t* out,
                               int64_t* str_dst, int32_t* err, hipStream_t st);
// Payload copy, one wave per row.
void launch_proto_encode_copy(const ProtoEncSpec* spec, int64_t n,
                              const int64_t* str_dst, uint8_t* out,
                              int64_t out_len, hipStream_t st);

// ---- json_decode.hip --------------------------------------------------------
#define JSON_MAX_FIELDS 16
#define JSON_MAX_PARENTS 8
#define JSON_MAX_NAME 24  // names are shorter than this
// Filled by the binding, passed to the kernels by value. A dotted schema name
// ("user.id") is the leaf "id" scoped to the parent object "user".
struct JsonSpec {
  int nf;  // <= JSON_MAX_FIELDS
  char names[JSON_MAX_FIELDS][JSON_MAX_NAME];  // leaf names
  int name_len[JSON_MAX_FIELDS];
  int kind[JSON_MAX_FIELDS];  // 0 → out_i64 (ints+bools), 1 → out_f64, 2 → str
  int slot[JSON_MAX_FIELDS];
  int parent[JSON_MAX_FIELDS];  // -1 = top level, else index into parents
  int np;                       // <= JSON_MAX_PARENTS
  char parents[JSON_MAX_PARENTS][JSON_MAX_NAME];
  int parent_len[JSON_MAX_PARENTS];
};
// use_wave: one wave per document instead of one thread
void launch_json_decode(const JsonSpec* spec, const uint8_t* data,
                        const int64_t* offsets, int64_t n_docs,
                        double* out_f64, int64_t* out_i64, int64_t* str_start,
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
