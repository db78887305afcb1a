// GPU JSON decode: one thread per document, extracting SCALAR fields of a
// KNOWN schema straight from the device-resident binary column into columnar
// outputs — the "GPU column builder kernel" of SURVEY §2.9 (the general
// schema-inference path stays host-side via pyarrow, per the §7 plan; this
// kernel covers the configured-schema hot path: flat JSON, numeric/bool
// fields, other keys skipped including nested objects/arrays/strings).
#include "common.h"
#include "kernels_api.h"

#define JSON_MAX_FIELDS 16
#define JSON_MAX_NAME 24

#define JSON_MAX_PARENTS 8

struct JsonSpec {
  int nf;
  char names[JSON_MAX_FIELDS][JSON_MAX_NAME];
  int name_len[JSON_MAX_FIELDS];
  int kind[JSON_MAX_FIELDS];  // 0 → out_i64 (ints+bools), 1 → out_f64, 2 → str
  int slot[JSON_MAX_FIELDS];
  int parent[JSON_MAX_FIELDS];  // -1 = top level, else index into parents
  int np;
  char parents[JSON_MAX_PARENTS][JSON_MAX_NAME];
  int parent_len[JSON_MAX_PARENTS];
};

DEV_INLINE bool is_ws(uint8_t c) {
  return c == ' ' || c == '\t' || c == '\n' || c == '\r';
}

// SWAR: does any byte of x equal '"' (0x22) or '\\' (0x5C)? Long strings
// are walked 8 bytes per iteration instead of 1 — the thread-per-doc parse
// was byte-loop bound at ~72 GB/s on string-heavy docs (profiles r13).
DEV_INLINE uint64_t haszero64(uint64_t v) {
  return (v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull;
}

DEV_INLINE bool has_quote_or_bslash(uint64_t x) {
  return (haszero64(x ^ 0x2222222222222222ull) |
          haszero64(x ^ 0x5C5C5C5C5C5C5C5Cull)) != 0;
}

DEV_INLINE uint64_t load8(const uint8_t* p) {
  uint64_t x;
  __builtin_memcpy(&x, p, 8);
  return x;
}

// skip a JSON value generically (string/number/object/array/literal)
DEV_INLINE int64_t skip_value(const uint8_t* d, int64_t p, int64_t end) {
  while (p < end && is_ws(d[p])) ++p;
  if (p >= end) return p;
  uint8_t c = d[p];
  if (c == '"') {
    ++p;
    while (p < end) {
      if (d[p] == '\\') p += 2;
      else if (d[p] == '"') return p + 1;
      else if (p + 8 <= end && !has_quote_or_bslash(load8(d + p))) p += 8;
      else ++p;
    }
    return p;
  }
  if (c == '{' || c == '[') {
    uint8_t open = c, close = (c == '{') ? '}' : ']';
    int depth = 0;
    while (p < end) {
      uint8_t x = d[p];
      if (x == '"') {
        ++p;
        while (p < end) {
          if (d[p] == '\\') p += 2;
          else if (d[p] == '"') { ++p; break; }
          else if (p + 8 <= end && !has_quote_or_bslash(load8(d + p)))
            p += 8;
          else ++p;
        }
        continue;
      }
      if (x == open) ++depth;
      else if (x == close) {
        --depth;
        if (depth == 0) return p + 1;
      }
      ++p;
    }
    return p;
  }
  // number / true / false / null
  while (p < end && d[p] != ',' && d[p] != '}' && d[p] != ']' &&
         !is_ws(d[p]))
    ++p;
  return p;
}

// parse a JSON number at p (after ws); returns value as double + intness
DEV_INLINE int64_t parse_number(const uint8_t* d, int64_t p, int64_t end,
                                double* out, bool* is_int) {
  bool neg = false;
  *is_int = true;
  if (p < end && (d[p] == '-' || d[p] == '+')) {
    neg = d[p] == '-';
    ++p;
  }
  double v = 0.0;
  while (p < end && d[p] >= '0' && d[p] <= '9') {
    v = v * 10.0 + (d[p] - '0');
    ++p;
  }
  if (p < end && d[p] == '.') {
    *is_int = false;
    ++p;
    double scale = 0.1;
    while (p < end && d[p] >= '0' && d[p] <= '9') {
      v += (d[p] - '0') * scale;
      scale *= 0.1;
      ++p;
    }
  }
  if (p < end && (d[p] == 'e' || d[p] == 'E')) {
    *is_int = false;
    ++p;
    bool eneg = false;
    if (p < end && (d[p] == '-' || d[p] == '+')) {
      eneg = d[p] == '-';
      ++p;
    }
    int ex = 0;
    while (p < end && d[p] >= '0' && d[p] <= '9') {
      ex = ex * 10 + (d[p] - '0');
      ++p;
    }
    double m = 1.0;
    for (int i = 0; i < ex; ++i) m *= 10.0;
    v = eneg ? v / m : v * m;
  }
  *out = neg ? -v : v;
  return p;
}

DEV_INLINE uint32_t hex4(const uint8_t* d, int64_t p) {
  uint32_t v = 0;
  for (int i = 0; i < 4; ++i) {
    uint8_t c = d[p + i];
    uint32_t x = (c >= '0' && c <= '9')   ? c - '0'
                 : (c >= 'a' && c <= 'f') ? c - 'a' + 10
                 : (c >= 'A' && c <= 'F') ? c - 'A' + 10
                                          : 0;
    v = (v << 4) | x;
  }
  return v;
}

// Walk a JSON string body (p = first char after the opening quote), computing
// the UNESCAPED byte length (simple escapes → 1 byte, \uXXXX → UTF-8 length,
// surrogate pairs → 4). Returns the position of the closing quote. The copy
// kernel below must mirror this walk byte-for-byte.
DEV_INLINE int64_t scan_string(const uint8_t* __restrict__ d, int64_t p,
                               int64_t end, int32_t* ulen) {
  int32_t u = 0;
  while (p < end && d[p] != '"') {
    if (d[p] != '\\' && p + 8 <= end &&
        !has_quote_or_bslash(load8(d + p))) {
      p += 8;
      u += 8;
      continue;
    }
    if (d[p] == '\\' && p + 1 < end) {
      uint8_t e = d[p + 1];
      if (e == 'u' && p + 5 < end) {
        uint32_t cp = hex4(d, p + 2);
        p += 6;
        if (cp >= 0xD800 && cp <= 0xDBFF && p + 5 < end && d[p] == '\\' &&
            d[p + 1] == 'u') {
          uint32_t lo = hex4(d, p + 2);
          if (lo >= 0xDC00 && lo <= 0xDFFF) {
            p += 6;
            u += 4;
            continue;
          }
        }
        u += cp < 0x80 ? 1 : (cp < 0x800 ? 2 : 3);
        continue;
      }
      p += 2;
      u += 1;
      continue;
    }
    ++p;
    ++u;
  }
  *ulen = u;
  return p;
}

DEV_INLINE int64_t unescape_copy(const uint8_t* __restrict__ d, int64_t p,
                                 int64_t end, uint8_t* __restrict__ out,
                                 int64_t w, int64_t wend) {
  while (w < wend && p < end && d[p] != '"') {
    if (d[p] != '\\' && p + 8 <= end && w + 8 <= wend &&
        !has_quote_or_bslash(load8(d + p))) {
      uint64_t x = load8(d + p);
      __builtin_memcpy(out + w, &x, 8);
      p += 8;
      w += 8;
      continue;
    }
    if (d[p] == '\\' && p + 1 < end) {
      uint8_t e = d[p + 1];
      if (e == 'u' && p + 5 < end) {
        uint32_t cp = hex4(d, p + 2);
        p += 6;
        if (cp >= 0xD800 && cp <= 0xDBFF && p + 5 < end && d[p] == '\\' &&
            d[p + 1] == 'u') {
          uint32_t lo = hex4(d, p + 2);
          if (lo >= 0xDC00 && lo <= 0xDFFF) {
            p += 6;
            cp = 0x10000 + (((cp - 0xD800) << 10) | (lo - 0xDC00));
            out[w++] = 0xF0 | (cp >> 18);
            out[w++] = 0x80 | ((cp >> 12) & 0x3F);
            out[w++] = 0x80 | ((cp >> 6) & 0x3F);
            out[w++] = 0x80 | (cp & 0x3F);
            continue;
          }
        }
        if (cp < 0x80) {
          out[w++] = (uint8_t)cp;
        } else if (cp < 0x800) {
          out[w++] = 0xC0 | (cp >> 6);
          out[w++] = 0x80 | (cp & 0x3F);
        } else {
          out[w++] = 0xE0 | (cp >> 12);
          out[w++] = 0x80 | ((cp >> 6) & 0x3F);
          out[w++] = 0x80 | (cp & 0x3F);
        }
        continue;
      }
      uint8_t v = e == 'n'   ? '\n'
                  : e == 't' ? '\t'
                  : e == 'r' ? '\r'
                  : e == 'b' ? '\b'
                  : e == 'f' ? '\f'
                             : e;  // \" \\ \/ and unknown escapes → literal
      out[w++] = v;
      p += 2;
      continue;
    }
    out[w++] = d[p++];
  }
  return w;
}

DEV_INLINE void json_parse_doc(const uint8_t* __restrict__ data,
                               int64_t p, int64_t end, int64_t boff,
                               int64_t i, int64_t n_docs,
                               const JsonSpec& spec,
                               double* __restrict__ out_f64,
                               int64_t* __restrict__ out_i64,
                               int64_t* __restrict__ str_start,
                               int32_t* __restrict__ str_ulen,
                               uint8_t* __restrict__ found,
                               int32_t* __restrict__ err,
                               int* __restrict__ fcnt);

// ======================= wave-cooperative parse ==============================
// For long documents the thread-per-doc walk is serialization-bound: even
// with SWAR it advances 8 B per dependent step. Here ONE WAVE owns a doc
// and scans 512 B per step: every lane SWAR-checks its own 8 B chunk for
// '"'/'\\', a ballot finds the first hit, and the (wave-uniform) state
// machine jumps there. Only lane 0 writes outputs. Dispatched when the
// batch's mean document length clears a threshold (launcher below);
// outputs are bit-identical to the thread-per-doc kernel.

// first position ≥ p whose byte is '"' or '\\' (or end)
DEV_INLINE int64_t wave_find_qb(const uint8_t* __restrict__ d, int64_t p,
                                int64_t end, int lane) {
  while (p < end) {
    int64_t base = p + (int64_t)lane * 8;
    uint64_t hits = 0;
    if (base < end) {
      if (base + 8 <= end) {
        uint64_t x = load8(d + base);
        hits = haszero64(x ^ 0x2222222222222222ull) |
               haszero64(x ^ 0x5C5C5C5C5C5C5C5Cull);
      } else {
        for (int i = 0; base + i < end; ++i) {
          uint8_t c = d[base + i];
          if (c == '"' || c == '\\') hits |= 0x80ull << (8 * i);
        }
      }
    }
    uint64_t lane_has = __ballot(hits != 0);
    if (lane_has) {
      int src = __ffsll((unsigned long long)lane_has) - 1;
      uint64_t h = __shfl((unsigned long long)hits, src, 64);
      int off = __builtin_ctzll(h) >> 3;
      return p + (int64_t)src * 8 + off;
    }
    p += 64 * 8;
  }
  return end;
}

// wave version of scan_string: returns closing-quote position, accumulates
// the unescaped length exactly like scan_string (escape handling runs
// wave-uniform — every lane computes the same values)
DEV_INLINE int64_t wave_scan_string(const uint8_t* __restrict__ d, int64_t p,
                                    int64_t end, int lane, int32_t* ulen) {
  int32_t u = 0;
  while (p < end) {
    int64_t q = wave_find_qb(d, p, end, lane);
    u += (int32_t)(q - p);
    p = q;
    if (p >= end || d[p] == '"') break;
    // backslash escape — mirror scan_string byte for byte
    if (p + 1 < end) {
      uint8_t e = d[p + 1];
      if (e == 'u' && p + 5 < end) {
        uint32_t cp = hex4(d, p + 2);
        p += 6;
        if (cp >= 0xD800 && cp <= 0xDBFF && p + 5 < end && d[p] == '\\' &&
            d[p + 1] == 'u') {
          uint32_t lo = hex4(d, p + 2);
          if (lo >= 0xDC00 && lo <= 0xDFFF) {
            p += 6;
            u += 4;
            continue;
          }
        }
        u += cp < 0x80 ? 1 : (cp < 0x800 ? 2 : 3);
        continue;
      }
      p += 2;
      u += 1;
      continue;
    }
    ++p;
    ++u;
  }
  *ulen = u;
  return p;
}

// wave version of skip_value (string bodies scanned 512 B/step)
DEV_INLINE int64_t wave_skip_value(const uint8_t* __restrict__ d, int64_t p,
                                   int64_t end, int lane) {
  while (p < end && is_ws(d[p])) ++p;
  if (p >= end) return p;
  uint8_t c = d[p];
  if (c == '"') {
    int32_t dummy;
    p = wave_scan_string(d, p + 1, end, lane, &dummy);
    return p < end ? p + 1 : p;
  }
  if (c == '{' || c == '[') {
    uint8_t open = c, close = (c == '{') ? '}' : ']';
    int depth = 0;
    while (p < end) {
      uint8_t x = d[p];
      if (x == '"') {
        int32_t dummy;
        p = wave_scan_string(d, p + 1, end, lane, &dummy);
        if (p < end) ++p;
        continue;
      }
      if (x == open) ++depth;
      else if (x == close) {
        --depth;
        if (depth == 0) return p + 1;
      }
      ++p;
    }
    return p;
  }
  while (p < end && d[p] != ',' && d[p] != '}' && d[p] != ']' &&
         !is_ws(d[p]))
    ++p;
  return p;
}

// LDS doc cache: each 128-doc tile's byte range is CONTIGUOUS in the binary
// column, so the block stages it with coalesced loads and threads then walk
// their documents out of LDS — the thread-per-doc global byte walk was
// latency-bound (each dependent 8 B load pays HBM latency with only a few
// waves per CU to hide it). Tiles larger than the cache parse from global.
#define JSON_BLOCK 128
#define JSON_LDS_BYTES (48 * 1024)

__global__ __launch_bounds__(JSON_BLOCK)
void json_decode_kernel(const uint8_t* __restrict__ data,
                        const int64_t* __restrict__ offsets,
                        int64_t n_docs, JsonSpec spec,
                        double* __restrict__ out_f64,  // [nd][n]
                        int64_t* __restrict__ out_i64,
                        int64_t* __restrict__ str_start,  // [ns][n]
                        int32_t* __restrict__ str_ulen,   // [ns][n]
                        uint8_t* __restrict__ found,  // [nf][n]
                        int32_t* __restrict__ err,
                        int32_t* __restrict__ found_count) {  // [nf]
  __shared__ uint8_t cache[JSON_LDS_BYTES];
  __shared__ int fcnt[JSON_MAX_FIELDS];
  for (int64_t tile = (int64_t)blockIdx.x * JSON_BLOCK; tile < n_docs;
       tile += (int64_t)gridDim.x * JSON_BLOCK) {
    int64_t tile_hi = tile + JSON_BLOCK < n_docs ? tile + JSON_BLOCK
                                                 : n_docs;
    const int64_t r0 = offsets[tile];
    const int64_t r1 = offsets[tile_hi];
    if (threadIdx.x < JSON_MAX_FIELDS) fcnt[threadIdx.x] = 0;
    const uint8_t* dv = data;
    int64_t boff = 0;
    if (r1 - r0 <= JSON_LDS_BYTES) {
      const int64_t len = r1 - r0;
      int64_t b = (int64_t)threadIdx.x * 8;
      for (; b + 8 <= len; b += (int64_t)JSON_BLOCK * 8)
        __builtin_memcpy(cache + b, data + r0 + b, 8);
      if (b < len)
        for (; b < len; ++b) cache[b] = data[r0 + b];
      dv = cache;
      boff = r0;
    }
    __syncthreads();  // cache staged + fcnt zeroed
    int64_t i = tile + threadIdx.x;
    if (i < tile_hi)
      json_parse_doc(dv, offsets[i] - boff, offsets[i + 1] - boff, boff, i,
                     n_docs, spec, out_f64, out_i64, str_start, str_ulen,
                     found, err, fcnt);
    __syncthreads();  // cache reused by the next tile
    if (threadIdx.x < JSON_MAX_FIELDS && fcnt[threadIdx.x])
      atomicAdd(&found_count[threadIdx.x], fcnt[threadIdx.x]);
  }
}

DEV_INLINE void json_parse_doc(const uint8_t* __restrict__ data,
                               int64_t p, int64_t end, int64_t boff,
                               int64_t i, int64_t n_docs,
                               const JsonSpec& spec,
                               double* __restrict__ out_f64,
                               int64_t* __restrict__ out_i64,
                               int64_t* __restrict__ str_start,
                               int32_t* __restrict__ str_ulen,
                               uint8_t* __restrict__ found,
                               int32_t* __restrict__ err,
                               int* __restrict__ fcnt) {
  {
    while (p < end && is_ws(data[p])) ++p;
    if (p >= end || data[p] != '{') {
      if (p < end) err[0] = 1;
      return;
    }
    ++p;
    int ctx = -1;  // current parent-object context (-1 = top level)
    for (;;) {
      while (p < end && (is_ws(data[p]) || data[p] == ',')) ++p;
      if (p >= end) break;
      if (data[p] == '}') {
        if (ctx < 0) break;  // end of document
        ctx = -1;            // pop out of the nested object
        ++p;
        continue;
      }
      if (data[p] != '"') { err[0] = 1; break; }
      // key
      int64_t k0 = ++p;
      while (p < end && data[p] != '"') {
        if (data[p] == '\\') ++p;
        ++p;
      }
      int klen = (int)(p - k0);
      ++p;  // closing quote
      while (p < end && is_ws(data[p])) ++p;
      if (p < end && data[p] == ':') ++p;
      while (p < end && is_ws(data[p])) ++p;
      // match against spec (fields are scoped to the current context)
      int fi = -1;
#pragma unroll
      for (int f = 0; f < JSON_MAX_FIELDS; ++f) {
        if (f < spec.nf && spec.name_len[f] == klen
            && spec.parent[f] == ctx) {
          bool eq = true;
          for (int c = 0; c < klen; ++c)
            if (spec.names[f][c] != (char)data[k0 + c]) { eq = false; break; }
          if (eq) { fi = f; break; }
        }
      }
      if (fi < 0) {
        // at top level, a key naming a parent object descends one level
        if (ctx < 0 && p < end && data[p] == '{') {
          int pi = -1;
          for (int q = 0; q < spec.np; ++q) {
            if (spec.parent_len[q] == klen) {
              bool eq = true;
              for (int c = 0; c < klen; ++c)
                if (spec.parents[q][c] != (char)data[k0 + c]) {
                  eq = false;
                  break;
                }
              if (eq) { pi = q; break; }
            }
          }
          if (pi >= 0) {
            ctx = pi;
            ++p;  // enter the object
            continue;
          }
        }
        p = skip_value(data, p, end);
        continue;
      }
      uint8_t c = p < end ? data[p] : 0;
      if (spec.kind[fi] == 2) {  // string field
        if (c != '"') {  // non-string value under a string schema → absent
          p = skip_value(data, p, end);
          continue;
        }
        int32_t ulen = 0;
        int64_t s0 = p + 1;
        p = scan_string(data, s0, end, &ulen);
        if (p < end) ++p;  // closing quote
        str_start[(int64_t)spec.slot[fi] * n_docs + i] = s0 + boff;
        str_ulen[(int64_t)spec.slot[fi] * n_docs + i] = ulen;
        found[(int64_t)fi * n_docs + i] = 1;
        atomicAdd(&fcnt[fi], 1);
        continue;
      }
      double v = 0.0;
      bool is_int = true;
      if (c == 't') { v = 1.0; p += 4; }
      else if (c == 'f') { v = 0.0; p += 5; }
      else if (c == 'n') { p += 4; continue; }  // null → absent
      else if (c == '"') { p = skip_value(data, p, end); continue; }
      else p = parse_number(data, p, end, &v, &is_int);
      if (spec.kind[fi] == 1)
        out_f64[(int64_t)spec.slot[fi] * n_docs + i] = v;
      else
        out_i64[(int64_t)spec.slot[fi] * n_docs + i] = (int64_t)v;
      found[(int64_t)fi * n_docs + i] = 1;
      atomicAdd(&fcnt[fi], 1);
    }
  }
}

// wave-cooperative twin of json_parse_doc: identical state machine, but
// string scans advance 512 B/step via wave_scan_string / wave_skip_value
// and only lane 0 writes. Every branch depends on wave-uniform values.
DEV_INLINE void json_parse_doc_wave(const uint8_t* __restrict__ data,
                                    int64_t p, int64_t end, int lane,
                                    int64_t i, int64_t n_docs,
                                    const JsonSpec& spec,
                                    double* __restrict__ out_f64,
                                    int64_t* __restrict__ out_i64,
                                    int64_t* __restrict__ str_start,
                                    int32_t* __restrict__ str_ulen,
                                    uint8_t* __restrict__ found,
                                    int32_t* __restrict__ err,
                                    int* __restrict__ fcnt) {
  while (p < end && is_ws(data[p])) ++p;
  if (p >= end || data[p] != '{') {
    if (p < end && lane == 0) err[0] = 1;
    return;
  }
  ++p;
  int ctx = -1;
  for (;;) {
    while (p < end && (is_ws(data[p]) || data[p] == ',')) ++p;
    if (p >= end) break;
    if (data[p] == '}') {
      if (ctx < 0) break;
      ctx = -1;
      ++p;
      continue;
    }
    if (data[p] != '"') {
      if (lane == 0) err[0] = 1;
      break;
    }
    int64_t k0 = ++p;
    while (p < end && data[p] != '"') {
      if (data[p] == '\\') ++p;
      ++p;
    }
    int klen = (int)(p - k0);
    ++p;
    while (p < end && is_ws(data[p])) ++p;
    if (p < end && data[p] == ':') ++p;
    while (p < end && is_ws(data[p])) ++p;
    int fi = -1;
#pragma unroll
    for (int f = 0; f < JSON_MAX_FIELDS; ++f) {
      if (f < spec.nf && spec.name_len[f] == klen
          && spec.parent[f] == ctx) {
        bool eq = true;
        for (int c = 0; c < klen; ++c)
          if (spec.names[f][c] != (char)data[k0 + c]) { eq = false; break; }
        if (eq) { fi = f; break; }
      }
    }
    if (fi < 0) {
      if (ctx < 0 && p < end && data[p] == '{') {
        int pi = -1;
        for (int q = 0; q < spec.np; ++q) {
          if (spec.parent_len[q] == klen) {
            bool eq = true;
            for (int c = 0; c < klen; ++c)
              if (spec.parents[q][c] != (char)data[k0 + c]) {
                eq = false;
                break;
              }
            if (eq) { pi = q; break; }
          }
        }
        if (pi >= 0) {
          ctx = pi;
          ++p;
          continue;
        }
      }
      p = wave_skip_value(data, p, end, lane);
      continue;
    }
    uint8_t c = p < end ? data[p] : 0;
    if (spec.kind[fi] == 2) {
      if (c != '"') {
        p = wave_skip_value(data, p, end, lane);
        continue;
      }
      int32_t ulen = 0;
      int64_t s0 = p + 1;
      p = wave_scan_string(data, s0, end, lane, &ulen);
      if (p < end) ++p;
      if (lane == 0) {
        str_start[(int64_t)spec.slot[fi] * n_docs + i] = s0;
        str_ulen[(int64_t)spec.slot[fi] * n_docs + i] = ulen;
        found[(int64_t)fi * n_docs + i] = 1;
        atomicAdd(&fcnt[fi], 1);
      }
      continue;
    }
    double v = 0.0;
    bool is_int = true;
    if (c == 't') { v = 1.0; p += 4; }
    else if (c == 'f') { v = 0.0; p += 5; }
    else if (c == 'n') { p += 4; continue; }
    else if (c == '"') { p = wave_skip_value(data, p, end, lane); continue; }
    else p = parse_number(data, p, end, &v, &is_int);
    if (lane == 0) {
      if (spec.kind[fi] == 1)
        out_f64[(int64_t)spec.slot[fi] * n_docs + i] = v;
      else
        out_i64[(int64_t)spec.slot[fi] * n_docs + i] = (int64_t)v;
      found[(int64_t)fi * n_docs + i] = 1;
      atomicAdd(&fcnt[fi], 1);
    }
  }
}

__global__ __launch_bounds__(256)
void json_decode_wave_kernel(const uint8_t* __restrict__ data,
                             const int64_t* __restrict__ offsets,
                             int64_t n_docs, JsonSpec spec,
                             double* __restrict__ out_f64,
                             int64_t* __restrict__ out_i64,
                             int64_t* __restrict__ str_start,
                             int32_t* __restrict__ str_ulen,
                             uint8_t* __restrict__ found,
                             int32_t* __restrict__ err,
                             int32_t* __restrict__ found_count) {
  __shared__ int fcnt[JSON_MAX_FIELDS];
  if (threadIdx.x < JSON_MAX_FIELDS) fcnt[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  int64_t wstride = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave; i < n_docs; i += wstride)
    json_parse_doc_wave(data, offsets[i], offsets[i + 1], lane, i, n_docs,
                        spec, out_f64, out_i64, str_start, str_ulen, found,
                        err, fcnt);
  __syncthreads();
  if (threadIdx.x < JSON_MAX_FIELDS && fcnt[threadIdx.x])
    atomicAdd(&found_count[threadIdx.x], fcnt[threadIdx.x]);
}

// copy-out pass for ONE string field: thread per doc, unescaping into the
// contiguous output at out_offs[i] (out_offs = exclusive cumsum of ulen)
__global__ void json_copy_strings_kernel(const uint8_t* __restrict__ data,
                                         const int64_t* __restrict__ start,
                                         const int64_t* __restrict__ out_offs,
                                         const uint8_t* __restrict__ found,
                                         int64_t n_docs, int64_t data_len,
                                         uint8_t* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n_docs; i += stride) {
    if (!found[i]) continue;
    unescape_copy(data, start[i], data_len, out, out_offs[i], out_offs[i + 1]);
  }
}

extern "C" void launch_json_decode(const uint8_t* data, const int64_t* offsets,
                                   int64_t n_docs, int nf, const char* names,
                                   const int* name_len, const int* kind,
                                   const int* slot, const int* parent, int np,
                                   const char* parents, const int* parent_len,
                                   double* out_f64,
                                   int64_t* out_i64, int64_t* str_start,
                                   int32_t* str_ulen, uint8_t* found,
                                   int32_t* err, int32_t* found_count,
                                   int use_wave, hipStream_t st) {
  JsonSpec spec{};
  spec.nf = nf > JSON_MAX_FIELDS ? JSON_MAX_FIELDS : nf;
  for (int f = 0; f < spec.nf; ++f) {
    spec.name_len[f] = name_len[f];
    spec.kind[f] = kind[f];
    spec.slot[f] = slot[f];
    spec.parent[f] = parent[f];
    for (int c = 0; c < name_len[f] && c < JSON_MAX_NAME; ++c)
      spec.names[f][c] = names[f * JSON_MAX_NAME + c];
  }
  spec.np = np > JSON_MAX_PARENTS ? JSON_MAX_PARENTS : np;
  for (int q = 0; q < spec.np; ++q) {
    spec.parent_len[q] = parent_len[q];
    for (int c = 0; c < parent_len[q] && c < JSON_MAX_NAME; ++c)
      spec.parents[q][c] = parents[q * JSON_MAX_NAME + c];
  }
  if (use_wave) {
    // wave-per-doc: 4 waves/block, grid-stride
    int grid = (int)((n_docs + 3) / 4);
    if (grid > 8192) grid = 8192;
    if (grid < 1) return;
    json_decode_wave_kernel<<<grid, 256, 0, st>>>(data, offsets, n_docs,
                                                  spec, out_f64, out_i64,
                                                  str_start, str_ulen,
                                                  found, err, found_count);
    return;
  }
  int grid = (int)((n_docs + JSON_BLOCK - 1) / JSON_BLOCK);
  if (grid > 4096) grid = 4096;
  if (grid < 1) return;
  json_decode_kernel<<<grid, JSON_BLOCK, 0, st>>>(data, offsets, n_docs,
                                                  spec,
                                           out_f64, out_i64, str_start,
                                           str_ulen, found, err,
                                           found_count);
}

// wave-per-doc copy: the thread-per-doc kernel above is divergence-bound at
// ~72 GB/s on long strings (profiles r13 / VERDICT #9). A wave first scans
// the string's bytes 64 at a time for '\\' (or an early '"', which implies
// escapes since unescaped length == raw length only without them); clean
// strings — the overwhelmingly common case — are then copied with all 64
// lanes coalesced; escaped ones fall back to the sequential unescaper on
// lane 0.
__global__ void json_copy_strings_wave_kernel(
    const uint8_t* __restrict__ data, const int64_t* __restrict__ start,
    const int64_t* __restrict__ out_offs, const uint8_t* __restrict__ found,
    int64_t n_docs, int64_t data_len, uint8_t* __restrict__ out) {
  int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  int lane = threadIdx.x & 63;
  int64_t wstride = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave; i < n_docs; i += wstride) {
    if (!found[i]) continue;
    int64_t w = out_offs[i];
    int64_t ulen = out_offs[i + 1] - w;
    int64_t p = start[i];
    bool esc = false;
    for (int64_t base = 0; base < ulen; base += 64) {
      int64_t off = base + lane;
      bool mine = off < ulen && p + off < data_len &&
                  (data[p + off] == '\\' || data[p + off] == '"');
      if (__ballot(mine)) {
        esc = true;
        break;
      }
    }
    if (!esc) {
      for (int64_t off = lane; off < ulen; off += 64)
        if (p + off < data_len) out[w + off] = data[p + off];
    } else if (lane == 0) {
      unescape_copy(data, p, data_len, out, w, w + ulen);
    }
  }
}

extern "C" void launch_json_copy_strings(const uint8_t* data,
                                         const int64_t* start,
                                         const int64_t* out_offs,
                                         const uint8_t* found, int64_t n_docs,
                                         int64_t data_len, uint8_t* out,
                                         hipStream_t st) {
  int grid = (int)((n_docs + 255) / 256);
  if (grid > 2048) grid = 2048;
  if (grid < 1) return;
  json_copy_strings_kernel<<<grid, 256, 0, st>>>(data, start, out_offs, found,
                                                 n_docs, data_len, out);
}

extern "C" void launch_json_copy_strings_wave(
    const uint8_t* data, const int64_t* start, const int64_t* out_offs,
    const uint8_t* found, int64_t n_docs, int64_t data_len, uint8_t* out,
    hipStream_t st) {
  // 4 waves per block, wave per doc
  int64_t waves = n_docs;
  int grid = (int)((waves * 64 + 255) / 256);
  if (grid > 8192) grid = 8192;
  if (grid < 1) return;
  json_copy_strings_wave_kernel<<<grid, 256, 0, st>>>(
      data, start, out_offs, found, n_docs, data_len, out);
}
