// GPU JSON decode: extracts the fields of a KNOWN schema straight from the
// device-resident binary column into columnar outputs — the "GPU column
// builder kernel" of SURVEY §2.9 (the general schema-inference path stays
// host-side via pyarrow, per the §7 plan; this file covers the
// configured-schema hot path). Numeric, bool and string fields, at top level
// or one object deep ("user.id"), at most JSON_MAX_FIELDS of them; every
// other key is skipped, nested objects/arrays/strings included. Strings are
// two passes: the parse records each string's start and unescaped length,
// and a copy kernel unescapes it into the output column.
//
// One document state machine serves two kernels. It is templated on a scan
// policy that answers "where is the next '"' or '\\'" — a thread walking
// 8 bytes per step, or a wave walking 512 — and says whether this lane
// stores results.
#include "common.h"
#include "kernels_api.h"

DEV_INLINE bool is_ws(uint8_t c) {
  return c == ' ' || c == '\t' || c == '\n' || c == '\r';
}

// SWAR: does any byte of x equal '"' (0x22) or '\\' (0x5C)? Long strings
// are walked 8 bytes per iteration instead of 1 — the thread-per-doc parse
// was byte-loop bound at ~72 GB/s on string-heavy docs (profiles r13).
DEV_INLINE uint64_t haszero64(uint64_t v) {
  return (v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull;
}

// 0x80 in every byte of x that is '"' or '\\' (and possibly in bytes above
// the first such byte)
DEV_INLINE uint64_t quote_or_bslash_mask(uint64_t x) {
  return haszero64(x ^ 0x2222222222222222ull) |
         haszero64(x ^ 0x5C5C5C5C5C5C5C5Cull);
}

DEV_INLINE bool has_quote_or_bslash(uint64_t x) {
  return quote_or_bslash_mask(x) != 0;
}

DEV_INLINE uint64_t load8(const uint8_t* p) {
  uint64_t x;
  __builtin_memcpy(&x, p, 8);
  return x;
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

// ============================ escapes ========================================
// What one backslash sequence stands for: where the walk continues and the
// 1..4 bytes it unescapes to (bytes[0] first). The length walk of the parse
// and the copy walk both go through decode_escape, so the bytes written are
// the bytes counted.
struct Escape {
  int64_t next;
  int n;
  uint8_t bytes[4];
};

// d[p] is a backslash. Simple escapes → 1 byte, unknown ones → the literal
// byte; \uXXXX → its UTF-8 form; a surrogate pair → one 4-byte sequence (a
// lone surrogate is encoded by itself, 3 bytes). A sequence cut off by `end`
// degrades: \u without four digits is the literal 'u', a final backslash is
// itself.
DEV_INLINE Escape decode_escape(const uint8_t* __restrict__ d, int64_t p,
                                int64_t end) {
  Escape r;
  if (!(p + 1 < end)) {
    r.next = p + 1;
    r.n = 1;
    r.bytes[0] = '\\';
    return r;
  }
  const uint8_t e = d[p + 1];
  if (e == 'u' && p + 5 < end) {
    uint32_t cp = hex4(d, p + 2);
    p += 6;
    if (cp >= 0xD800 && cp <= 0xDBFF && p + 5 < end && d[p] == '\\' &&
        d[p + 1] == 'u') {
      uint32_t lo = hex4(d, p + 2);
      if (lo >= 0xDC00 && lo <= 0xDFFF) {
        cp = 0x10000 + (((cp - 0xD800) << 10) | (lo - 0xDC00));
        r.next = p + 6;
        r.n = 4;
        r.bytes[0] = 0xF0 | (cp >> 18);
        r.bytes[1] = 0x80 | ((cp >> 12) & 0x3F);
        r.bytes[2] = 0x80 | ((cp >> 6) & 0x3F);
        r.bytes[3] = 0x80 | (cp & 0x3F);
        return r;
      }
    }
    r.next = p;
    if (cp < 0x80) {
      r.n = 1;
      r.bytes[0] = (uint8_t)cp;
    } else if (cp < 0x800) {
      r.n = 2;
      r.bytes[0] = 0xC0 | (cp >> 6);
      r.bytes[1] = 0x80 | (cp & 0x3F);
    } else {
      r.n = 3;
      r.bytes[0] = 0xE0 | (cp >> 12);
      r.bytes[1] = 0x80 | ((cp >> 6) & 0x3F);
      r.bytes[2] = 0x80 | (cp & 0x3F);
    }
    return r;
  }
  r.next = p + 2;
  r.n = 1;
  r.bytes[0] = e == 'n'   ? '\n'
               : e == 't' ? '\t'
               : e == 'r' ? '\r'
               : e == 'b' ? '\b'
               : e == 'f' ? '\f'
                          : e;  // \" \\ \/ and unknown escapes → literal
  return r;
}

// ============================ scan policies ==================================
// find_qb: first position ≥ p whose byte is '"' or '\\', or end.
// stores:  whether this lane writes the document's results.

// One thread owns the document: 8 bytes per step.
struct ThreadScan {
  DEV_INLINE bool stores() const { return true; }
  DEV_INLINE int64_t find_qb(const uint8_t* __restrict__ d, int64_t p,
                             int64_t end) const {
    while (p < end) {
      if (d[p] == '"' || d[p] == '\\') return p;
      if (p + 8 <= end && !has_quote_or_bslash(load8(d + p))) p += 8;
      else ++p;
    }
    return end;
  }
};

// One wave owns the document: every lane SWAR-checks its own 8 B chunk, a
// ballot finds the first hit, 512 B per step. For long documents the
// thread-per-doc walk is serialization-bound: even with SWAR it advances 8 B
// per dependent step. The ballot and the shuffle need all 64 lanes here
// together, which the invariant at json_parse_doc guarantees.
struct WaveScan {
  int lane;
  DEV_INLINE bool stores() const { return lane == 0; }
  DEV_INLINE int64_t find_qb(const uint8_t* __restrict__ d, int64_t p,
                             int64_t end) const {
    while (p < end) {
      int64_t base = p + (int64_t)lane * 8;
      uint64_t hits = 0;
      if (base < end) {
        if (base + 8 <= end) {
          hits = quote_or_bslash_mask(load8(d + base));
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
};

// Walk a JSON string body (p = first char after the opening quote), computing
// the UNESCAPED byte length. Returns the position of the closing quote, or
// end.
template <typename Scan>
DEV_INLINE int64_t scan_string(const Scan& sc, const uint8_t* __restrict__ d,
                               int64_t p, int64_t end, int32_t* ulen) {
  int32_t u = 0;
  while (p < end) {
    int64_t q = sc.find_qb(d, p, end);
    u += (int32_t)(q - p);
    p = q;
    if (p >= end || d[p] == '"') break;
    Escape e = decode_escape(d, p, end);
    p = e.next;
    u += e.n;
  }
  *ulen = u;
  return p;
}

// Skip a string whose value nobody wants (p = first char after the opening
// quote): a backslash hides the byte after it, whatever that is. Returns the
// position after the closing quote, or ≥ end.
template <typename Scan>
DEV_INLINE int64_t skip_string(const Scan& sc, const uint8_t* __restrict__ d,
                               int64_t p, int64_t end) {
  while (p < end) {
    p = sc.find_qb(d, p, end);
    if (p >= end) break;
    if (d[p] == '"') return p + 1;
    p += 2;
  }
  return p;
}

// skip a JSON value generically (string/number/object/array/literal)
template <typename Scan>
DEV_INLINE int64_t skip_value(const Scan& sc, const uint8_t* __restrict__ d,
                              int64_t p, int64_t end) {
  while (p < end && is_ws(d[p])) ++p;
  if (p >= end) return p;
  uint8_t c = d[p];
  if (c == '"') return skip_string(sc, d, p + 1, end);
  if (c == '{' || c == '[') {
    uint8_t open = c, close = (c == '{') ? '}' : ']';
    int depth = 0;
    while (p < end) {
      uint8_t x = d[p];
      if (x == '"') {
        p = skip_string(sc, d, p + 1, end);
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

// The copy walk: unescape the string body at p into out[w, wend), where
// wend - w is the length scan_string counted for it.
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
    if (d[p] == '\\') {
      Escape e = decode_escape(d, p, end);
      out[w++] = e.bytes[0];
      if (e.n > 1) out[w++] = e.bytes[1];
      if (e.n > 2) out[w++] = e.bytes[2];
      if (e.n > 3) out[w++] = e.bytes[3];
      p = e.next;
      continue;
    }
    out[w++] = d[p++];
  }
  return w;
}

// ============================ the document ===================================
// Parse document i = data[p, end) against the spec. Positions recorded in
// str_start are p-relative plus boff (data may be a staged copy that starts
// boff bytes into the column).
//
// INVARIANT for Scan = WaveScan: all 64 lanes of the wave run this function
// together on the same document, and every branch below (and in skip_value,
// scan_string and decode_escape) depends only on values that all lanes
// computed identically from the same bytes — find_qb returns the same
// position in every lane. So the wave never diverges, the ballot inside
// find_qb always sees 64 lanes, and `sc.stores()` is the only lane-dependent
// test; it guards nothing but stores.
template <typename Scan>
DEV_INLINE void json_parse_doc(const Scan& sc,
                               const uint8_t* __restrict__ data,
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
  while (p < end && is_ws(data[p])) ++p;
  if (p >= end || data[p] != '{') {
    if (p < end && sc.stores()) err[0] = 1;
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
    if (data[p] != '"') {
      if (sc.stores()) err[0] = 1;
      break;
    }
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
      p = skip_value(sc, data, p, end);
      continue;
    }
    uint8_t c = p < end ? data[p] : 0;
    if (spec.kind[fi] == 2) {  // string field
      if (c != '"') {  // non-string value under a string schema → absent
        p = skip_value(sc, data, p, end);
        continue;
      }
      int32_t ulen = 0;
      int64_t s0 = p + 1;
      p = scan_string(sc, data, s0, end, &ulen);
      if (p < end) ++p;  // closing quote
      if (sc.stores()) {
        str_start[(int64_t)spec.slot[fi] * n_docs + i] = s0 + boff;
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
    else if (c == 'n') { p += 4; continue; }  // null → absent
    else if (c == '"') { p = skip_value(sc, data, p, end); continue; }
    else p = parse_number(data, p, end, &v, &is_int);
    if (sc.stores()) {
      if (spec.kind[fi] == 1)
        out_f64[(int64_t)spec.slot[fi] * n_docs + i] = v;
      else
        out_i64[(int64_t)spec.slot[fi] * n_docs + i] = (int64_t)v;
      found[(int64_t)fi * n_docs + i] = 1;
      atomicAdd(&fcnt[fi], 1);
    }
  }
}

// Thread per document. LDS doc cache: each 128-doc tile's byte range is
// CONTIGUOUS in the binary column, so the block stages it with coalesced
// loads and threads then walk their documents out of LDS — the
// thread-per-doc global byte walk was latency-bound (each dependent 8 B load
// pays HBM latency with only a few waves per CU to hide it). Tiles larger
// than the cache parse from global.
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
      json_parse_doc(ThreadScan{}, dv, offsets[i] - boff,
                     offsets[i + 1] - boff, boff, i, n_docs, spec, out_f64,
                     out_i64, str_start, str_ulen, found, err, fcnt);
    __syncthreads();  // cache reused by the next tile
    if (threadIdx.x < JSON_MAX_FIELDS && fcnt[threadIdx.x])
      atomicAdd(&found_count[threadIdx.x], fcnt[threadIdx.x]);
  }
}

// Wave per document, straight from global memory. Dispatched when the batch's
// mean document length clears a threshold (the binding decides); on valid
// JSON its outputs are bit-identical to the thread-per-doc kernel's.
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
  const WaveScan sc{(int)(threadIdx.x & 63)};
  int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  int64_t wstride = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave; i < n_docs; i += wstride)
    json_parse_doc(sc, data, offsets[i], offsets[i + 1], 0, i, n_docs, spec,
                   out_f64, out_i64, str_start, str_ulen, found, err, fcnt);
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

extern "C" {

void launch_json_decode(const JsonSpec* spec, const uint8_t* data,
                        const int64_t* offsets, int64_t n_docs,
                        double* out_f64, int64_t* out_i64, int64_t* str_start,
                        int32_t* str_ulen, uint8_t* found, int32_t* err,
                        int32_t* found_count, int use_wave, hipStream_t st) {
  if (n_docs < 1) return;
  if (use_wave)  // 4 waves per block
    json_decode_wave_kernel<<<capped_grid(n_docs, 4, 8192), 256, 0, st>>>(
        data, offsets, n_docs, *spec, out_f64, out_i64, str_start, str_ulen,
        found, err, found_count);
  else
    json_decode_kernel<<<capped_grid(n_docs, JSON_BLOCK, 4096), JSON_BLOCK, 0,
                         st>>>(data, offsets, n_docs, *spec, out_f64, out_i64,
                               str_start, str_ulen, found, err, found_count);
}

void launch_json_copy_strings(const uint8_t* data, const int64_t* start,
                              const int64_t* out_offs, const uint8_t* found,
                              int64_t n_docs, int64_t data_len, uint8_t* out,
                              hipStream_t st) {
  if (n_docs < 1) return;
  json_copy_strings_kernel<<<capped_grid(n_docs), 256, 0, st>>>(
      data, start, out_offs, found, n_docs, data_len, out);
}

void launch_json_copy_strings_wave(const uint8_t* data, const int64_t* start,
                                   const int64_t* out_offs,
                                   const uint8_t* found, int64_t n_docs,
                                   int64_t data_len, uint8_t* out,
                                   hipStream_t st) {
  if (n_docs < 1) return;
  // 4 waves per block, wave per doc
  json_copy_strings_wave_kernel<<<capped_grid(n_docs, 4, 8192), 256, 0, st>>>(
      data, start, out_offs, found, n_docs, data_len, out);
}

}  // extern "C"
