// like.hip -- a12: LikeExpr (physical-expr/src/expressions/like.rs:103), i.e. arrow-string 50.0.0 like / ilike / nlike / nilike (third-party, pinned in
// datafusion-cli/Cargo.lock; the rules are restated in like_match.h).
//
// A scalar pattern is compiled on the host into anchored prefix, anchored suffix and the ordered middle segments between `%`s.  Three kernels serve it:
//   k_like_anchor   no middle segment (`lit`, `lit%`, `%lit`, `a%b`, `%`, ``): one lane per row compares at the row's start and end; the pattern bytes are
//                   kernel arguments (scalar loads).  No bitmap.
//   k_like_scan +   patterns with middle segments and no `_`: the value bytes [offsets[0], offsets[n]) are read ONCE as one contiguous stream, 16 B per lane,
//   k_like_resolve  LIKE_TILE bytes per workgroup plus a halo of LIKE_HALO bytes in LDS; for every part (prefix, middles, suffix) and every byte position the
//                   scan writes one bit "this part starts here" to a bitmap in global memory (1 bit per value byte and part).  The resolve pass gives every row
//                   one lane that reads bitmap words only: the prefix's bit at the row's start, the suffix's bit at end - suffix length, and per middle segment
//                   the next set bit at or after the cursor (find-first-set over 64-bit words), the cursor never passing end - suffix length.  A match that
//                   lies across two rows has its bit set but fails `start + length <= end` of either row.
//   k_like_row      everything else (`_`, ILIKE letters k / s that also match a non-ASCII scalar, patterns beyond LIKE_BYTES bytes or LIKE_PARTS parts,
//                   dictionary values decoded per row, and a pattern COLUMN, parsed per row): one lane per row walks characters with like_match.
// Results are bit-packed with one ballot per 64 rows; bits past `length` are zero whatever the operands' own last words hold.
#include "device_utils.h"
#include "like_match.h"

namespace dfgpu {

constexpr int LIKE_TILE = 4096;       // value bytes per workgroup of k_like_scan: 256 lanes x 16 B
constexpr int LIKE_HALO = 256;        // bytes staged behind a tile: a part is at most LIKE_HALO bytes long
constexpr int LIKE_PARTS = 6;         // prefix + suffix + up to 4 middle segments
constexpr int LIKE_BYTES = 256;       // all parts together

struct LikeParts {
  int32_t n, has_prefix, has_suffix, exact, ci, negated;      // parts in pattern order: [prefix] middles.. [suffix]
  int32_t off[LIKE_PARTS], len[LIKE_PARTS];
  uint64_t* bits[LIKE_PARTS];
  uint8_t bytes[LIKE_BYTES];                                  // ILIKE: lower case
};
struct LikeOperand { ColView v; int32_t scalar; };

// offsets[0], offsets[n] of the value column and the scalar pattern (length, validity, up to LIKE_BYTES bytes) in one read-back: slots 0..3 and 5..36; slot 4 is
// the flag word of k_like_row, cleared here
__global__ void k_like_probe(const int32_t* voff, int64_t n, const int32_t* poff, const uint8_t* pbytes, const uint64_t* pvalid, uint64_t* scratch) {
  const int t = threadIdx.x;
  const int32_t p0 = poff ? poff[0] : 0, plen = poff ? poff[1] - p0 : 0;
  if (t == 0) {
    scratch[0] = voff ? (uint64_t)(int64_t)voff[0] : 0; scratch[1] = voff ? (uint64_t)(int64_t)voff[n] : 0;
    scratch[2] = (uint64_t)(int64_t)plen; scratch[3] = (!pvalid || (pvalid[0] & 1)) ? 1 : 0; scratch[4] = 0;
  }
  if (t < LIKE_BYTES / 8) {
    uint64_t w = 0;
    if (plen <= LIKE_BYTES) for (int b = 0; b < 8; b++) { const int k = t * 8 + b; if (k < plen) w |= (uint64_t)pbytes[p0 + k] << (8 * b); }
    scratch[5 + t] = w;
  }
}

__device__ inline bool like_resolve_cell(const LikeOperand& o, int64_t i, int64_t* r) { return cell_resolve(o.v, o.scalar ? 0 : i, r); }

// one lane per row, exact for every pattern.  check_ascii: under ILIKE a pattern with a byte >= 0x80 raises flag bit 0 (the host answers NOT_IMPLEMENTED)
__global__ void __launch_bounds__(BLOCK) k_like_row(LikeOperand val, LikeOperand pat, int64_t n, int ci, int negated, int check_ascii, uint64_t* out_bits, uint64_t* out_valid,
                                                    unsigned long long* flag) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  bool v = false, ok = false;
  if (i < n) {
    int64_t a, b; const bool va = like_resolve_cell(val, i, &a), vb = like_resolve_cell(pat, i, &b);
    if (va && vb) {
      ok = true;
      const int32_t vo = val.v.offsets[a], vn = val.v.offsets[a + 1] - vo, po = pat.v.offsets[b], pn = pat.v.offsets[b + 1] - po;
      const uint8_t* p = (const uint8_t*)pat.v.values + po;
      if (check_ascii) { bool high = false; for (int32_t k = 0; k < pn; k++) high |= p[k] >= 0x80; if (high) atomicOr(flag, 1ull); }
      v = like_match((const uint8_t*)val.v.values + vo, vn, p, pn, ci != 0) != (negated != 0);
    }
  }
  const uint64_t mv = ballot64(v), mo = ballot64(ok);
  if (lane_id() == 0 && (i >> 6) < ((n + 63) >> 6)) { out_bits[i >> 6] = mv; if (out_valid) out_valid[i >> 6] = mo; }
}

__device__ inline bool like_bytes_equal(const uint8_t* v, const uint8_t* p, int32_t len, int ci) {
  for (int32_t k = 0; k < len; k++) if ((ci ? like_lower(v[k]) : v[k]) != p[k]) return false;
  return true;
}
// no middle segment: prefix at the row's start, suffix at its end (both may be absent), `exact` = the row is the prefix
__global__ void __launch_bounds__(BLOCK) k_like_anchor(const uint8_t* values, const int32_t* offsets, const uint64_t* valid, int64_t n, LikeParts P, uint64_t* out_bits, uint64_t* out_valid) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  bool v = false, ok = false;
  if (i < n && valid_at(valid, i)) {
    ok = true;
    const int32_t s = offsets[i], e = offsets[i + 1], len = e - s;
    const int32_t pl = P.has_prefix ? P.len[0] : 0, sl = P.has_suffix ? P.len[P.n - 1] : 0;
    bool m = P.exact ? len == pl : len >= pl + sl;
    if (m && pl) m = like_bytes_equal(values + s, P.bytes + P.off[0], pl, P.ci);
    if (m && sl) m = like_bytes_equal(values + (e - sl), P.bytes + P.off[P.n - 1], sl, P.ci);
    v = m != (P.negated != 0);
  }
  const uint64_t mv = ballot64(v), mo = ballot64(ok);
  if (lane_id() == 0 && (i >> 6) < ((n + 63) >> 6)) { out_bits[i >> 6] = mv; if (out_valid) out_valid[i >> 6] = mo; }
}

__device__ inline uint32_t like_fold4(uint32_t w) {       // ASCII A..Z -> a..z in four bytes at once; bytes >= 0x80 stay
  const uint32_t x = w & 0x7f7f7f7fu, ge_a = x + 0x3f3f3f3fu, gt_z = x + 0x25252525u;
  return w | (((ge_a & ~gt_z & ~w) & 0x80808080u) >> 2);
}
// 16 stream bytes at position p (a multiple of 16; base + p is 16-byte aligned).  Only bytes inside [lo, total) are read: a chunk wholly inside is one 16-B load,
// the ragged head and tail of the stream are loaded byte by byte, everything else is zero
__device__ inline uint4 like_load_chunk(const uint8_t* base, int64_t p, int64_t lo, int64_t total, int ci) {
  uint4 x = make_uint4(0, 0, 0, 0);
  if (p >= lo && p + 16 <= total) x = *(const uint4*)(base + p);
  else if (p + 16 > lo && p < total) {
    uint32_t w[4] = {0, 0, 0, 0};
    for (int b = 0; b < 16; b++) { const int64_t q = p + b; if (q >= lo && q < total) w[b >> 2] |= (uint32_t)base[q] << (8 * (b & 3)); }
    x = make_uint4(w[0], w[1], w[2], w[3]);
  }
  if (ci) { x.x = like_fold4(x.x); x.y = like_fold4(x.y); x.z = like_fold4(x.z); x.w = like_fold4(x.w); }
  return x;
}
// Stream positions count from `base`, the 16-byte boundary at or below the first value byte; the value bytes are the positions [lo, total).  Tile t = positions
// [t * LIKE_TILE, (t + 1) * LIKE_TILE) plus the halo.  Every lane tests the first byte of each part against its own 16 bytes in registers and verifies the
// candidates against LDS; a part matches at p only if p >= lo and p + length <= total.  Every lane writes its 16 bits of every bitmap (zeros past the stream), so
// the bitmaps need no clearing.
__global__ void __launch_bounds__(256) k_like_scan(const uint8_t* base, int64_t lo, int64_t total, LikeParts P) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[LIKE_TILE + LIKE_HALO];
  const int t = threadIdx.x;
  const int64_t p0 = (int64_t)blockIdx.x * LIKE_TILE + t * 16;
  const uint4 x = like_load_chunk(base, p0, lo, total, P.ci);
  *(uint4*)(tile + t * 16) = x;
  if (t < LIKE_HALO / 16) *(uint4*)(tile + LIKE_TILE + t * 16) = like_load_chunk(base, (int64_t)(blockIdx.x + 1) * LIKE_TILE + t * 16, lo, total, P.ci);
  __syncthreads();
  const uint32_t w[4] = {x.x, x.y, x.z, x.w};
  for (int s = 0; s < P.n; s++) {
    const int32_t len = P.len[s]; const uint8_t* pat = P.bytes + P.off[s]; const uint32_t first = pat[0];
    uint32_t m = 0;
#pragma unroll
    for (int b = 0; b < 16; b++) {
      if (((w[b >> 2] >> (8 * (b & 3))) & 0xffu) != first) continue;
      const int64_t p = p0 + b;
      if (p < lo || p + len > total) continue;
      bool eq = true;
      for (int32_t k = 1; k < len && eq; k++) eq = tile[t * 16 + b + k] == pat[k];
      if (eq) m |= 1u << b;
    }
    ((uint16_t*)P.bits[s])[p0 >> 4] = (uint16_t)m;
  }
}
// one lane per row over the bitmaps alone; shift = stream position of value byte 0 (positions = offsets + shift)
__global__ void __launch_bounds__(BLOCK) k_like_resolve(const int32_t* offsets, const uint64_t* valid, int64_t n, int64_t shift, LikeParts P, uint64_t* out_bits, uint64_t* out_valid) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  bool v = false, ok = false;
  if (i < n && valid_at(valid, i)) {
    ok = true;
    int64_t c = offsets[i] + shift, e = offsets[i + 1] + shift;
    int s = 0, last = P.n; bool m = true;
    if (P.has_prefix) { const int32_t l = P.len[0]; m = c + l <= e && bit_get(P.bits[0], c); c += l; s = 1; }
    if (m && P.has_suffix) { const int32_t l = P.len[P.n - 1]; m = c + l <= e && bit_get(P.bits[P.n - 1], e - l); e -= l; }
    if (P.has_suffix) last--;
    for (; m && s < last; s++) {
      const int32_t l = P.len[s]; const int64_t lim = e - l;       // the last admissible start
      if (c > lim) { m = false; break; }
      const uint64_t* bits = P.bits[s];
      int64_t wd = c >> 6; uint64_t x = bits[wd] & (~0ull << (c & 63));
      while (!x && ((wd + 1) << 6) <= lim) x = bits[++wd];
      const int64_t pos = (wd << 6) + (x ? __ffsll((unsigned long long)x) - 1 : 64);
      if (!x || pos > lim) { m = false; break; }
      c = pos + l;
    }
    v = m != (P.negated != 0);
  }
  const uint64_t mv = ballot64(v), mo = ballot64(ok);
  if (lane_id() == 0 && (i >> 6) < ((n + 63) >> 6)) { out_bits[i >> 6] = mv; if (out_valid) out_valid[i >> 6] = mo; }
}

static bool like_may_have_nulls(const dfgpu_array* a) { return a->validity != nullptr || (a->dictionary && a->dictionary->validity != nullptr); }
static const uint64_t* like_words(const BufferPtr& b) { return b ? (const uint64_t*)b->ptr : nullptr; }

// compiled parts -> kernel argument; false = more parts or bytes than the argument holds
static bool like_parts_of(const LikeCompiled& c, bool ci, bool negated, LikeParts* P) {
  std::vector<const std::vector<LikeToken>*> parts;
  if (c.has_prefix && !c.prefix.empty()) parts.push_back(&c.prefix);
  for (auto& m : c.middles) parts.push_back(&m);
  if (c.has_suffix && !c.exact) parts.push_back(&c.suffix);
  if (parts.size() > (size_t)LIKE_PARTS) return false;
  memset(P, 0, sizeof(*P));
  P->n = (int32_t)parts.size(); P->has_prefix = c.has_prefix && !c.prefix.empty(); P->has_suffix = c.has_suffix && !c.exact; P->exact = c.exact; P->ci = ci; P->negated = negated;
  int32_t at = 0;
  for (size_t k = 0; k < parts.size(); k++) {
    const int32_t l = (int32_t)parts[k]->size();
    if (l > LIKE_HALO || at + l > LIKE_BYTES) return false;
    P->off[k] = at; P->len[k] = l;
    for (int32_t j = 0; j < l; j++) P->bytes[at + j] = (*parts[k])[(size_t)j].byte;
    at += l;
  }
  return true;
}

static void like_launch_row(dfgpu_ctx* ctx, const dfgpu_array* values, const dfgpu_array* pattern, bool scalar, bool negated, bool ci, bool check_ascii, dfgpu_array* out) {
  KernelTimer kt_(ctx, "k_like_row");
  const int64_t n = values->length;
  LikeOperand v{make_view(values), 0}, p{make_view(pattern), scalar ? 1 : 0};
  hipLaunchKernelGGL(k_like_row, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, ctx->stream, v, p, n, ci ? 1 : 0, negated ? 1 : 0, check_ascii ? 1 : 0,
                     (uint64_t*)out->values->ptr, out->validity ? (uint64_t*)out->validity->ptr : nullptr, (unsigned long long*)(ctx->d_scratch64 + 4));
  KERNEL_CHECK();
  if (check_ascii && read_scratch(ctx, 4)) fail(DFGPU_NOT_IMPLEMENTED, "ILIKE with a non-ASCII pattern is not implemented: only ASCII patterns are case-folded on the device");
}

}  // namespace dfgpu

using namespace dfgpu;
extern "C" {

dfgpu_status dfgpu_like(dfgpu_ctx* ctx, const dfgpu_array* values, const dfgpu_array* pattern, int32_t pattern_is_scalar, int32_t negated, int32_t case_insensitive, dfgpu_array** out) {
  return guard(ctx, [&] {
    if (!values || !pattern || !out) fail(DFGPU_INVALID_ARGUMENT, "like: null argument");
    const bool scalar = pattern_is_scalar != 0, ci = case_insensitive != 0, neg = negated != 0, dict = values->type == DFGPU_DICTIONARY;
    if (pattern->type != DFGPU_UTF8) fail(DFGPU_INVALID_ARGUMENT, "like: the pattern has type %d, expected Utf8; the planner coerces first", pattern->type);
    if (dict ? (!values->dictionary || values->dictionary->type != DFGPU_UTF8) : values->type != DFGPU_UTF8)
      fail(DFGPU_INVALID_ARGUMENT, "like: the value has type %d, expected Utf8; the planner coerces first", logical_type(values));
    if (dict && !scalar) fail(DFGPU_INVALID_ARGUMENT, "like: a dictionary value needs a scalar pattern; the planner coerces first");
    if (scalar && pattern->length != 1) fail(DFGPU_INVALID_ARGUMENT, "like: a scalar pattern must have length 1, not %lld", (long long)pattern->length);
    if (!scalar && pattern->length != values->length) fail(DFGPU_INVALID_ARGUMENT, "like: operand lengths differ (%lld vs %lld)", (long long)values->length, (long long)pattern->length);
    const int64_t n = values->length;
    if (n == 0) { *out = new_fixed(ctx, DFGPU_BOOL, 0); return; }
    const bool need_valid = like_may_have_nulls(values) || pattern->validity != nullptr;
    if (!scalar) {                // a pattern column: parsed per row
      ArrayHolder h(new_fixed(ctx, DFGPU_BOOL, n, 0, 0, need_valid));
      if (ci) HIP_CHECK(hipMemsetAsync(ctx->d_scratch64 + 4, 0, 8, ctx->stream));
      like_launch_row(ctx, values, pattern, false, neg, ci, ci, h.get());
      if (need_valid) h.get()->null_count = -1;
      *out = h.release(); return;
    }
    // the scalar pattern and the bounds of the value stream, in one read-back
    hipLaunchKernelGGL(k_like_probe, dim3(1), dim3(64), 0, ctx->stream, dict ? nullptr : (const int32_t*)values->offsets->ptr, n, (const int32_t*)pattern->offsets->ptr,
                       pattern->values ? (const uint8_t*)pattern->values->ptr : nullptr, like_words(pattern->validity), ctx->d_scratch64);
    KERNEL_CHECK();
    const uint64_t* sc = read_scratch_range(ctx, 0, 5 + LIKE_BYTES / 8);
    const int64_t s0 = (int64_t)sc[0], s1 = (int64_t)sc[1], plen = (int64_t)sc[2];
    if (!sc[3]) { ArrayHolder h(new_fixed(ctx, DFGPU_BOOL, n, 0, 0, true)); h.get()->null_count = n; *out = h.release(); return; }       // NULL pattern: every row is NULL
    if (plen < 0) fail(DFGPU_INVALID_ARGUMENT, "like: the pattern's offsets decrease");
    const bool host_pattern = plen <= LIKE_BYTES;
    uint8_t pbytes[LIKE_BYTES]; memcpy(pbytes, sc + 5, LIKE_BYTES);
    LikeCompiled c; if (host_pattern) c = like_compile(pbytes, (int32_t)plen, ci);
    if (host_pattern && ci && c.non_ascii) fail(DFGPU_NOT_IMPLEMENTED, "ILIKE with a non-ASCII pattern is not implemented: only ASCII patterns are case-folded on the device");
    if (dict && values->dictionary->length < n) {          // once per dictionary entry, then the codes (as dfgpu_binary does for column vs scalar)
      dfgpu_array* dres = nullptr;
      dfgpu_status st = dfgpu_like(ctx, values->dictionary, pattern, 1, negated, case_insensitive, &dres);
      if (st != DFGPU_OK) fail(st, "%s", ctx->err.c_str());
      ArrayHolder dh(dres);
      *out = dict_predicate_map(ctx, values, dres); return;
    }
    ArrayHolder h(new_fixed(ctx, DFGPU_BOOL, n, 0, 0, need_valid));
    uint64_t* ob = (uint64_t*)h.get()->values->ptr; uint64_t* ov = need_valid ? (uint64_t*)h.get()->validity->ptr : nullptr;
    if (need_valid) h.get()->null_count = -1;
    LikeParts P;
    if (!dict && host_pattern && like_streamable(c, ci) && like_parts_of(c, ci, neg, &P)) {
      if (s0 < 0 || s1 < s0 || (s1 > s0 && (!values->values || !values->values->ptr)) || (values->values && (uint64_t)s1 > values->values->bytes)) fail(DFGPU_INVALID_ARGUMENT, "like: value offsets [%lld, %lld) lie outside the values buffer", (long long)s0, (long long)s1);
      const uint8_t* vb = values->values ? (const uint8_t*)values->values->ptr : nullptr;
      if (c.middles.empty()) {
        KernelTimer kt_(ctx, "k_like_anchor");
        hipLaunchKernelGGL(k_like_anchor, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, ctx->stream, vb, (const int32_t*)values->offsets->ptr, like_words(values->validity), n, P, ob, ov);
        KERNEL_CHECK(); *out = h.release(); return;
      }
      if (s1 > s0 && vb) {
        const int64_t mis = (int64_t)(((uintptr_t)vb + (uint64_t)s0) & 15), total = mis + (s1 - s0), ntiles = (total + LIKE_TILE - 1) / LIKE_TILE;
        const size_t per_part = (size_t)ntiles * (LIKE_TILE / 8);
        BufferPtr bitmaps = alloc_buffer(ctx, per_part * (size_t)P.n);
        for (int k = 0; k < P.n; k++) P.bits[k] = (uint64_t*)((uint8_t*)bitmaps->ptr + per_part * (size_t)k);
        { KernelTimer kt_(ctx, "k_like_scan");
          hipLaunchKernelGGL(k_like_scan, dim3(grid_for(ntiles, 1)), dim3(256), 0, ctx->stream, vb + s0 - mis, mis, total, P); }
        { KernelTimer kt_(ctx, "k_like_resolve");
          hipLaunchKernelGGL(k_like_resolve, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, ctx->stream, (const int32_t*)values->offsets->ptr, like_words(values->validity), n, mis - s0, P, ob, ov); }
        KERNEL_CHECK(); *out = h.release(); return;
      }
    }
    like_launch_row(ctx, values, pattern, true, neg, ci, ci && !host_pattern, h.get());        // k_like_probe cleared the flag word
    *out = h.release();
  });
}

}  // extern "C"
