// like_match.h -- the LIKE / ILIKE rules of arrow-string 50.0.0 (`like`, `ilike`, `nlike`, `nilike`), restated from their published behaviour, as plain
// host + device code: the one-row matcher of k_like_row and the host-side compilation of a scalar pattern into anchored prefix, anchored suffix and the
// ordered middle segments between `%`s.  No HIP type is used here, so the file also compiles as plain C++.
//
// The pattern is read left to right: `%` = any run of characters (also none), `_` = exactly one Unicode scalar, a backslash in front of `%` or `_` = that
// literal character, a backslash in front of anything else (or ending the pattern) = a literal backslash, everything else matches itself byte for byte.  The
// match is anchored at both ends.  ILIKE (ASCII patterns only) folds ASCII letters; the pattern letters k and s also match U+212A (Kelvin sign, E2 84 AA) and
// U+017F (long s, C5 BF), the only two non-ASCII scalars whose simple case folding is ASCII.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define LIKE_HD __host__ __device__
#else
#define LIKE_HD
#endif

namespace dfgpu {

LIKE_HD inline uint8_t like_lower(uint8_t c) { return (c >= 'A' && c <= 'Z') ? (uint8_t)(c | 0x20) : c; }
LIKE_HD inline bool like_cont(uint8_t c) { return (c & 0xC0) == 0x80; }                  // UTF-8 continuation byte

// bytes of v (rem > 0 of them left) that the literal pattern byte c consumes; 0 = no match
LIKE_HD inline int32_t like_literal(const uint8_t* v, int32_t rem, uint8_t c, bool ci) {
  if (!ci) return v[0] == c ? 1 : 0;
  const uint8_t f = like_lower(c);
  if (like_lower(v[0]) == f) return 1;
  if (f == 'k' && rem >= 3 && v[0] == 0xE2 && v[1] == 0x84 && v[2] == 0xAA) return 3;
  if (f == 's' && rem >= 2 && v[0] == 0xC5 && v[1] == 0xBF) return 2;
  return 0;
}

// One row against one pattern.  Greedy matching that remembers the last `%` only: on a mismatch the run that `%` stands for grows by one character and the
// rest of the pattern is tried again.  That is exact for patterns whose only repetition is `%` (the leftmost admissible place for what follows a `%` never
// rules out a match further right), so nothing is backtracked across a `%`.  The value position only ever rests on character boundaries: `_` and the growth of
// a `%` run step over continuation bytes, and literal pattern bytes are themselves whole characters of a valid UTF-8 pattern.
LIKE_HD inline bool like_match(const uint8_t* v, int32_t vn, const uint8_t* p, int32_t pn, bool ci) {
  int32_t vi = 0, pi = 0, star_p = -1, star_v = 0;
  for (;;) {
    if (pi < pn) {
      uint8_t c = p[pi]; int32_t step = 1; bool any = false;
      if (c == '%') { star_p = ++pi; star_v = vi; if (pi == pn) return true; continue; }
      if (c == '_') any = true;
      else if (c == '\\' && pi + 1 < pn && (p[pi + 1] == '%' || p[pi + 1] == '_')) { c = p[pi + 1]; step = 2; }
      if (vi < vn) {
        int32_t adv;
        if (any) { adv = 1; while (vi + adv < vn && like_cont(v[vi + adv])) adv++; }
        else adv = like_literal(v + vi, vn - vi, c, ci);
        if (adv) { vi += adv; pi += step; continue; }
      }
    } else if (vi == vn) return true;
    if (star_p < 0 || star_v >= vn) return false;
    star_v++; while (star_v < vn && like_cont(v[star_v])) star_v++;
    vi = star_v; pi = star_p;
  }
}

// ---- a scalar pattern, compiled once on the host
struct LikeToken { uint8_t byte; bool any; };                       // a literal byte, or any one character
struct LikeCompiled {
  bool has_prefix = false, has_suffix = false;                      // the pattern does not start / end with `%`; without any `%` the whole pattern is the prefix and `exact`
  bool exact = false;
  std::vector<LikeToken> prefix, suffix;
  std::vector<std::vector<LikeToken>> middles;                      // non-empty segments, in order
  bool any_token = false;                                           // some part holds `_`
  bool folds_beyond_ascii = false;                                  // ILIKE: some literal is k or s, which also match a non-ASCII scalar
  bool non_ascii = false;                                           // some pattern byte is >= 0x80
};
inline LikeCompiled like_compile(const uint8_t* p, int32_t pn, bool ci) {
  LikeCompiled c; std::vector<std::vector<LikeToken>> parts(1); bool any_percent = false;
  for (int32_t i = 0; i < pn; i++) {
    uint8_t b = p[i];
    if (b >= 0x80) c.non_ascii = true;
    if (b == '%') { any_percent = true; parts.emplace_back(); continue; }
    if (b == '_') { parts.back().push_back(LikeToken{0, true}); c.any_token = true; continue; }
    if (b == '\\' && i + 1 < pn && (p[i + 1] == '%' || p[i + 1] == '_')) b = p[++i];
    if (ci) { b = like_lower(b); if (b == 'k' || b == 's') c.folds_beyond_ascii = true; }
    parts.back().push_back(LikeToken{b, false});
  }
  if (!any_percent) { c.exact = c.has_prefix = true; c.prefix = parts[0]; return c; }
  c.has_prefix = !parts.front().empty(); c.has_suffix = !parts.back().empty();
  c.prefix = parts.front(); c.suffix = parts.back();
  for (size_t k = 1; k + 1 < parts.size(); k++) if (!parts[k].empty()) c.middles.push_back(parts[k]);
  return c;
}
// what the byte-parallel kernels take: every part is a plain byte string, also after ASCII folding
inline bool like_streamable(const LikeCompiled& c, bool ci) { return !c.any_token && !(ci && (c.folds_beyond_ascii || c.non_ascii)); }

}  // namespace dfgpu
