// scalar_fn.hip -- a12: ScalarFunctionExpr (physical-expr/src/scalar_function.rs, dispatch in functions.rs) for the built-in functions the measured queries call:
//   date_part(part, Date32) -> Float64      datetime_expressions.rs:1019-1061 (arrow-arith temporal kernels over chrono), epoch :1128-1130
//   date_part(part, Timestamp) -> Float64   the same, all fourteen parts (to_ticks :1063-1076, epoch :1116-1126)      k_ts_part<UNIT, PART, VEC>
//   date_trunc(granularity, Timestamp) -> Timestamp   datetime_expressions.rs:429-692                                   k_ts_trunc<UNIT, GRAN, VEC>
//   character_length(Utf8)  -> Int32        unicode_expressions.rs:42-60      code points, not bytes
//   substr(Utf8, start [, count]) -> Utf8   unicode_expressions.rs:361-415
//   left / right(Utf8, n)   -> Utf8         unicode_expressions.rs:65-91, :206-
//   starts_with(Utf8, Utf8) -> Boolean      string_expressions.rs:509         a byte-prefix test
// A NULL in any argument of a row makes the row NULL.  Scalar arguments are length-1 arrays read with stride 0.
//
// date_part: civil-from-days in 64-bit integer arithmetic (days since 1970-01-01 -> proleptic Gregorian year / month / day; the divisions by 146097, 36524, 1460
// and 153 are by constants), so no Int32 day count overflows or faults.  Outside 0001-01-01 .. 9999-12-31 the value is whatever that arithmetic gives (the
// reference answers NULL only beyond chrono's own range; nothing pins that).  hour is 0.0 for a date, epoch is days * 86400.0; the sub-hour parts are
// NOT_IMPLEMENTED for Date32 (a Timestamp has them: see the Timestamp section below).  k_date_part gives every lane four days (one 16-B load, two 16-B stores) when the slice is 16-byte aligned.
//
// Strings: one pass turns each row into a byte range [begin, end) of the source (or into its number of code points).  A code point starts at every byte b with
// (b & 0xC0) != 0x80; these lead bytes are counted a word at a time (popcount over a masked 8- or 16-byte load), never byte by byte.
//   k_str_range<LaneOps> / k_char_length<LaneOps>   one lane per row: 8-byte words of the row, the search for code point k stops at the word that holds it
//   k_str_range<WaveOps> / k_char_length<WaveOps>   one wave per row: the lanes cover 16 B each (aligned 16-B loads, 1 KiB per step) and combine with a wave
//                                                   prefix over the per-lane lead-byte counts; the search stops at the step that holds code point k
// The host picks one of the two from values_bytes / length (STR_WAVE_ROW_BYTES) -- both known without a read-back.  Neither walks past the code point it looks
// for, so a row prefix (left(s, n > 0), substr(s, start <= 1, count)) touches the head of each row only.  Utf8 results: lengths -> exclusive_scan_u32 -> offsets,
// the byte total through the mailbox, then k_str_copy (the wave-cooperative copy of k_take_utf8_copy with per-row source positions).
// A negative substr count on a selected row whose string, start and count are all non-NULL raises DFGPU_FLAG_SUBSTR_LENGTH.
// A dictionary column that is the only column and has fewer entries than rows is evaluated once per entry: a Utf8 result stays a dictionary over the same codes,
// other results are gathered through the codes.  Every other dictionary argument (a dictionary as large as the column, one beside another column, a substr whose
// count can raise and every date_trunc -- their errors belong to rows) is decoded with a take and goes row by row.
#include <strings.h>
#include "device_utils.h"

namespace dfgpu {

constexpr int64_t STR_MAX = 0x7fffffff;              // Utf8 offsets are Int32: no row holds more code points than this

enum { DP_YEAR = 0, DP_QUARTER, DP_MONTH, DP_WEEK, DP_DAY, DP_DOY, DP_DOW, DP_HOUR, DP_EPOCH, DP_MINUTE, DP_SECOND, DP_MILLISECOND, DP_MICROSECOND, DP_NANOSECOND, DP_COUNT };      // from DP_MINUTE on: Timestamp only

// ---------------------------------------------------------------- date_part
__device__ inline bool dp_leap(int64_t y) { return (y % 4 == 0) && (y % 100 != 0 || y % 400 == 0); }
// the parts that depend on the day number alone (year .. dow), days since 1970-01-01
template <int PART> __device__ inline double day_part_of(int64_t days) {
  const int dow = (int)(((days % 7) + 11) % 7);                    // 1970-01-01 was a Thursday; days from Sunday
  if (PART == DP_DOW) return (double)dow;
  // civil from days: eras of 400 years = 146097 days starting on 0000-03-01
  const int64_t z = days + 719468;
  const int64_t era = (z >= 0 ? z : z - 146096) / 146097;
  const uint32_t doe = (uint32_t)(z - era * 146097);               // [0, 146096]
  const uint32_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;      // [0, 399]
  const uint32_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);    // [0, 365], from March 1
  const uint32_t mp = (5 * doy + 2) / 153;                         // [0, 11], March = 0
  const uint32_t d = doy - (153 * mp + 2) / 5 + 1;
  const uint32_t m = mp < 10 ? mp + 3 : mp - 9;
  const int64_t y = (int64_t)yoe + era * 400 + (m <= 2 ? 1 : 0);
  if (PART == DP_YEAR) return (double)y;
  if (PART == DP_MONTH) return (double)m;
  if (PART == DP_QUARTER) return (double)((m - 1) / 3 + 1);
  if (PART == DP_DAY) return (double)d;
  const int leap = dp_leap(y) ? 1 : 0;
  const int yday = m >= 3 ? (int)doy + 60 + leap : (int)doy - 305;        // 1-based day of the year
  if (PART == DP_DOY) return (double)yday;
  // ISO-8601 week: the week with the year's first Thursday is week 1
  const int wd = (dow + 6) % 7 + 1;                                // Monday = 1 .. Sunday = 7
  int week = (yday - wd + 10) / 7;
  if (week < 1) week = (yday + 365 + (dp_leap(y - 1) ? 1 : 0) - wd + 10) / 7;      // the last week of the year before
  else if (week == 53 && yday - (365 + leap) - wd + 10 >= 7) week = 1;            // already week 1 of the next year
  return (double)week;
}
template <int PART> __device__ inline double date_part_of(int32_t days32) {
  if (PART == DP_HOUR) return 0.0;
  if (PART == DP_EPOCH) return (double)days32 * 86400.0;
  return day_part_of<PART>(days32);
}
// VEC: `in` and `out` are 16-byte aligned; every lane takes four days per step, the ragged tail goes one day per lane
template <int PART, bool VEC> __global__ void __launch_bounds__(BLOCK) k_date_part(const int32_t* __restrict__ in, int64_t n, double* __restrict__ out) {
  const int64_t tid = (int64_t)blockIdx.x * BLOCK + threadIdx.x, stride = (int64_t)gridDim.x * BLOCK;
  if (VEC) {
    const int64_t n4 = n >> 2;
    for (int64_t g = tid; g < n4; g += stride) {
      const int4 d = ((const int4*)in)[g];
      double2 lo, hi;
      lo.x = date_part_of<PART>(d.x); lo.y = date_part_of<PART>(d.y); hi.x = date_part_of<PART>(d.z); hi.y = date_part_of<PART>(d.w);
      ((double2*)out)[2 * g] = lo; ((double2*)out)[2 * g + 1] = hi;
    }
    const int64_t i = (n4 << 2) + tid;
    if (i < n) out[i] = date_part_of<PART>(in[i]);
  } else {
    for (int64_t i = tid; i < n; i += stride) out[i] = date_part_of<PART>(in[i]);
  }
}
template <int PART> static void launch_date_part(dfgpu_ctx* ctx, const int32_t* in, int64_t n, double* out) {
  const bool vec = (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
  if (vec) hipLaunchKernelGGL((k_date_part<PART, true>), dim3(grid_for((n >> 2) + 4, BLOCK, (int64_t)ctx->num_cus * 8)), dim3(BLOCK), 0, ctx->stream, in, n, out);
  else hipLaunchKernelGGL((k_date_part<PART, false>), dim3(grid_for(n, BLOCK, (int64_t)ctx->num_cus * 8)), dim3(BLOCK), 0, ctx->stream, in, n, out);
}

// ---------------------------------------------------------------- Timestamp: date_part and date_trunc
// UNIT: 0 second, 1 millisecond, 2 microsecond, 3 nanosecond -- a template parameter, so every division below is by a compile-time constant
template <int UNIT> struct TsUnit { static constexpr int64_t PER_SEC = UNIT == 0 ? 1ll : UNIT == 1 ? 1000ll : UNIT == 2 ? 1000000ll : 1000000000ll; static constexpr int64_t PER_DAY = 86400ll * PER_SEC; };
__device__ inline int64_t floor_div(int64_t a, int64_t b) { const int64_t q = a / b; return (a % b != 0 && (a < 0)) ? q - 1 : q; }      // b > 0: div_euclid

// date_part over a Timestamp (datetime_expressions.rs:1019-1142): the instant is split with floor semantics (arrow's split_second is div_euclid / rem_euclid)
// into days, second of the day and nanosecond of the second.  second .. nanosecond keep the operation order of to_ticks (:1063-1076) and epoch that of :1123-1126,
// with contraction off: no fma of the add and the multiply, the division stays a division -- the results are those of IEEE double evaluation.
template <int UNIT, int PART> __device__ inline double ts_part_of(int64_t v) {
#pragma clang fp contract(off)
  constexpr int64_t U = TsUnit<UNIT>::PER_SEC;
  if (PART == DP_EPOCH) return (double)v / (double)U;
  const int64_t sec = floor_div(v, U);
  const int64_t days = floor_div(sec, 86400);
  if (PART <= DP_DOW) return day_part_of<PART>(days);
  const int32_t sod = (int32_t)(sec - days * 86400);               // [0, 86399]
  if (PART == DP_HOUR) return (double)(sod / 3600);
  if (PART == DP_MINUTE) return (double)((sod % 3600) / 60);
  const int64_t rem = v % U;                                       // no product: sec * U leaves an Int64 for v next to INT64_MIN
  const int32_t nanos = (int32_t)((rem < 0 ? rem + U : rem) * (1000000000ll / U));      // [0, 999999999]
  const double s = (double)(sod % 60) + (double)nanos / 1000000000.0;
  const double frac = PART == DP_SECOND ? 1.0 : PART == DP_MILLISECOND ? 1000.0 : PART == DP_MICROSECOND ? 1000000.0 : 1000000000.0;
  return s * frac;
}
// VEC: `in` and `out` are 16-byte aligned; every lane takes two instants per step (one 16-B load, one 16-B store), the odd last row goes alone
template <int UNIT, int PART, bool VEC> __global__ void __launch_bounds__(BLOCK) k_ts_part(const int64_t* __restrict__ in, int64_t n, double* __restrict__ out) {
  const int64_t tid = (int64_t)blockIdx.x * BLOCK + threadIdx.x, stride = (int64_t)gridDim.x * BLOCK;
  if (VEC) {
    const int64_t n2 = n >> 1;
    for (int64_t g = tid; g < n2; g += stride) {
      const longlong2 t = ((const longlong2*)in)[g];
      double2 r; r.x = ts_part_of<UNIT, PART>(t.x); r.y = ts_part_of<UNIT, PART>(t.y);
      ((double2*)out)[g] = r;
    }
    if (tid == 0 && (n & 1)) out[n - 1] = ts_part_of<UNIT, PART>(in[n - 1]);
  } else {
    for (int64_t i = tid; i < n; i += stride) out[i] = ts_part_of<UNIT, PART>(in[i]);
  }
}

// date_trunc (datetime_expressions.rs:429-692).  The reference converts every unit to nanoseconds, clears the fields below the granularity on a chrono
// NaiveDateTime (floor semantics, week = back to Monday) and divides back with `/`; here the same is computed in the column's own unit:
//   year .. second        floor to the period (civil arithmetic for year / quarter / month)
//   millisecond, microsecond   general_date_trunc's integer division, which truncates TOWARD ZERO: -1500 us at 'millisecond' is -1000 us, while -1500 ms at
//                         'second' is -2000 ms.  A granularity as fine as the unit or finer is the identity.
// The reference is defined only where the instant and its truncation fit an Int64 of nanoseconds; a row outside that window raises DFGPU_FLAG_TS_RANGE (the
// caller passes null for NULL or deselected rows' flag word) and gets 0.
enum { TG_YEAR = 0, TG_QUARTER, TG_MONTH, TG_WEEK, TG_DAY, TG_HOUR, TG_MINUTE, TG_SECOND, TG_MILLISECOND, TG_MICROSECOND, TG_COUNT };
__device__ inline int64_t days_from_civil(int64_t y, uint32_t m) {          // day number of y-m-01
  y -= m <= 2 ? 1 : 0;
  const int64_t era = (y >= 0 ? y : y - 399) / 400;
  const uint32_t yoe = (uint32_t)(y - era * 400);
  const uint32_t doy = (153 * (m > 2 ? m - 3 : m + 9) + 2) / 5;
  const uint32_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  return era * 146097 + (int64_t)doe - 719468;
}
template <int UNIT, int GRAN> __device__ inline int64_t ts_trunc_of(int64_t v, bool* out_of_range) {
  constexpr int64_t U = TsUnit<UNIT>::PER_SEC, DAY = TsUnit<UNIT>::PER_DAY, NS = 1000000000ll / U;      // NS: nanoseconds per unit
  constexpr int64_t LO = INT64_MIN / NS, HI = INT64_MAX / NS;             // the window in this unit (`/` rounds toward zero: inward on both sides)
  if (v < LO || v > HI) { *out_of_range = true; return 0; }
  if (GRAN >= TG_MILLISECOND) {
    constexpr int64_t G = GRAN == TG_MILLISECOND ? 1000ll : 1000000ll;    // granules per second
    if (U > G) { constexpr int64_t D = U / G; return v / D * D; }
    return v;
  }
  if (GRAN >= TG_DAY) {                                                    // a fixed period that divides the day
    constexpr int64_t P = GRAN == TG_DAY ? DAY : GRAN == TG_HOUR ? 3600 * U : GRAN == TG_MINUTE ? 60 * U : U;
    const int64_t q = floor_div(v, P);
    if (q < LO / P) { *out_of_range = true; return 0; }                    // q * P would lie below the window
    return q * P;
  }
  const int64_t days = floor_div(v, DAY);                                 // |days| <= 106752 inside the window
  int64_t first;
  if (GRAN == TG_WEEK) { const int64_t wd = (days % 7 + 10) % 7; first = days - wd; }      // 1970-01-01 was a Thursday: days since Monday
  else {
    const int64_t z = days + 719468;
    const int64_t era = (z >= 0 ? z : z - 146096) / 146097;
    const uint32_t doe = (uint32_t)(z - era * 146097);
    const uint32_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
    const uint32_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
    const uint32_t mp = (5 * doy + 2) / 153;
    const uint32_t m = mp < 10 ? mp + 3 : mp - 9;
    const int64_t y = (int64_t)yoe + era * 400 + (m <= 2 ? 1 : 0);
    first = days_from_civil(y, GRAN == TG_YEAR ? 1u : GRAN == TG_QUARTER ? (m - 1) / 3 * 3 + 1 : m);
  }
  if (first < LO / DAY) { *out_of_range = true; return 0; }
  return first * DAY;
}
struct TsTruncArgs { const int64_t* in; int64_t* out; const uint64_t* valid; const uint64_t* selected; uint32_t* flags; int64_t* bad; };      // bad: d_scratch64[TS_BAD_SLOT] receives one of the instants that raised, for check_flags' message

template <int UNIT, int GRAN> __device__ inline int64_t ts_trunc_row(const TsTruncArgs& A, int64_t i, int64_t v) {
  bool oor = false;
  const int64_t r = ts_trunc_of<UNIT, GRAN>(v, &oor);
  if (oor && valid_at(A.valid, i) && valid_at(A.selected, i)) { atomicOr(A.flags, DFGPU_FLAG_TS_RANGE); *A.bad = v; }
  return r;
}
template <int UNIT, int GRAN, bool VEC> __global__ void __launch_bounds__(BLOCK) k_ts_trunc(TsTruncArgs A, int64_t n) {
  const int64_t tid = (int64_t)blockIdx.x * BLOCK + threadIdx.x, stride = (int64_t)gridDim.x * BLOCK;
  if (VEC) {
    const int64_t n2 = n >> 1;
    for (int64_t g = tid; g < n2; g += stride) {
      const longlong2 t = ((const longlong2*)A.in)[g];
      longlong2 r; r.x = ts_trunc_row<UNIT, GRAN>(A, 2 * g, t.x); r.y = ts_trunc_row<UNIT, GRAN>(A, 2 * g + 1, t.y);
      ((longlong2*)A.out)[g] = r;
    }
    if (tid == 0 && (n & 1)) A.out[n - 1] = ts_trunc_row<UNIT, GRAN>(A, n - 1, A.in[n - 1]);
  } else {
    for (int64_t i = tid; i < n; i += stride) A.out[i] = ts_trunc_row<UNIT, GRAN>(A, i, A.in[i]);
  }
}
template <int UNIT, int PART> static void launch_ts_part(dfgpu_ctx* ctx, const int64_t* in, int64_t n, double* out) {
  const bool vec = (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
  if (vec) hipLaunchKernelGGL((k_ts_part<UNIT, PART, true>), dim3(grid_for((n >> 1) + 1, BLOCK, (int64_t)ctx->num_cus * 8)), dim3(BLOCK), 0, ctx->stream, in, n, out);
  else hipLaunchKernelGGL((k_ts_part<UNIT, PART, false>), dim3(grid_for(n, BLOCK, (int64_t)ctx->num_cus * 8)), dim3(BLOCK), 0, ctx->stream, in, n, out);
}
template <int UNIT> static void launch_ts_part_unit(dfgpu_ctx* ctx, int part, const int64_t* in, int64_t n, double* out) {
  switch (part) {
#define TP_CASE(P) case P: launch_ts_part<UNIT, P>(ctx, in, n, out); break;
    TP_CASE(DP_YEAR) TP_CASE(DP_QUARTER) TP_CASE(DP_MONTH) TP_CASE(DP_WEEK) TP_CASE(DP_DAY) TP_CASE(DP_DOY) TP_CASE(DP_DOW) TP_CASE(DP_HOUR) TP_CASE(DP_EPOCH)
    TP_CASE(DP_MINUTE) TP_CASE(DP_SECOND) TP_CASE(DP_MILLISECOND) TP_CASE(DP_MICROSECOND) TP_CASE(DP_NANOSECOND)
#undef TP_CASE
    default: fail(DFGPU_INTERNAL, "date_part: part %d", part);
  }
}
template <int UNIT, int GRAN> static void launch_ts_trunc(dfgpu_ctx* ctx, const TsTruncArgs& A, int64_t n) {
  const bool vec = (((uintptr_t)A.in | (uintptr_t)A.out) & 15) == 0;
  if (vec) hipLaunchKernelGGL((k_ts_trunc<UNIT, GRAN, true>), dim3(grid_for((n >> 1) + 1, BLOCK, (int64_t)ctx->num_cus * 8)), dim3(BLOCK), 0, ctx->stream, A, n);
  else hipLaunchKernelGGL((k_ts_trunc<UNIT, GRAN, false>), dim3(grid_for(n, BLOCK, (int64_t)ctx->num_cus * 8)), dim3(BLOCK), 0, ctx->stream, A, n);
}
template <int UNIT> static void launch_ts_trunc_unit(dfgpu_ctx* ctx, int gran, const TsTruncArgs& A, int64_t n) {
  switch (gran) {
#define TG_CASE(G) case G: launch_ts_trunc<UNIT, G>(ctx, A, n); break;
    TG_CASE(TG_YEAR) TG_CASE(TG_QUARTER) TG_CASE(TG_MONTH) TG_CASE(TG_WEEK) TG_CASE(TG_DAY) TG_CASE(TG_HOUR) TG_CASE(TG_MINUTE) TG_CASE(TG_SECOND) TG_CASE(TG_MILLISECOND) TG_CASE(TG_MICROSECOND)
#undef TG_CASE
    default: fail(DFGPU_INTERNAL, "date_trunc: granularity %d", gran);
  }
}

// the scalar part name (length, validity, up to 16 bytes) in one read-back: slots 0..3
__global__ void k_fn_probe_name(const int32_t* off, const uint8_t* bytes, const uint64_t* valid, uint64_t* scratch) {
  if (threadIdx.x) return;
  const int32_t p0 = off[0], len = off[1] - p0;
  scratch[0] = (uint64_t)(int64_t)len; scratch[1] = (!valid || (valid[0] & 1)) ? 1 : 0;
  uint64_t w[2] = {0, 0};
  if (len > 0 && len <= 16) for (int b = 0; b < len; b++) w[b >> 3] |= (uint64_t)bytes[p0 + b] << (8 * (b & 7));
  scratch[2] = w[0]; scratch[3] = w[1];
}

// ---------------------------------------------------------------- lead bytes of UTF-8
// bit 7 of every byte of w that starts a code point: a byte continues one iff its bit 7 is set and its bit 6 is clear
__device__ inline uint64_t lead_mask(uint64_t w) { return ~(w & (~w << 1)) & 0x8080808080808080ull; }
__device__ inline int nth_lead(uint64_t m, int k) {              // byte number of set bit k (0-based) of a lead mask that has more than k bits
  for (; k > 0; k--) m &= m - 1;
  return (__ffsll((unsigned long long)m) - 1) >> 3;
}
constexpr uint64_t NO_LEADS = 0x8080808080808080ull;             // eight continuation bytes: what stands in for bytes outside the row

struct LaneOps {          // one lane owns the row: 8-byte words from the row's first byte on (unaligned loads), the ragged last word byte by byte
  __device__ static uint64_t word(const uint8_t* v, int32_t p, int32_t e) {
    uint64_t w;
    if (e - p >= 8) { __builtin_memcpy(&w, v + p, 8); return w; }
    w = NO_LEADS;
    for (int b = 0; b < e - p; b++) w = (w & ~(0xffull << (8 * b))) | ((uint64_t)v[p + b] << (8 * b));
    return w;
  }
  // position of the lead byte of code point k (0-based) of [s, e); e when the range holds at most k code points
  __device__ static int32_t skip(const uint8_t* v, int32_t s, int32_t e, int64_t k) {
    if (k <= 0) return s;
    for (int32_t p = s; p < e; p += 8) {
      const uint64_t m = lead_mask(word(v, p, e));
      const int c = __popcll((unsigned long long)m);
      if ((int64_t)c > k) return p + nth_lead(m, (int)k);
      k -= c;
    }
    return e;
  }
  __device__ static int64_t count(const uint8_t* v, int32_t s, int32_t e) {
    int64_t c = 0;
    for (int32_t p = s; p < e; p += 8) c += __popcll((unsigned long long)lead_mask(word(v, p, e)));
    return c;
  }
  __device__ static bool writer() { return true; }
};

struct WaveOps {          // one wave owns the row; every argument is wave-uniform.  Chunks are the aligned 16-byte blocks of memory the row touches
  // lead masks of the chunk at address a: bytes outside [lo, hi) count as continuation bytes and are not read
  __device__ static void chunk(const uint8_t* a, const uint8_t* lo, const uint8_t* hi, uint64_t* m0, uint64_t* m1) {
    uint64_t w0 = NO_LEADS, w1 = NO_LEADS;
    if (a >= lo && a + 16 <= hi) { const uint4 x = *(const uint4*)a; w0 = (uint64_t)x.x | ((uint64_t)x.y << 32); w1 = (uint64_t)x.z | ((uint64_t)x.w << 32); }
    else if (a + 16 > lo && a < hi) {
      for (int b = 0; b < 8; b++) if (a + b >= lo && a + b < hi) w0 = (w0 & ~(0xffull << (8 * b))) | ((uint64_t)a[b] << (8 * b));
      for (int b = 0; b < 8; b++) if (a + 8 + b >= lo && a + 8 + b < hi) w1 = (w1 & ~(0xffull << (8 * b))) | ((uint64_t)a[8 + b] << (8 * b));
    }
    *m0 = lead_mask(w0); *m1 = lead_mask(w1);
  }
  __device__ static int32_t skip(const uint8_t* v, int32_t s, int32_t e, int64_t k) {
    if (k <= 0 || s >= e) return s;
    const uint8_t* lo = v + s; const uint8_t* hi = v + e;
    const uint8_t* a0 = (const uint8_t*)((uintptr_t)lo & ~(uintptr_t)15);
    const int lane = lane_id();
    int64_t seen = 0;
    for (const uint8_t* base = a0; base < hi; base += 16 * WAVE) {         // wave-uniform trip count
      const uint8_t* a = base + 16 * lane;
      uint64_t m0, m1; chunk(a, lo, hi, &m0, &m1);
      const int c0 = __popcll((unsigned long long)m0), c = c0 + __popcll((unsigned long long)m1);
      const int inc = wave_inclusive_sum(c);
      const int total = __shfl(inc, 63, 64);
      if (seen + total > k) {                                              // code point k starts in this step, in exactly one lane's chunk
        const int64_t before = seen + inc - c;
        const bool mine = before <= k && k < before + c;
        int32_t pos = 0;
        if (mine) { const int r = (int)(k - before); pos = (int32_t)(a - v) + (r < c0 ? nth_lead(m0, r) : 8 + nth_lead(m1, r - c0)); }
        const uint64_t who = ballot64(mine);
        return __shfl(pos, __ffsll((unsigned long long)who) - 1, 64);
      }
      seen += total;
    }
    return e;
  }
  __device__ static int64_t count(const uint8_t* v, int32_t s, int32_t e) {
    if (s >= e) return 0;
    const uint8_t* lo = v + s; const uint8_t* hi = v + e;
    const uint8_t* a0 = (const uint8_t*)((uintptr_t)lo & ~(uintptr_t)15);
    int64_t c = 0;
    for (const uint8_t* base = a0; base < hi; base += 16 * WAVE) {
      uint64_t m0, m1; chunk(base + 16 * lane_id(), lo, hi, &m0, &m1);
      c += __popcll((unsigned long long)m0) + __popcll((unsigned long long)m1);
    }
    return wave_sum(c);
  }
  __device__ static bool writer() { return lane_id() == 0; }
};

struct StrCol { const uint8_t* values; const int32_t* offsets; int32_t stride; };          // stride 0: a scalar
struct IntCol { const int64_t* p; int32_t stride; };
struct RangeArgs { int32_t fn, nargs; StrCol s; IntCol a, b; const uint64_t* valid; const uint64_t* selected; };      // valid: all arguments together, one bit per row (or null)

__device__ inline int64_t clamp_chars(uint64_t k) { return k > (uint64_t)STR_MAX ? STR_MAX : (int64_t)k; }
// the byte range [*begin, *end) of row i's result inside s.values; the row is not NULL
template <class OPS> __device__ inline void str_range(const RangeArgs& A, int64_t i, int32_t* begin, int32_t* end, uint32_t* flags) {
  const int64_t r = i * A.s.stride;
  const int32_t s = A.s.offsets[r], e = A.s.offsets[r + 1];
  const uint8_t* v = A.s.values;
  const int64_t x = A.a.p[i * A.a.stride];
  int64_t skip = 0, take = -1;                                     // code points; take < 0: to the end of the row
  *begin = *end = s;
  if (A.fn == DFGPU_FN_SUBSTR) {
    if (x >= 1) skip = clamp_chars((uint64_t)x - 1);
    if (A.nargs == 3) {
      const int64_t c = A.b.p[i * A.b.stride];
      if (c < 0) { if (OPS::writer() && (A.selected == nullptr || bit_get(A.selected, i))) atomicOr(flags, DFGPU_FLAG_SUBSTR_LENGTH); return; }
      if (x >= 1) take = clamp_chars((uint64_t)c);
      else { const int64_t t = c + (x == INT64_MIN ? x : x - 1); take = t > 0 ? clamp_chars((uint64_t)t) : 0; }        // c >= 0 and the other term < 0: no overflow
    }
  } else if (A.fn == DFGPU_FN_LEFT) {
    if (x == 0) return;
    if (x > 0) take = clamp_chars((uint64_t)x);
    else { const uint64_t drop = 0 - (uint64_t)x; const uint64_t len = (uint64_t)OPS::count(v, s, e); if (len <= drop) return; take = (int64_t)(len - drop); }
  } else {          // RIGHT
    if (x == 0) return;
    if (x < 0) skip = clamp_chars(0 - (uint64_t)x);
    else { const uint64_t len = (uint64_t)OPS::count(v, s, e); skip = len > (uint64_t)x ? (int64_t)(len - (uint64_t)x) : 0; }
  }
  if (take == 0) return;
  const int32_t b = OPS::skip(v, s, e, skip);
  *begin = b; *end = take < 0 ? e : OPS::skip(v, b, e, take);
}

// ROWS_PER_BLOCK = BLOCK for LaneOps, BLOCK / WAVE for WaveOps
template <class OPS, int ROWS> __device__ inline int64_t row_of_thread() { return ROWS == BLOCK ? (int64_t)blockIdx.x * BLOCK + threadIdx.x : (int64_t)blockIdx.x * ROWS + (threadIdx.x >> 6); }

template <class OPS, int ROWS> __global__ void __launch_bounds__(BLOCK) k_str_range(RangeArgs A, int64_t n, uint32_t* lens, uint32_t* begins, uint32_t* flags) {
  const int64_t i = row_of_thread<OPS, ROWS>();
  if (i >= n) return;                                              // wave-uniform for WaveOps: a wave has one row
  int32_t b = 0, e = 0;
  if (valid_at(A.valid, i)) str_range<OPS>(A, i, &b, &e, flags);
  if (OPS::writer()) { lens[i] = (uint32_t)(e - b); begins[i] = (uint32_t)b; }
}
template <class OPS, int ROWS> __global__ void __launch_bounds__(BLOCK) k_char_length(StrCol s, const uint64_t* valid, int64_t n, int32_t* out) {
  const int64_t i = row_of_thread<OPS, ROWS>();
  if (i >= n) return;
  int64_t c = 0;
  if (valid_at(valid, i)) { const int64_t r = i * s.stride; c = OPS::count(s.values, s.offsets[r], s.offsets[r + 1]); }
  if (OPS::writer()) out[i] = (int32_t)c;
}

// The wave-cooperative copy of k_take_utf8_copy (select.hip): one wave per 64 output rows, whose bytes are one contiguous span of the output; the lanes copy it
// byte-interleaved and every byte finds its row by a 6-step search over the wave's 64 row starts.  Source positions come from `begins`.
__global__ void __launch_bounds__(BLOCK) k_str_copy(const uint8_t* src, const uint32_t* begins, const uint64_t* out_off64, int64_t n, int32_t* out_off, uint8_t* out, uint64_t total) {
  const int lane = lane_id();
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;                      // rows 0 .. n (row n only carries the final offset)
  const uint64_t o = i < n ? out_off64[i] : total;
  const uint64_t next = i + 1 < n ? out_off64[i + 1] : total;
  if (i <= n) out_off[i] = (int32_t)o;
  int64_t s = 0;
  if (i < n && next > o) s = (int64_t)begins[i];
  const uint64_t wbeg = __shfl((unsigned long long)o, 0, 64), wend = __shfl((unsigned long long)next, 63, 64);
  const uint32_t rel = (uint32_t)(o - wbeg);
  for (uint64_t pb = wbeg; pb < wend; pb += WAVE) {                                    // wave-uniform trip count
    const uint64_t p = pb + (uint64_t)lane; const bool act = p < wend;
    const uint32_t pr = (uint32_t)((act ? p : wend - 1) - wbeg);
    int lo = 0;                                                                        // largest r with rel_r <= pr: among rows starting at p the last one, which is the one with bytes
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) { int mid = lo + step; uint32_t om = (uint32_t)__shfl((int)rel, mid & 63, 64); if (mid < WAVE && om <= pr) lo = mid; }
    const uint32_t orow = (uint32_t)__shfl((int)rel, lo, 64);
    const int64_t srow = (int64_t)__shfl((long long)s, lo, 64);
    if (act) out[p] = src[srow + (int64_t)(pr - orow)];
  }
}

// starts_with: one lane per row, the result bit-packed by one ballot per 64 rows (bits past n are zero)
__global__ void __launch_bounds__(BLOCK) k_starts_with(StrCol s, StrCol p, const uint64_t* valid, int64_t n, uint64_t* out_bits) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  bool v = false;
  if (i < n && valid_at(valid, i)) {
    const int64_t rs = i * s.stride, rp = i * p.stride;
    const int32_t so = s.offsets[rs], sl = s.offsets[rs + 1] - so, po = p.offsets[rp], pl = p.offsets[rp + 1] - po;
    if (pl <= sl) {
      v = true;
      for (int32_t k = 0; k < pl && v; k++) v = s.values[so + k] == p.values[po + k];
    }
  }
  const uint64_t m = ballot64(v);
  if (lane_id() == 0 && (i >> 6) < ((n + 63) >> 6)) out_bits[i >> 6] = m;
}

// the validity of a result: the AND of its arguments' validity words (a scalar's bit 0 stands for every row); bits past n are zero
struct ValidSrc { const uint64_t* w; int32_t scalar; };
__global__ void __launch_bounds__(BLOCK) k_valid_and(ValidSrc a, ValidSrc b, ValidSrc c, int64_t n, uint64_t* out) {
  const int64_t wi = (int64_t)blockIdx.x * BLOCK + threadIdx.x, nw = (n + 63) >> 6;
  if (wi >= nw) return;
  uint64_t x = ~0ull;
  if (a.w) x &= a.scalar ? ((a.w[0] & 1) ? ~0ull : 0ull) : a.w[wi];
  if (b.w) x &= b.scalar ? ((b.w[0] & 1) ? ~0ull : 0ull) : b.w[wi];
  if (c.w) x &= c.scalar ? ((c.w[0] & 1) ? ~0ull : 0ull) : c.w[wi];
  if (wi == nw - 1 && (n & 63)) x &= (1ull << (n & 63)) - 1;
  out[wi] = x;
}

// a fixed-width result per dictionary entry gathered through the codes; a NULL or out-of-range code and a NULL entry give NULL
template <typename T> __global__ void __launch_bounds__(BLOCK) k_dict_gather(const void* keys, int key_type, const uint64_t* key_valid, int64_t n, const T* dvals, const uint64_t* dvalid,
                                                                             int64_t dict_len, T* out, uint64_t* out_valid) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  bool ok = false; T v = T(0);
  if (i < n && valid_at(key_valid, i)) {
    const int64_t c = key_at(keys, key_type, i);
    if (c >= 0 && c < dict_len && valid_at(dvalid, c)) { ok = true; v = dvals[c]; }
  }
  if (i < n) out[i] = v;
  if (out_valid) { const uint64_t m = ballot64(ok); if (lane_id() == 0 && (i >> 6) < ((n + 63) >> 6)) out_valid[i >> 6] = m; }
}

// ---------------------------------------------------------------- host side
static bool host_scalar_i64(const dfgpu_array* a, int64_t* v) {          // the value of a non-NULL Int64 scalar whose host mirror exists (an imported literal)
  if (!a || a->type != DFGPU_INT64 || a->length != 1 || !a->has_host_scalar || !a->host_scalar_valid) return false;
  memcpy(v, a->host_scalar, 8); return true;
}
static bool host_scalar_null(const dfgpu_array* a) { return a && a->length == 1 && a->has_host_scalar && !a->host_scalar_valid; }      // a NULL literal
// the values of a dictionary column as a plain column: take(dictionary, codes)
static dfgpu_array* decode_dictionary(dfgpu_ctx* ctx, const dfgpu_array* d) {
  ArrayHolder codes(new_array(ctx, d->key_type, d->length));
  codes.get()->values = d->values; codes.get()->validity = d->validity; codes.get()->null_count = d->validity ? d->null_count : 0;
  dfgpu_array* wide = nullptr;
  dfgpu_status st = dfgpu_cast(ctx, codes.get(), DFGPU_INT64, 0, 0, &wide);
  if (st != DFGPU_OK) fail(st, "%s", ctx->err.c_str());
  ArrayHolder w(wide);
  ArrayHolder out(take_impl(ctx, d->dictionary, wide->values->ptr, 8, wide->validity ? (const uint64_t*)wide->validity->ptr : nullptr, d->length));
  check_flags(ctx, "scalar_function: dictionary codes");
  return out.release();
}
static const uint64_t* words_of(const BufferPtr& b) { return b ? (const uint64_t*)b->ptr : nullptr; }

// validity of the result over n rows: none, one non-scalar argument's own buffer (shared, not copied), or the AND of several
static BufferPtr result_validity(dfgpu_ctx* ctx, const dfgpu_array* const* args, const int32_t* scalar, int32_t nargs, int64_t n, int64_t* null_count) {
  ValidSrc src[3] = {{nullptr, 0}, {nullptr, 0}, {nullptr, 0}}; int k = 0; const dfgpu_array* only = nullptr;
  for (int32_t j = 0; j < nargs; j++) if (args[j]->validity) { src[k++] = ValidSrc{(const uint64_t*)args[j]->validity->ptr, scalar[j] ? 1 : 0}; only = args[j]; }
  if (k == 0) { *null_count = 0; return nullptr; }
  if (k == 1 && !src[0].scalar) { *null_count = only->null_count; return only->validity; }
  BufferPtr out = alloc_buffer(ctx, bitmap_bytes(n));
  hipLaunchKernelGGL(k_valid_and, dim3(grid_for((n + 63) >> 6, BLOCK)), dim3(BLOCK), 0, ctx->stream, src[0], src[1], src[2], n, (uint64_t*)out->ptr);
  KERNEL_CHECK();
  *null_count = -1; return out;
}
static StrCol str_col(const dfgpu_array* a, int32_t scalar) { return StrCol{a->values ? (const uint8_t*)a->values->ptr : nullptr, (const int32_t*)a->offsets->ptr, scalar ? 0 : 1}; }
static IntCol int_col(const dfgpu_array* a, int32_t scalar) { return IntCol{(const int64_t*)a->values->ptr, scalar ? 0 : 1}; }

static int date_part_code(const char* name, size_t len) {
  static const char* names[DP_COUNT] = {"year", "quarter", "month", "week", "day", "doy", "dow", "hour", "epoch", "minute", "second", "millisecond", "microsecond", "nanosecond"};
  for (int p = 0; p < DP_COUNT; p++) if (strlen(names[p]) == len && !strncasecmp(names[p], name, len)) return p;
  return -1;
}
static int date_trunc_code(const char* name, size_t len) {
  static const char* names[TG_COUNT] = {"year", "quarter", "month", "week", "day", "hour", "minute", "second", "millisecond", "microsecond"};
  for (int g = 0; g < TG_COUNT; g++) if (strlen(names[g]) == len && !strncasecmp(names[g], name, len)) return g;
  return -1;
}
// the scalar Utf8 name argument of date_part / date_trunc: its length (negative: offsets decrease), validity and first 16 bytes
static int64_t probe_name(dfgpu_ctx* ctx, const dfgpu_array* part, bool* valid, char name[17]) {
  hipLaunchKernelGGL(k_fn_probe_name, dim3(1), dim3(64), 0, ctx->stream, (const int32_t*)part->offsets->ptr, part->values ? (const uint8_t*)part->values->ptr : nullptr, words_of(part->validity), ctx->d_scratch64);
  KERNEL_CHECK();
  const uint64_t* sc = read_scratch_range(ctx, 0, 4);
  *valid = sc[1] != 0; memset(name, 0, 17); memcpy(name, sc + 2, 16);
  return (int64_t)sc[0];
}

static dfgpu_array* date_part(dfgpu_ctx* ctx, const dfgpu_array* part, const dfgpu_array* dates) {
  const int64_t n = dates->length;
  bool part_valid = false; char name[17];
  const int64_t len = probe_name(ctx, part, &part_valid, name);
  if (!part_valid) { ArrayHolder h(new_fixed(ctx, DFGPU_FLOAT64, n, 0, 0, true)); if (n) HIP_CHECK(hipMemsetAsync(h.get()->values->ptr, 0, (size_t)n * 8, ctx->stream)); h.get()->null_count = n; return h.release(); }
  if (len < 0) fail(DFGPU_INVALID_ARGUMENT, "date_part: the part name's offsets decrease");
  const int p = len <= 16 ? date_part_code(name, (size_t)len) : -1;
  const bool ts = is_timestamp(dates->type);
  if (p >= DP_MINUTE && !ts) fail(DFGPU_NOT_IMPLEMENTED, "date_part('%s', Date32) is not implemented on the device", name);
  if (p < 0) fail(DFGPU_EXECUTION, "Date part '%s' not supported", len <= 16 ? name : "(a name of more than 16 bytes)");
  ArrayHolder h(new_fixed(ctx, DFGPU_FLOAT64, n));
  if (dates->validity) { h.get()->validity = dates->validity; h.get()->null_count = dates->null_count; }       // shared, not copied
  if (n) {
    KernelTimer kt_(ctx, ts ? "k_ts_part" : "k_date_part");
    const int32_t* in = (const int32_t*)dates->values->ptr; double* out = (double*)h.get()->values->ptr;
    if (ts) {
      const int64_t* tin = (const int64_t*)dates->values->ptr;
      switch (dates->type) {
        case DFGPU_TIMESTAMP_SECOND: launch_ts_part_unit<0>(ctx, p, tin, n, out); break;
        case DFGPU_TIMESTAMP_MILLISECOND: launch_ts_part_unit<1>(ctx, p, tin, n, out); break;
        case DFGPU_TIMESTAMP_MICROSECOND: launch_ts_part_unit<2>(ctx, p, tin, n, out); break;
        default: launch_ts_part_unit<3>(ctx, p, tin, n, out); break;
      }
    } else switch (p) {
#define DP_CASE(P) case P: launch_date_part<P>(ctx, in, n, out); break;
      DP_CASE(DP_YEAR) DP_CASE(DP_QUARTER) DP_CASE(DP_MONTH) DP_CASE(DP_WEEK) DP_CASE(DP_DAY) DP_CASE(DP_DOY) DP_CASE(DP_DOW) DP_CASE(DP_HOUR) DP_CASE(DP_EPOCH)
#undef DP_CASE
    }
    KERNEL_CHECK();
  }
  return h.release();
}

// date_trunc(granularity, Timestamp) -> Timestamp of the same unit; `gran` is a scalar (the caller checked), `ts` a plain column or a scalar (a dictionary was
// decoded: errors belong to rows)
static dfgpu_array* date_trunc(dfgpu_ctx* ctx, const dfgpu_array* gran, const dfgpu_array* ts) {
  const int64_t n = ts->length;
  bool gran_valid = false; char name[17];
  const int64_t len = probe_name(ctx, gran, &gran_valid, name);
  if (!gran_valid) fail(DFGPU_EXECUTION, "Granularity of `date_trunc` must be non-null scalar Utf8");
  if (len < 0) fail(DFGPU_INVALID_ARGUMENT, "date_trunc: the granularity's offsets decrease");
  const int g = len <= 16 ? date_trunc_code(name, (size_t)len) : -1;
  if (g < 0) fail(DFGPU_EXECUTION, "Unsupported date_trunc granularity: %s", len <= 16 ? name : "(a name of more than 16 bytes)");
  ArrayHolder h(new_fixed(ctx, ts->type, n));
  if (ts->validity) { h.get()->validity = ts->validity; h.get()->null_count = ts->null_count; }       // shared, not copied
  if (n) {
    KernelTimer kt_(ctx, "k_ts_trunc");
    const TsTruncArgs A{(const int64_t*)ts->values->ptr, (int64_t*)h.get()->values->ptr, words_of(ts->validity), row_selection_words(ctx, n), ctx->d_flags, (int64_t*)(ctx->d_scratch64 + TS_BAD_SLOT)};
    switch (ts->type) {
      case DFGPU_TIMESTAMP_SECOND: launch_ts_trunc_unit<0>(ctx, g, A, n); break;
      case DFGPU_TIMESTAMP_MILLISECOND: launch_ts_trunc_unit<1>(ctx, g, A, n); break;
      case DFGPU_TIMESTAMP_MICROSECOND: launch_ts_trunc_unit<2>(ctx, g, A, n); break;
      default: launch_ts_trunc_unit<3>(ctx, g, A, n); break;
    }
    KERNEL_CHECK();
    check_flags(ctx, "date_trunc");
  }
  return h.release();
}

static dfgpu_array* empty_result(dfgpu_ctx* ctx, int32_t type) {
  if (type != DFGPU_UTF8) return new_fixed(ctx, type, 0);
  ArrayHolder h(new_array(ctx, DFGPU_UTF8, 0));
  h.get()->offsets = alloc_buffer(ctx, 4, true); h.get()->values = alloc_buffer(ctx, 0); h.get()->null_count = 0;
  return h.release();
}

// strings in, strings / Int32 / Boolean out; no dictionary argument
static dfgpu_array* string_function(dfgpu_ctx* ctx, int32_t fn, const dfgpu_array* const* args, const int32_t* scalar, int32_t nargs, int64_t n) {
  int64_t nulls = 0;
  BufferPtr valid = result_validity(ctx, args, scalar, nargs, n, &nulls);
  const dfgpu_array* s = args[0];
  const StrCol sc = str_col(s, scalar[0]);
  // rows of the first argument that average STR_WAVE_ROW_BYTES (option string_wave_row_bytes) or more get a wave each (values_bytes bounds a view's bytes from above)
  bool wave = !scalar[0] && s->values_bytes / n >= ctx->string_wave_row_bytes;
  if (fn == DFGPU_FN_STARTS_WITH) {
    ArrayHolder h(new_fixed(ctx, DFGPU_BOOL, n));
    if (valid) { h.get()->validity = valid; h.get()->null_count = nulls; }
    KernelTimer kt_(ctx, "k_starts_with");
    hipLaunchKernelGGL(k_starts_with, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, ctx->stream, sc, str_col(args[1], scalar[1]), words_of(valid), n, (uint64_t*)h.get()->values->ptr);
    KERNEL_CHECK(); return h.release();
  }
  if (fn == DFGPU_FN_CHARACTER_LENGTH) {
    ArrayHolder h(new_fixed(ctx, DFGPU_INT32, n));
    if (valid) { h.get()->validity = valid; h.get()->null_count = nulls; }
    KernelTimer kt_(ctx, "k_char_length");
    if (wave) hipLaunchKernelGGL((k_char_length<WaveOps, BLOCK / WAVE>), dim3(grid_for(n, BLOCK / WAVE)), dim3(BLOCK), 0, ctx->stream, sc, words_of(valid), n, (int32_t*)h.get()->values->ptr);
    else hipLaunchKernelGGL((k_char_length<LaneOps, BLOCK>), dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, ctx->stream, sc, words_of(valid), n, (int32_t*)h.get()->values->ptr);
    KERNEL_CHECK(); return h.release();
  }
  // SUBSTR / LEFT / RIGHT
  RangeArgs A{}; A.fn = fn; A.nargs = nargs; A.s = sc; A.a = int_col(args[1], scalar[1]); A.b = nargs == 3 ? int_col(args[2], scalar[2]) : IntCol{nullptr, 0};
  A.valid = words_of(valid); A.selected = row_selection_words(ctx, n);
  int64_t x = 0, c = 0;
  const bool x_known = host_scalar_i64(args[1], &x) && scalar[1], c_known = nargs == 3 && scalar[2] && host_scalar_i64(args[2], &c);
  const bool can_raise = fn == DFGPU_FN_SUBSTR && nargs == 3 && !(c_known && c >= 0);
  // a short row prefix (left(s, n > 0), substr(s, start <= 1, count) with literal arguments) reads the head of each row only: a lane does that as well as a wave
  int64_t prefix = -1;
  if (fn == DFGPU_FN_LEFT && x_known && x > 0) prefix = x;
  if (fn == DFGPU_FN_SUBSTR && nargs == 3 && x_known && x <= 1 && c_known && c >= 0) prefix = c;
  // p code points span at most 4 p bytes: the lane walks no further than in a row of 4 p bytes, which the threshold gives to the lane kernel (left(s, 3) and
  // left(s, 31) over rows of 32 .. 1024 bytes: the lane kernel is 2.3 to 11 times faster throughout, profiles/scalar_fn_microbench.json)
  if (prefix >= 0 && prefix * 4 < ctx->string_wave_row_bytes) wave = false;
  BufferPtr lens = alloc_buffer(ctx, (size_t)n * 4), begins = alloc_buffer(ctx, (size_t)n * 4), off64 = alloc_buffer(ctx, (size_t)(n + 1) * 8);
  { KernelTimer kt_(ctx, "k_str_range");
    if (wave) hipLaunchKernelGGL((k_str_range<WaveOps, BLOCK / WAVE>), dim3(grid_for(n, BLOCK / WAVE)), dim3(BLOCK), 0, ctx->stream, A, n, (uint32_t*)lens->ptr, (uint32_t*)begins->ptr, ctx->d_flags);
    else hipLaunchKernelGGL((k_str_range<LaneOps, BLOCK>), dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, ctx->stream, A, n, (uint32_t*)lens->ptr, (uint32_t*)begins->ptr, ctx->d_flags);
    KERNEL_CHECK(); }
  exclusive_scan_u32(ctx, (const uint32_t*)lens->ptr, (uint64_t*)off64->ptr, n, ctx->d_scratch64 + 61);
  const uint64_t total = read_scratch(ctx, 61);
  if (can_raise) check_flags(ctx, "substr");
  if (total > 0x7FFFFFFFull) fail(DFGPU_EXECUTION, "Arrow error: offset overflow: Utf8 output of %llu bytes exceeds i32 offsets", (unsigned long long)total);
  ArrayHolder h(new_array(ctx, DFGPU_UTF8, n)); dfgpu_array* o = h.get();
  o->values = alloc_buffer(ctx, (size_t)total); o->values_bytes = (int64_t)total; o->offsets = alloc_buffer(ctx, (size_t)(n + 1) * 4);
  if (valid) { o->validity = valid; o->null_count = nulls; } else o->null_count = 0;
  { KernelTimer kt_(ctx, "k_str_copy");
    hipLaunchKernelGGL(k_str_copy, dim3(grid_for(n + 1, BLOCK)), dim3(BLOCK), 0, ctx->stream, sc.values, (const uint32_t*)begins->ptr, (const uint64_t*)off64->ptr, n, (int32_t*)o->offsets->ptr,
                       (uint8_t*)o->values->ptr, total);
    KERNEL_CHECK(); }
  return h.release();
}

// args[dk] is a dictionary column and the only argument that is not a scalar: `dres` holds the result per dictionary entry
static dfgpu_array* through_codes(dfgpu_ctx* ctx, const dfgpu_array* dcol, dfgpu_array* dres_owned) {
  ArrayHolder dres(dres_owned);
  const int64_t n = dcol->length;
  if (dres.get()->type == DFGPU_UTF8) {          // a dictionary over the same codes; entries may repeat
    ArrayHolder h(new_array(ctx, DFGPU_DICTIONARY, n));
    dfgpu_array* o = h.get();
    o->key_type = dcol->key_type; o->values = dcol->values; o->validity = dcol->validity; o->null_count = dcol->validity ? dcol->null_count : 0;
    o->dictionary = dres.release();
    return h.release();
  }
  if (dres.get()->type == DFGPU_BOOL) return dict_predicate_map(ctx, dcol, dres.get());
  const bool nv = dcol->validity || dres.get()->validity;
  ArrayHolder h(new_fixed(ctx, dres.get()->type, n, 0, 0, nv));
  if (n) {
    KernelTimer kt_(ctx, "k_dict_gather");
    uint64_t* ov = nv ? (uint64_t*)h.get()->validity->ptr : nullptr;
    if (type_width(dres.get()->type) == 8)
      hipLaunchKernelGGL((k_dict_gather<uint64_t>), dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, ctx->stream, dcol->values->ptr, dcol->key_type, words_of(dcol->validity), n,
                         (const uint64_t*)dres.get()->values->ptr, words_of(dres.get()->validity), dres.get()->length, (uint64_t*)h.get()->values->ptr, ov);
    else
      hipLaunchKernelGGL((k_dict_gather<uint32_t>), dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, ctx->stream, dcol->values->ptr, dcol->key_type, words_of(dcol->validity), n,
                         (const uint32_t*)dres.get()->values->ptr, words_of(dres.get()->validity), dres.get()->length, (uint32_t*)h.get()->values->ptr, ov);
    KERNEL_CHECK();
  }
  if (nv) h.get()->null_count = -1;
  return h.release();
}

}  // namespace dfgpu

using namespace dfgpu;
extern "C" {

dfgpu_status dfgpu_scalar_function(dfgpu_ctx* ctx, int32_t fn, const dfgpu_array* const* args, const int32_t* arg_is_scalar, int32_t nargs, dfgpu_array** out) {
  return guard(ctx, [&] {
    if (!args || !arg_is_scalar || !out) fail(DFGPU_INVALID_ARGUMENT, "scalar_function: null argument");
    if (nargs < 1 || nargs > 3) fail(DFGPU_NOT_IMPLEMENTED, "scalar_function: function %d with %d arguments is not implemented on the device", fn, nargs);
    for (int32_t k = 0; k < nargs; k++) if (!args[k]) fail(DFGPU_INVALID_ARGUMENT, "scalar_function: null argument");
    // the table of include/dfgpu.h: argument counts and logical types
    static const int32_t I = DFGPU_INT64, U = DFGPU_UTF8, D = DFGPU_DATE32, T = -1;      // T: a Timestamp of any unit; D of DATE_PART takes one too
    int32_t want[3] = {0, 0, 0}, result = 0; bool ok = false;
    switch (fn) {
      case DFGPU_FN_DATE_PART: ok = nargs == 2; want[0] = U; want[1] = D; result = DFGPU_FLOAT64; break;
      case DFGPU_FN_CHARACTER_LENGTH: ok = nargs == 1; want[0] = U; result = DFGPU_INT32; break;
      case DFGPU_FN_SUBSTR: ok = nargs == 2 || nargs == 3; want[0] = U; want[1] = I; want[2] = I; result = U; break;
      case DFGPU_FN_LEFT: case DFGPU_FN_RIGHT: ok = nargs == 2; want[0] = U; want[1] = I; result = U; break;
      case DFGPU_FN_STARTS_WITH: ok = nargs == 2; want[0] = U; want[1] = U; result = DFGPU_BOOL; break;
      case DFGPU_FN_DATE_TRUNC: ok = nargs == 2; want[0] = U; want[1] = T; break;          // result: the type of argument 1
      default: fail(DFGPU_NOT_IMPLEMENTED, "scalar_function: function %d is not implemented on the device", fn);
    }
    if (!ok) fail(DFGPU_NOT_IMPLEMENTED, "scalar_function: function %d with %d arguments is not implemented on the device", fn, nargs);
    int64_t n = -1; int dk = -1; bool decode_only = false;
    for (int32_t k = 0; k < nargs; k++) {
      const dfgpu_array* a = args[k];
      if (a->type == DFGPU_DICTIONARY && !a->dictionary) fail(DFGPU_INVALID_ARGUMENT, "scalar_function: dictionary argument without a dictionary");
      const bool ts_arg = is_timestamp(logical_type(a)) && (want[k] == T || (want[k] == D && fn == DFGPU_FN_DATE_PART));
      if (want[k] == T && ts_arg) result = logical_type(a);
      if (logical_type(a) != want[k] && !ts_arg) fail(DFGPU_NOT_IMPLEMENTED, "scalar_function: function %d takes type %d as argument %d, not %d; the planner coerces first", fn, want[k], k, logical_type(a));
      if (arg_is_scalar[k]) { if (a->length != 1) fail(DFGPU_INVALID_ARGUMENT, "scalar_function: a scalar argument must have length 1, not %lld", (long long)a->length); }
      else if (n < 0) n = a->length;
      else if (n != a->length) fail(DFGPU_INVALID_ARGUMENT, "scalar_function: argument lengths differ (%lld vs %lld)", (long long)n, (long long)a->length);
      if (a->type == DFGPU_DICTIONARY) { if (dk >= 0 || arg_is_scalar[k]) decode_only = true; if (dk < 0) dk = k; }        // several dictionaries, or a dictionary scalar: decoded one by one
    }
    if (n < 0) n = 1;                          // every argument is a scalar
    if (fn == DFGPU_FN_DATE_PART && !arg_is_scalar[0]) fail(DFGPU_NOT_IMPLEMENTED, "date_part: the part name must be a scalar");
    if (fn == DFGPU_FN_DATE_TRUNC && (!arg_is_scalar[0] || args[0]->type == DFGPU_DICTIONARY)) fail(DFGPU_EXECUTION, "Granularity of `date_trunc` must be non-null scalar Utf8");
    if (dk >= 0) {
      // Once per dictionary entry and then through the codes, when that is less work (a dictionary smaller than the column, as dfgpu_like decides) and the
      // only column; a substr that can raise stays with the rows, because its errors belong to rows inside the row selection, not to dictionary entries.
      bool per_entry = !decode_only && args[dk]->dictionary->length < n;
      for (int32_t k = 0; k < nargs; k++) if (k != dk && !arg_is_scalar[k]) per_entry = false;
      int64_t c = 0;
      if (fn == DFGPU_FN_SUBSTR && nargs == 3 && !host_scalar_null(args[2]) && !(host_scalar_i64(args[2], &c) && c >= 0)) per_entry = false;
      if (fn == DFGPU_FN_DATE_TRUNC) per_entry = false;          // a row outside the nanosecond window raises: rows, not entries
      if (!per_entry) {                        // decode, then row by row
        ArrayHolder decoded(decode_dictionary(ctx, args[dk]));
        const dfgpu_array* plain[3] = {nullptr, nullptr, nullptr};
        for (int32_t k = 0; k < nargs; k++) plain[k] = k == dk ? decoded.get() : args[k];
        dfgpu_status st = dfgpu_scalar_function(ctx, fn, plain, arg_is_scalar, nargs, out);
        if (st != DFGPU_OK) fail(st, "%s", ctx->err.c_str());
        return;
      }
      const dfgpu_array* inner[3] = {nullptr, nullptr, nullptr}; int32_t sc[3] = {0, 0, 0};
      for (int32_t k = 0; k < nargs; k++) { inner[k] = k == dk ? args[k]->dictionary : args[k]; sc[k] = k == dk ? 0 : 1; }
      dfgpu_array* dres = nullptr;
      dfgpu_status st = dfgpu_scalar_function(ctx, fn, inner, sc, nargs, &dres);
      if (st != DFGPU_OK) fail(st, "%s", ctx->err.c_str());
      *out = through_codes(ctx, args[dk], dres); return;
    }
    if (n == 0) { *out = empty_result(ctx, result); return; }
    if (fn == DFGPU_FN_DATE_PART) { *out = date_part(ctx, args[0], args[1]); return; }
    if (fn == DFGPU_FN_DATE_TRUNC) { *out = date_trunc(ctx, args[0], args[1]); return; }
    *out = string_function(ctx, fn, args, arg_is_scalar, nargs, n);
  });
}

}  // extern "C"
