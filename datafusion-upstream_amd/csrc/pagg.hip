// pagg.hip -- partitioned pre-aggregation for high-cardinality, unclustered group keys: every partition's groups live in LDS.
//
// Reference semantics: the Partial stage of a two-phase aggregation (AggregateMode::Partial, physical-plan/src/aggregates/mod.rs:64-100;
// GroupedHashAggregateStream::group_aggregate_batch, row_hash.rs:524-613) applied to ONE batch inside the operator: the batch is reduced
// to (group key, partial state...) rows, which the caller interns (GroupValues::intern, group_values/primitive.rs:112-149) and merges
// (GroupsAccumulator::merge_batch, prim_op.rs:119-127; average.rs:472-509; count.rs:135-170) exactly as a Final stage would.
//
// Why: with more groups than an LDS cache holds, dfgpu_acc_update_batch pays one memory-side atomic per row and state array
// (~24 G/s: 8.5 ms per 100 M rows for SUM + COUNT) and groups.hip one random 64-byte sector per row for the key table.  Here the rows
// are split by key hash (radix_partition.h, one pass) into P partitions so that a partition's distinct keys fit an LDS table
// (4096 slots of key + first row + row count + one 8-byte state per aggregate); one workgroup per partition accumulates its rows with
// LDS atomics and writes one row per group.  If a partition holds more keys than the table (the cardinality estimate was low, or
// the keys are skewed towards it) the workgroup flushes the table and goes on: a key may then leave in several partial rows, which
// the merge downstream adds up -- never wrong, only less reduction.
//
// Order: partial rows come back sorted by the first input row of their group, so interning them numbers the groups in first-seen order
// of the ORIGINAL batch (group_values/primitive.rs:137-141).  Integer / count states are exact; Float64 sums are added in a different
// order than row order (as every multi-partition plan of the reference does): within 1e-9 relative of the sequential sum.
#include "device_utils.h"
#include "radix_partition.h"

namespace dfgpu {

constexpr uint64_t PA_EMPTY = ~0ull;
constexpr int PA_NT = 1024;
constexpr int PA_MAX_AGGS = 6;
enum { PA_SUM_I64 = 0, PA_SUM_F64 = 1, PA_MIN_I64 = 2, PA_MAX_I64 = 3, PA_MIN_U64 = 4, PA_MAX_U64 = 5, PA_MIN_F64 = 6, PA_MAX_F64 = 7, PA_NONE = 8,
       PA_SUM_I128_LO = 9, PA_SUM_I128_HI = 10, PA_SUM_I128_SX = 11,
       PA_COUNT_FLAG = 12 };      // COUNT_FLAG: the cell counts the rows whose flag bit is set (the non-NULL values of a nullable argument): a wrapping Int64 sum of the bit      // SX: the high word is the sign extension of the low one (Decimal128 of precision <= 18 moves 8 bytes per row through the partition)      // Decimal128 SUM / AVG: two neighbouring cells, the low add's returned value gives the carry (exact mod 2^128, as acc.hip does in HBM)

// Nullable arguments: the validity bits of the (at most 8) nullable value columns travel through the partition as ONE byte per row (vflag; bit b = value column b is valid in
// that row).  flag_bit[a] >= 0: cell a takes its row's value only where that bit is set (a NULL adds the operation's identity, i.e. nothing); a COUNT_FLAG cell sums the bit.
struct PaPlan { int32_t n_acc; int32_t op[PA_MAX_AGGS]; const uint64_t* val[PA_MAX_AGGS]; int32_t vstride[PA_MAX_AGGS]; uint64_t* out[PA_MAX_AGGS]; int32_t has_i128; const uint8_t* vflag; int32_t flag_bit[PA_MAX_AGGS]; };      // val[a][i * vstride[a]]: a Decimal128 column is two cells of stride 2

__device__ inline uint64_t pa_identity(int op) {
  switch (op) {
    case PA_MIN_I64: return (uint64_t)INT64_MAX; case PA_MAX_I64: return (uint64_t)INT64_MIN; case PA_MIN_U64: return ~0ull; case PA_MAX_U64: return 0ull;
    case PA_MIN_F64: return 0x7FEFFFFFFFFFFFFFull /* f64::MAX */; case PA_MAX_F64: return 0xFFEFFFFFFFFFFFFFull /* f64::MIN */;      // the reference's starting values (min_max.rs:102-139): `cur < new` never lets +-inf beyond them or a NaN in
    default: return 0ull;
  }
}
__device__ inline void pa_apply(int op, unsigned long long* cell, uint64_t v) {
  switch (op) {
    case PA_SUM_I64: case PA_COUNT_FLAG: atomicAdd(cell, (unsigned long long)v); break;                                   // wrapping, sum.rs:137
    case PA_SUM_F64: atomicAdd((double*)cell, __longlong_as_double((long long)v)); break;
    // MIN / MAX: a cell only ever moves one way, so a value that does not improve on a plain (possibly stale) read of it cannot improve on the cell: no atomic.  After a
    // group's first few rows that is nearly every row (the expected number of new maxima among n values is ln n), and on a hot slot it takes the read-modify-write queue away
    case PA_MIN_I64: if ((long long)v < *(volatile long long*)cell) atomicMin((long long*)cell, (long long)v); break;
    case PA_MAX_I64: if ((long long)v > *(volatile long long*)cell) atomicMax((long long*)cell, (long long)v); break;
    case PA_MIN_U64: if (v < *(volatile unsigned long long*)cell) atomicMin(cell, (unsigned long long)v); break;
    case PA_MAX_U64: if (v > *(volatile unsigned long long*)cell) atomicMax(cell, (unsigned long long)v); break;
    case PA_MIN_F64: { double d = __longlong_as_double((long long)v); if (d == d && d < *(volatile double*)cell) atomicMin((double*)cell, d); break; }     // `if *cur > new` (min_max.rs:124-139) is false for a NaN: NaN inputs never enter, whatever the order
    case PA_MAX_F64: { double d = __longlong_as_double((long long)v); if (d == d && d > *(volatile double*)cell) atomicMax((double*)cell, d); break; }
    default: break;
  }
}
__device__ inline uint64_t pa_combine(int op, uint64_t a, uint64_t b) {          // what pa_apply's atomic does, on two values
  switch (op) {
    case PA_SUM_I64: case PA_COUNT_FLAG: return a + b;
    case PA_SUM_F64: return (uint64_t)__double_as_longlong(__longlong_as_double((long long)a) + __longlong_as_double((long long)b));
    case PA_MIN_I64: return (long long)a < (long long)b ? a : b; case PA_MAX_I64: return (long long)a > (long long)b ? a : b;
    case PA_MIN_U64: return a < b ? a : b; case PA_MAX_U64: return a > b ? a : b;
    case PA_MIN_F64: { const double x = __longlong_as_double((long long)a), y = __longlong_as_double((long long)b); return y == y && (x != x || y < x) ? b : a; }      // a NaN never wins
    case PA_MAX_F64: { const double x = __longlong_as_double((long long)a), y = __longlong_as_double((long long)b); return y == y && (x != x || y > x) ? b : a; }
    default: return a;
  }
}
__device__ inline uint32_t pa_slot(uint64_t k, int cbits) {
  uint32_t lo = (uint32_t)k, hi = (uint32_t)(k >> 32);
  uint32_t a = lo ^ (hi * 0x9E3779B1u), x = a * 0x85EBCA6Bu; x ^= x >> 13;
  return (x * 0xC2B2AE35u) >> (32 - cbits);
}

__global__ void k_pa_max_len(const uint32_t* pstart, uint32_t P, unsigned long long* out) {
  uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; uint32_t len = p < P ? pstart[p + 1] - pstart[p] : 0;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) { uint32_t o = __shfl_xor(len, d, 64); len = o > len ? o : len; }
  if (lane_id() == 0 && len) atomicMax(out, (unsigned long long)len);
}
// one workgroup per partition (and slice).  LDS: keys u64[C + 1] | acc[n_acc] u64[C + 1] | first u32[C + 1] | cnt u32[C + 1]; slot C belongs to the key
// that equals the EMPTY marker.  Rows are taken PA_NT at a time with a barrier in between; before a chunk the table is flushed if the
// chunk could fill it beyond 7/8.
// (partition, slice) work items of the skewed case: item_start[p] = first item of partition p, item_start[P] = number of items.  A 2-D grid over
// (partition, max slices) would be mostly empty workgroups, and an empty workgroup still queues for a CU's LDS behind the ones doing work: the slices of the one
// long partition then start milliseconds late.
__global__ void __launch_bounds__(PA_NT) k_pa_items(const uint32_t* pstart, uint32_t P, uint32_t slice, uint32_t* item_start) {
  __shared__ uint32_t wsum[PA_NT / WAVE]; __shared__ uint32_t carry_sh;
  if (threadIdx.x == 0) carry_sh = 0;
  __syncthreads();
  for (uint32_t p0 = 0; p0 < P; p0 += PA_NT) {
    const uint32_t p = p0 + threadIdx.x; uint32_t c = 0;
    if (p < P) { const uint32_t len = pstart[p + 1] - pstart[p]; c = (uint32_t)(((uint64_t)len + slice - 1) / slice); }
    const uint32_t inc = wave_inclusive_sum(c);
    if (lane_id() == 63) wsum[threadIdx.x >> 6] = inc;
    __syncthreads();
    uint32_t run = carry_sh + inc - c, tot = 0;
    for (int w = 0; w < PA_NT / WAVE; w++) { if (w < (int)(threadIdx.x >> 6)) run += wsum[w]; tot += wsum[w]; }
    if (p < P) item_start[p] = run;
    __syncthreads();
    if (threadIdx.x == 0) carry_sh += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) item_start[P] = carry_sh;
}
// two-level partition: fine partition = (low hash bits -> P2) * P1 + (high hash bits -> P1)
__device__ inline uint32_t pa_fine_pid(uint64_t k, uint32_t P1, uint32_t P2) { uint64_t h = mix64(k); return (uint32_t)(((h & 0xFFFFFFFFull) * (uint64_t)P2) >> 32) * P1 + rp_pid(h, P1); }
template <bool I128, bool FLAGS>          // I128: the plan holds Decimal128 cell pairs / strided value columns; FLAGS: some argument is nullable (flag byte per row).  The plain instantiation is the round-2 kernel (the I128 branches cost it 6 %, the flag tests 15 %)
__global__ void __launch_bounds__(PA_NT) k_pa_aggregate(const uint64_t* pkey, const uint32_t* prow, PaPlan plan_arg, const uint32_t* pstart, const uint32_t* item_start, uint32_t P, int cbits, uint32_t slice,
                                                      uint64_t* orec /* records of `rs` words: key, count, accumulator cells */, int rs, uint32_t* ofirst, unsigned long long* cursor /*[0] rows written, [2] tables flushed before their partition ended*/,
                                                      uint32_t P1, uint32_t P2, uint32_t* misplaced /* two-level partition (P1 != 0): set when a row sits in a partition its key does not hash to */) {
  extern __shared__ unsigned long long pa_lds[];
  const uint32_t C = 1u << cbits, M = C - 1, C1 = C + 1;
  unsigned long long* keys = pa_lds; unsigned long long* acc = pa_lds + C1;
  uint32_t* first = (uint32_t*)(pa_lds + (size_t)C1 * (1 + plan_arg.n_acc)); uint32_t* cnt = first + C1;
  __shared__ uint32_t nfilled, wsum[PA_NT / WAVE], out_base; __shared__ PaPlan splan;
  if (threadIdx.x == 0) splan = plan_arg;              // the per-aggregate loops index the plan at run time: from LDS, not from the by-value argument
  __syncthreads();
  const PaPlan& plan = splan;
  // a partition far above the average size (skewed keys) is cut into slices of `slice` rows, each with a table of its own: workgroup = one item of item_start
  uint32_t p = blockIdx.x, sl = 0; const int lane = lane_id();
  if (item_start) {
    if (blockIdx.x >= item_start[P]) return;
    uint32_t lo = 0, hi = P - 1;
    while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (item_start[mid] <= blockIdx.x) lo = mid; else hi = mid - 1; }
    p = lo; sl = blockIdx.x - item_start[p];
  }
  const uint32_t p0 = pstart[p], p1 = pstart[p + 1];
  if ((uint64_t)sl * slice >= (uint64_t)(p1 - p0)) return;
  const uint32_t q0 = p0 + sl * slice, q1 = (uint64_t)q0 + slice < (uint64_t)p1 ? q0 + slice : p1;
  auto reset = [&]() {
    for (uint32_t s = threadIdx.x; s < C1; s += PA_NT) { keys[s] = PA_EMPTY; first[s] = 0xFFFFFFFFu; cnt[s] = 0;
      for (int a = 0; a < plan.n_acc; a++) acc[(size_t)a * C1 + s] = pa_identity(plan.op[a]); }
    if (threadIdx.x == 0) nfilled = 0;
  };
  auto flush = [&]() {      // occupied slots -> one output row each; slot ranks by a block scan over PER consecutive slots per thread
    const uint32_t per = (C1 + PA_NT - 1) / PA_NT, s0 = threadIdx.x * per; uint32_t c = 0;
    for (uint32_t j = 0; j < per; j++) { uint32_t s = s0 + j; if (s < C1 && cnt[s]) c++; }
    uint32_t inc = wave_inclusive_sum(c);
    if (lane == 63) wsum[threadIdx.x >> 6] = inc;
    __syncthreads();
    uint32_t run = inc - c, tot = 0;
    for (int w = 0; w < PA_NT / WAVE; w++) { if (w < (int)(threadIdx.x >> 6)) run += wsum[w]; tot += wsum[w]; }
    if (threadIdx.x == 0) out_base = tot ? (uint32_t)atomicAdd(cursor, (unsigned long long)tot) : 0u;
    __syncthreads();
    uint32_t o = out_base + run;
    for (uint32_t j = 0; j < per; j++) { uint32_t s = s0 + j; if (s < C1 && cnt[s]) {
      uint64_t* rec = orec + (size_t)o * (size_t)rs; rec[0] = s == C ? PA_EMPTY : keys[s]; rec[1] = cnt[s]; ofirst[o] = first[s];
      for (int a = 0; a < plan.n_acc; a++) rec[2 + a] = acc[(size_t)a * C1 + s];
      o++; } }
    __syncthreads();
  };
  reset();
  __syncthreads();
  // the next chunk's row (key, row number, value cells) is loaded while the current one goes through the table
  uint64_t kn = 0, vn[PA_MAX_AGGS]; uint32_t rn = 0;
  const int na = plan_arg.n_acc;
  const uint8_t* vflag = plan_arg.vflag;
  // a row's cells as the table takes them: the value, or -- for a cell bound to a flag bit -- the operation's identity where the bit is clear (a NULL argument), the bit itself for a COUNT_FLAG cell
  auto load_cells = [&](uint32_t ic, uint64_t* v) {
#pragma unroll
    for (int a = 0; a < PA_MAX_AGGS; a++) v[a] = a < na && (!FLAGS || plan_arg.val[a]) ? plan_arg.val[a][I128 ? (size_t)ic * plan_arg.vstride[a] : (size_t)ic] : 0;
    if constexpr (FLAGS) {
      const uint32_t f = vflag[ic];
#pragma unroll
      for (int a = 0; a < PA_MAX_AGGS; a++) if (a < na && plan_arg.flag_bit[a] >= 0) {
        const bool set = (f >> plan_arg.flag_bit[a]) & 1u; const int op = plan_arg.op[a];
        v[a] = op == PA_COUNT_FLAG ? (uint64_t)set : set ? v[a] : (op == PA_SUM_I128_LO || op == PA_SUM_I128_HI || op == PA_SUM_I128_SX) ? 0ull : pa_identity(op);
      }
    }
  };
  { const uint32_t i = q0 + threadIdx.x, ic = i < q1 ? i : q1 - 1; kn = pkey[ic]; rn = prow ? prow[ic] : 0u; load_cells(ic, vn); }
  for (uint32_t i0 = q0; i0 < q1; i0 += PA_NT) {
    if (nfilled + PA_NT > C - C / 8) { __syncthreads(); flush(); reset(); if (threadIdx.x == 0) atomicAdd(cursor + 2, 1ull); __syncthreads(); }      // nfilled is only written between barriers: uniform
    const uint32_t i = i0 + threadIdx.x; const bool on = i < q1;
    const uint64_t k = kn; const uint32_t row = rn; uint64_t v[PA_MAX_AGGS];
    if (P1 && on && (i & 3u) == 0 && pa_fine_pid(k, P1, P2) != p) *misplaced = 1u;     // the partition bounds came from a binary search that relies on the order the two passes leave: every 4th row re-hashed as an assertion
#pragma unroll
    for (int a = 0; a < PA_MAX_AGGS; a++) v[a] = vn[a];
    { const uint32_t i2 = i + PA_NT, ic = i2 < q1 ? i2 : q1 - 1; kn = pkey[ic]; rn = prow ? prow[ic] : 0u; load_cells(ic, vn); }
    // Skewed keys: when at least 16 lanes of a wave carry the key of its first active lane, those lanes are combined in registers (shuffles) and the leader
    // alone touches the table: one LDS atomic per state instead of one per row on a slot every wave of the workgroup is hammering.  (Trying the last combined key
    // first -- a key with a fifth to a half of its partition's rows sits in the first lane only that often -- was measured on the Zipf ClickBench shape and changed
    // nothing: 2.34 -> 2.49 ms, round 4 call r; the partitions there hold several warm keys each, not one.  Keeping the hot key's rows in accumulators of the lanes' own
    // and combining them once, when another key takes over or the slice ends, was tried as well (call aa): Zipf 2.36 -> 2.16 ms, but every other shape lost 10-30 % to the
    // longer loop body -- uniform ClickBench 1.07 -> 1.27 ms, 20 M groups 1.64 -> 1.75, three keys + Decimal128 1.04 -> 1.35 -- and it was taken out again.  Nor did trying up to three candidate keys per round with DPP reductions in place of the shuffles (call ai): Zipf 2.36 -> 3.04 ms at the same threshold
    // of 16 lanes, 3.5 / 3.8 ms at 8 / 4; uniform 1.07 -> 1.2 ms.)
    uint32_t cntv = 1; uint32_t rowv = row; bool mine = on;
    {
      const uint64_t act = ballot64(on);
      const int lead = act ? __ffsll((long long)act) - 1 : 0;
      const uint32_t k0lo = (uint32_t)__shfl((int)(uint32_t)k, lead, 64), k0hi = (uint32_t)__shfl((int)(uint32_t)(k >> 32), lead, 64);
      const bool member = on && (uint32_t)k == k0lo && (uint32_t)(k >> 32) == k0hi;
      const uint64_t mem = ballot64(member);
      if (__popcll(mem) >= 16 && !I128) {
        uint32_t r = member ? row : 0xFFFFFFFFu;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) { uint32_t o = (uint32_t)__shfl_xor((int)r, d, 64); r = o < r ? o : r; }
#pragma unroll
        for (int a = 0; a < PA_MAX_AGGS; a++) if (a < na) {
          const int op = plan_arg.op[a]; uint64_t x = member ? v[a] : pa_identity(op);
#pragma unroll
          for (int d = 32; d > 0; d >>= 1) { uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), d, 64); x = pa_combine(op, x, ((uint64_t)hi << 32) | lo); }
          if (lane == lead) v[a] = x;
        }
        if (lane == lead) { cntv = (uint32_t)__popcll(mem); rowv = r; } else if (member) mine = false;
      }
    }
    uint32_t s = C; bool fresh = false;
    if (mine) {
      if (k != PA_EMPTY) {
        s = pa_slot(k, cbits);
        for (;;) {
          unsigned long long old = keys[s];
          if (old == PA_EMPTY) { old = atomicCAS(&keys[s], (unsigned long long)PA_EMPTY, (unsigned long long)k); if (old == PA_EMPTY) { fresh = true; break; } }
          if (old == k) break;
          s = (s + 1) & M;
        }
      }
      if (rowv < first[s]) atomicMin(&first[s], rowv);           // a stale read only costs a redundant atomic
      atomicAdd(&cnt[s], cntv);
#pragma unroll
      for (int a = 0; a < PA_MAX_AGGS; a++) if (a < na) {
        const int op = plan_arg.op[a];
        if (!I128) pa_apply(op, &acc[(size_t)a * C1 + s], v[a]);
        else if (op == PA_SUM_I128_LO && plan_arg.op[a + 1 < PA_MAX_AGGS ? a + 1 : a] == PA_SUM_I128_SX) {            // value = sign-extended 64 bits
          const int ah = a + 1 < PA_MAX_AGGS ? a + 1 : a;
          const unsigned long long lo = v[a], old = atomicAdd(&acc[(size_t)a * C1 + s], lo);
          const unsigned long long hi = (unsigned long long)((long long)lo >> 63) + (unsigned long long)(old + lo < old);
          if (hi) atomicAdd(&acc[(size_t)ah * C1 + s], hi);
        } else if (op == PA_SUM_I128_LO) {            // a + 1 is the high word's cell
          const int ah = a + 1 < PA_MAX_AGGS ? a + 1 : a;      // a LO cell is never the last one (the host lays pairs out); the clamp keeps the unrolled index in range
          const unsigned long long lo = v[a], old = atomicAdd(&acc[(size_t)a * C1 + s], lo);
          const unsigned long long hi = v[ah] + (unsigned long long)(old + lo < old);
          if (hi) atomicAdd(&acc[(size_t)ah * C1 + s], hi);
        } else if (op != PA_SUM_I128_HI && op != PA_SUM_I128_SX) pa_apply(op, &acc[(size_t)a * C1 + s], v[a]);
      }
    }
    uint64_t fb = ballot64(fresh);
    if (lane == 0 && fb) atomicAdd(&nfilled, (uint32_t)__popcll(fb));
    __syncthreads();
  }
  flush();
}

// sample of the batch: distinct keys among `s` evenly spaced rows (open-addressing u64 table of `cap` slots) and how many sampled
// rows are not smaller than their predecessor row (clustered input keeps the run-numbering path of groups.hip)
template <typename T>
__global__ void __launch_bounds__(BLOCK) k_pa_sample(const T* keys, const uint64_t* mask, int64_t n, int64_t s, int64_t stride, unsigned long long* table, uint64_t cap_mask, unsigned long long* out /*[0] distinct, [1] non-decreasing pairs, [2] pairs*/) {
  uint32_t nf = 0, nn = 0, np = 0;
  for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < s; j += (int64_t)gridDim.x * BLOCK) {
    int64_t i = j * stride;
    if (i >= n || (mask && !bit_get(mask, i))) continue;
    T kt = keys[i]; if (i > 0) { np++; nn += keys[i - 1] <= kt; }
    uint64_t k = (uint64_t)(int64_t)kt;
    uint64_t kk = k == PA_EMPTY ? 0x5555555555555555ull : k;                 // the marker value itself: folded onto another key (estimate only)
    uint64_t h = mix64(kk) & cap_mask;
    for (;;) {
      unsigned long long old = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // frequent keys: no atomic once they are in
      if (old == PA_EMPTY) { old = atomicCAS(&table[h], (unsigned long long)PA_EMPTY, (unsigned long long)kk); if (old == PA_EMPTY) { nf++; break; } }
      if (old == kk) break;
      h = (h + 1) & cap_mask;
    }
  }
  nf = wave_sum(nf); nn = wave_sum(nn); np = wave_sum(np);                    // one atomic per workgroup and counter: same-address atomics serialise
  __shared__ uint32_t sh[3][BLOCK / WAVE];
  if (lane_id() == 0) { sh[0][threadIdx.x >> 6] = nf; sh[1][threadIdx.x >> 6] = nn; sh[2][threadIdx.x >> 6] = np; }
  __syncthreads();
  if (threadIdx.x < 3) { uint32_t t = 0; for (int w = 0; w < BLOCK / WAVE; w++) t += sh[threadIdx.x][w]; if (t) atomicAdd(&out[threadIdx.x], (unsigned long long)t); }
}

// ---- two-level partition (more groups than 2048 partitions bring into LDS): pass 1 splits on the high hash bits into P1 partitions, pass 2 is a STABLE
// split of pass 1's output on the low hash bits into P2 <= 256 -- an LSD radix sort on two digits, so the rows end up ordered by (p2, p1): P1 * P2
// contiguous partitions.  Their boundaries are read off the partitioned keys.
struct RpHashU64Low {
  const uint64_t* keys;
  __device__ inline bool operator()(int64_t i, uint32_t P, uint32_t* pid, uint64_t* key) const { *key = keys[i]; *pid = (uint32_t)(((mix64(*key) & 0xFFFFFFFFull) * (uint64_t)P) >> 32); return true; }
};
// starts[f] = first row of fine partition f (starts[Pt] = m): after the two passes the rows are ordered by fine partition, so every bound is a binary search over
// the keys (27 probes for 100 M rows, ~9 000 partitions) instead of a pass over them; k_pa_aggregate verifies the order it relies on row by row
__global__ void __launch_bounds__(BLOCK) k_pa_bounds(const uint64_t* __restrict__ pkey, uint32_t m, uint32_t P1, uint32_t P2, uint32_t Pt, uint32_t* __restrict__ starts /*[Pt + 1]*/) {
  const uint32_t f = blockIdx.x * BLOCK + threadIdx.x; if (f > Pt) return;
  uint32_t lo = 0, hi = m;                                      // first row whose fine partition is >= f
  while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (pa_fine_pid(pkey[mid], P1, P2) < f) lo = mid + 1; else hi = mid; }
  starts[f] = f == Pt ? m : lo;
}

// first-seen order without a sort: every partial row's first input row is a distinct row number, so its rank among them is the number of marked rows in front of it --
// mark the rows in a bitmap over the input, prefix-count the words, read the rank back
__global__ void __launch_bounds__(BLOCK) k_pa_mark(const uint32_t* __restrict__ first, int64_t m, unsigned long long* bits) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; if (i < m) { const uint32_t f = first[i]; atomicOr(&bits[f >> 6], 1ull << (f & 63)); }
}
__global__ void __launch_bounds__(BLOCK) k_pa_popc(const uint64_t* __restrict__ bits, int64_t nw, uint32_t* __restrict__ pc) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; if (i < nw) pc[i] = (uint32_t)__popcll(bits[i]);
}
__global__ void __launch_bounds__(BLOCK) k_pa_rank_perm(const uint32_t* __restrict__ first, int64_t m, const uint64_t* __restrict__ bits, const uint32_t* __restrict__ pref, uint32_t* __restrict__ perm) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; if (i >= m) return;
  const uint32_t f = first[i]; const uint32_t r = pref[f >> 6] + (uint32_t)__popcll(bits[f >> 6] & ((1ull << (f & 63)) - 1ull));
  perm[r] = (uint32_t)i;
}

// Many partial rows (millions): the inverse map.  inv[first row of partial row j] = j is one random 4-byte store per partial row into an n-entry array; the permutation in
// first-seen order is then the non-empty entries of inv in array order -- two streaming passes (count, write) instead of four passes of a stable sort over (first row, j) words
// (20 M partial rows of 100 M input rows: 1.3 ms of sort passes).  First rows are distinct (a row belongs to one partial row), so the stores never collide.
constexpr int INV_PER = 16;             // consecutive entries per lane
__global__ void __launch_bounds__(BLOCK) k_pa_inv(const uint32_t* __restrict__ first, int64_t m, uint32_t* __restrict__ inv) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; if (i < m) inv[first[i]] = (uint32_t)i;
}
template <bool WRITE>
__global__ void __launch_bounds__(BLOCK) k_pa_inv_compact(const uint32_t* __restrict__ inv, int64_t n, uint32_t* __restrict__ counts, uint32_t* __restrict__ perm) {
  const int64_t base = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * INV_PER;
  uint32_t v[INV_PER]; uint32_t c = 0;
  if (base + INV_PER <= n) {
#pragma unroll
    for (int q = 0; q < INV_PER / 4; q++) { const uint4 x = ((const uint4*)(inv + base))[q]; v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w; }
  } else {
#pragma unroll
    for (int q = 0; q < INV_PER; q++) v[q] = base + q < n ? inv[base + q] : 0xFFFFFFFFu;
  }
#pragma unroll
  for (int q = 0; q < INV_PER; q++) c += v[q] != 0xFFFFFFFFu;
  __shared__ uint32_t lds[BLOCK / WAVE];
  uint32_t tot; uint32_t ex = block_exclusive_sum<uint32_t>(c, lds, &tot);
  if (!WRITE) { if (threadIdx.x == 0) counts[blockIdx.x] = tot; return; }
  uint32_t o = counts[blockIdx.x] + ex;
#pragma unroll
  for (int q = 0; q < INV_PER; q++) if (v[q] != 0xFFFFFFFFu) perm[o++] = v[q];
}
// many partial rows, general form: (first row << jb | partial row) words through LSD passes of the stable partition, 8 bytes moving per row and pass
__global__ void __launch_bounds__(BLOCK) k_pa_order_words(const uint32_t* __restrict__ first, int64_t m, int jb, uint64_t* __restrict__ words) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; if (i < m) words[i] = ((uint64_t)first[i] << jb) | (uint64_t)i;
}
__global__ void __launch_bounds__(BLOCK) k_pa_perm_of_words(const uint64_t* __restrict__ words, int64_t m, int jb, uint32_t* __restrict__ perm) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; if (i < m) perm[i] = (uint32_t)(words[i] & ((1ull << jb) - 1ull));
}
// every output column of the partial rows in one pass over the permutation: a row's record (key, count, cells) is one or two 32-byte reads
struct PaEmit { int32_t n; int32_t word[2 + 2 * PA_MAX_AGGS]; void* dst[2 + 2 * PA_MAX_AGGS]; int32_t narrow[2 + 2 * PA_MAX_AGGS]; int32_t dstride[2 + 2 * PA_MAX_AGGS], doff[2 + 2 * PA_MAX_AGGS]; };      // narrow: store the low 32 bits; dst[i * dstride + doff]
template <int RS>
__global__ void __launch_bounds__(BLOCK) k_pa_emit(PaEmit e, const uint64_t* __restrict__ recs, const uint32_t* __restrict__ perm, int64_t m) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; if (i >= m) return;
  const uint32_t j = perm ? perm[i] : (uint32_t)i; uint64_t v[RS];
  const ulonglong2* r = (const ulonglong2*)(recs + (size_t)j * RS);
#pragma unroll
  for (int q = 0; q < RS / 2; q++) { const ulonglong2 t = r[q]; v[2 * q] = t.x; v[2 * q + 1] = t.y; }
#pragma unroll
  for (int c = 0; c < 2 + 2 * PA_MAX_AGGS; c++) if (c < e.n) {
    uint64_t x = 0;
#pragma unroll
    for (int w = 0; w < RS; w++) if (e.word[c] == w) x = v[w];
    if (e.narrow[c]) ((uint32_t*)e.dst[c])[i] = (uint32_t)x; else ((uint64_t*)e.dst[c])[(size_t)i * e.dstride[c] + e.doff[c]] = x;
  }
}

// ---- 2..4 integer key columns -> one u64: key = sum over columns of (value - min + (nullable ? 1 : 0)) * stride; digit 0 of a nullable column = NULL (its own group,
// group_values/row.rs:94-146 treats NULL as a value).  The ranges multiply to < 2^62, so the packed key never equals PA_EMPTY.
struct PaPackCols { int32_t n; const void* v[4]; const uint64_t* valid[4]; int32_t type[4]; long long mn[4]; unsigned long long stride[4], range[4]; int32_t nullable[4]; };
// One row per thread and step.  Measured per 100 M rows x 3 key columns (both kernels together): this form 1.67 ms; four rows per thread, consecutive rows 1.92 ms,
// lane-contiguous rows 1.94 ms -- neither unrolled form helped, so the simple one stays (the per-element type switch of key_at is the suspect, not measured apart).
// step > 1: every step-th row only (the optimistic ranges of a large batch come from a sample; k_pa_pack then checks every row against them)
__global__ void __launch_bounds__(BLOCK) k_pa_cols_minmax(PaPackCols pc, const uint64_t* mask, int64_t n, int64_t step, long long* mm /*[2 * n] min, max*/) {
  long long lo[4] = { INT64_MAX, INT64_MAX, INT64_MAX, INT64_MAX }, hi[4] = { INT64_MIN, INT64_MIN, INT64_MIN, INT64_MIN };
  for (int64_t i = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * step; i < n; i += (int64_t)gridDim.x * BLOCK * step) {
    if (mask && !bit_get(mask, i)) continue;
#pragma unroll
    for (int c = 0; c < 4; c++) if (c < pc.n && valid_at(pc.valid[c], i)) { const long long x = key_at(pc.v[c], pc.type[c], i); lo[c] = x < lo[c] ? x : lo[c]; hi[c] = x > hi[c] ? x : hi[c]; }
  }
#pragma unroll
  for (int c = 0; c < 4; c++) if (c < pc.n) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const long long a = __shfl_xor(lo[c], d, 64), b = __shfl_xor(hi[c], d, 64); lo[c] = a < lo[c] ? a : lo[c]; hi[c] = b > hi[c] ? b : hi[c]; }
    if (lane_id() == 0 && lo[c] <= hi[c]) { atomicMin(&mm[2 * c], lo[c]); atomicMax(&mm[2 * c + 1], hi[c]); }       // one pair per wave
  }
}
// *outside (optional) is raised when a value lies outside [mn, mn + range): the ranges were an estimate and the caller packs again with exact ones
__global__ void __launch_bounds__(BLOCK) k_pa_pack(PaPackCols pc, int64_t n, uint64_t* out, unsigned long long* outside) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; if (i >= n) return;
  unsigned long long k = 0; bool bad = false;
#pragma unroll
  for (int c = 0; c < 4; c++) if (c < pc.n) {
    const bool ok = valid_at(pc.valid[c], i);
    const unsigned long long off = ok ? (unsigned long long)(key_at(pc.v[c], pc.type[c], i) - pc.mn[c]) : 0ull;         // wraps to a huge value below mn
    bad |= ok && off >= pc.range[c] - (unsigned long long)pc.nullable[c];
    k += (ok ? off + (unsigned long long)pc.nullable[c] : 0ull) * pc.stride[c];
  }
  out[i] = bad ? 0ull : k;
  if (outside && __ballot(bad) && lane_id() == 0) *outside = 1ull;
}
// packed keys of the partial rows -> column c of the group keys (values as 64-bit patterns narrowed by the caller's type width; validity word by word)
template <typename T>
__global__ void __launch_bounds__(BLOCK) k_pa_unpack(const uint64_t* packed, int64_t m, unsigned long long stride, unsigned long long range, long long mn, int nullable, T* out, uint64_t* valid) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; bool ok = true; 
  if (i < m) { const unsigned long long dgt = (packed[i] / stride) % range; ok = !nullable || dgt != 0; out[i] = ok ? (T)((long long)(dgt - (unsigned long long)nullable) + mn) : (T)0; }
  if (valid) { const uint64_t b = ballot64(i < m && ok); if (lane_id() == 0 && i < ((m + 63) / 64) * 64) valid[i >> 6] = b; }
}

struct PaFlagCols { int32_t n; const uint64_t* valid[8]; };
__global__ void __launch_bounds__(BLOCK) k_pa_flags(PaFlagCols fc, int64_t n, uint8_t* out) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; if (i >= n) return;
  uint32_t f = 0;
#pragma unroll
  for (int b = 0; b < 8; b++) if (b < fc.n) f |= (uint32_t)bit_get(fc.valid[b], i) << b;
  out[i] = (uint8_t)f;
}
// validity bitmap of a state column: a group whose nullable argument held no value has a NULL state
__global__ void __launch_bounds__(BLOCK) k_pa_state_valid(const uint64_t* __restrict__ nvalid, int64_t m, uint64_t* __restrict__ valid) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  const uint64_t b = ballot64(i < m && nvalid[i] != 0);
  if (lane_id() == 0 && i < ((m + 63) / 64) * 64) valid[i >> 6] = b;
}

// ---------------------------------------------------------------------------------------------- host side: one function per stage, dfgpu_agg_preaggregate_flags at the end calls them in order
// The slots of ctx->d_scratch64 this file uses.  The numbers are shared with other files (rp_partition's totals among them): they do not move.
enum PaSlot {
  PA_SLOT_SAMPLE = 0,          // [3] k_pa_sample: distinct keys, non-decreasing pairs, pairs
  PA_SLOT_ROWS_L1 = 9,         // rows the first partition level moved (those the selection kept); the word-sort ordering passes leave their totals here afterwards
  PA_SLOT_ROWS_L2 = 10,        // rows the second level moved
  PA_SLOT_MISPLACED = 11,      // k_pa_aggregate, two-level only: a row sat in a partition its key does not hash to
  PA_SLOT_WRITTEN = 12,        // k_pa_aggregate's cursor [0]: partial rows written
  PA_SLOT_LONGEST = 13,        // k_pa_max_len: rows of the longest partition
  PA_SLOT_EARLY = 14,          // k_pa_aggregate's cursor [2]: tables flushed before their partition ended
  PA_SLOT_KEY_MINMAX = 16,     // [8] k_pa_cols_minmax: min, max of up to four key columns
  PA_SLOT_OUTSIDE = 24         // k_pa_pack: some value lay outside the estimated ranges
};

// every decline: NOT_IMPLEMENTED (the plan layer groups the batch the ordinary way), and the verdict memo goes (see PaVerdictMemo::clear)
[[noreturn]] static void pa_skip(dfgpu_ctx* ctx, const char* why) { ctx->pa_memo.clear(); fail(DFGPU_NOT_IMPLEMENTED, "agg_preaggregate: %s", why); }

// ---- stage 1: the key columns
struct PaKeys { const dfgpu_array* const* cols; int32_t nkeys; bool is_dict, packed; int32_t ktype; int64_t n; };      // ktype: what the kernels read the one key per row as (UInt64 once packed)
static bool pa_key_type_ok(int32_t t) { return t == DFGPU_INT64 || t == DFGPU_UINT64 || t == DFGPU_INT32 || t == DFGPU_UINT32 || t == DFGPU_DATE32; }
static bool pa_plain_int(int32_t t) { switch (t) { case DFGPU_INT8: case DFGPU_INT16: case DFGPU_INT32: case DFGPU_INT64: case DFGPU_DATE32: case DFGPU_UINT8: case DFGPU_UINT16: case DFGPU_UINT32: case DFGPU_UINT64: return true; default: return false; } }
static PaKeys pa_check_keys(dfgpu_ctx* ctx, const dfgpu_array* const* keys, int32_t nkeys, int32_t n_aggs) {
  if (!ctx->agg_partitioned) pa_skip(ctx, "switched off (option agg_partitioned)");
  if (nkeys < 1 || nkeys > 4) pa_skip(ctx, "one to four key columns");
  const dfgpu_array* key = keys[0]; PaKeys k{}; k.cols = keys; k.nkeys = nkeys; k.n = key->length;
  // A dictionary key column is pre-aggregated by its CODES: codes with equal dictionary values leave as separate partial rows, which
  // interning the emitted dictionary array merges (dictionary keys intern by value).
  k.is_dict = nkeys == 1 && key->type == DFGPU_DICTIONARY;
  // Several key columns, or one with NULLs, travel as ONE packed u64 (value ranges multiplied out, NULL = digit 0 of its column): the partial rows' keys are unpacked again
  k.packed = nkeys > 1 || (!k.is_dict && key->validity);
  if (k.packed) { for (int c = 0; c < nkeys; c++) if (!keys[c] || !pa_plain_int(storage_type(keys[c]->type)) || keys[c]->length != k.n) pa_skip(ctx, "integer / Date32 key columns (not dictionary-encoded) when there are several or one carries NULLs"); }
  k.ktype = k.packed ? DFGPU_UINT64 : k.is_dict ? key->key_type : key->type;
  if (!k.packed && (!pa_key_type_ok(storage_type(k.ktype)) || key->validity)) pa_skip(ctx, "a 4- or 8-byte integer key column (or dictionary codes of that width)");
  if (k.n < ctx->agg_partitioned_min_rows || k.n > 0xFFFF0000ll) pa_skip(ctx, "batch below agg_partitioned_min_rows");
  if (n_aggs > 16) pa_skip(ctx, "at most 16 aggregates");
  return k;
}

// ---- stage 2: accumulator plan: one 8-byte LDS cell per SUM / MIN / MAX; COUNT and AVG counts come from the row count (value columns carry no NULLs)
// A nullable argument (accumulate.rs:126-233: NULL values take no part; a group that saw none has a NULL state): its validity travels as one bit of a per-row flag byte,
// its cells skip the NULL rows, and one COUNT_FLAG cell per nullable column counts the values seen -- COUNT(x), AVG's count and the validity of SUM / MIN / MAX states.
struct PaCells {
  PaPlan plan{}; int cell_of[16], nvalid_of[16];          // aggregate i: its (first) value cell and the COUNT_FLAG cell of its nullable argument, -1 = none
  const dfgpu_array* cell_src[PA_MAX_AGGS]; int cell_word[PA_MAX_AGGS]; bool cell_cast[PA_MAX_AGGS] = {};      // cell c reads word cell_word[c] of its source's rows (cell_cast: of their doubles)
  const dfgpu_array* flag_src[8]; int n_flags = 0;       // the nullable value columns: bit b of a row's flag byte = flag_src[b] holds a value there
  const dfgpu_array* srcs[PA_MAX_AGGS]; bool src_cast[PA_MAX_AGGS] = {}; int src_of[PA_MAX_AGGS], n_src = 0;      // the distinct value columns the partition moves (a Decimal128 column once, 16 bytes wide)
};
// value_casts[i] == DFGPU_FLOAT64 over an integer column: the argument is CAST(column AS DOUBLE) (what AVG / SUM over an integer column are planned as); the column is
// converted while the partition moves it -- the cast's own pass (400 MB read, 800 MB written per 100 M Int32 rows: 0.40 ms) does not run
static bool pa_cast_f64(const dfgpu_array* const* values, const int32_t* value_casts, int i) { return value_casts && value_casts[i] == DFGPU_FLOAT64 && values[i] && (values[i]->type == DFGPU_INT32 || values[i]->type == DFGPU_INT64); }
static int pa_flag_of(dfgpu_ctx* ctx, PaCells& pl, const dfgpu_array* v) {
  for (int b = 0; b < pl.n_flags; b++) if (pl.flag_src[b] == v) return b;
  if (pl.n_flags == 8) pa_skip(ctx, "at most 8 nullable value columns");
  pl.flag_src[pl.n_flags] = v; return pl.n_flags++;
}
static int pa_count_cell(dfgpu_ctx* ctx, PaCells& pl, const dfgpu_array* v) {           // the COUNT_FLAG cell of a nullable column (one per column)
  PaPlan& plan = pl.plan; const int b = pa_flag_of(ctx, pl, v);
  for (int j = 0; j < plan.n_acc; j++) if (plan.op[j] == PA_COUNT_FLAG && plan.flag_bit[j] == b) return j;
  if (plan.n_acc + 1 > PA_MAX_AGGS) pa_skip(ctx, "at most 6 accumulator cells (a nullable argument takes one more for its count)");
  const int c = plan.n_acc++; plan.op[c] = PA_COUNT_FLAG; plan.flag_bit[c] = b; pl.cell_src[c] = nullptr; pl.cell_word[c] = 0; return c;
}
static int pa_cell_op(dfgpu_ctx* ctx, int32_t kind, const dfgpu_array* v, bool asf) {          // the operation of aggregate `kind` over column v (asf: over its values cast to Float64)
  const bool i64 = !asf && storage_type(v->type) == DFGPU_INT64, u64 = !asf && v->type == DFGPU_UINT64, f64 = asf || v->type == DFGPU_FLOAT64, d128 = v->type == DFGPU_DECIMAL128;
  if (!i64 && !u64 && !f64 && !d128) pa_skip(ctx, "Int64 / UInt64 / Float64 / Decimal128 aggregate arguments");
  if (is_timestamp(v->type) && kind != DFGPU_AGG_MIN && kind != DFGPU_AGG_MAX) pa_skip(ctx, "MIN / MAX / COUNT over a Timestamp (SUM and AVG are refused, as in the reference)");
  switch (kind) {
    case DFGPU_AGG_SUM: return d128 ? PA_SUM_I128_LO : f64 ? PA_SUM_F64 : PA_SUM_I64;
    case DFGPU_AGG_AVG: if (!f64 && !d128) pa_skip(ctx, "AVG over Float64 / Decimal128"); return d128 ? PA_SUM_I128_LO : PA_SUM_F64;
    case DFGPU_AGG_MIN: if (d128) pa_skip(ctx, "MIN over Decimal128"); return f64 ? PA_MIN_F64 : i64 ? PA_MIN_I64 : PA_MIN_U64;
    case DFGPU_AGG_MAX: if (d128) pa_skip(ctx, "MAX over Decimal128"); return f64 ? PA_MAX_F64 : i64 ? PA_MAX_I64 : PA_MAX_U64;
    default: pa_skip(ctx, "SUM / AVG / COUNT / MIN / MAX");
  }
}
static int pa_value_cell(dfgpu_ctx* ctx, PaCells& pl, int op, const dfgpu_array* v, bool asf) {          // the cell (pair) of `op` over v: SUM(x) and AVG(x) share one
  PaPlan& plan = pl.plan; const bool d128 = v->type == DFGPU_DECIMAL128;
  int c = -1; for (int j = 0; j < plan.n_acc; j++) if (plan.op[j] == op && pl.cell_src[j] == v && pl.cell_cast[j] == asf) c = j;
  if (c >= 0) return c;
  const int need = d128 ? 2 : 1;
  if (plan.n_acc + need > PA_MAX_AGGS) pa_skip(ctx, "at most 6 accumulator cells (a Decimal128 sum takes two)");
  c = plan.n_acc; plan.n_acc += need; plan.op[c] = op; pl.cell_src[c] = v; pl.cell_word[c] = 0; pl.cell_cast[c] = asf;
  const int fbit = v->validity ? pa_flag_of(ctx, pl, v) : -1; plan.flag_bit[c] = fbit;
  if (d128) { const bool fits64 = v->precision > 0 && v->precision <= 18;      // |unscaled value| < 10^18 < 2^63: the high word carries no information
    plan.op[c + 1] = fits64 ? PA_SUM_I128_SX : PA_SUM_I128_HI; pl.cell_src[c + 1] = v; pl.cell_word[c + 1] = fits64 ? 0 : 1; plan.flag_bit[c + 1] = fbit; plan.has_i128 = 1; }
  return c;
}
static PaCells pa_plan_cells(dfgpu_ctx* ctx, const int32_t* kinds, const dfgpu_array* const* values, const int32_t* value_casts, int32_t n_aggs, int64_t n) {
  PaCells pl{}; PaPlan& plan = pl.plan;
  for (int i = 0; i < n_aggs; i++) if (value_casts && value_casts[i] != 0 && !pa_cast_f64(values, value_casts, i)) pa_skip(ctx, "an argument cast other than Int32 / Int64 -> Float64");
  for (int c = 0; c < PA_MAX_AGGS; c++) { plan.flag_bit[c] = -1; pl.cell_src[c] = nullptr; }
  for (int i = 0; i < n_aggs; i++) {
    const dfgpu_array* v = values[i]; pl.cell_of[i] = -1; pl.nvalid_of[i] = -1;
    if (v && (v->length != n || v->type == DFGPU_DICTIONARY)) pa_skip(ctx, "value columns of the batch's length, not dictionary-encoded");
    if (v && v->validity) pl.nvalid_of[i] = pa_count_cell(ctx, pl, v);
    if (kinds[i] == DFGPU_AGG_COUNT) continue;
    if (!v) pa_skip(ctx, "aggregate without an argument");
    const bool asf = pa_cast_f64(values, value_casts, i);
    pl.cell_of[i] = pa_value_cell(ctx, pl, pa_cell_op(ctx, kinds[i], v, asf), v, asf);
  }
  for (int c = 0; c < plan.n_acc; c++) {
    pl.src_of[c] = -1; if (!pl.cell_src[c]) continue;
    int j = -1; for (int q = 0; q < pl.n_src; q++) if (pl.srcs[q] == pl.cell_src[c] && pl.src_cast[q] == pl.cell_cast[c]) j = q;
    if (j < 0) { j = pl.n_src; pl.src_cast[pl.n_src] = pl.cell_cast[c]; pl.srcs[pl.n_src++] = pl.cell_src[c]; }
    pl.src_of[c] = j;
  }
  return pl;
}
// a Decimal128 column of precision <= 18 moves its low 8 bytes only; any other Decimal128 column 16 bytes a row
static bool pa_src_lo16(const dfgpu_array* a) { return a->type == DFGPU_DECIMAL128 && a->precision > 0 && a->precision <= 18; }
static int pa_src_width(const dfgpu_array* a) { return a->type == DFGPU_DECIMAL128 && !pa_src_lo16(a) ? 16 : 8; }

// ---- stage 3: 2..4 key columns (or a nullable one) -> one u64 per row
struct PaPacked { BufferPtr buf; PaPackCols pc{}; };
// min / range / stride of every column from the measured (min, max) pairs; false when the ranges multiply beyond 2^62.  estimate: the pairs come from a sample and are
// widened by their own width on either side
static bool pa_pack_ranges(PaPackCols& pc, const uint64_t* mm, bool estimate) {
  unsigned __int128 prod = 1;
  for (int c = pc.n - 1; c >= 0; c--) {
    __int128 lo = (long long)mm[2 * c], hi = (long long)mm[2 * c + 1]; if (lo > hi) lo = hi = 0;              // a column of NULLs only (or none sampled)
    if (estimate) { const __int128 w = hi - lo + 1; lo -= w; hi += w; if (lo < (__int128)INT64_MIN) lo = INT64_MIN; if (hi > (__int128)INT64_MAX) hi = INT64_MAX; }
    const unsigned __int128 range = (unsigned __int128)(hi - lo) + 1 + (unsigned)pc.nullable[c];
    if (range > ((unsigned __int128)1 << 62)) return false;
    pc.mn[c] = (long long)lo; pc.range[c] = (unsigned long long)range; pc.stride[c] = (unsigned long long)prod; prod *= range;
    if (prod > ((unsigned __int128)1 << 62)) return false;
  }
  return true;
}
static PaPacked pa_pack_keys(dfgpu_ctx* ctx, const PaKeys& k, const uint64_t* mk, bool cached) {
  PaPacked p; PaPackCols& pc = p.pc; const int64_t n = k.n;
  pc.n = k.nkeys;
  for (int c = 0; c < k.nkeys; c++) { const dfgpu_array* col = k.cols[c];
    pc.v[c] = col->values->ptr; pc.valid[c] = col->validity ? (const uint64_t*)col->validity->ptr : nullptr; pc.type[c] = storage_type(col->type); pc.nullable[c] = col->validity ? 1 : 0;
    const int w = type_width(col->type); if (w != 1 && w != 2 && w != 4 && w != 8) fail(DFGPU_INTERNAL, "agg_preaggregate: key column %d of type %d has no integer width", c, col->type); }      // the kernels read w bytes per row: checked here, not assumed there
  if (cached) { const PaVerdictMemo& memo = ctx->pa_memo; p.buf = memo.pack; for (int c = 0; c < k.nkeys; c++) { pc.mn[c] = memo.pack_min[c]; pc.stride[c] = memo.pack_stride[c]; pc.range[c] = memo.pack_range[c]; } return p; }
  // Ranges: exact (one pass over the key columns) for small batches; for large ones the min / max of every step-th row, widened by their own width on either side -- the pack
  // pass checks every row against them and the exact pass only runs when a row falls outside (saves a pass of 16 B per row: 0.8 ms per 100 M rows x 3 columns)
  zero_scratch(ctx);
  const int64_t step0 = n >= ctx->agg_pack_estimate_min_rows ? std::max<int64_t>(2, n >> 19) : 1;
  for (int attempt = 0; attempt < 2; attempt++) {
    const int64_t step = attempt == 0 ? step0 : 1; const bool estimate = step > 1;
    long long init[8]; for (int c = 0; c < 4; c++) { init[2 * c] = INT64_MAX; init[2 * c + 1] = INT64_MIN; }
    HIP_CHECK(hipMemcpyAsync(ctx->d_scratch64 + PA_SLOT_KEY_MINMAX, init, sizeof init, hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipMemsetAsync(ctx->d_scratch64 + PA_SLOT_OUTSIDE, 0, 8, ctx->stream));
    { KernelTimer kt_(ctx, "pa_pack");
      hipLaunchKernelGGL(k_pa_cols_minmax, dim3(grid_for((n + step - 1) / step, BLOCK * 8, ctx->num_cus * 8)), dim3(BLOCK), 0, ctx->stream, pc, mk, n, step, (long long*)(ctx->d_scratch64 + PA_SLOT_KEY_MINMAX));
      KERNEL_CHECK(); }
    const uint64_t* mm = read_scratch_range(ctx, PA_SLOT_KEY_MINMAX, 8);
    ctx->count_sync("sync:pa_pack_ranges");
    if (!pa_pack_ranges(pc, mm, estimate)) { if (estimate) continue; pa_skip(ctx, "key value ranges multiply beyond 2^62 (no packed key)"); }      // the widened estimate does not fit: try the exact ranges
    if (!p.buf) p.buf = alloc_buffer(ctx, (size_t)n * 8);
    { KernelTimer kt_(ctx, "pa_pack");
      hipLaunchKernelGGL(k_pa_pack, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, ctx->stream, pc, n, (uint64_t*)p.buf->ptr, estimate ? (unsigned long long*)(ctx->d_scratch64 + PA_SLOT_OUTSIDE) : nullptr);
      KERNEL_CHECK(); }
    if (!estimate || read_scratch(ctx, PA_SLOT_OUTSIDE) == 0) break;          // exact ranges, or every row inside the estimated ones
    ctx->count_sync("sync:pa_pack_outside");
  }
  return p;
}

// ---- stage 4: the sample: clustered? how many groups?  (a verdict-only call leaves its sample, and its packed keys, for the call that follows on the same columns)
struct PaSample { double distinct, nondecreasing, pairs; };
template <typename T>
static void launch_pa_sample(dfgpu_ctx* ctx, const void* kptr, const uint64_t* mk, int64_t n, int64_t s, const BufferPtr& table, uint64_t cap) {
  hipLaunchKernelGGL((k_pa_sample<T>), dim3(grid_for(s, BLOCK * 8, 256)), dim3(BLOCK), 0, ctx->stream, (const T*)kptr, mk, n, s, n / s, (unsigned long long*)table->ptr, cap - 1, (unsigned long long*)(ctx->d_scratch64 + PA_SLOT_SAMPLE));
}
static PaSample pa_sample(dfgpu_ctx* ctx, const PaKeys& k, const PaPacked& pk, const void* kptr, const uint64_t* mk, bool cached, bool verdict_only) {
  PaVerdictMemo& memo = ctx->pa_memo; const int64_t n = k.n;
  if (cached) { const PaSample smp{ (double)memo.sample[0], (double)memo.sample[1], (double)memo.sample[2] }; memo.clear(); return smp; }
  const int64_t s = n < (1 << 19) ? n : (1 << 19); const uint64_t cap = 1ull << 21;
  BufferPtr table = alloc_buffer(ctx, cap * 8); HIP_CHECK(hipMemsetAsync(table->ptr, 0xFF, cap * 8, ctx->stream));
  HIP_CHECK(hipMemsetAsync(ctx->d_scratch64 + PA_SLOT_SAMPLE, 0, 24, ctx->stream));
  { KernelTimer kt_(ctx, "pa_sample");
    switch (storage_type(k.ktype)) {
      case DFGPU_INT64: launch_pa_sample<int64_t>(ctx, kptr, mk, n, s, table, cap); break; case DFGPU_UINT64: launch_pa_sample<uint64_t>(ctx, kptr, mk, n, s, table, cap); break;
      case DFGPU_UINT32: launch_pa_sample<uint32_t>(ctx, kptr, mk, n, s, table, cap); break; default: launch_pa_sample<int32_t>(ctx, kptr, mk, n, s, table, cap); break; }
    KERNEL_CHECK(); }
  ctx->count_sync("sync:pa_sample"); fetch_to_pinned(ctx, PA_SLOT_SAMPLE, ctx->d_scratch64 + PA_SLOT_SAMPLE, 24);
  const uint64_t* h = ctx->h_pinned + PA_SLOT_SAMPLE;
  if (verdict_only) {          // the one place the memo is written
    memo.key = k.cols[0]->values->ptr; memo.mask = (const void*)mk; memo.n = n; for (int q = 0; q < 3; q++) memo.sample[q] = h[q];
    memo.pack = pk.buf; memo.pack_n = k.packed ? k.nkeys : 0;
    for (int c = 0; c < k.nkeys && k.packed; c++) { memo.pack_min[c] = pk.pc.mn[c]; memo.pack_stride[c] = pk.pc.stride[c]; memo.pack_range[c] = pk.pc.range[c]; }
  }
  return PaSample{ (double)h[0], (double)h[1], (double)h[2] };
}

// ---- stage 5: distinct keys D of the batch from d distinct among ss sampled rows: d = D (1 - exp(-ss / D)).  Returns why the batch is declined, or nullptr and *D_out.
static const char* pa_estimate_groups(const PaSample& smp, int64_t n, bool force, double* D_out) {
  const double d = smp.distinct, nondec = smp.nondecreasing, pairs = smp.pairs, ss = pairs + 1;
  if (pairs > 0 && nondec >= 0.98 * pairs && !force) return "keys arrive clustered (run numbering is cheaper)";
  double D = d;
  if (d >= 0.999 * ss) D = 1e12; else { double lo = d, hi = 1e12; for (int it = 0; it < 200; it++) { double mid = 0.5 * (lo + hi); double e = mid * (1.0 - exp(-ss / mid)); if (e < d) lo = mid; else hi = mid; } D = 0.5 * (lo + hi); }
  if (D > (double)n) D = (double)n;
  if (!force) {
    if (D < 3000) return "few groups (the LDS cache of the accumulators holds them)";
    if (D > (double)n / 3.0) return "fewer than three rows per group (pre-aggregation would not reduce the batch)";
  }
  *D_out = D; return nullptr;
}

// ---- stage 6: table size, partition counts, slice length, record size
struct PaGeometry { int cbits, cell_bytes; int64_t P, P1, P2; bool two_level; int64_t slice; int rs; };      // P = P1 * P2 partitions of tables of 2^cbits slots; rs: words of a partial row's record
static PaGeometry pa_geometry(double D, double d, int64_t n, int n_acc, int num_cus) {
  PaGeometry g{};
  g.cell_bytes = 16 + 8 * n_acc; g.cbits = 12; while (g.cbits > 6 && (((size_t)1 << g.cbits) + 1) * g.cell_bytes > 150 * 1024) g.cbits--;
  // groups a partition may hold: 0.55 of the table, and not more than the table takes before the kernel flushes it early (k_pa_aggregate: nfilled + PA_NT > C - C / 8 --
  // with five or six cells the table has 2048 slots and that bound, 768, is the smaller one: at 0.55 x 2048 every partition was cut and its keys left in two partial rows)
  const double table = (double)(1u << g.cbits), room = table - table / 8 - (double)PA_NT;
  const double per_part = room > 0 && 0.85 * room < 0.55 * table ? 0.85 * room : 0.55 * table;
  const double Dp = D > 4.0 * d ? D : 4.0 * d;          // skewed keys: the uniform model underestimates the tail, stay on the many-partitions side
  int64_t P = (int64_t)(Dp / per_part) + 1; if (P < 64) P = 64;
  // beyond 2048 partitions one pass writes bursts too short to pay (measured: P = 8192 slower than the atomics it replaces): two passes, P1 x P2
  g.two_level = P > 2048;
  int64_t P1 = P, P2 = 1;
  if (g.two_level) { P2 = P > 2048 * 128 ? 256 : 128; P1 = (P + P2 - 1) / P2; if (P1 < 16) P1 = 16; if (P1 > 2048) P1 = 2048; P = P1 * P2; }
  else { if (P > n / 2048 + 1) P = n / 2048 + 1; if (P > num_cus) P = std::min<int64_t>(2048, (P + num_cus - 1) / num_cus * num_cus); P1 = P; }
  g.P = P; g.P1 = P1; g.P2 = P2;
  // a partial row leaves the table as ONE record (key, count, cells; 4 or 8 words): the emit gathers a row with one or two sector reads instead of one per column
  g.rs = 2 + n_acc <= 4 ? 4 : 8;
  g.slice = (n / P + 1) * 3 / 2; if (g.slice < 65536) g.slice = 65536;          // uniform keys never split (a partition is within a percent of the average)
  return g;
}

// ---- stage 7: partition (key, row, value cells, flag byte) by key hash
struct PaRows { BufferPtr pkey, prow, pflag, starts; std::vector<BufferPtr> pval; uint32_t P = 0; };      // the moved columns; starts: u32[P + 1], first row of every partition
template <typename T>
static RpResult pa_partition_by(dfgpu_ctx* ctx, const void* kptr, const uint64_t* mk, int64_t n, uint32_t P1, const RpCols& cols) {
  return rp_partition(ctx, RpHashInt<T>{ (const T*)kptr, nullptr, mk }, n, P1, cols, false, ctx->d_scratch64 + PA_SLOT_ROWS_L1, "pa_hist", "pa_scan", "pa_scatter");
}
// the row number travels with a row only to find every group's first row (first-seen order): with DFGPU_PREAGG_ANY_ORDER it stays behind -- 4 of the 20..28 bytes a row
// costs each partition level and the aggregation's read
static PaRows pa_partition(dfgpu_ctx* ctx, const void* kptr, int32_t ktype, const uint64_t* mk, int64_t n, const PaCells& pl, uint32_t P1, bool first_seen) {
  PaRows r; const int n_src = pl.n_src, n_flags = pl.n_flags;
  r.pkey = alloc_buffer(ctx, (size_t)n * 8); if (first_seen) r.prow = alloc_buffer(ctx, (size_t)n * 4); r.pval.resize((size_t)n_src);
  BufferPtr flags_in;          // the flag byte of every row: bit b = nullable value column b holds a value there
  if (n_flags) {
    flags_in = alloc_buffer(ctx, (size_t)n + 64); r.pflag = alloc_buffer(ctx, (size_t)n + 64);
    PaFlagCols fc{}; fc.n = n_flags; for (int b = 0; b < n_flags; b++) fc.valid[b] = (const uint64_t*)pl.flag_src[b]->validity->ptr;
    hipLaunchKernelGGL(k_pa_flags, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, ctx->stream, fc, n, (uint8_t*)flags_in->ptr);
    KERNEL_CHECK();
  }
  RpCols cols{}; cols.n = 1 + n_src + (n_flags ? 1 : 0); cols.rowid_dst = r.prow ? (uint32_t*)r.prow->ptr : nullptr;
  if (n_flags) cols.c[1 + n_src] = RpCol{ flags_in->ptr, r.pflag->ptr, 1, RP_RAW, 0 };
  cols.c[0] = RpCol{ kptr, r.pkey->ptr, 8, RP_HASHKEY, ktype };
  for (int j = 0; j < n_src; j++) { const dfgpu_array* a = pl.srcs[j]; const int w = pa_src_width(a);
    r.pval[(size_t)j] = alloc_buffer(ctx, (size_t)n * (size_t)w);
    cols.c[1 + j] = pl.src_cast[j] ? RpCol{ a->values->ptr, r.pval[(size_t)j]->ptr, 8, RP_CASTF64, a->type } : RpCol{ a->values->ptr, r.pval[(size_t)j]->ptr, 8 * (w / 8), pa_src_lo16(a) ? RP_LO16 : RP_RAW, 0 }; }
  RpResult res;
  switch (storage_type(ktype)) {
    case DFGPU_INT64: case DFGPU_UINT64: res = pa_partition_by<int64_t>(ctx, kptr, mk, n, P1, cols); break;
    case DFGPU_UINT32: res = pa_partition_by<uint32_t>(ctx, kptr, mk, n, P1, cols); break;
    default: res = pa_partition_by<int32_t>(ctx, kptr, mk, n, P1, cols); break; }
  r.starts = res.starts; r.P = res.P;
  return r;
}
// second level: a stable split of level 1's output on the low hash bits; the bounds of the P1 * P2 fine partitions are read off the moved keys
static PaRows pa_partition_fine(dfgpu_ctx* ctx, PaRows in, const uint64_t* mk, int64_t n, const PaCells& pl, const PaGeometry& g) {
  const int n_src = pl.n_src;
  const int64_t m1 = mk ? (int64_t)read_scratch(ctx, PA_SLOT_ROWS_L1) : n;          // rows the selection kept
  PaRows r; r.pkey = alloc_buffer(ctx, (size_t)n * 8); if (in.prow) r.prow = alloc_buffer(ctx, (size_t)n * 4); r.pval.resize((size_t)n_src);
  if (in.pflag) r.pflag = alloc_buffer(ctx, (size_t)n + 64);
  const int c0 = in.prow ? 2 : 1;          // columns in front of the value columns: key (, row number)
  RpCols c2{}; c2.n = c0 + n_src + (in.pflag ? 1 : 0);
  if (in.pflag) c2.c[c0 + n_src] = RpCol{ in.pflag->ptr, r.pflag->ptr, 1, RP_RAW, 0 };
  c2.c[0] = RpCol{ in.pkey->ptr, r.pkey->ptr, 8, RP_RAW, 0 }; if (in.prow) c2.c[1] = RpCol{ in.prow->ptr, r.prow->ptr, 4, RP_RAW, 0 };
  for (int j = 0; j < n_src; j++) { const int w = pa_src_width(pl.srcs[j]); r.pval[(size_t)j] = alloc_buffer(ctx, (size_t)n * (size_t)w); c2.c[c0 + j] = RpCol{ in.pval[(size_t)j]->ptr, r.pval[(size_t)j]->ptr, w, RP_RAW, 0 }; }
  (void)rp_partition(ctx, RpHashU64Low{ (const uint64_t*)in.pkey->ptr }, m1, (uint32_t)g.P2, c2, true, ctx->d_scratch64 + PA_SLOT_ROWS_L2, "pa_hist2", "pa_scan2", "pa_scatter2", true, true);
  in = PaRows{};          // level 1's buffers go back to the allocator
  HIP_CHECK(hipMemsetAsync(ctx->d_scratch64 + PA_SLOT_MISPLACED, 0, 8, ctx->stream));
  r.starts = alloc_buffer(ctx, (size_t)(g.P + 1) * 4); r.P = (uint32_t)g.P;
  { KernelTimer kt_(ctx, "pa_bounds");
    hipLaunchKernelGGL(k_pa_bounds, dim3(grid_for(g.P + 1, BLOCK)), dim3(BLOCK), 0, ctx->stream, (const uint64_t*)r.pkey->ptr, (uint32_t)m1, (uint32_t)g.P1, (uint32_t)g.P2, (uint32_t)g.P, (uint32_t*)r.starts->ptr);
    KERNEL_CHECK(); }
  return r;
}
// where the aggregation reads its cells: once, from the rows of the last level
static void pa_bind_cells(PaPlan& plan, const PaCells& pl, const PaRows& rows) {
  plan.vflag = pl.n_flags ? (const uint8_t*)rows.pflag->ptr : nullptr;
  for (int c = 0; c < plan.n_acc; c++) { const int j = pl.src_of[c];
    if (j < 0) { plan.vstride[c] = 1; plan.val[c] = nullptr; continue; }
    plan.vstride[c] = pa_src_width(pl.srcs[j]) / 8; plan.val[c] = (const uint64_t*)rows.pval[(size_t)j]->ptr + pl.cell_word[c]; }
}

// ---- stage 8: aggregate every partition out of LDS
struct PaPartial { BufferPtr orec, ofirst; int64_t m = 0, n_slices = 1; uint64_t early = 0; };      // m records of rs words and their groups' first rows; n_slices > 1 or early != 0: some key may have left in several rows
template <bool I128, bool FLAGS>
static void launch_pa_aggregate(dfgpu_ctx* ctx, const PaRows& rows, const PaPlan& plan, const BufferPtr& items, const PaGeometry& g, unsigned grid, const PaPartial& out) {
  HIP_CHECK(hipFuncSetAttribute((const void*)k_pa_aggregate<I128, FLAGS>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024));      // per device: set on every call, no process-wide flag
  hipLaunchKernelGGL((k_pa_aggregate<I128, FLAGS>), dim3(grid), dim3(PA_NT), (((size_t)1 << g.cbits) + 1) * g.cell_bytes, ctx->stream, (const uint64_t*)rows.pkey->ptr, rows.prow ? (const uint32_t*)rows.prow->ptr : (const uint32_t*)nullptr, plan,
                     (const uint32_t*)rows.starts->ptr, (const uint32_t*)items->ptr, (uint32_t)g.P, g.cbits, (uint32_t)g.slice, (uint64_t*)out.orec->ptr, g.rs, (uint32_t*)out.ofirst->ptr, (unsigned long long*)(ctx->d_scratch64 + PA_SLOT_WRITTEN),
                     g.two_level ? (uint32_t)g.P1 : 0u, (uint32_t)g.P2, (uint32_t*)(ctx->d_scratch64 + PA_SLOT_MISPLACED));
}
static PaPartial pa_aggregate(dfgpu_ctx* ctx, PaRows rows, const PaPlan& plan, const PaGeometry& g, int64_t n, bool is_dict) {          // takes the rows over: they are released when it returns
  const int64_t P = g.P;
  PaPartial out; out.orec = alloc_buffer(ctx, (size_t)n * (size_t)g.rs * 8); out.ofirst = alloc_buffer(ctx, (size_t)n * 4);
  HIP_CHECK(hipMemsetAsync(ctx->d_scratch64 + PA_SLOT_WRITTEN, 0, 24, ctx->stream));          // written, longest, early
  hipLaunchKernelGGL(k_pa_max_len, dim3((unsigned)((P + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, ctx->stream, (const uint32_t*)rows.starts->ptr, (uint32_t)P, (unsigned long long*)(ctx->d_scratch64 + PA_SLOT_LONGEST));
  KERNEL_CHECK();
  // whether any partition is longer than a slice (skewed keys) is the device's to know: the (partition, slice) work list is always built, the longest partition comes back
  // with the aggregate's own read-back below (one host round trip less per call)
  { KernelTimer kt_(ctx, "pa_aggregate");
    BufferPtr items = alloc_buffer(ctx, (size_t)(P + 1) * 4);            // sum over partitions of ceil(len / slice) <= P + n / slice
    hipLaunchKernelGGL(k_pa_items, dim3(1), dim3(PA_NT), 0, ctx->stream, (const uint32_t*)rows.starts->ptr, (uint32_t)P, (uint32_t)g.slice, (uint32_t*)items->ptr);
    const unsigned grid = (unsigned)(P + n / g.slice + 1);
    if (plan.vflag) { if (plan.has_i128) launch_pa_aggregate<true, true>(ctx, rows, plan, items, g, grid, out); else launch_pa_aggregate<false, true>(ctx, rows, plan, items, g, grid, out); }
    else { if (plan.has_i128) launch_pa_aggregate<true, false>(ctx, rows, plan, items, g, grid, out); else launch_pa_aggregate<false, false>(ctx, rows, plan, items, g, grid, out); }
    KERNEL_CHECK(); }
  const uint64_t* back = read_scratch_range(ctx, PA_SLOT_MISPLACED, 4);          // misplaced, written, longest, early: one read-back
  const uint64_t misplaced = back[0], written = back[PA_SLOT_WRITTEN - PA_SLOT_MISPLACED], longest = back[PA_SLOT_LONGEST - PA_SLOT_MISPLACED]; out.early = back[PA_SLOT_EARLY - PA_SLOT_MISPLACED];
  out.m = (int64_t)written; out.n_slices = longest ? ((int64_t)longest + g.slice - 1) / g.slice : 1;
  if (g.two_level && (uint32_t)misplaced != 0) fail(DFGPU_INTERNAL, "agg_preaggregate: the two-level partition left rows out of partition order");
  // every key left in exactly one partial row unless a hot partition was cut into slices or a table overflowed mid-partition: the plan layer then
  // needs no hash table to number the groups of a first batch (option "agg_preaggregate_distinct", read only)
  ctx->pa_last_distinct = out.n_slices == 1 && !is_dict && out.early == 0;          // dictionary codes: two codes may carry one value
  return out;
}

// ---- stage 9: the permutation that puts the partial rows in first-seen order of their groups (ofirst: every partial row's first input row, all distinct); one route per size
static void pa_perm_small_sort(dfgpu_ctx* ctx, uint32_t* ofirst, int64_t m, uint32_t* perm) {          // below 32768 partial rows: a pair sort
  launch_iota_u32(ctx, perm, m, 0);
  radix_sort_pairs_u32(ctx, ofirst, perm, m, 32);
}
static void pa_perm_mark_rank(dfgpu_ctx* ctx, const uint32_t* ofirst, int64_t m, int64_t n, uint32_t* perm) {          // no sort: mark the first rows in a bitmap over the input, rank = marked rows in front
  const int64_t nw = (n + 63) / 64;
  BufferPtr bits = alloc_buffer(ctx, (size_t)nw * 8, true), pref = alloc_buffer(ctx, (size_t)(nw + 1) * 4);
  hipLaunchKernelGGL(k_pa_mark, dim3(grid_for(m, BLOCK)), dim3(BLOCK), 0, ctx->stream, ofirst, m, (unsigned long long*)bits->ptr);
  hipLaunchKernelGGL(k_pa_popc, dim3(grid_for(nw, BLOCK)), dim3(BLOCK), 0, ctx->stream, (const uint64_t*)bits->ptr, nw, (uint32_t*)pref->ptr);
  exclusive_scan_u32_inplace32(ctx, (uint32_t*)pref->ptr, nw, nullptr);
  hipLaunchKernelGGL(k_pa_rank_perm, dim3(grid_for(m, BLOCK)), dim3(BLOCK), 0, ctx->stream, ofirst, m, (const uint64_t*)bits->ptr, (const uint32_t*)pref->ptr, perm);
  KERNEL_CHECK();
}
static void pa_perm_inverse_map(dfgpu_ctx* ctx, const uint32_t* ofirst, int64_t m, int64_t n, uint32_t* perm) {          // millions of partial rows: inv[first row] = partial row, compacted (see k_pa_inv)
  BufferPtr inv = alloc_buffer(ctx, (size_t)n * 4 + 64);
  HIP_CHECK(hipMemsetAsync(inv->ptr, 0xFF, (size_t)n * 4, ctx->stream));
  hipLaunchKernelGGL(k_pa_inv, dim3(grid_for(m, BLOCK)), dim3(BLOCK), 0, ctx->stream, ofirst, m, (uint32_t*)inv->ptr);
  const int64_t nblk = grid_for(n, BLOCK * INV_PER);
  BufferPtr cnts = alloc_buffer(ctx, (size_t)(nblk + 1) * 4);
  hipLaunchKernelGGL((k_pa_inv_compact<false>), dim3((unsigned)nblk), dim3(BLOCK), 0, ctx->stream, (const uint32_t*)inv->ptr, n, (uint32_t*)cnts->ptr, (uint32_t*)nullptr);
  exclusive_scan_u32_inplace32(ctx, (uint32_t*)cnts->ptr, nblk, nullptr);
  hipLaunchKernelGGL((k_pa_inv_compact<true>), dim3((unsigned)nblk), dim3(BLOCK), 0, ctx->stream, (const uint32_t*)inv->ptr, n, (uint32_t*)cnts->ptr, perm);
  KERNEL_CHECK();
}
static void pa_perm_word_sort(dfgpu_ctx* ctx, const uint32_t* ofirst, int64_t m, int64_t n, uint32_t* perm) {          // the same sizes, general form: LSD passes over (first row << jb | partial row) words
  int jb = 1; while (((uint64_t)(m - 1) >> jb) != 0) jb++;
  int fb = 1; while (((uint64_t)(n - 1) >> fb) != 0) fb++;
  BufferPtr w0 = alloc_buffer(ctx, (size_t)m * 8), w1 = alloc_buffer(ctx, (size_t)m * 8);
  hipLaunchKernelGGL(k_pa_order_words, dim3(grid_for(m, BLOCK)), dim3(BLOCK), 0, ctx->stream, ofirst, m, jb, (uint64_t*)w0->ptr);
  uint64_t* wa = (uint64_t*)w0->ptr; uint64_t* wb = (uint64_t*)w1->ptr;
  const int npass = (fb + 7) / 8, dbits = (fb + npass - 1) / npass;
  for (int shift = 0; shift < fb; shift += dbits) {
    const int bits = fb - shift < dbits ? fb - shift : dbits;
    RpCols rc{}; rc.n = 1; rc.c[0] = RpCol{ nullptr, wb, 8, RP_HASHKEY, 0 };
    (void)rp_partition(ctx, RpHashDigit{ wa, shift + jb, (1u << bits) - 1u }, m, 1u << bits, rc, true, ctx->d_scratch64 + PA_SLOT_ROWS_L1, "pa_order_hist", "pa_order_scan", "pa_order_scatter", false);
    std::swap(wa, wb);
  }
  hipLaunchKernelGGL(k_pa_perm_of_words, dim3(grid_for(m, BLOCK)), dim3(BLOCK), 0, ctx->stream, (const uint64_t*)wa, m, jb, perm);
  KERNEL_CHECK();
}
static void pa_first_seen_perm(dfgpu_ctx* ctx, uint32_t* ofirst, int64_t m, int64_t n, uint32_t* perm) {
  KernelTimer kt_(ctx, "pa_order");
  if (m < 32768) pa_perm_small_sort(ctx, ofirst, m, perm);
  else if (m <= (4 << 20)) pa_perm_mark_rank(ctx, ofirst, m, n, perm);       // beyond a few million rows the random atomics and rank look-ups lose to the sort (20 M: 1.44 ms against 1.28)
  else if (ctx->agg_order_inverse_map) pa_perm_inverse_map(ctx, ofirst, m, n, perm);
  else pa_perm_word_sort(ctx, ofirst, m, n, perm);
}

// ---- stage 10: the partial rows' columns: states, state validity, keys
static void pa_emit_add(PaEmit& em, int word, void* dst, int narrow, int dstride = 1, int doff = 0) {          // output column: word `word` of every record -> dst[i * dstride + doff]
  if (em.n >= 2 + 2 * PA_MAX_AGGS) fail(DFGPU_NOT_IMPLEMENTED, "agg_preaggregate: more output columns than one emit pass writes");
  em.word[em.n] = word; em.dst[em.n] = dst; em.narrow[em.n] = narrow; em.dstride[em.n] = dstride; em.doff[em.n] = doff; em.n++;
}
struct PaAggArgs { const int32_t* kinds; const dfgpu_array* const* values; const int32_t* value_casts; int32_t n_aggs; };
// the state arrays of aggregate i (st[2 i], st[2 i + 1]) and their columns of the emit pass; returns the state whose validity follows the values-seen count, or nullptr
static dfgpu_array* pa_state_arrays(dfgpu_ctx* ctx, const PaAggArgs& a, const PaCells& pl, int i, int64_t m, PaEmit& em, ArrayHolder* st) {
  const dfgpu_array* v = a.values[i]; const int32_t kind = a.kinds[i]; const int cell = 2 + pl.cell_of[i];
  auto counts_as = [&](int32_t type) { dfgpu_array* x = new_fixed(ctx, type, m); pa_emit_add(em, pl.nvalid_of[i] >= 0 ? 2 + pl.nvalid_of[i] : 1, x->values->ptr, 0); return x; };
  auto cell_as = [&](int32_t type) { dfgpu_array* x = new_fixed(ctx, type, m); pa_emit_add(em, cell, x->values->ptr, 0); return x; };
  // Decimal128 sums: state type Decimal128(min(38, p + 10), s) (sum.rs:75-86, average.rs:96-110); the two cells interleave into 16-byte values
  auto dec_as = [&]() { dfgpu_array* x = new_fixed(ctx, DFGPU_DECIMAL128, m, std::min(38, v->precision + 10), v->scale); pa_emit_add(em, cell, x->values->ptr, 0, 2, 0); pa_emit_add(em, cell + 1, x->values->ptr, 0, 2, 1); return x; };
  const bool d128 = v && v->type == DFGPU_DECIMAL128;
  if (kind == DFGPU_AGG_COUNT) st[0].a = counts_as(DFGPU_INT64);                                                       // count.rs: Int64 state
  else if (kind == DFGPU_AGG_AVG) { st[0].a = counts_as(DFGPU_UINT64); st[1].a = d128 ? dec_as() : cell_as(DFGPU_FLOAT64); }   // average.rs:392-430: (counts, sums)
  else if (d128) st[0].a = dec_as();
  else st[0].a = cell_as(pa_cast_f64(a.values, a.value_casts, i) ? DFGPU_FLOAT64 : v->type);          // SUM / MIN / MAX of an 8-byte type: state type == input type (sum.rs:75-86, min_max.rs:102-139)
  return pl.nvalid_of[i] >= 0 && kind != DFGPU_AGG_COUNT ? st[kind == DFGPU_AGG_AVG ? 1 : 0].get() : nullptr;
}
template <typename T>
static void launch_pa_unpack(dfgpu_ctx* ctx, const uint64_t* packed, int64_t m, const PaPackCols& pc, int c, void* dst, uint64_t* valid) {
  hipLaunchKernelGGL((k_pa_unpack<T>), dim3(grid_for(((m + 63) / 64) * 64, BLOCK)), dim3(BLOCK), 0, ctx->stream, packed, m, pc.stride[c], pc.range[c], pc.mn[c], pc.nullable[c], (T*)dst, valid);
}
// the packed keys of the partial rows back into their columns (NULL digits -> validity)
static void pa_unpack_keys(dfgpu_ctx* ctx, const PaKeys& k, const PaPackCols& pc, const dfgpu_array* packed, int64_t m, dfgpu_array** out_keys) {
  std::vector<ArrayHolder> kc((size_t)k.nkeys); const uint64_t* src = (const uint64_t*)packed->values->ptr;
  for (int c = 0; c < k.nkeys; c++) {
    kc[(size_t)c].a = new_fixed(ctx, k.cols[c]->type, m, 0, 0, pc.nullable[c] != 0);
    uint64_t* vb = pc.nullable[c] ? (uint64_t*)kc[(size_t)c].get()->validity->ptr : nullptr; void* dst = kc[(size_t)c].get()->values->ptr;
    if (m) switch (type_width(k.cols[c]->type)) {
      case 1: launch_pa_unpack<uint8_t>(ctx, src, m, pc, c, dst, vb); break; case 2: launch_pa_unpack<uint16_t>(ctx, src, m, pc, c, dst, vb); break;
      case 4: launch_pa_unpack<uint32_t>(ctx, src, m, pc, c, dst, vb); break; default: launch_pa_unpack<uint64_t>(ctx, src, m, pc, c, dst, vb); break; }
    kc[(size_t)c].get()->null_count = pc.nullable[c] ? -1 : 0;
  }
  KERNEL_CHECK();
  for (int c = 0; c < k.nkeys; c++) out_keys[c] = kc[(size_t)c].release();
}
static void pa_emit(dfgpu_ctx* ctx, const PaPartial& part, const uint32_t* perm /* nullptr: the records leave as the partitions wrote them */, int rs, const PaCells& pl, const PaKeys& k, const PaPackCols& pc,
                    const PaAggArgs& a, dfgpu_array** out_keys, dfgpu_array** out_states) {
  KernelTimer kt_(ctx, "pa_emit");
  const int64_t m = part.m; const PaPlan& plan = pl.plan; const dim3 grid(grid_for(m, BLOCK));
  ArrayHolder ok(new_fixed(ctx, k.ktype, m));
  PaEmit em{}; pa_emit_add(em, 0, ok.get()->values->ptr, type_width(k.ktype) == 8 ? 0 : 1);
  std::vector<ArrayHolder> st((size_t)a.n_aggs * 2);
  // the values-seen count of every nullable column, once (UInt64 words): COUNT(x) / AVG counts copy it, state validities derive from it
  std::vector<BufferPtr> nval_buf((size_t)PA_MAX_AGGS);
  for (int c = 0; c < plan.n_acc; c++) if (plan.op[c] == PA_COUNT_FLAG) { nval_buf[(size_t)c] = alloc_buffer(ctx, (size_t)(m + 1) * 8); pa_emit_add(em, 2 + c, nval_buf[(size_t)c]->ptr, 0); }
  std::vector<std::pair<dfgpu_array*, int>> need_valid;          // (state array, its COUNT_FLAG cell)
  for (int i = 0; i < a.n_aggs; i++) if (dfgpu_array* s = pa_state_arrays(ctx, a, pl, i, m, em, &st[(size_t)2 * i])) need_valid.emplace_back(s, pl.nvalid_of[i]);
  if (m) { if (rs == 4) hipLaunchKernelGGL(k_pa_emit<4>, grid, dim3(BLOCK), 0, ctx->stream, em, (const uint64_t*)part.orec->ptr, perm, m); else hipLaunchKernelGGL(k_pa_emit<8>, grid, dim3(BLOCK), 0, ctx->stream, em, (const uint64_t*)part.orec->ptr, perm, m); }
  KERNEL_CHECK();
  for (auto& nv : need_valid) {          // NullState::build (accumulate.rs:328-356): the state of a group that saw no value is NULL
    nv.first->validity = alloc_buffer(ctx, bitmap_bytes(m) + 8); nv.first->null_count = -1;
    if (m) hipLaunchKernelGGL(k_pa_state_valid, dim3(grid_for(((m + 63) / 64) * 64, BLOCK)), dim3(BLOCK), 0, ctx->stream, (const uint64_t*)nval_buf[(size_t)nv.second]->ptr, m, (uint64_t*)nv.first->validity->ptr);
    KERNEL_CHECK();
  }
  if (k.is_dict) {           // DictionaryArray::try_new(codes, the input's dictionary)
    dfgpu_array* d = nullptr; dfgpu_status st2 = dfgpu_array_make_dictionary(ctx, ok.get(), k.cols[0]->dictionary, &d);
    if (st2 != DFGPU_OK) fail(st2, "%s", ctx->err.c_str());
    out_keys[0] = d;
  } else if (k.packed) pa_unpack_keys(ctx, k, pc, ok.get(), m, out_keys);
  else out_keys[0] = ok.release();
  for (int i = 0; i < a.n_aggs; i++) { out_states[2 * i] = st[(size_t)2 * i].release(); out_states[2 * i + 1] = st[(size_t)2 * i + 1].release(); }
}

}  // namespace dfgpu

using namespace dfgpu;
extern "C" dfgpu_status dfgpu_agg_preaggregate(dfgpu_ctx* ctx, const dfgpu_array* const* keys, int32_t nkeys, const int32_t* kinds, const dfgpu_array* const* values, int32_t n_aggs,
                                               const dfgpu_array* opt_mask, dfgpu_array** out_keys, dfgpu_array** out_states) {
  return dfgpu_agg_preaggregate_flags(ctx, keys, nkeys, kinds, values, nullptr, n_aggs, opt_mask, 0, out_keys, out_states);
}
extern "C" dfgpu_status dfgpu_agg_preaggregate_flags(dfgpu_ctx* ctx, const dfgpu_array* const* keys, int32_t nkeys, const int32_t* kinds, const dfgpu_array* const* values, const int32_t* value_casts, int32_t n_aggs,
                                                     const dfgpu_array* opt_mask, int32_t flags, dfgpu_array** out_keys, dfgpu_array** out_states) {
  return guard(ctx, [&] {
    const bool first_seen = ctx->first_seen_group_order && !(flags & DFGPU_PREAGG_ANY_ORDER);
    const bool verdict_only = out_keys == nullptr;         // would this batch be taken?  (key column + selection only; see include/dfgpu.h)
    if (!keys || (!verdict_only && n_aggs && (!kinds || !values || !out_states))) fail(DFGPU_INVALID_ARGUMENT, "agg_preaggregate: null argument");
    if (verdict_only) n_aggs = 0;
    const PaKeys k = pa_check_keys(ctx, keys, nkeys, n_aggs); const int64_t n = k.n;
    PaCells cells = pa_plan_cells(ctx, kinds, values, value_casts, n_aggs, n);
    const uint64_t* mk = nullptr; BufferPtr mask = effective_mask(ctx, opt_mask, n); if (mask) mk = (const uint64_t*)mask->ptr;
    const bool cached = ctx->pa_memo.answers(keys[0]->values->ptr, mk, n, k.packed, nkeys);          // the verdict-only call before this one sampled (and packed) these columns
    PaPacked pk; if (k.packed) pk = pa_pack_keys(ctx, k, mk, cached);
    const void* kptr = k.packed ? pk.buf->ptr : keys[0]->values->ptr;
    const PaSample smp = pa_sample(ctx, k, pk, kptr, mk, cached, verdict_only);
    double D = 0;
    if (const char* why = pa_estimate_groups(smp, n, ctx->agg_partitioned_force, &D)) pa_skip(ctx, why);
    if (verdict_only) return;
    const PaGeometry g = pa_geometry(D, smp.distinct, n, cells.plan.n_acc, ctx->num_cus);
    PaRows rows = pa_partition(ctx, kptr, k.ktype, mk, n, cells, (uint32_t)g.P1, first_seen);
    pk.buf.reset();          // the packed keys have moved
    if (g.two_level) rows = pa_partition_fine(ctx, std::move(rows), mk, n, cells, g);
    pa_bind_cells(cells.plan, cells, rows);
    const PaPartial part = pa_aggregate(ctx, std::move(rows), cells.plan, g, n, k.is_dict);
    BufferPtr perm = alloc_buffer(ctx, (size_t)(part.m + 1) * 4);
    if (first_seen) pa_first_seen_perm(ctx, (uint32_t*)part.ofirst->ptr, part.m, n, (uint32_t*)perm->ptr);
    pa_emit(ctx, part, first_seen ? (const uint32_t*)perm->ptr : nullptr, g.rs, cells, k, pk.pc, PaAggArgs{ kinds, values, value_casts, n_aggs }, out_keys, out_states);
  });
}
