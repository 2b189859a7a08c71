// comoments.hip -- a9: COVAR_SAMP / COVAR_POP / CORR / REGR_SLOPE .. REGR_SXY per group for AggregateExec on gfx950 (dfgpu_comoments, a sibling of dfgpu_moments).
//
// Reference: physical-expr/src/aggregate/covariance.rs:225-406 (CovarianceAccumulator: state :263-270, update :272-311, merge :354-382, evaluate :384-401),
// correlation.rs:134-246 (a covariance and two population-stddev accumulators over the same filtered pairs) and regr.rs:228-466 (state :254-262, update :265-306,
// evaluate :420-460); row-at-a-time Accumulators behind GroupsAccumulatorAdapter.  `a` is argument 0 and `b` argument 1 (REGR: a = y, b = x).
//
// State lives in HBM, one slot per group: count (u64), mean_a, mean_b, m2_a, m2_b, c_ab (f64); COVAR carries no m2 (FULL = false: neither computed nor stored).  A group
// without a row is all zero bits.  update_batch and merge_batch are the same passes over WEIGHTED ROWS -- a value row is (c = 1, means = the pair cast `as f64`, m2s = 0,
// c_ab = 0) and counts only when BOTH arguments are valid; a state row takes no part when c = 0 or one of its columns is NULL -- into a per-batch scratch of ten 8-byte
// cells per group (eight for COVAR), which k_comoments_fold then merges into the state:
//   pass 1  N_b = sum c, S_a = sum c * mean_a, S_b likewise, and per argument the largest and the smallest mean seen (below)
//   means   one thread per group: S_a, S_b become the batch means A_b, B_b in place: the one value where min = max, else S / N_b
//   pass 2  M2_a = sum (m2_a + c * (mean_a - A_b)^2), M2_b likewise (FULL only), C_b = sum (c_ab + c * (mean_a - A_b) * (mean_b - B_b)), A_b / B_b read from the row's group
//   fold    one thread per group: (N_b, A_b, B_b, M2_a, M2_b, C_b) into the state by the reference's merge formulas (covariance.rs:365-379, variance.rs:290-300); scratch cleared
// The values and the group ids are read twice: 40 B per row of two Float64 arguments.  One path per batch of `total` known groups, as in moments.hip:
//   LDS     total <= COMOMENTS_LDS_GROUPS (1024): per-workgroup partials, seven cells per group in pass 1 and three in pass 2, in arrays of 512 groups (28 KiB / 12 KiB) while
//           total <= COMOMENTS_LDS_SMALL and of 1024 groups (56 KiB / 24 KiB: two workgroups a CU in pass 1) above; a wave whose active lanes all carry one id reduces
//           first and adds once; one global atomic per touched group and cell at the end
//   GLOBAL  otherwise: the same wave-uniform shortcut, else one global atomic per row and cell
//
// A CONSTANT ARGUMENT GIVES AN EXACT ZERO.  The reference branches on exact zeros (CORR: 0.0 when a population stddev is 0.0; REGR_SLOPE / INTERCEPT / R2: NULL when
// var_pop == 0.0), and its recurrence keeps m2 at exactly 0.0 while every row of a group carries one value (delta is 0 every time).  S / N does not: for a constant 0.1 it
// can differ from 0.1 in the last place and m2 comes out as 1e-34.  So pass 1 keeps, per group and argument, the maximum and the minimum of the means in an order-preserving
// u64 encoding (float_key; both as integer atomicMax, the minimum of the complement, so that a scratch of zero bits is neutral for both and NaNs order like any other bit
// pattern).  Where they are equal every row carried that very bit pattern and it IS the batch mean: every deviation, and with it m2 and the group's share of c_ab, is exactly
// 0 (NaN for a constant NaN or Inf: x - x, as in the reference).  The fold keeps the stored mean bit for bit when the batch mean equals it (m0 * c0 / nc + mb * c / nc
// drifts), and takes the batch as it is when the group had no row before, so the next batch's delta is 0 again.
//
// Everything here is compiled with contraction off: the evaluate kernel is compared with IEEE evaluation of the reference's expressions, and an fma in a deviation product
// would not be the product the zero argument relies on.
#include "acc_cells.h"
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#pragma clang fp contract(off)

using namespace dfgpu;

enum { CO_COUNT = 0, CO_MEAN_A = 1, CO_MEAN_B = 2, CO_M2_A = 3, CO_M2_B = 4, CO_C_AB = 5, CO_CELLS = 6 };

struct dfgpu_comoments {
  dfgpu_ctx* ctx = nullptr; int kind = 0; int32_t in_type_a = 0, in_type_b = 0;
  int64_t n = 0, cap = 0;
  BufferPtr st[CO_CELLS];             // 8 B per group each; COVAR leaves CO_M2_A and CO_M2_B unallocated
  BufferPtr scratch; int64_t scratch_cap = 0;      // CoScratch's arrays, scratch_cap cells each; all zero between batches
};

namespace dfgpu {

constexpr int COMOMENTS_LDS_GROUPS = 1024;      // up to here the LDS path
constexpr int COMOMENTS_LDS_SMALL = 512;        // up to here with the smaller arrays

static bool comoment_kind(int kind) { return kind >= DFGPU_AGG_COVAR_SAMP && kind <= DFGPU_AGG_REGR_SXY; }
static bool comoment_full(int kind) { return kind >= DFGPU_AGG_CORR; }              // carries m2_a and m2_b
static bool comoment_input(int32_t t) { return is_signed_int(t) || is_unsigned_int(t) || is_float(t); }
// the state columns of a kind, in the reference's order, as indices into dfgpu_comoments::st
static int comoment_columns(int kind, const int** order) {
  static const int covar[4] = {CO_COUNT, CO_MEAN_A, CO_MEAN_B, CO_C_AB};                                  // count, mean1, mean2, algo_const (covariance.rs:263-270)
  static const int corr[6] = {CO_COUNT, CO_MEAN_A, CO_M2_A, CO_MEAN_B, CO_M2_B, CO_C_AB};                 // count, mean1, m2_1, mean2, m2_2, algo_const (correlation.rs:152-161)
  static const int regr[6] = {CO_COUNT, CO_MEAN_B, CO_MEAN_A, CO_M2_B, CO_M2_A, CO_C_AB};                 // count, mean_x, mean_y, m2_x, m2_y, algo_const (regr.rs:254-262): x is argument 1
  if (!comoment_full(kind)) { *order = covar; return 4; }
  *order = kind == DFGPU_AGG_CORR ? corr : regr; return 6;
}

// order-preserving: a < b as bit patterns of the total order <=> float_key(a) < float_key(b); equal keys <=> equal bit patterns
__device__ inline uint64_t float_key(double x) { const uint64_t b = (uint64_t)__double_as_longlong(x); return (b >> 63) ? ~b : (b | 0x8000000000000000ull); }
__device__ inline double float_unkey(uint64_t k) { return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k)); }
__device__ inline uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) { const uint64_t o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
  return v;
}

// The weighted rows of a batch: value rows (col[0] = a, col[1] = b) or the state columns of a Partial stage, col[CO_*]
struct CoRows { ColView col[CO_CELLS]; int is_state, a_float, a_unsigned, b_float, b_unsigned; };
struct CoRow { uint64_t c; double mean_a, mean_b, m2_a, m2_b, c_ab; };
// per-batch scratch, `cap` cells each: N_b | S_a -> A_b | S_b -> B_b | max key a | max ~key a | max key b | max ~key b | C_b | M2_a | M2_b (the last two FULL only)
struct CoScratch { uint64_t* n; double *sa, *sb; uint64_t *hi_a, *lo_a, *hi_b, *lo_b; double *c, *qa, *qb; };

__device__ inline double co_value(const ColView& v, int64_t r, int is_f, int is_u) {               // cast(values, Float64) (covariance.rs:273-274)
  return is_f ? acc_cell_f64(v, r) : is_u ? (double)(uint64_t)acc_cell_int(v, r) : (double)(int64_t)acc_cell_int(v, r);
}
template <bool FULL> __device__ inline bool comoment_row(const CoRows& R, int64_t i, CoRow* o) {
  int64_t r0, r1;
  if (!cell_resolve(R.col[0], i, &r0)) return false;
  if (!R.is_state) {
    if (!cell_resolve(R.col[1], i, &r1)) return false;               // a pair counts only when both are valid (covariance.rs:291-293, correlation.rs:169-177, regr.rs:285-287)
    o->c = 1; o->m2_a = o->m2_b = o->c_ab = 0.0;
    o->mean_a = co_value(R.col[0], r0, R.a_float, R.a_unsigned); o->mean_b = co_value(R.col[1], r1, R.b_float, R.b_unsigned);
    return true;
  }
  const uint64_t cc = ((const uint64_t*)R.col[CO_COUNT].values)[r0];
  if (cc == 0) return false;                                          // covariance.rs:362-364, regr.rs:369-371
  int64_t r[CO_CELLS];
  for (int k = CO_MEAN_A; k < CO_CELLS; k++) { if (!FULL && (k == CO_M2_A || k == CO_M2_B)) continue; if (!cell_resolve(R.col[k], i, &r[k])) return false; }
  o->c = cc; o->mean_a = ((const double*)R.col[CO_MEAN_A].values)[r[CO_MEAN_A]]; o->mean_b = ((const double*)R.col[CO_MEAN_B].values)[r[CO_MEAN_B]];
  o->c_ab = ((const double*)R.col[CO_C_AB].values)[r[CO_C_AB]]; o->m2_a = o->m2_b = 0.0;
  if constexpr (FULL) { o->m2_a = ((const double*)R.col[CO_M2_A].values)[r[CO_M2_A]]; o->m2_b = ((const double*)R.col[CO_M2_B].values)[r[CO_M2_B]]; }
  return true;
}

// the row of lane i, or act = false: GID_NONE, filtered, out of range (flagged) and NULL rows take no part
template <bool FULL> __device__ inline bool comoment_load(const CoRows& R, const uint32_t* gids, const uint64_t* fbits, const uint64_t* fvalid, int64_t i, int64_t n, int64_t total,
                                                          uint32_t* flags, uint32_t* g, CoRow* row) {
  if (i >= n) return false;
  *g = gids[i];
  bool act = *g != GID_NONE && filter_pass(fbits, fvalid, i);
  if (act && (int64_t)*g >= total) { atomicOr(flags, DFGPU_FLAG_OOB); act = false; }
  return act && comoment_row<FULL>(R, i, row);
}

// PASS 1: N_b, S_a, S_b and the four extrema keys.  NS = 3 sums (the count among them), NK = 4 keys.
template <int LDS_GROUPS, bool FULL>        // LDS_GROUPS 0: the GLOBAL path
__global__ void __launch_bounds__(BLOCK) k_comoments_pass1(CoRows R, const uint32_t* gids, const uint64_t* fbits, const uint64_t* fvalid, int64_t n, int64_t total, CoScratch sc, uint32_t* flags) {
  constexpr bool LDS = LDS_GROUPS > 0; constexpr int G = LDS ? LDS_GROUPS : 1;
  __shared__ uint64_t s_n[G]; __shared__ double s_sa[G], s_sb[G]; __shared__ uint64_t s_k[4][G];
  if constexpr (LDS) {            // total <= LDS_GROUPS
    for (int g = threadIdx.x; g < total; g += BLOCK) { s_n[g] = 0; s_sa[g] = 0.0; s_sb[g] = 0.0; s_k[0][g] = s_k[1][g] = s_k[2][g] = s_k[3][g] = 0; }
    __syncthreads();
  }
  const int lane = lane_id();
  const int64_t n_round = (n + WAVE - 1) / WAVE * WAVE;             // whole waves enter every iteration: the ballots and shuffles need all lanes
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n_round; i += (int64_t)gridDim.x * BLOCK) {
    uint32_t g = GID_NONE; CoRow row{};
    const bool act = comoment_load<FULL>(R, gids, fbits, fvalid, i, n, total, flags, &g, &row);
    const uint64_t am = ballot64(act);
    if (am == 0) continue;                                           // wave-uniform
    uint64_t c = act ? row.c : 0; double xa = 0.0, xb = 0.0; uint64_t k[4] = {0, 0, 0, 0};      // zero is neutral for the sums and for the key maxima
    if (act) { xa = (double)c * row.mean_a; xb = (double)c * row.mean_b; k[0] = float_key(row.mean_a); k[1] = ~k[0]; k[2] = float_key(row.mean_b); k[3] = ~k[2]; }
    const int first = __ffsll((unsigned long long)am) - 1;
    const uint32_t g0 = __shfl(g, first, 64);
    bool add = act;
    if (ballot64(act && g != g0) == 0) {                             // every active lane carries g0: one add per wave
      c = wave_sum(c); xa = wave_sum(xa); xb = wave_sum(xb);
#pragma unroll
      for (int j = 0; j < 4; j++) k[j] = wave_max_u64(k[j]);
      add = lane == first;
    }
    if (!add) continue;
    if constexpr (LDS) {
      atomicAdd((unsigned long long*)&s_n[g], (unsigned long long)c); unsafeAtomicAdd(&s_sa[g], xa); unsafeAtomicAdd(&s_sb[g], xb);
#pragma unroll
      for (int j = 0; j < 4; j++) atomicMax((unsigned long long*)&s_k[j][g], (unsigned long long)k[j]);
    } else {
      atomicAdd((unsigned long long*)&sc.n[g], (unsigned long long)c); unsafeAtomicAdd(&sc.sa[g], xa); unsafeAtomicAdd(&sc.sb[g], xb);
      atomicMax((unsigned long long*)&sc.hi_a[g], (unsigned long long)k[0]); atomicMax((unsigned long long*)&sc.lo_a[g], (unsigned long long)k[1]);
      atomicMax((unsigned long long*)&sc.hi_b[g], (unsigned long long)k[2]); atomicMax((unsigned long long*)&sc.lo_b[g], (unsigned long long)k[3]);
    }
  }
  if constexpr (LDS) {
    __syncthreads();
    for (int g = threadIdx.x; g < total; g += BLOCK) {
      const uint64_t c = s_n[g];
      if (c == 0) continue;                                          // no row of this workgroup
      atomicAdd((unsigned long long*)&sc.n[g], (unsigned long long)c); unsafeAtomicAdd(&sc.sa[g], s_sa[g]); unsafeAtomicAdd(&sc.sb[g], s_sb[g]);
      atomicMax((unsigned long long*)&sc.hi_a[g], (unsigned long long)s_k[0][g]); atomicMax((unsigned long long*)&sc.lo_a[g], (unsigned long long)s_k[1][g]);
      atomicMax((unsigned long long*)&sc.hi_b[g], (unsigned long long)s_k[2][g]); atomicMax((unsigned long long*)&sc.lo_b[g], (unsigned long long)s_k[3][g]);
    }
  }
}

// S_a, S_b -> the batch means A_b, B_b, in place: the one value every row carried where the largest and the smallest key are equal, else S / N_b
__global__ void __launch_bounds__(BLOCK) k_comoments_means(CoScratch sc, int64_t total) {
  const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (g >= total) return;
  const uint64_t c = sc.n[g];
  if (c == 0) return;
  const uint64_t ha = sc.hi_a[g], la = ~sc.lo_a[g], hb = sc.hi_b[g], lb = ~sc.lo_b[g];
  sc.sa[g] = ha == la ? float_unkey(ha) : sc.sa[g] / (double)c;
  sc.sb[g] = hb == lb ? float_unkey(hb) : sc.sb[g] / (double)c;
}

// PASS 2: C_b and, FULL, M2_a and M2_b; the batch means are read from the row's group (the row counted in pass 1: N_b >= 1)
template <int LDS_GROUPS, bool FULL>
__global__ void __launch_bounds__(BLOCK) k_comoments_pass2(CoRows R, const uint32_t* gids, const uint64_t* fbits, const uint64_t* fvalid, int64_t n, int64_t total, CoScratch sc, uint32_t* flags) {
  constexpr bool LDS = LDS_GROUPS > 0; constexpr int G = LDS ? LDS_GROUPS : 1;
  __shared__ double s_c[G]; __shared__ double s_qa[FULL ? G : 1], s_qb[FULL ? G : 1];
  if constexpr (LDS) {
    for (int g = threadIdx.x; g < total; g += BLOCK) { s_c[g] = 0.0; if constexpr (FULL) { s_qa[g] = 0.0; s_qb[g] = 0.0; } }
    __syncthreads();
  }
  const int lane = lane_id();
  const int64_t n_round = (n + WAVE - 1) / WAVE * WAVE;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n_round; i += (int64_t)gridDim.x * BLOCK) {
    uint32_t g = GID_NONE; CoRow row{};
    const bool act = comoment_load<FULL>(R, gids, fbits, fvalid, i, n, total, flags, &g, &row);
    const uint64_t am = ballot64(act);
    if (am == 0) continue;
    double xc = 0.0, xqa = 0.0, xqb = 0.0;
    if (act) {
      const double w = (double)row.c, da = row.mean_a - sc.sa[g], db = row.mean_b - sc.sb[g];
      xc = row.c_ab + w * da * db;
      if constexpr (FULL) { xqa = row.m2_a + w * da * da; xqb = row.m2_b + w * db * db; }
    }
    const int first = __ffsll((unsigned long long)am) - 1;
    const uint32_t g0 = __shfl(g, first, 64);
    bool add = act;
    if (ballot64(act && g != g0) == 0) {
      xc = wave_sum(xc); if constexpr (FULL) { xqa = wave_sum(xqa); xqb = wave_sum(xqb); }
      add = lane == first;
    }
    if (!add) continue;
    if constexpr (LDS) { unsafeAtomicAdd(&s_c[g], xc); if constexpr (FULL) { unsafeAtomicAdd(&s_qa[g], xqa); unsafeAtomicAdd(&s_qb[g], xqb); } }
    else { unsafeAtomicAdd(&sc.c[g], xc); if constexpr (FULL) { unsafeAtomicAdd(&sc.qa[g], xqa); unsafeAtomicAdd(&sc.qb[g], xqb); } }
  }
  if constexpr (LDS) {
    __syncthreads();
    for (int g = threadIdx.x; g < total; g += BLOCK) {
      const double xc = s_c[g]; if (xc != 0.0) unsafeAtomicAdd(&sc.c[g], xc);                // NaN != 0: it is added
      if constexpr (FULL) { const double xa = s_qa[g], xb = s_qb[g]; if (xa != 0.0) unsafeAtomicAdd(&sc.qa[g], xa); if (xb != 0.0) unsafeAtomicAdd(&sc.qb[g], xb); }
    }
  }
}

// one mean of the merge (covariance.rs:366-369), except that a batch mean equal to the stored one leaves it as it is: the formula drifts in the last place
__device__ inline double co_merge_mean(double m0, double c0, double mb, double c, double nc) { return mb == m0 ? m0 : m0 * c0 / nc + mb * c / nc; }

// merge_batch of ONE state row per touched group (covariance.rs:365-379, variance.rs:290-300), scratch cleared for the next batch
template <bool FULL>
__global__ void __launch_bounds__(BLOCK) k_comoments_fold(CoScratch sc, int64_t total, uint64_t* count, double* mean_a, double* mean_b, double* m2_a, double* m2_b, double* c_ab) {
  const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (g >= total) return;
  const uint64_t c = sc.n[g];
  if (c == 0) return;                       // no row of the batch: the other cells are untouched zeros
  const double ab = sc.sa[g], bb = sc.sb[g], cb = sc.c[g]; double qa = 0.0, qb = 0.0;
  if constexpr (FULL) { qa = sc.qa[g]; qb = sc.qb[g]; sc.qa[g] = 0.0; sc.qb[g] = 0.0; }
  sc.n[g] = 0; sc.sa[g] = 0.0; sc.sb[g] = 0.0; sc.hi_a[g] = 0; sc.lo_a[g] = 0; sc.hi_b[g] = 0; sc.lo_b[g] = 0; sc.c[g] = 0.0;
  const uint64_t c0 = count[g];
  if (c0 == 0) {                            // the group's first rows: the batch is the state (0 * c0 / nc + mb * c / nc need not give mb back)
    count[g] = c; mean_a[g] = ab; mean_b[g] = bb; c_ab[g] = cb;
    if constexpr (FULL) { m2_a[g] = qa; m2_b[g] = qb; }
    return;
  }
  const uint64_t nc = c0 + c; const double f0 = (double)c0, fb = (double)c, fn = (double)nc;
  const double a0 = mean_a[g], b0 = mean_b[g], da = a0 - ab, db = b0 - bb;
  count[g] = nc; mean_a[g] = co_merge_mean(a0, f0, ab, fb, fn); mean_b[g] = co_merge_mean(b0, f0, bb, fb, fn);
  c_ab[g] = c_ab[g] + cb + da * db * f0 * fb / fn;
  if constexpr (FULL) { m2_a[g] = m2_a[g] + qa + da * da * f0 * fb / fn; m2_b[g] = m2_b[g] + qb + db * db * f0 * fb / fn; }
}

// evaluate.  COVAR (covariance.rs:384-401): c_ab / count or c_ab / (count - 1), NULL when that divisor is 0.  CORR (correlation.rs:218-236 over variance.rs:305-328,
// stddev.rs:223-232): NULL at count 0; 0.0 at count 1 (a population stddev of one row is 0.0) and when s1 or s2 is 0.0; else c / s1 / s2.  REGR_* (regr.rs:420-460).
__global__ void __launch_bounds__(BLOCK) k_comoments_evaluate(const uint64_t* count, const double* mean_a, const double* mean_b, const double* m2_a, const double* m2_b, const double* c_ab,
                                                              int64_t n, int kind, double* out, uint64_t* valid) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  bool ok = false;
  if (i < n) {
    const uint64_t c = count[i]; const double fc = (double)c, cab = c_ab[i]; double v = 0.0;
    if (kind == DFGPU_AGG_COVAR_POP) { ok = c > 0; if (ok) v = cab / fc; }
    else if (kind == DFGPU_AGG_COVAR_SAMP) { ok = c > 1; if (ok) v = cab / (double)(c - 1); }
    else if (kind == DFGPU_AGG_CORR) {
      ok = c > 0;
      if (c > 1) { const double cv = cab / fc, s1 = sqrt(m2_a[i] / fc), s2 = sqrt(m2_b[i] / fc); v = (s1 == 0.0 || s2 == 0.0) ? 0.0 : cv / s1 / s2; }
    } else {                                                           // a = y, b = x
      const double cov = cab / fc, var_x = m2_b[i] / fc, var_y = m2_a[i] / fc;
      switch (kind) {
        case DFGPU_AGG_REGR_SLOPE: ok = !(c <= 1 || var_x == 0.0); v = cov / var_x; break;
        case DFGPU_AGG_REGR_INTERCEPT: { const double slope = cov / var_x; ok = !(c <= 1 || var_x == 0.0); v = mean_a[i] - slope * mean_b[i]; break; }
        case DFGPU_AGG_REGR_COUNT: ok = true; v = fc; break;
        case DFGPU_AGG_REGR_R2: ok = !(c <= 1 || var_x == 0.0 || var_y == 0.0); v = (cov * cov) / (var_x * var_y); break;
        case DFGPU_AGG_REGR_AVGX: ok = c >= 1; v = mean_b[i]; break;
        case DFGPU_AGG_REGR_AVGY: ok = c >= 1; v = mean_a[i]; break;
        case DFGPU_AGG_REGR_SXX: ok = c >= 1; v = m2_b[i]; break;
        case DFGPU_AGG_REGR_SYY: ok = c >= 1; v = m2_a[i]; break;
        default: ok = c >= 1; v = cab; break;                          // REGR_SXY
      }
      if (!ok) v = 0.0;
    }
    out[i] = v;
  }
  const uint64_t m = ballot64(ok);
  if (lane_id() == 0 && i < n) valid[i >> 6] = m;
}

static int comoment_scratch_cells(const dfgpu_comoments* m) { return comoment_full(m->kind) ? 10 : 8; }
static CoScratch comoment_scratch(const dfgpu_comoments* m) {
  CoScratch s{};
  if (!m->scratch) return s;              // no group known: every id is out of range and no cell is touched
  uint64_t* p = (uint64_t*)m->scratch->ptr; const int64_t w = m->scratch_cap;
  s.n = p; s.sa = (double*)(p + w); s.sb = (double*)(p + 2 * w); s.hi_a = p + 3 * w; s.lo_a = p + 4 * w; s.hi_b = p + 5 * w; s.lo_b = p + 6 * w; s.c = (double*)(p + 7 * w);
  if (comoment_full(m->kind)) { s.qa = (double*)(p + 8 * w); s.qb = (double*)(p + 9 * w); }
  return s;
}

static void comoments_resize(dfgpu_comoments* m, int64_t total) {
  dfgpu_ctx* ctx = m->ctx;
  if (total <= m->n) return;
  const bool full = comoment_full(m->kind);
  if (total > m->cap) {
    int64_t nc = m->cap ? m->cap : 1024; while (nc < total) nc *= 2;
    for (int k = 0; k < CO_CELLS; k++) {
      if (!full && (k == CO_M2_A || k == CO_M2_B)) continue;
      BufferPtr b = alloc_buffer(ctx, (size_t)nc * 8);
      if (m->n) HIP_CHECK(hipMemcpyAsync(b->ptr, m->st[k]->ptr, (size_t)m->n * 8, hipMemcpyDeviceToDevice, ctx->stream));
      m->st[k] = b;
    }
    m->cap = nc;
  }
  const size_t at = (size_t)m->n * 8, add = (size_t)(total - m->n) * 8;        // all-zero bits: count 0, every f64 cell 0.0
  for (int k = 0; k < CO_CELLS; k++) if (m->st[k]) HIP_CHECK(hipMemsetAsync((char*)m->st[k]->ptr + at, 0, add, ctx->stream));
  if (m->cap > m->scratch_cap) { m->scratch = alloc_buffer(ctx, (size_t)m->cap * 8 * comoment_scratch_cells(m), true); m->scratch_cap = m->cap; }      // the old scratch held zeros only
  m->n = total;
}

// One batch of weighted rows into the state: grow, pass 1, means, pass 2, fold.  A zero-row batch grows the state.
template <int LDS_GROUPS, bool FULL> static void comoments_launch(dfgpu_ctx* ctx, dfgpu_comoments* m, const CoRows& R, const dfgpu_array* gids, const dfgpu_array* filt, int64_t total) {
  const int64_t n = gids->length; constexpr bool lds = LDS_GROUPS > 0;
  const dim3 grid(lds ? grid_for(n, BLOCK * 32, ctx->num_cus * 4) : grid_for(n, BLOCK * 8, ctx->num_cus * 8));       // LDS: >= 8192 rows per workgroup amortise the flush
  const uint32_t* ids = (const uint32_t*)gids->values->ptr;
  const uint64_t* fb = filt ? (const uint64_t*)filt->values->ptr : nullptr; const uint64_t* fv = filt && filt->validity ? (const uint64_t*)filt->validity->ptr : nullptr;
  const CoScratch sc = comoment_scratch(m);
  hipLaunchKernelGGL((k_comoments_pass1<LDS_GROUPS, FULL>), grid, dim3(BLOCK), 0, ctx->stream, R, ids, fb, fv, n, total, sc, ctx->d_flags);
  if (total == 0) return;                 // every row was out of range: flagged, nothing else to do
  hipLaunchKernelGGL(k_comoments_means, dim3(grid_for(total, BLOCK)), dim3(BLOCK), 0, ctx->stream, sc, total);
  hipLaunchKernelGGL((k_comoments_pass2<LDS_GROUPS, FULL>), grid, dim3(BLOCK), 0, ctx->stream, R, ids, fb, fv, n, total, sc, ctx->d_flags);
  hipLaunchKernelGGL(k_comoments_fold<FULL>, dim3(grid_for(total, BLOCK)), dim3(BLOCK), 0, ctx->stream, sc, total, (uint64_t*)m->st[CO_COUNT]->ptr, (double*)m->st[CO_MEAN_A]->ptr,
                     (double*)m->st[CO_MEAN_B]->ptr, FULL ? (double*)m->st[CO_M2_A]->ptr : nullptr, FULL ? (double*)m->st[CO_M2_B]->ptr : nullptr, (double*)m->st[CO_C_AB]->ptr);
}
static void comoments_batch(dfgpu_ctx* ctx, dfgpu_comoments* m, const CoRows& R, const dfgpu_array* gids, const dfgpu_array* filt, int64_t total, const char* what) {
  if (total < 0) fail(DFGPU_INVALID_ARGUMENT, "%s: total_num_groups %lld", what, (long long)total);
  comoments_resize(m, total);
  if (gids->length == 0) return;
  materialize_ids(ctx, gids);
  KernelTimer kt_(ctx, "k_comoments_update");
  const bool full = comoment_full(m->kind);
  if (total <= COMOMENTS_LDS_SMALL) { if (full) comoments_launch<COMOMENTS_LDS_SMALL, true>(ctx, m, R, gids, filt, total); else comoments_launch<COMOMENTS_LDS_SMALL, false>(ctx, m, R, gids, filt, total); }
  else if (total <= COMOMENTS_LDS_GROUPS) { if (full) comoments_launch<COMOMENTS_LDS_GROUPS, true>(ctx, m, R, gids, filt, total); else comoments_launch<COMOMENTS_LDS_GROUPS, false>(ctx, m, R, gids, filt, total); }
  else { if (full) comoments_launch<0, true>(ctx, m, R, gids, filt, total); else comoments_launch<0, false>(ctx, m, R, gids, filt, total); }
  KERNEL_CHECK();
  check_flags(ctx, what);
}
static void check_comoment_batch_args(const dfgpu_array* gids, const dfgpu_array* filt) {
  if (gids->type != DFGPU_UINT32) fail(DFGPU_INVALID_ARGUMENT, "group ids must be a UINT32 array");
  if (filt && (filt->type != DFGPU_BOOL || filt->length != gids->length)) fail(DFGPU_INVALID_ARGUMENT, "opt_filter must be a Boolean array of the batch length");
}
static void check_comoment_values(const dfgpu_array* v, const dfgpu_array* gids, int32_t in_type, const char* which) {
  if (v->length != gids->length) fail(DFGPU_INVALID_ARGUMENT, "%s (%lld rows) and group ids (%lld rows) differ in length", which, (long long)v->length, (long long)gids->length);
  if (logical_type(v) != in_type) fail(DFGPU_INVALID_ARGUMENT, "accumulator created for input type %d got %s of type %d", in_type, which, logical_type(v));
}
static dfgpu_array* comoments_column(dfgpu_ctx* ctx, const dfgpu_comoments* m, int32_t type, const BufferPtr& src) {
  ArrayHolder h(new_fixed(ctx, type, m->n));
  if (m->n) HIP_CHECK(hipMemcpyAsync(h.get()->values->ptr, src->ptr, (size_t)m->n * 8, hipMemcpyDeviceToDevice, ctx->stream));
  h.get()->null_count = 0;
  return h.release();
}

}  // namespace dfgpu

extern "C" {

dfgpu_status dfgpu_comoments_new(dfgpu_ctx* ctx, int32_t kind, int32_t in_type_a, int32_t in_type_b, dfgpu_comoments** out) {
  return guard(ctx, [&] {
    if (!out) fail(DFGPU_INVALID_ARGUMENT, "comoments_new: null argument");
    if (!comoment_kind(kind)) fail(DFGPU_INVALID_ARGUMENT, "comoments_new: aggregate kind %d is not COVAR_SAMP / COVAR_POP / CORR / REGR_*", kind);
    if (!comoment_input(in_type_a) || !comoment_input(in_type_b)) fail(DFGPU_NOT_IMPLEMENTED, "aggregate kind %d over types (%d, %d)", kind, in_type_a, in_type_b);
    std::unique_ptr<dfgpu_comoments> m(new dfgpu_comoments()); m->ctx = ctx; m->kind = kind; m->in_type_a = in_type_a; m->in_type_b = in_type_b;
    *out = m.release();
  });
}
void dfgpu_comoments_free(dfgpu_comoments* m) { delete m; }
int64_t dfgpu_comoments_size(const dfgpu_comoments* m) { return m ? (m->cap * (comoment_full(m->kind) ? 6 : 4) + m->scratch_cap * comoment_scratch_cells(m)) * 8 : 0; }

dfgpu_status dfgpu_comoments_update_batch(dfgpu_ctx* ctx, dfgpu_comoments* m, const dfgpu_array* values_a, const dfgpu_array* values_b, const dfgpu_array* gids, const dfgpu_array* filt, int64_t total) {
  return guard(ctx, [&] {
    if (!m || !gids) fail(DFGPU_INVALID_ARGUMENT, "comoments_update_batch: null argument");
    check_comoment_batch_args(gids, filt);
    if (gids->length == 0) { comoments_batch(ctx, m, CoRows{}, gids, filt, total, "comoments_update_batch"); return; }      // self.values.resize(total_num_groups, ..) with nothing to accumulate; the values may be NULL
    if (!values_a || !values_b) fail(DFGPU_INVALID_ARGUMENT, "comoments_update_batch: both value arrays required");
    check_comoment_values(values_a, gids, m->in_type_a, "first values"); check_comoment_values(values_b, gids, m->in_type_b, "second values");
    CoRows R{}; R.col[0] = make_view(values_a); R.col[1] = make_view(values_b);
    R.a_float = is_float(m->in_type_a); R.a_unsigned = is_unsigned_int(m->in_type_a); R.b_float = is_float(m->in_type_b); R.b_unsigned = is_unsigned_int(m->in_type_b);
    comoments_batch(ctx, m, R, gids, filt, total, "comoments_update_batch");
  });
}

dfgpu_status dfgpu_comoments_merge_batch(dfgpu_ctx* ctx, dfgpu_comoments* m, const dfgpu_array* const* st, int32_t nst, const dfgpu_array* gids, const dfgpu_array* filt, int64_t total) {
  return guard(ctx, [&] {
    if (!m || !st || !gids) fail(DFGPU_INVALID_ARGUMENT, "comoments_merge_batch: null argument");
    const int* order; const int want = comoment_columns(m->kind, &order);
    // nothing is merged unless every column can be
    bool good = nst == want;
    for (int k = 0; good && k < want; k++) good = st[k] && st[k]->type == (k == 0 ? DFGPU_UINT64 : DFGPU_FLOAT64);
    if (!good) fail(DFGPU_INVALID_ARGUMENT, "comoments merge of kind %d expects %d columns (UInt64 counts, then Float64)", m->kind, want);
    check_comoment_batch_args(gids, filt);
    for (int k = 0; k < want; k++) if (st[k]->length != gids->length)
      fail(DFGPU_INVALID_ARGUMENT, "state column %d (%lld rows) and group ids (%lld rows) differ in length", k, (long long)st[k]->length, (long long)gids->length);
    CoRows R{}; R.is_state = 1;
    for (int k = 0; k < want; k++) R.col[order[k]] = make_view(st[k]);
    comoments_batch(ctx, m, R, gids, filt, total, "comoments_merge_batch");
  });
}

dfgpu_status dfgpu_comoments_state(dfgpu_ctx* ctx, dfgpu_comoments* m, dfgpu_array** out_states) {
  return guard(ctx, [&] {
    if (!m || !out_states) fail(DFGPU_INVALID_ARGUMENT, "comoments_state: null argument");
    const int* order; const int want = comoment_columns(m->kind, &order);
    std::vector<ArrayHolder> cols;
    for (int k = 0; k < want; k++) cols.emplace_back(comoments_column(ctx, m, k == 0 ? DFGPU_UINT64 : DFGPU_FLOAT64, m->st[order[k]]));
    for (int k = 0; k < want; k++) out_states[k] = cols[k].release();
  });
}

dfgpu_status dfgpu_comoments_evaluate(dfgpu_ctx* ctx, dfgpu_comoments* m, dfgpu_array** out) {
  return guard(ctx, [&] {
    if (!m || !out) fail(DFGPU_INVALID_ARGUMENT, "comoments_evaluate: null argument");
    ArrayHolder h(new_fixed(ctx, DFGPU_FLOAT64, m->n, 0, 0, true));
    if (m->n) {
      const bool full = comoment_full(m->kind);
      hipLaunchKernelGGL(k_comoments_evaluate, dim3(grid_for(m->n, BLOCK)), dim3(BLOCK), 0, ctx->stream, (const uint64_t*)m->st[CO_COUNT]->ptr, (const double*)m->st[CO_MEAN_A]->ptr,
                         (const double*)m->st[CO_MEAN_B]->ptr, full ? (const double*)m->st[CO_M2_A]->ptr : nullptr, full ? (const double*)m->st[CO_M2_B]->ptr : nullptr,
                         (const double*)m->st[CO_C_AB]->ptr, m->n, m->kind, (double*)h.get()->values->ptr, (uint64_t*)h.get()->validity->ptr);
      KERNEL_CHECK();
    }
    h.get()->null_count = -1;
    *out = h.release();
  });
}

}  // extern "C"
