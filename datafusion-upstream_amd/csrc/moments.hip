// moments.hip -- a9: VAR_SAMP / VAR_POP / STDDEV_SAMP / STDDEV_POP per group for AggregateExec on gfx950 (dfgpu_moments, a handle of its own beside dfgpu_acc).
//
// Reference: physical-expr/src/aggregate/variance.rs:202-333 (VarianceAccumulator: state :234-240, update :242-259, merge :280-303, evaluate :305-328) and
// stddev.rs:202-235; row-at-a-time Accumulators behind GroupsAccumulatorAdapter.
//
// State lives in HBM, one slot per group: count (u64), mean (f64), m2 (f64); a group without a value holds (0, 0.0, 0.0).  update_batch and merge_batch are the same two
// passes over WEIGHTED ROWS -- a value row is (c = 1, mean = x cast `as f64`, m2 = 0), a state row is (c, mean, m2) and takes no part when c = 0 -- into a per-batch
// scratch of three 8-byte cells per group, which k_moments_fold then merges into the state:
//   pass 1  N_b = sum c, S_b = sum c * mean
//   pass 2  M2_b = sum (m2 + c * (mean - S_b / N_b)^2), S_b / N_b read from the row's group
//   fold    one thread per group: (N_b, S_b / N_b, M2_b) into (count, mean, m2) by the reference's merge formula (variance.rs:290-300); N_b = 0 is skipped, the scratch cleared
// Several rows of a batch may carry one group (Final sees a partial row per input partition): sums are atomic, a per-row merge of a three-word state is not.  The values and
// the group ids are read twice: 24 B per Float64 row against SUM's 12.  A batch of `total` known groups takes ONE path (moments_pass):
//   LDS     total <= MOMENTS_LDS_GROUPS (1024: 16 KiB of LDS in pass 1, 8 KiB in pass 2): per-workgroup partials of the pass's cells; a wave whose active lanes all carry
//           one group id adds once after a wave_sum (no GROUP BY, few groups), else every lane does an LDS atomic; one global atomic per touched group and cell at the end
//   GLOBAL  otherwise: the same wave-uniform shortcut, else one global atomic per row and cell
// The results depend on the order of the rows in the reference too (Welford's recurrence): <= 1e-9 relative; NULL-ness, counts and the 0.0 at count 1 are exact.
#include "acc_cells.h"
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

using namespace dfgpu;

struct dfgpu_moments {
  dfgpu_ctx* ctx = nullptr; int kind = 0; int32_t in_type = 0;
  int64_t n = 0, cap = 0;
  BufferPtr count, mean, m2;          // 8 B per group each
  BufferPtr scratch; int64_t scratch_cap = 0;      // N_b | S_b | M2_b, scratch_cap cells each; all zero between batches
};

namespace dfgpu {

constexpr int MOMENTS_LDS_GROUPS = 1024;

// The weighted rows of a batch: values (v alone) or the three state columns of a Partial stage (v = counts)
struct MomentRows { ColView v, mean, m2; int is_state, in_float, in_unsigned; };

__device__ inline bool moment_row(const MomentRows& R, int64_t i, uint64_t* c, double* mean, double* m2) {
  int64_t r;
  if (!cell_resolve(R.v, i, &r)) return false;
  if (!R.is_state) {              // cast(values, Float64) (variance.rs:243)
    *c = 1; *m2 = 0.0;
    *mean = R.in_float ? acc_cell_f64(R.v, r) : R.in_unsigned ? (double)(uint64_t)acc_cell_int(R.v, r) : (double)(int64_t)acc_cell_int(R.v, r);
    return true;
  }
  const uint64_t cc = ((const uint64_t*)R.v.values)[r];
  int64_t rm, rq;
  if (cc == 0 || !cell_resolve(R.mean, i, &rm) || !cell_resolve(R.m2, i, &rq)) return false;       // variance.rs:287-289
  *c = cc; *mean = ((const double*)R.mean.values)[rm]; *m2 = ((const double*)R.m2.values)[rq];
  return true;
}

// PASS 1 adds (c, c * mean) to (cell_n, cell_x) = (N_b, S_b); PASS 2 adds m2 + c * (mean - mean_b)^2 to cell_x = M2_b and reads N_b, S_b
template <int PASS, bool LDS>
__global__ void __launch_bounds__(BLOCK) k_moments_pass(MomentRows R, const uint32_t* gids, const uint64_t* fbits, const uint64_t* fvalid, int64_t n, int64_t total,
                                                        uint64_t* sc_n, double* sc_s, double* sc_m2, uint32_t* flags) {
  __shared__ uint64_t s_n[LDS && PASS == 1 ? MOMENTS_LDS_GROUPS : 1]; __shared__ double s_x[LDS ? MOMENTS_LDS_GROUPS : 1];
  double* const cell_x = PASS == 1 ? sc_s : sc_m2;
  if constexpr (LDS) {            // total <= MOMENTS_LDS_GROUPS
    for (int g = threadIdx.x; g < total; g += BLOCK) { if constexpr (PASS == 1) s_n[g] = 0; s_x[g] = 0.0; }
    __syncthreads();
  }
  const int lane = lane_id();
  const int64_t n_round = (n + WAVE - 1) / WAVE * WAVE;             // whole waves enter every iteration: the ballots and shuffles need all lanes
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n_round; i += (int64_t)gridDim.x * BLOCK) {
    uint32_t g = GID_NONE; uint64_t c = 0; double mean = 0.0, m2 = 0.0; bool act = false;
    if (i < n) {
      g = gids[i];
      act = g != GID_NONE && filter_pass(fbits, fvalid, i);
      if (act && (int64_t)g >= total) { atomicOr(flags, DFGPU_FLAG_OOB); act = false; }
      if (act) act = moment_row(R, i, &c, &mean, &m2);
    }
    const uint64_t am = ballot64(act);
    if (am == 0) continue;                                           // wave-uniform
    double x = 0.0;
    if (act) {
      if constexpr (PASS == 1) x = (double)c * mean;
      else { const double d = mean - sc_s[g] / (double)sc_n[g]; x = m2 + (double)c * d * d; }       // the row counted in pass 1: N_b >= 1
    } else c = 0;
    const int first = __ffsll((unsigned long long)am) - 1;
    const uint32_t g0 = __shfl(g, first, 64);
    bool add = act;
    if (ballot64(act && g != g0) == 0) {                             // every active lane carries g0: one add per wave
      x = wave_sum(x); if constexpr (PASS == 1) c = wave_sum(c);
      add = lane == first;
    }
    if (!add) continue;
    if constexpr (LDS) { if constexpr (PASS == 1) atomicAdd((unsigned long long*)&s_n[g], (unsigned long long)c); unsafeAtomicAdd(&s_x[g], x); }
    else { if constexpr (PASS == 1) atomicAdd((unsigned long long*)&sc_n[g], (unsigned long long)c); unsafeAtomicAdd(&cell_x[g], x); }
  }
  if constexpr (LDS) {
    __syncthreads();
    for (int g = threadIdx.x; g < total; g += BLOCK) {
      if constexpr (PASS == 1) { const uint64_t c = s_n[g]; if (c) { atomicAdd((unsigned long long*)&sc_n[g], (unsigned long long)c); unsafeAtomicAdd(&cell_x[g], s_x[g]); } }
      else { const double x = s_x[g]; if (x != 0.0) unsafeAtomicAdd(&cell_x[g], x); }        // NaN != 0: it is added
    }
  }
}

// merge_batch of ONE state row per touched group (variance.rs:290-300), scratch cleared for the next batch
__global__ void __launch_bounds__(BLOCK) k_moments_fold(uint64_t* sc_n, double* sc_s, double* sc_m2, int64_t total, uint64_t* count, double* mean, double* m2) {
  const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (g >= total) return;
  const uint64_t c = sc_n[g];
  if (c == 0) return;                       // no row of the batch: S_b and M2_b are untouched zeros
  const double mb = sc_s[g] / (double)c, qb = sc_m2[g];
  sc_n[g] = 0; sc_s[g] = 0.0; sc_m2[g] = 0.0;
  const uint64_t c0 = count[g], nc = c0 + c; const double m0 = mean[g];
  const double nm = m0 * (double)c0 / (double)nc + mb * (double)c / (double)nc;
  const double delta = m0 - mb;
  const double nq = m2[g] + qb + delta * delta * (double)c0 * (double)c / (double)nc;
  count[g] = nc; mean[g] = nm; m2[g] = nq;
}

// evaluate (variance.rs:305-328, stddev.rs:223-232): count 0 -> NULL; count 1 -> 0.0 (population) / NULL (sample); else m2 / count or m2 / (count - 1), STDDEV its root
__global__ void __launch_bounds__(BLOCK) k_moments_evaluate(const uint64_t* count, const double* m2, int64_t n, int population, int root, double* out, uint64_t* valid) {
  const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  bool ok = false;
  if (i < n) {
    const uint64_t c = count[i]; double v = 0.0;
    ok = c > 1 || (c == 1 && population);
    if (c > 1) { v = m2[i] / (double)(population ? c : c - 1); if (root) v = sqrt(v); }
    out[i] = v;
  }
  const uint64_t m = ballot64(ok);
  if (lane_id() == 0 && i < n) valid[i >> 6] = m;
}

static bool moment_kind(int kind) { return kind >= DFGPU_AGG_VAR_SAMP && kind <= DFGPU_AGG_STDDEV_POP; }
static bool moment_input(int32_t t) { return is_signed_int(t) || is_unsigned_int(t) || is_float(t); }

static void moments_resize(dfgpu_moments* m, int64_t total) {
  dfgpu_ctx* ctx = m->ctx;
  if (total <= m->n) return;
  if (total > m->cap) {
    int64_t nc = m->cap ? m->cap : 1024; while (nc < total) nc *= 2;
    BufferPtr c = alloc_buffer(ctx, (size_t)nc * 8), a = alloc_buffer(ctx, (size_t)nc * 8), q = alloc_buffer(ctx, (size_t)nc * 8);
    if (m->n) { HIP_CHECK(hipMemcpyAsync(c->ptr, m->count->ptr, (size_t)m->n * 8, hipMemcpyDeviceToDevice, ctx->stream));
                HIP_CHECK(hipMemcpyAsync(a->ptr, m->mean->ptr, (size_t)m->n * 8, hipMemcpyDeviceToDevice, ctx->stream));
                HIP_CHECK(hipMemcpyAsync(q->ptr, m->m2->ptr, (size_t)m->n * 8, hipMemcpyDeviceToDevice, ctx->stream)); }
    m->count = c; m->mean = a; m->m2 = q; m->cap = nc;
  }
  const size_t at = (size_t)m->n * 8, add = (size_t)(total - m->n) * 8;        // all-zero bits: (0, 0.0, 0.0)
  HIP_CHECK(hipMemsetAsync((char*)m->count->ptr + at, 0, add, ctx->stream));
  HIP_CHECK(hipMemsetAsync((char*)m->mean->ptr + at, 0, add, ctx->stream));
  HIP_CHECK(hipMemsetAsync((char*)m->m2->ptr + at, 0, add, ctx->stream));
  if (m->cap > m->scratch_cap) { m->scratch = alloc_buffer(ctx, (size_t)m->cap * 24, true); m->scratch_cap = m->cap; }      // the old scratch held zeros only
  m->n = total;
}

template <int PASS> static void moments_pass(dfgpu_ctx* ctx, const MomentRows& R, const dfgpu_array* gids, const dfgpu_array* filt, int64_t total, uint64_t* sc_n, double* sc_s, double* sc_m2) {
  const int64_t n = gids->length; const bool lds = total <= MOMENTS_LDS_GROUPS;
  const dim3 grid(lds ? grid_for(n, BLOCK * 32, ctx->num_cus * 4) : grid_for(n, BLOCK * 8, ctx->num_cus * 8));       // LDS: >= 8192 rows per workgroup amortise the flush
  hipLaunchKernelGGL((lds ? k_moments_pass<PASS, true> : k_moments_pass<PASS, false>), grid, dim3(BLOCK), 0, ctx->stream, R, (const uint32_t*)gids->values->ptr,
                     filt ? (const uint64_t*)filt->values->ptr : nullptr, filt && filt->validity ? (const uint64_t*)filt->validity->ptr : nullptr, n, total, sc_n, sc_s, sc_m2, ctx->d_flags);
}

// One batch of weighted rows into the state: grow, pass 1, pass 2, fold.  A zero-row batch grows the state.
static void moments_batch(dfgpu_ctx* ctx, dfgpu_moments* m, const MomentRows& R, const dfgpu_array* gids, const dfgpu_array* filt, int64_t total, const char* what) {
  if (total < 0) fail(DFGPU_INVALID_ARGUMENT, "%s: total_num_groups %lld", what, (long long)total);
  moments_resize(m, total);
  if (gids->length == 0) return;
  materialize_ids(ctx, gids);
  KernelTimer kt_(ctx, "k_moments_update");
  uint64_t* sc_n = m->scratch ? (uint64_t*)m->scratch->ptr : nullptr;           // no group known: every id is out of range and no cell is touched
  double* sc_s = (double*)(sc_n + (sc_n ? m->scratch_cap : 0)); double* sc_m2 = sc_s + (sc_n ? m->scratch_cap : 0);
  moments_pass<1>(ctx, R, gids, filt, total, sc_n, sc_s, sc_m2);
  moments_pass<2>(ctx, R, gids, filt, total, sc_n, sc_s, sc_m2);
  if (total) hipLaunchKernelGGL(k_moments_fold, dim3(grid_for(total, BLOCK)), dim3(BLOCK), 0, ctx->stream, sc_n, sc_s, sc_m2, total, (uint64_t*)m->count->ptr, (double*)m->mean->ptr, (double*)m->m2->ptr);
  KERNEL_CHECK();
  check_flags(ctx, what);
}
static void check_moment_batch_args(const dfgpu_array* gids, const dfgpu_array* filt) {
  if (gids->type != DFGPU_UINT32) fail(DFGPU_INVALID_ARGUMENT, "group ids must be a UINT32 array");
  if (filt && (filt->type != DFGPU_BOOL || filt->length != gids->length)) fail(DFGPU_INVALID_ARGUMENT, "opt_filter must be a Boolean array of the batch length");
}
static dfgpu_array* moments_column(dfgpu_ctx* ctx, const dfgpu_moments* m, int32_t type, const BufferPtr& src) {
  ArrayHolder h(new_fixed(ctx, type, m->n));
  if (m->n) HIP_CHECK(hipMemcpyAsync(h.get()->values->ptr, src->ptr, (size_t)m->n * 8, hipMemcpyDeviceToDevice, ctx->stream));
  h.get()->null_count = 0;
  return h.release();
}

}  // namespace dfgpu

extern "C" {

dfgpu_status dfgpu_moments_new(dfgpu_ctx* ctx, int32_t kind, int32_t in_type, dfgpu_moments** out) {
  return guard(ctx, [&] {
    if (!out) fail(DFGPU_INVALID_ARGUMENT, "moments_new: null argument");
    if (!moment_kind(kind)) fail(DFGPU_INVALID_ARGUMENT, "moments_new: aggregate kind %d is not VAR_SAMP / VAR_POP / STDDEV_SAMP / STDDEV_POP", kind);
    if (!moment_input(in_type)) fail(DFGPU_NOT_IMPLEMENTED, "aggregate kind %d over type %d", kind, in_type);
    std::unique_ptr<dfgpu_moments> m(new dfgpu_moments()); m->ctx = ctx; m->kind = kind; m->in_type = in_type;
    *out = m.release();
  });
}
void dfgpu_moments_free(dfgpu_moments* m) { delete m; }
int64_t dfgpu_moments_size(const dfgpu_moments* m) { return m ? (m->cap + m->scratch_cap) * 24 : 0; }

dfgpu_status dfgpu_moments_update_batch(dfgpu_ctx* ctx, dfgpu_moments* m, const dfgpu_array* values, const dfgpu_array* gids, const dfgpu_array* filt, int64_t total) {
  return guard(ctx, [&] {
    if (!m || !gids) fail(DFGPU_INVALID_ARGUMENT, "moments_update_batch: null argument");
    check_moment_batch_args(gids, filt);
    if (gids->length == 0) { moments_batch(ctx, m, MomentRows{}, gids, filt, total, "moments_update_batch"); return; }      // self.values.resize(total_num_groups, ..) with nothing to accumulate; values may be NULL
    if (!values) fail(DFGPU_INVALID_ARGUMENT, "moments_update_batch: values required");
    if (values->length != gids->length) fail(DFGPU_INVALID_ARGUMENT, "values (%lld rows) and group ids (%lld rows) differ in length", (long long)values->length, (long long)gids->length);
    if (logical_type(values) != m->in_type) fail(DFGPU_INVALID_ARGUMENT, "accumulator created for input type %d got values of type %d", m->in_type, logical_type(values));
    MomentRows R{}; R.v = make_view(values); R.in_float = is_float(m->in_type); R.in_unsigned = is_unsigned_int(m->in_type);
    moments_batch(ctx, m, R, gids, filt, total, "moments_update_batch");
  });
}

dfgpu_status dfgpu_moments_merge_batch(dfgpu_ctx* ctx, dfgpu_moments* m, const dfgpu_array* const* st, int32_t nst, const dfgpu_array* gids, const dfgpu_array* filt, int64_t total) {
  return guard(ctx, [&] {
    if (!m || !st || !gids) fail(DFGPU_INVALID_ARGUMENT, "moments_merge_batch: null argument");
    // nothing is merged unless all three columns can be (the dfgpu_acc_merge_batch behaviour for AVG)
    if (nst != 3 || !st[0] || !st[1] || !st[2] || st[0]->type != DFGPU_UINT64 || st[1]->type != DFGPU_FLOAT64 || st[2]->type != DFGPU_FLOAT64)
      fail(DFGPU_INVALID_ARGUMENT, "moments merge expects (UInt64 counts, Float64 means, Float64 m2s)");
    check_moment_batch_args(gids, filt);
    for (int k = 0; k < 3; k++) if (st[k]->length != gids->length)
      fail(DFGPU_INVALID_ARGUMENT, "state column %d (%lld rows) and group ids (%lld rows) differ in length", k, (long long)st[k]->length, (long long)gids->length);
    MomentRows R{}; R.v = make_view(st[0]); R.mean = make_view(st[1]); R.m2 = make_view(st[2]); R.is_state = 1;
    moments_batch(ctx, m, R, gids, filt, total, "moments_merge_batch");
  });
}

dfgpu_status dfgpu_moments_state(dfgpu_ctx* ctx, dfgpu_moments* m, dfgpu_array** out_states) {
  return guard(ctx, [&] {
    if (!m || !out_states) fail(DFGPU_INVALID_ARGUMENT, "moments_state: null argument");
    ArrayHolder c(moments_column(ctx, m, DFGPU_UINT64, m->count)), a(moments_column(ctx, m, DFGPU_FLOAT64, m->mean)), q(moments_column(ctx, m, DFGPU_FLOAT64, m->m2));
    out_states[0] = c.release(); out_states[1] = a.release(); out_states[2] = q.release();
  });
}

dfgpu_status dfgpu_moments_evaluate(dfgpu_ctx* ctx, dfgpu_moments* m, dfgpu_array** out) {
  return guard(ctx, [&] {
    if (!m || !out) fail(DFGPU_INVALID_ARGUMENT, "moments_evaluate: null argument");
    ArrayHolder h(new_fixed(ctx, DFGPU_FLOAT64, m->n, 0, 0, true));
    if (m->n) {
      const int population = m->kind == DFGPU_AGG_VAR_POP || m->kind == DFGPU_AGG_STDDEV_POP, root = m->kind == DFGPU_AGG_STDDEV_SAMP || m->kind == DFGPU_AGG_STDDEV_POP;
      hipLaunchKernelGGL(k_moments_evaluate, dim3(grid_for(m->n, BLOCK)), dim3(BLOCK), 0, ctx->stream, (const uint64_t*)m->count->ptr, (const double*)m->m2->ptr, m->n, population, root,
                         (double*)h.get()->values->ptr, (uint64_t*)h.get()->validity->ptr);
      KERNEL_CHECK();
    }
    h.get()->null_count = -1;
    *out = h.release();
  });
}

}  // extern "C"
