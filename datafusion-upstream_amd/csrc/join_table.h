// join_table.h -- the build side of a HashJoinExec as the device sees it (shared by join.hip and pjoin.hip).
#pragma once
#include "device_utils.h"

namespace dfgpu {
// radix-partitioned build side (pjoin.hip): (key widened to 64 bits, original build row) grouped by partition of the key hash, sized so
// that one partition's open-addressing table fits 64 KB of LDS (two workgroups per CU; 128 KB at most)
struct PartitionedBuild {
  uint32_t P = 0; int sbits = 0;            // partitions; log2 of the LDS table slots
  int64_t rows = 0;                         // selected, non-NULL build rows
  BufferPtr recs;                           // RpRec12 {key lo, key hi, ref}[..], partition-major: ref = build row (unique keys) or group number (dups)
  BufferPtr starts;                         // u32[P + 1] over recs
  bool hashed = false;                      // record keys are keyset hashes of the key columns (any number, any type, NULLs under null_equals_null): a match is a candidate, verified against the columns
  bool dups = false;                        // a build key repeats: recs holds one record per DISTINCT key, the rows of a key are a CSR
  BufferPtr grp_start, grp_cnt, csr_rows;   // u32[groups] into csr_rows / rows of the group; u32[rows] build rows, ascending inside a group
};
enum class JoinRep { HASH, RANK, RANK_RUNS, PARTITIONED };        // what a dfgpu_join_table is (see there)
}  // namespace dfgpu

struct dfgpu_join_table {
  dfgpu_ctx* ctx = nullptr;
  int64_t n_build = 0; int32_t nkeys = 0; bool null_equals_null = false;
  std::vector<dfgpu_array*> keys; dfgpu::KeySet ks{};
  // What the table is, set once by the builder that took it (dfgpu_join_build tries them in this order):
  //   RANK         rank index (build_rank_index, build_rank_index_unsorted): unique single integer key, no hash table at all.  The bitmap IS the table:
  //                build row = rank of the key's bit among the set bits (word prefix + popcount), mapped through sel_rows when a build selection is fused
  //                or the keys are unsorted; rank_identity = the keys are key_min + row, so the row is the key offset.
  //   RANK_RUNS    the keys are non-decreasing WITH repeats (a sorted foreign key): sel_rows[r] = first build row of the r-th distinct key, its rows are
  //                the run up to sel_rows[r + 1] (or n_build) -- the CSR of the hash path without hashing or sorting
  //   PARTITIONED  probes of large batches run partition by partition out of LDS (part, pjoin.hip)
  //   HASH         the general open-addressing table (build_hash_table), with the membership bitmap in front when the key domain allows
  dfgpu::JoinRep rep = dfgpu::JoinRep::HASH;
  // The open-addressing table: HASH's own, or built by the first probe the table's representation cannot serve (a dictionary-encoded or otherwise
  // differently typed probe column, a batch below join_partitioned_min_probe).  Mutable: the probe holds the table const; a probe-built table changes
  // no result, only the path of later probes.
  mutable uint64_t capacity = 0; mutable int cap_bits = 0;
  mutable dfgpu::BufferPtr slots;        // u64[capacity]
  mutable dfgpu::BufferPtr slot_count;   // u32[capacity]   rows per key group
  mutable dfgpu::BufferPtr slot_start;   // u32[capacity]   CSR start (non-unique only)
  mutable dfgpu::BufferPtr csr_rows;     // u32[n_inserted] build rows ordered by (slot, row) (non-unique only)
  mutable bool unique = true;
  dfgpu::BufferPtr build_mask;   // effective opt_mask words or null
  dfgpu::BufferPtr visited;      // u64 words over n_build
  // exact membership bitmap over [key_min, key_min + range) for single integer keys with a dense domain: the probe tests
  // one bit (L2 / Infinity Cache resident, perfectly local for clustered keys) and touches the hash table for matches only.
  // A HASH build side that is tiny against its key range (a few thousand order keys out of 600 M) gets no bitmap up front but lazy_row_slot; a probe
  // batch of >= range / 16 rows builds the bitmap on arrival (clearing range / 8 bytes is then small against streaming the probe keys) and drops it.
  // Mutable with the hash table: the lazy bitmap arrives with a probe, and build_hash_table, which sets key_min / range at build time, also builds a probe's table.
  mutable dfgpu::BufferPtr bitmap, lazy_row_slot; mutable int64_t key_min = 0; mutable uint64_t range = 0;
  bool rank_identity = false;
  // key packing: 2..4 integer key columns whose value ranges multiply to < 2^40 are packed into ONE Int64 key (sum of (k - min) * stride):
  // tuple equality == packed equality, and the single-key paths (rank index, bitmap prefilter) apply.  The table then holds the packed
  // column as its only key; probes pack their tuples with the same parameters (a component outside the build range = NULL = no match).
  int pack_n = 0; int32_t pack_types[dfgpu::MAX_KEYS] = {0}; int64_t pack_min[dfgpu::MAX_KEYS] = {0}; uint64_t pack_range[dfgpu::MAX_KEYS] = {0}, pack_stride[dfgpu::MAX_KEYS] = {0};
  dfgpu::BufferPtr rank_prefix;  // u32[range / 64]   set bits before each bitmap word
  bool have_minmax = false; long long sel_min = 0, sel_max = 0;      // min / max of the selected build keys, once some builder has computed them
  dfgpu_array* sel_rows = nullptr;   // u32[selected] ascending build rows (masked builds only)
  std::unique_ptr<dfgpu::PartitionedBuild> part;   // PARTITIONED only
  mutable int64_t mem = 0;
  ~dfgpu_join_table() { for (auto* a : keys) dfgpu_array_release(a); if (sel_rows) dfgpu_array_release(sel_rows); }
};

namespace dfgpu {
// pjoin.hip
bool pj_build(dfgpu_ctx* ctx, dfgpu_join_table* t);      // false = not taken (nothing kept): a build the partitioned join is not for, or one it declines
bool pj_probe_eligible(dfgpu_ctx* ctx, const dfgpu_join_table* t, const dfgpu_array* const* probe_keys, int32_t nkeys, int64_t n);
void pj_probe(dfgpu_ctx* ctx, const dfgpu_join_table* t, const dfgpu_array* const* probe_keys, int32_t nkeys, const uint64_t* mask, dfgpu_array** out_build, dfgpu_array** out_probe);
// join.hip
void selected_key_range(dfgpu_ctx* ctx, const dfgpu_join_table* t, const char* sync, long long* lo, long long* hi);   // min / max of the selected non-NULL keys (lo > hi: none)

// The pairs of m matches that each emit a run of build rows: count(cnt) writes the run lengths (and whatever expand reads besides), their exclusive scan gives
// every match its first pair and the total (read back), then expand(cnt, offsets, out_build, out_probe) writes the pairs into ob / op.
template <typename Count, typename Expand>
void expand_matches(dfgpu_ctx* ctx, int64_t m, ArrayHolder& ob, ArrayHolder& op, Count&& count, Expand&& expand) {
  BufferPtr cnt = alloc_buffer(ctx, (size_t)(m + 1) * 4), offs = alloc_buffer(ctx, (size_t)(m + 1) * 8);
  int64_t total = 0;
  if (m) {
    count((uint32_t*)cnt->ptr);
    KERNEL_CHECK();
    exclusive_scan_u32(ctx, (const uint32_t*)cnt->ptr, (uint64_t*)offs->ptr, m, ctx->d_scratch64 + 8);
    total = (int64_t)read_scratch(ctx, 8);
  }
  if (total > 0xFFFFFFF0ll) fail(DFGPU_RESOURCES_EXHAUSTED, "join output of %lld rows for one probe batch; split the probe batch", (long long)total);
  ob.a = new_fixed(ctx, DFGPU_UINT64, total); op.a = new_fixed(ctx, DFGPU_UINT32, total);
  if (total) expand((const uint32_t*)cnt->ptr, (const uint64_t*)offs->ptr, (uint64_t*)ob.get()->values->ptr, (uint32_t*)op.get()->values->ptr);
  KERNEL_CHECK();
}
}  // namespace dfgpu
