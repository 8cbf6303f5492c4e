/*
 *  rerank_internal.h - what the calls over LISTED pairs share on the host (rerank.c: szs_rocm_rerank*; fuzzy_find.c:
 *  szs_rocm_fuzzy_find*; fuzzy_search.c: szs_rocm_fuzzy_search*, for its strings and its winners - its tiles and lists are
 *  selection_internal.h's): the block and staging budgets, the deal of a block's rows by descending query length, and the skeleton
 *  of such a call (listed_pairs.c): its preamble, the validation of indices, the scratch, the two sides as the kernels read them, and
 *  the bracket around a block's launches.  Policy stays with the callers: which engines, which lengths, what an unusable side means.
 */
#ifndef SZS_RERANK_INTERNAL_H_
#define SZS_RERANK_INTERNAL_H_

#include "szs_internal.h"

#include <string.h>

#define SZS_RERANK_STAGE_BYTES ((size_t)128 << 20) /* a block's dense copy of an array the device cannot reach */
#define SZS_RERANK_MOST_ROWS ((size_t)1 << 20)     /* rows of a block: bounds the kernel's row list */
#define SZS_RERANK_EMPTY (~(uint64_t)0)            /* SZ_SIZE_MAX: the empty slot top-k emits */

static inline uint64_t szs_tape_offset(szs_input_t const *input, void const *offsets, size_t i) {
    return input->kind == szs_input_u32tape_k ? ((uint32_t const *)offsets)[i] : ((uint64_t const *)offsets)[i];
}

/** What the blocks of one call over listed pairs share. */
typedef struct {
    szs_engine_s *engine;
    hipStream_t stream;
    int device;
    size_t k, row_stride, block;
    void const *offsets[2];  /* of the queries' tape and of the pool's, where the host can read them */
    szs_rerank_side_t sides[2];
    uint32_t *query_lengths; /* per query; ~0: more than the call takes, or offsets that descend */
    uint32_t *flags, *order, *device_order;
    uint64_t *landed;
    unsigned long long *device_counters;
    szs_rocm_call_profile_t total;
    /* the scratch of the two sides, between szs_listed_reserve and szs_listed_prepare_* */
    int refs_needed[2];
    size_t refs_count[2];
    uint64_t *addresses;
    uint32_t *gathered_lengths; /* of the side prepared last, where it needed refs */
    szs_string_ref_t *pinned_refs, *device_refs;
} szs_listed_call_t;

/** The preamble: binds the scope's GPU, makes the engine follow the device, creates the engine's event pair once per device. */
sz_status_t szs_listed_open(szs_listed_call_t *call, szs_engine_s *engine, szs_scope_s *scope, size_t k, size_t row_stride,
                            char const **error_message);

/** Is every index of `rows` rows of `k` slots, `row_stride` apart, empty or below `count`?  For indices the host can read: validated
 *  before anything is launched. */
int szs_listed_indices_ok(uint64_t const *indices, size_t rows, size_t k, size_t row_stride, size_t count);

/** The offsets of both tapes where the host can read them: as they are, or copied to the host - once per call.  `candidates` NULL:
 *  the self form, the pool is the queries. */
sz_status_t szs_listed_offsets(szs_listed_call_t *call, szs_input_t const *queries, szs_input_t const *candidates,
                               char const **error_message);

/** The rows of a block: what the kernel's row list takes and - `within_stage_budget` - what keeps a dense copy of k slots a row
 *  within SZS_RERANK_STAGE_BYTES. */
size_t szs_listed_block_rows(size_t q_count, size_t k, int within_stage_budget);

/**
 *  The scratch of a call, laid out in ONE place and reserved in the engine's rerank buffers (szs_internal.h: grow-only, released
 *  with the engine): query lengths, gathered addresses and lengths on the host; flags, landed counters, row list and refs in pinned
 *  memory; counters, row list and refs on the device.  The caller's extra parts - `host_extra` and `pinned_extra` bytes, two each -
 *  come back as `extras[0 .. 4)`.  `kernels` 0: no kernel will run - no refs, no device buffers.  `staged_arrays`: dense copies of a
 *  block x k array for what the device cannot reach.  `call->block` is set by the caller.
 */
sz_status_t szs_listed_reserve(szs_listed_call_t *call, szs_input_t const *queries, szs_input_t const *candidates, int kernels,
                               size_t const host_extra[2], size_t const pinned_extra[2], size_t staged_arrays, void *extras[4],
                               char const **error_message);

/** The queries as the kernels read them, and their lengths: ~0 for one of more than `longest_query` bytes or one whose offsets
 *  descend.  `*usable` 0: the kernels cannot reach the strings (or the side is malformed) - the lengths are not filled in. */
sz_status_t szs_listed_prepare_queries(szs_listed_call_t *call, szs_input_t const *queries, uint32_t longest_query, int *usable,
                                       char const **error_message);
/** The candidates as the kernels read them; NULL: the self form, the queries' side again. */
sz_status_t szs_listed_prepare_candidates(szs_listed_call_t *call, szs_input_t const *candidates, int *usable, char const **error_message);

/**
 *  The bracket around a block's launches, each step only while `error` is hipSuccess.  `begin`: clears the flags and the device's
 *  counters, uploads `dealt` rows of `order`, records the start.  `end`: records the stop, downloads the counters.  `finish`: drains
 *  the stream - a HIP error goes to `*hip_error` - maps the kernels' flags to a status (UNFIT: the caller's `unfit_status` and
 *  `unfit_message`), reads the elapsed time and adds the block to `call->total`: `launches`, the counters, `bytes_per_pair` of
 *  offsets, indices and outputs for every scored pair.  Staging copies between them stay with the caller.
 */
hipError_t szs_listed_block_begin(szs_listed_call_t *call, size_t dealt, hipError_t error);
hipError_t szs_listed_block_end(szs_listed_call_t *call, hipError_t error);
sz_status_t szs_listed_block_finish(szs_listed_call_t *call, hipError_t error, hipError_t *hip_error, unsigned launches, uint32_t longest,
                                    size_t bytes_per_pair, sz_status_t unfit_status, char const *unfit_message, char const **error_message);

/** The end of a call whose profile is `call->total` as it stands, behind its loop over the blocks: drains the stream - synchronous,
 *  also when the call fails - and reports `status` where a block failed (its message is set), else the HIP `error` of the blocks or of
 *  the drain; on success the engine's last profile becomes the sums over the call with the host time since `started`. */
sz_status_t szs_listed_close(szs_listed_call_t *call, sz_status_t status, hipError_t error, double started, char const **error_message);

/* ---- fuzzy find's own steps (fuzzy_find.c), which the search (fuzzy_search.c) runs on the rows it has found ---------------------- */

/** What the blocks of one fuzzy-find call share. */
typedef struct {
    szs_listed_call_t listed;
    uint64_t const *indices; /* NULL: the dense form */
    uint64_t *distances, *ends, *starts; /* `starts` NULL: the plain call - one launch a block */
    int stage_indices, stage_distances, stage_ends, stage_starts;
} szs_fuzzy_find_call_t;

/** Which of the call's arrays the device cannot reach (`stage_*`), from its pointers; returns the dense block x k copies they take. */
size_t szs_fuzzy_find_stage(szs_fuzzy_find_call_t *call);
/** Both sides as the kernels read them.  A query of more than SZS_RERANK_LONGEST_QUERY bytes (`long_query`: the message), offsets that
 *  descend and strings the device cannot read fail the call here, before anything is launched. */
sz_status_t szs_fuzzy_find_prepare(szs_fuzzy_find_call_t *call, szs_input_t const *queries, szs_input_t const *candidates,
                                   char const *long_query, char const **error_message);
/** Rows [q0, q0 + rows) - at most `listed.block` - of the call: one launch of hip/myers_fuzzy_find.hip, with `starts` the launch of
 *  hip/myers_fuzzy_spans.hip behind it; drains the stream and adds the block to `listed.total`. */
sz_status_t szs_fuzzy_find_block(szs_fuzzy_find_call_t *call, size_t q0, size_t rows, hipError_t *hip_error, char const **error_message);

/* ---- fuzzy scan's cut (fuzzy_scan.c), which the bounded scans (fuzzy_scan_matches.c) share ---------------------------------------- */

/** How a text of `n` bytes is cut for a block of `rows` rows: the bytes of a piece, the pieces, and the chunks of 64 pieces - the
 *  workgroups of a row.  Both constants are choices, not measurements. */
typedef struct {
    uint64_t piece, pieces, chunks;
} fuzzy_scan_cut_t;

fuzzy_scan_cut_t fuzzy_scan_cut(size_t rows, uint64_t n);

/**
 *  The rows of a block whose query has at most SZS_RERANK_LONGEST_QUERY bytes into `order`, longest query first (a counting sort of
 *  the lengths 256 ... 0): the rows of a wavefront then share a width.  `lengths`: the block's, ~0 where no kernel takes the row.
 */
static inline size_t szs_deal_short_rows(uint32_t const *lengths, size_t rows, uint32_t *order, uint32_t *longest) {
    uint32_t bins[SZS_RERANK_LONGEST_QUERY + 2];
    size_t dealt = 0;
    *longest = 0;
    memset(bins, 0, sizeof(bins));
    for (size_t r = 0; r < rows; ++r)
        if (lengths[r] <= SZS_RERANK_LONGEST_QUERY) ++bins[SZS_RERANK_LONGEST_QUERY - lengths[r] + 1], ++dealt;
    for (size_t b = 1; b < SZS_RERANK_LONGEST_QUERY + 2; ++b) bins[b] += bins[b - 1];
    for (size_t r = 0; r < rows; ++r) {
        if (lengths[r] > SZS_RERANK_LONGEST_QUERY) continue;
        order[bins[SZS_RERANK_LONGEST_QUERY - lengths[r]]++] = (uint32_t)r;
        if (lengths[r] > *longest) *longest = lengths[r];
    }
    return dealt;
}

#endif /* SZS_RERANK_INTERNAL_H_ */
