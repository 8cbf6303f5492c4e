/*
 *  fuzzy_scan_matches.c - the two BOUNDED scans of every query inside ONE long text, on one call path
 *  (include/stringzillas/stringzillas_rocm.h):
 *  - szs_rocm_fuzzy_scan_matches* (DESIGN.md section 4.12): EVERY end within a distance bound - counts[q] = the columns j in [1, n]
 *    with D[m][j] <= max_distance, and the leftmost `limit` of them as ends[q][i] = j, distances[q][i] = D[m][j];
 *  - szs_rocm_fuzzy_scan_occurrences* (section 4.13): ONE span per occurrence - counts[q] = the columns that also have D[m][j] <
 *    D[m][j - 1] and (j == n or D[m][j] <= D[m][j + 1]), the leftmost `limit` of them the same way and - where the call asks for them
 *    - starts[q][i] = szs_rocm_fuzzy_find_spans' start.
 *  The slots behind a row's count hold 2^64 - 1.
 *
 *  The call is the skeleton of listed_pairs.c (rerank_internal.h), as fuzzy_scan.c is, around the kernels that the entry's
 *  fuzzy_bounded_t names (hip/myers_fuzzy_matches.hip, hip/myers_fuzzy_occurrences.hip): per block the count, the offsets and - with
 *  limit > 0 - the fill of the matrices with 0xFF bytes, the write and, with `starts`, the reverse pass, on one stream inside one event
 *  pair.  The text is cut by fuzzy_scan.c's own rule (fuzzy_scan_cut: the same pieces, the same knob, the same probe).  Outputs the
 *  device cannot reach are staged densely per block and copied home.  The scratch - 64 piece counts and one chunk count per (row,
 *  chunk) - lies in the engine's staging buffer, ahead of the staged outputs.
 */
#include "rerank_internal.h"

#define SZS_FUZZY_MATCHES_MOST_LIMIT ((size_t)1 << 24)          /* a choice, not a measurement: one row of outputs is then 256 MiB */
#define SZS_FUZZY_MATCHES_SCRATCH_BYTES ((uint64_t)256 << 20)   /* a block's piece and chunk counts; a choice, not a measurement */
#define SZS_FUZZY_MATCHES_MOST_WORKGROUPS ((uint64_t)0x7FFFFFFF) /* the grid of a launch */
#define SZS_FUZZY_MATCHES_LANES 64u                              /* the pieces of a chunk */

/** What tells one bounded scan from the other. */
typedef struct {
    int (*count)(szs_rerank_side_t const *, uint64_t, uint32_t, void const *, uint64_t, uint64_t, uint32_t, uint32_t *, uint32_t *, uint32_t *,
                 unsigned long long *, void *);
    int (*write)(szs_rerank_side_t const *, uint64_t, uint32_t, void const *, uint64_t, uint64_t, uint32_t, uint32_t, uint32_t const *,
                 uint32_t const *, uint64_t *, uint64_t *, uint32_t *, unsigned long long *, void *);
    int with_starts; /* a fourth output may be asked for, and the blocks fit the grid of its launch whether it is or not */
    char const *most_limit, *engine, *long_query;
} fuzzy_bounded_t;

static fuzzy_bounded_t const fuzzy_matches = {
    szs_hip_levenshtein_fuzzy_matches_count, szs_hip_levenshtein_fuzzy_matches_write, 0, "The limit must be at most 2^24 matches a query",
    "Fuzzy scan matches needs an initialized unit-cost byte Levenshtein engine",
    "A query of more than 256 bytes: beyond what fuzzy scan matches takes"};
static fuzzy_bounded_t const fuzzy_occurrences = {
    szs_hip_levenshtein_fuzzy_occurrences_count, szs_hip_levenshtein_fuzzy_occurrences_write, 1,
    "The limit must be at most 2^24 occurrences a query", "Fuzzy scan occurrences needs an initialized unit-cost byte Levenshtein engine",
    "A query of more than 256 bytes: beyond what fuzzy scan occurrences takes"};

/** What the blocks of one call share. */
typedef struct {
    szs_fuzzy_find_call_t find; /* its `listed` and the queries' side; nothing else of it is used */
    fuzzy_bounded_t const *which;
    void const *text;
    uint64_t text_length;
    fuzzy_scan_cut_t cut;
    uint32_t bound;
    size_t limit;
    uint64_t *outputs[4];                  /* the caller's counts, distances, ends, starts; a matrix NULL where the call has none */
    int stage[4];                          /* the device cannot reach it */
    uint32_t *piece_counts, *chunk_counts; /* device: block x chunks x 64 and block x chunks dwords */
    uint64_t *staged;                      /* device: dense outputs of a block, where the device cannot reach the caller's */
} fuzzy_bounded_call_t;

/** The bytes of a block's scratch - 64 piece counts and one chunk count per (row, chunk) - a multiple of 16. */
static uint64_t fuzzy_matches_scratch(uint64_t rows, uint64_t chunks) {
    return (rows * chunks * (SZS_FUZZY_MATCHES_LANES + 1) * sizeof(uint32_t) + 15) & ~(uint64_t)15;
}

/** The rows of a block: listed_pairs.c's with `limit` slots a row, fewer where rows x chunks would pass the grid's 2^31 - 1 workgroups,
 *  and fewer again where the block's scratch would pass SZS_FUZZY_MATCHES_SCRATCH_BYTES.  At least one. */
static size_t fuzzy_matches_block_rows(size_t q_count, size_t limit, int within_stage_budget, uint64_t n, fuzzy_scan_cut_t *cut) {
    size_t block = szs_listed_block_rows(q_count, limit ? limit : 1, within_stage_budget);
    *cut = fuzzy_scan_cut(block, n);
    if (!cut->chunks) return block;
    if (block > SZS_FUZZY_MATCHES_MOST_WORKGROUPS / cut->chunks) block = (size_t)(SZS_FUZZY_MATCHES_MOST_WORKGROUPS / cut->chunks);
    uint64_t const row_bytes = cut->chunks * (SZS_FUZZY_MATCHES_LANES + 1) * sizeof(uint32_t);
    if (block > SZS_FUZZY_MATCHES_SCRATCH_BYTES / row_bytes) block = (size_t)(SZS_FUZZY_MATCHES_SCRATCH_BYTES / row_bytes);
    return block < 1 ? 1 : block; /* a text below 4 GiB has at most 2^20 chunks: one row's scratch is at most 260 MiB */
}

/** One block: the count, the offsets, the matrices filled with ones, the write and the starts; what was staged goes home.  An empty
 *  text launches nothing: zeros for the counts, ones for the matrices. */
static sz_status_t fuzzy_bounded_block(fuzzy_bounded_call_t *call, size_t q0, size_t rows, hipError_t *hip_error, char const **error_message) {
    szs_listed_call_t *const listed = &call->find.listed;
    hipStream_t const stream = listed->stream;
    size_t const limit = call->limit;
    uint32_t longest = 0;
    for (size_t r = 0; r < rows; ++r) /* every row has at most 256 bytes: the caller saw to it */
        if (listed->query_lengths[q0 + r] > longest) longest = listed->query_lengths[q0 + r];

    /* all staged (dense), or all the caller's; [0] the counts, [1 .. 4) the matrices */
    int const dense_outputs = call->stage[0] || call->stage[1] || call->stage[2] || call->stage[3];
    size_t const cells[4] = {rows, rows * limit, rows * limit, rows * limit};
    uint64_t *kernel[4];
    for (int a = 0; a < 4; ++a) {
        if (!call->outputs[a]) kernel[a] = NULL;
        else if (dense_outputs) kernel[a] = a ? call->staged + listed->block * (1 + (size_t)(a - 1) * limit) : call->staged;
        else kernel[a] = call->outputs[a] + q0 * (a ? limit : 1);
    }
    unsigned launches = 0;
    hipError_t error = szs_listed_block_begin(listed, 0, hipSuccess);
    if (call->text_length) {
        if (error == hipSuccess)
            error = (hipError_t)call->which->count(&listed->sides[0], q0, (uint32_t)rows, call->text, call->text_length, call->cut.piece,
                                                   call->bound, call->piece_counts, call->chunk_counts, listed->flags, listed->device_counters,
                                                   stream);
        if (error == hipSuccess)
            error = (hipError_t)szs_hip_levenshtein_fuzzy_matches_offsets((uint32_t)rows, call->cut.chunks, call->chunk_counts, kernel[0], stream);
        launches = 2;
    }
    else if (error == hipSuccess) error = hipMemsetAsync(kernel[0], 0, cells[0] * sizeof(uint64_t), stream);
    for (int a = 1; a < 4; ++a)
        if (error == hipSuccess && kernel[a]) error = hipMemsetAsync(kernel[a], 0xFF, cells[a] * sizeof(uint64_t), stream);
    if (error == hipSuccess && limit && call->text_length) {
        error = (hipError_t)call->which->write(&listed->sides[0], q0, (uint32_t)rows, call->text, call->text_length, call->cut.piece,
                                               call->bound, (uint32_t)limit, call->piece_counts, call->chunk_counts, kernel[1], kernel[2],
                                               listed->flags, listed->device_counters, stream);
        launches = 3;
        if (error == hipSuccess && kernel[3]) {
            error = (hipError_t)szs_hip_levenshtein_fuzzy_occurrence_starts(&listed->sides[0], q0, (uint32_t)rows, call->text, call->text_length,
                                                                            (uint32_t)limit, kernel[0], kernel[1], kernel[2], kernel[3],
                                                                            listed->flags, listed->device_counters, stream);
            launches = 4;
        }
    }
    error = szs_listed_block_end(listed, error);
    for (int a = 0; a < 4; ++a)
        if (error == hipSuccess && dense_outputs && kernel[a])
            error = hipMemcpyAsync(call->outputs[a] + q0 * (a ? limit : 1), kernel[a], cells[a] * sizeof(uint64_t),
                                   call->stage[a] ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, stream);
    return szs_listed_block_finish(listed, error, hip_error, launches, longest, 2 * 4 + 8, sz_unexpected_dimensions_k, call->which->long_query,
                                   error_message);
}

/** The one call path.  `starts` NULL: no fourth output, no reverse pass - always so where `which` has none. */
static sz_status_t fuzzy_bounded_call(fuzzy_bounded_t const *which, szs_engine_s *engine, szs_scope_s *scope, szs_input_t const *queries,
                                      void const *text, size_t text_length, size_t max_distance, size_t limit, size_t *counts,
                                      size_t *distances, size_t *starts, size_t *ends, char const **error_message) {
    double const started = szs_now_milliseconds();
    if ((uint64_t)text_length > 0xFFFFFFFFull) return szs_report(sz_unexpected_dimensions_k, error_message, "The text must have less than 4 GiB");
    if (limit > SZS_FUZZY_MATCHES_MOST_LIMIT) return szs_report(sz_unexpected_dimensions_k, error_message, which->most_limit);
    if (!engine || engine->magic != SZS_ENGINE_MAGIC || engine->family != szs_family_levenshtein_k || !engine->is_unit_cost)
        return szs_report(sz_status_unknown_k, error_message, which->engine);
    if (!queries) return szs_report(sz_status_unknown_k, error_message, "Queries must not be null");
    if (!queries->count) return szs_report(sz_success_k, error_message, NULL);
    if (!counts) return szs_report(sz_status_unknown_k, error_message, "Counts must not be null");
    if (limit && (!distances || !ends)) return szs_report(sz_status_unknown_k, error_message, "Distances and ends must not be null");
    if (!text && text_length) return szs_report(sz_status_unknown_k, error_message, "Text must not be null");
    size_t const q_count = queries->count;

    fuzzy_bounded_call_t call;
    memset(&call, 0, sizeof(call));
    szs_listed_call_t *const listed = &call.find.listed;
    sz_status_t status = szs_listed_open(listed, engine, scope, limit ? limit : 1, limit ? limit : 1, error_message);
    if (status != sz_success_k) return status;
    if (text_length && !szs_classify_pointer(text).device_accessible)
        return szs_report(sz_status_unknown_k, error_message, "The text is not memory the device can read");
    call.which = which, call.text = text, call.text_length = text_length, call.limit = limit;
    call.bound = max_distance > SZS_RERANK_LONGEST_QUERY ? SZS_RERANK_LONGEST_QUERY : (uint32_t)max_distance; /* D[m][j] <= m <= 256 */
    call.outputs[0] = (uint64_t *)counts;
    if (limit) call.outputs[1] = (uint64_t *)distances, call.outputs[2] = (uint64_t *)ends, call.outputs[3] = (uint64_t *)starts;
    status = szs_listed_offsets(listed, queries, NULL, error_message);
    if (status != sz_success_k) return status;

    /* blocks of rows; the device's words: a block's scratch, then dense copies of the outputs the device cannot reach */
    int dense_outputs = 0;
    size_t matrices = 0;
    for (int a = 0; a < 4; ++a) {
        call.stage[a] = call.outputs[a] && !szs_classify_pointer(call.outputs[a]).device_accessible;
        dense_outputs |= call.stage[a];
        matrices += a && call.outputs[a];
    }
    size_t block = fuzzy_matches_block_rows(q_count, limit, dense_outputs, text_length, &call.cut);
    /* the grid of the starts: rows x ceil(limit / 64) workgroups, at least 2^13 - 1 rows at the largest limit */
    uint64_t const slot_groups = which->with_starts ? ((uint64_t)limit + SZS_FUZZY_MATCHES_LANES - 1) / SZS_FUZZY_MATCHES_LANES : 0;
    if (slot_groups && block > SZS_FUZZY_MATCHES_MOST_WORKGROUPS / slot_groups) block = (size_t)(SZS_FUZZY_MATCHES_MOST_WORKGROUPS / slot_groups);
    listed->block = block;
    size_t const no_extras[2] = {0, 0};
    void *extras[4];
    status = szs_listed_reserve(listed, queries, NULL, 1, no_extras, no_extras, 0, extras, error_message);
    uint64_t const scratch_bytes = fuzzy_matches_scratch(block, call.cut.chunks);
    uint64_t const staged_bytes = dense_outputs ? (uint64_t)block * (1 + matrices * limit) * sizeof(uint64_t) : 0;
    if (status == sz_success_k)
        status = szs_buffer_reserve(&engine->device_rerank_staged, szs_memory_device_k, listed->device, (size_t)(scratch_bytes + staged_bytes + 16),
                                    error_message);
    if (status != sz_success_k) return status;
    call.piece_counts = (uint32_t *)engine->device_rerank_staged.pointer;
    call.chunk_counts = call.piece_counts + block * call.cut.chunks * SZS_FUZZY_MATCHES_LANES;
    call.staged = (uint64_t *)((char *)engine->device_rerank_staged.pointer + scratch_bytes);

    /* a query beyond the kernel's bit-vector fails the call here, before anything is launched */
    status = szs_fuzzy_find_prepare(&call.find, queries, NULL, which->long_query, error_message);
    if (status != sz_success_k) return status;

    hipError_t error = hipSuccess;
    for (size_t q0 = 0; q0 < q_count && status == sz_success_k && error == hipSuccess; q0 += block)
        status = fuzzy_bounded_block(&call, q0, q_count - q0 < block ? q_count - q0 : block, &error, error_message);
    return szs_listed_close(listed, status, error, started, error_message);
}

sz_status_t szs_engine_fuzzy_scan_matches(szs_engine_s *engine, szs_scope_s *scope, szs_input_t const *queries, void const *text,
                                          size_t text_length, size_t max_distance, size_t limit, size_t *counts, size_t *distances,
                                          size_t *ends, char const **error_message) {
    return fuzzy_bounded_call(&fuzzy_matches, engine, scope, queries, text, text_length, max_distance, limit, counts, distances, NULL, ends,
                              error_message);
}

sz_status_t szs_engine_fuzzy_scan_occurrences(szs_engine_s *engine, szs_scope_s *scope, szs_input_t const *queries, void const *text,
                                              size_t text_length, size_t max_distance, size_t limit, size_t *counts, size_t *distances,
                                              size_t *starts, size_t *ends, char const **error_message) {
    return fuzzy_bounded_call(&fuzzy_occurrences, engine, scope, queries, text, text_length, max_distance, limit, counts, distances, starts,
                              ends, error_message);
}
