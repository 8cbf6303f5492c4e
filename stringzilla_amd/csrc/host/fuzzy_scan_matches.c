/*
 *  fuzzy_scan_matches.c - EVERY end within a distance bound of every query inside ONE long text (szs_rocm_fuzzy_scan_matches*,
 *  include/stringzillas/stringzillas_rocm.h): counts[q] = the columns j in [1, n] with D[m][j] <= max_distance,
 *  and the leftmost `limit` of them as ends[q][i] = j, distances[q][i] = D[m][j]; the slots behind them hold 2^64 - 1.
 *
 *  The call is the skeleton of listed_pairs.c (rerank_internal.h), as fuzzy_scan.c is, around the three kernels of
 *  hip/myers_fuzzy_matches.hip: per block the count, the offsets and - with limit > 0 - the fill of both matrices with 0xFF bytes and
 *  the write, on one stream inside one event pair.  The text is cut by fuzzy_scan.c's own rule (fuzzy_scan_cut: the same pieces, the
 *  same knob, the same probe).  Outputs the device cannot reach are staged densely per block and copied home.  The scratch - 64 piece
 *  counts and one chunk count per (row, chunk) - lies in the engine's staging buffer, ahead of the staged outputs.
 */
#include "rerank_internal.h"

/* (SZS_FUZZY_MATCHES_*, fuzzy_matches_scratch and fuzzy_matches_block_rows are declared in rerank_internal.h:
 * szs_rocm_fuzzy_scan_occurrences* - fuzzy_scan_occurrences.c - has the same scratch and the same blocks) */
static char const fuzzy_matches_long_query[] = "A query of more than 256 bytes: beyond what fuzzy scan matches takes";

/** What the blocks of one call share. */
typedef struct {
    szs_fuzzy_find_call_t find; /* its `listed` and the queries' side; nothing else of it is used */
    void const *text;
    uint64_t text_length;
    fuzzy_scan_cut_t cut;
    uint32_t bound;
    size_t limit;
    uint64_t *counts, *distances, *ends; /* the caller's; the matrices NULL with limit 0 */
    int stage_counts, stage_distances, stage_ends;
    uint32_t *piece_counts, *chunk_counts; /* device: block x chunks x 64 and block x chunks dwords */
    uint64_t *staged;                      /* device: dense outputs of a block, where the device cannot reach the caller's */
} fuzzy_matches_call_t;

/** The bytes of a block's scratch, a multiple of 16. */
uint64_t fuzzy_matches_scratch(uint64_t rows, uint64_t chunks) {
    return (rows * chunks * (SZS_FUZZY_MATCHES_LANES + 1) * sizeof(uint32_t) + 15) & ~(uint64_t)15;
}

/** The rows of a block: listed_pairs.c's with `limit` slots a row, fewer where rows x chunks would pass the grid's 2^31 - 1 workgroups,
 *  and fewer again where the block's scratch would pass SZS_FUZZY_MATCHES_SCRATCH_BYTES.  At least one. */
size_t fuzzy_matches_block_rows(size_t q_count, size_t limit, int within_stage_budget, uint64_t n, fuzzy_scan_cut_t *cut) {
    size_t block = szs_listed_block_rows(q_count, limit ? limit : 1, within_stage_budget);
    *cut = fuzzy_scan_cut(block, n);
    if (!cut->chunks) return block;
    if (block > SZS_FUZZY_MATCHES_MOST_WORKGROUPS / cut->chunks) block = (size_t)(SZS_FUZZY_MATCHES_MOST_WORKGROUPS / cut->chunks);
    uint64_t const row_bytes = cut->chunks * (SZS_FUZZY_MATCHES_LANES + 1) * sizeof(uint32_t);
    if (block > SZS_FUZZY_MATCHES_SCRATCH_BYTES / row_bytes) block = (size_t)(SZS_FUZZY_MATCHES_SCRATCH_BYTES / row_bytes);
    return block < 1 ? 1 : block; /* a text below 4 GiB has at most 2^20 chunks: one row's scratch is at most 260 MiB */
}

/** One block: the count, the offsets, both matrices filled with ones and the write; what was staged goes home.  An empty text
 *  launches nothing: zeros for the counts, ones for the matrices. */
static sz_status_t fuzzy_matches_block(fuzzy_matches_call_t *call, size_t q0, size_t rows, hipError_t *hip_error, char const **error_message) {
    szs_listed_call_t *const listed = &call->find.listed;
    hipStream_t const stream = listed->stream;
    size_t const limit = call->limit;
    uint32_t longest = 0;
    for (size_t r = 0; r < rows; ++r) /* every row has at most 256 bytes: the caller saw to it */
        if (listed->query_lengths[q0 + r] > longest) longest = listed->query_lengths[q0 + r];

    /* all staged (dense), or all the caller's */
    int const dense_outputs = call->stage_counts || call->stage_distances || call->stage_ends;
    uint64_t *kernel_counts = call->counts + q0, *kernel_distances = limit ? call->distances + q0 * limit : NULL;
    uint64_t *kernel_ends = limit ? call->ends + q0 * limit : NULL;
    if (dense_outputs) {
        kernel_counts = call->staged;
        if (limit) kernel_distances = call->staged + listed->block, kernel_ends = kernel_distances + listed->block * limit;
    }
    size_t const count_bytes = rows * sizeof(uint64_t), matrix_bytes = rows * limit * sizeof(uint64_t);
    unsigned launches = 0;
    hipError_t error = szs_listed_block_begin(listed, 0, hipSuccess);
    if (call->text_length) {
        if (error == hipSuccess)
            error = (hipError_t)szs_hip_levenshtein_fuzzy_matches_count(&listed->sides[0], q0, (uint32_t)rows, call->text, call->text_length,
                                                                        call->cut.piece, call->bound, call->piece_counts, call->chunk_counts,
                                                                        listed->flags, listed->device_counters, stream);
        if (error == hipSuccess)
            error = (hipError_t)szs_hip_levenshtein_fuzzy_matches_offsets((uint32_t)rows, call->cut.chunks, call->chunk_counts, kernel_counts, stream);
        launches = 2;
    }
    else if (error == hipSuccess) error = hipMemsetAsync(kernel_counts, 0, count_bytes, stream);
    if (error == hipSuccess && limit) error = hipMemsetAsync(kernel_distances, 0xFF, matrix_bytes, stream);
    if (error == hipSuccess && limit) error = hipMemsetAsync(kernel_ends, 0xFF, matrix_bytes, stream);
    if (error == hipSuccess && limit && call->text_length) {
        error = (hipError_t)szs_hip_levenshtein_fuzzy_matches_write(&listed->sides[0], q0, (uint32_t)rows, call->text, call->text_length,
                                                                    call->cut.piece, call->bound, (uint32_t)limit, call->piece_counts,
                                                                    call->chunk_counts, kernel_distances, kernel_ends, listed->flags,
                                                                    listed->device_counters, stream);
        launches = 3;
    }
    error = szs_listed_block_end(listed, error);
    if (error == hipSuccess && dense_outputs)
        error = hipMemcpyAsync(call->counts + q0, kernel_counts, count_bytes, call->stage_counts ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                               stream);
    if (error == hipSuccess && dense_outputs && limit)
        error = hipMemcpyAsync(call->distances + q0 * limit, kernel_distances, matrix_bytes,
                               call->stage_distances ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, stream);
    if (error == hipSuccess && dense_outputs && limit)
        error = hipMemcpyAsync(call->ends + q0 * limit, kernel_ends, matrix_bytes,
                               call->stage_ends ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, stream);
    return szs_listed_block_finish(listed, error, hip_error, launches, longest, 2 * 4 + 8, sz_unexpected_dimensions_k, fuzzy_matches_long_query,
                                   error_message);
}

sz_status_t szs_engine_fuzzy_scan_matches(szs_engine_s *engine, szs_scope_s *scope, szs_input_t const *queries, void const *text,
                                          size_t text_length, size_t max_distance, size_t limit, size_t *counts, size_t *distances,
                                          size_t *ends, char const **error_message) {
    double const started = szs_now_milliseconds();
    if ((uint64_t)text_length > 0xFFFFFFFFull) return szs_report(sz_unexpected_dimensions_k, error_message, "The text must have less than 4 GiB");
    if (limit > SZS_FUZZY_MATCHES_MOST_LIMIT) return szs_report(sz_unexpected_dimensions_k, error_message, "The limit must be at most 2^24 matches a query");
    if (!engine || engine->magic != SZS_ENGINE_MAGIC || engine->family != szs_family_levenshtein_k || !engine->is_unit_cost)
        return szs_report(sz_status_unknown_k, error_message, "Fuzzy scan matches needs an initialized unit-cost byte Levenshtein engine");
    if (!queries) return szs_report(sz_status_unknown_k, error_message, "Queries must not be null");
    if (!queries->count) return szs_report(sz_success_k, error_message, NULL);
    if (!counts) return szs_report(sz_status_unknown_k, error_message, "Counts must not be null");
    if (limit && (!distances || !ends)) return szs_report(sz_status_unknown_k, error_message, "Distances and ends must not be null");
    if (!text && text_length) return szs_report(sz_status_unknown_k, error_message, "Text must not be null");
    size_t const q_count = queries->count;

    fuzzy_matches_call_t call;
    memset(&call, 0, sizeof(call));
    szs_listed_call_t *const listed = &call.find.listed;
    sz_status_t status = szs_listed_open(listed, engine, scope, limit ? limit : 1, limit ? limit : 1, error_message);
    if (status != sz_success_k) return status;
    if (text_length && !szs_classify_pointer(text).device_accessible)
        return szs_report(sz_status_unknown_k, error_message, "The text is not memory the device can read");
    call.text = text, call.text_length = text_length, call.limit = limit;
    call.bound = max_distance > SZS_RERANK_LONGEST_QUERY ? SZS_RERANK_LONGEST_QUERY : (uint32_t)max_distance; /* D[m][j] <= m <= 256 */
    call.counts = (uint64_t *)counts, call.distances = limit ? (uint64_t *)distances : NULL, call.ends = limit ? (uint64_t *)ends : NULL;
    status = szs_listed_offsets(listed, queries, NULL, error_message);
    if (status != sz_success_k) return status;

    /* blocks of rows; the device's words: a block's scratch, then dense copies of the outputs the device cannot reach */
    call.stage_counts = !szs_classify_pointer(counts).device_accessible;
    call.stage_distances = limit && !szs_classify_pointer(distances).device_accessible;
    call.stage_ends = limit && !szs_classify_pointer(ends).device_accessible;
    int const dense_outputs = call.stage_counts || call.stage_distances || call.stage_ends;
    size_t const block = listed->block = fuzzy_matches_block_rows(q_count, limit, dense_outputs, text_length, &call.cut);
    size_t const no_extras[2] = {0, 0};
    void *extras[4];
    status = szs_listed_reserve(listed, queries, NULL, 1, no_extras, no_extras, 0, extras, error_message);
    uint64_t const scratch_bytes = fuzzy_matches_scratch(block, call.cut.chunks);
    uint64_t const staged_bytes = dense_outputs ? (uint64_t)block * (1 + 2 * limit) * sizeof(uint64_t) : 0;
    if (status == sz_success_k)
        status = szs_buffer_reserve(&engine->device_rerank_staged, szs_memory_device_k, listed->device, (size_t)(scratch_bytes + staged_bytes + 16),
                                    error_message);
    if (status != sz_success_k) return status;
    call.piece_counts = (uint32_t *)engine->device_rerank_staged.pointer;
    call.chunk_counts = call.piece_counts + block * call.cut.chunks * SZS_FUZZY_MATCHES_LANES;
    call.staged = (uint64_t *)((char *)engine->device_rerank_staged.pointer + scratch_bytes);

    /* a query beyond the kernel's bit-vector fails the call here, before anything is launched */
    status = szs_fuzzy_find_prepare(&call.find, queries, NULL, fuzzy_matches_long_query, error_message);
    if (status != sz_success_k) return status;

    hipError_t error = hipSuccess;
    for (size_t q0 = 0; q0 < q_count && status == sz_success_k && error == hipSuccess; q0 += block)
        status = fuzzy_matches_block(&call, q0, q_count - q0 < block ? q_count - q0 : block, &error, error_message);
    hipError_t const drained = hipStreamSynchronize(listed->stream); /* synchronous, also when it fails */
    if (status != sz_success_k) return status;
    if (error == hipSuccess) error = drained;
    if (error != hipSuccess) return szs_report_hip(error, error_message);
    engine->last_profile = listed->total; /* the sums over the call; every other field blank */
    engine->last_profile.host_milliseconds = szs_now_milliseconds() - started;
    return szs_report(sz_success_k, error_message, NULL);
}
