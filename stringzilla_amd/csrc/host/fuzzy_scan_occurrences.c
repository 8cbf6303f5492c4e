/*
 *  fuzzy_scan_occurrences.c - ONE span per occurrence of every query inside ONE long text (szs_rocm_fuzzy_scan_occurrences*,
 *  include/stringzillas/stringzillas_rocm.h): counts[q] = the columns j in [1, n] with D[m][j] <= max_distance,
 *  D[m][j] < D[m][j - 1] and (j == n or D[m][j] <= D[m][j + 1]), and the leftmost `limit` of them as ends[q][i] = j, distances[q][i] =
 *  D[m][j] and - where the call asks for them - starts[q][i] = szs_rocm_fuzzy_find_spans' start; the slots behind them hold 2^64 - 1.
 *
 *  The call is the skeleton of listed_pairs.c (rerank_internal.h), as fuzzy_scan_matches.c is, and shares that call's blocks, scratch
 *  and cut (fuzzy_matches_block_rows, fuzzy_matches_scratch, fuzzy_scan_cut), around the kernels of hip/myers_fuzzy_occurrences.hip:
 *  per block the count, the offsets (hip/myers_fuzzy_matches.hip's, as it is) and - with limit > 0 - the fill of the matrices with 0xFF
 *  bytes, the write and, with `starts`, the reverse pass, on one stream inside one event pair.  Outputs the device cannot reach are
 *  staged densely per block and copied home.
 */
#include "rerank_internal.h"

static char const fuzzy_occurrences_long_query[] = "A query of more than 256 bytes: beyond what fuzzy scan occurrences takes";

/** What the blocks of one call share. */
typedef struct {
    szs_fuzzy_find_call_t find; /* its `listed` and the queries' side; nothing else of it is used */
    void const *text;
    uint64_t text_length;
    fuzzy_scan_cut_t cut;
    uint32_t bound;
    size_t limit;
    uint64_t *outputs[4];                  /* the caller's counts, distances, ends, starts; a matrix NULL where the call has none */
    int stage[4];                          /* the device cannot reach it */
    uint32_t *piece_counts, *chunk_counts; /* device: block x chunks x 64 and block x chunks dwords */
    uint64_t *staged;                      /* device: dense outputs of a block, where the device cannot reach the caller's */
} fuzzy_occurrences_call_t;

/** One block: the count, the offsets, the matrices filled with ones, the write and the starts; what was staged goes home.  An empty
 *  text launches nothing: zeros for the counts, ones for the matrices. */
static sz_status_t fuzzy_occurrences_block(fuzzy_occurrences_call_t *call, size_t q0, size_t rows, hipError_t *hip_error,
                                           char const **error_message) {
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
            error = (hipError_t)szs_hip_levenshtein_fuzzy_occurrences_count(&listed->sides[0], q0, (uint32_t)rows, call->text, call->text_length,
                                                                            call->cut.piece, call->bound, call->piece_counts,
                                                                            call->chunk_counts, listed->flags, listed->device_counters, stream);
        if (error == hipSuccess)
            error = (hipError_t)szs_hip_levenshtein_fuzzy_matches_offsets((uint32_t)rows, call->cut.chunks, call->chunk_counts, kernel[0], stream);
        launches = 2;
    }
    else if (error == hipSuccess) error = hipMemsetAsync(kernel[0], 0, cells[0] * sizeof(uint64_t), stream);
    for (int a = 1; a < 4; ++a)
        if (error == hipSuccess && kernel[a]) error = hipMemsetAsync(kernel[a], 0xFF, cells[a] * sizeof(uint64_t), stream);
    if (error == hipSuccess && limit && call->text_length) {
        error = (hipError_t)szs_hip_levenshtein_fuzzy_occurrences_write(&listed->sides[0], q0, (uint32_t)rows, call->text, call->text_length,
                                                                        call->cut.piece, call->bound, (uint32_t)limit, call->piece_counts,
                                                                        call->chunk_counts, kernel[1], kernel[2], listed->flags,
                                                                        listed->device_counters, stream);
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
    return szs_listed_block_finish(listed, error, hip_error, launches, longest, 2 * 4 + 8, sz_unexpected_dimensions_k,
                                   fuzzy_occurrences_long_query, error_message);
}

sz_status_t szs_engine_fuzzy_scan_occurrences(szs_engine_s *engine, szs_scope_s *scope, szs_input_t const *queries, void const *text,
                                              size_t text_length, size_t max_distance, size_t limit, size_t *counts, size_t *distances,
                                              size_t *starts, size_t *ends, char const **error_message) {
    double const started = szs_now_milliseconds();
    if ((uint64_t)text_length > 0xFFFFFFFFull) return szs_report(sz_unexpected_dimensions_k, error_message, "The text must have less than 4 GiB");
    if (limit > SZS_FUZZY_MATCHES_MOST_LIMIT)
        return szs_report(sz_unexpected_dimensions_k, error_message, "The limit must be at most 2^24 occurrences a query");
    if (!engine || engine->magic != SZS_ENGINE_MAGIC || engine->family != szs_family_levenshtein_k || !engine->is_unit_cost)
        return szs_report(sz_status_unknown_k, error_message, "Fuzzy scan occurrences needs an initialized unit-cost byte Levenshtein engine");
    if (!queries) return szs_report(sz_status_unknown_k, error_message, "Queries must not be null");
    if (!queries->count) return szs_report(sz_success_k, error_message, NULL);
    if (!counts) return szs_report(sz_status_unknown_k, error_message, "Counts must not be null");
    if (limit && (!distances || !ends)) return szs_report(sz_status_unknown_k, error_message, "Distances and ends must not be null");
    if (!text && text_length) return szs_report(sz_status_unknown_k, error_message, "Text must not be null");
    size_t const q_count = queries->count;

    fuzzy_occurrences_call_t call;
    memset(&call, 0, sizeof(call));
    szs_listed_call_t *const listed = &call.find.listed;
    sz_status_t status = szs_listed_open(listed, engine, scope, limit ? limit : 1, limit ? limit : 1, error_message);
    if (status != sz_success_k) return status;
    if (text_length && !szs_classify_pointer(text).device_accessible)
        return szs_report(sz_status_unknown_k, error_message, "The text is not memory the device can read");
    call.text = text, call.text_length = text_length, call.limit = limit;
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
    uint64_t const slot_groups = ((uint64_t)limit + SZS_FUZZY_MATCHES_LANES - 1) / SZS_FUZZY_MATCHES_LANES;
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
    status = szs_fuzzy_find_prepare(&call.find, queries, NULL, fuzzy_occurrences_long_query, error_message);
    if (status != sz_success_k) return status;

    hipError_t error = hipSuccess;
    for (size_t q0 = 0; q0 < q_count && status == sz_success_k && error == hipSuccess; q0 += block)
        status = fuzzy_occurrences_block(&call, q0, q_count - q0 < block ? q_count - q0 : block, &error, error_message);
    hipError_t const drained = hipStreamSynchronize(listed->stream); /* synchronous, also when it fails */
    if (status != sz_success_k) return status;
    if (error == hipSuccess) error = drained;
    if (error != hipSuccess) return szs_report_hip(error, error_message);
    engine->last_profile = listed->total; /* the sums over the call; every other field blank */
    engine->last_profile.host_milliseconds = szs_now_milliseconds() - started;
    return szs_report(sz_success_k, error_message, NULL);
}
