/*
 *  fuzzy_find.c - the best match of a query INSIDE each listed candidate (szs_rocm_fuzzy_find*, include/stringzillas/stringzillas_rocm.h;
 *  DESIGN.md section 4.9): distances[q][r] = the fewest edits that turn queries[q] into some substring of candidates[indices[q][r]],
 *  ends[q][r] = the smallest exclusive byte offset at which such a substring ends; szs_rocm_fuzzy_find_spans* add starts[q][r] = where
 *  the shortest such substring that ends there begins - a second launch (hip/myers_fuzzy_spans.hip) behind the first, on the same
 *  stream and inside the same event pair, and only in a call that asks for it.
 *
 *  The call is the skeleton of listed_pairs.c (rerank_internal.h) around two kernels: blocks of at most 2^20 rows, every row of a block
 *  in ONE launch of hip/myers_fuzzy_find.hip, dealt by descending query length; the kernel reads the indices and writes the outputs
 *  where they are when the device can reach them, else through a dense copy of the block - one 2-D copy per array.  There is no other
 *  route: no engine call computes a semi-global distance, so an engine that is not unit-cost byte Levenshtein, a query of more than
 *  SZS_RERANK_LONGEST_QUERY bytes and strings the device cannot read are refused.
 */
#include "rerank_internal.h"

static char const fuzzy_find_long_query[] = "A query of more than 256 bytes: beyond what fuzzy find takes";

/** One block: stages what the device cannot reach, launches the kernel once over every row - and the kernel of the starts behind it,
 *  where the call asks for them - brings the outputs home, reads the flags. */
sz_status_t szs_fuzzy_find_block(szs_fuzzy_find_call_t *call, size_t q0, size_t rows, hipError_t *hip_error, char const **error_message) {
    szs_listed_call_t *const listed = &call->listed;
    hipStream_t const stream = listed->stream;
    size_t const k = listed->k, row_stride = listed->row_stride, row_bytes = k * sizeof(uint64_t), pitch = row_stride * sizeof(uint64_t);
    uint32_t longest = 0;
    size_t const dealt = szs_deal_short_rows(listed->query_lengths + q0, rows, listed->order, &longest); /* every row: the caller saw to it */
    unsigned const widest = longest ? (longest + 31) / 32 : 1;

    uint64_t *staged = (uint64_t *)listed->engine->device_rerank_staged.pointer;
    uint64_t const *kernel_indices = call->indices ? call->indices + q0 * row_stride : NULL;
    uint64_t *kernel_distances = call->distances + q0 * row_stride, *kernel_ends = call->ends ? call->ends + q0 * row_stride : NULL;
    uint64_t *kernel_starts = call->starts ? call->starts + q0 * row_stride : NULL;
    size_t indices_stride = row_stride;
    hipError_t error = hipSuccess;
    if (call->stage_indices) {
        error = hipMemcpy2DAsync(staged, row_bytes, call->indices + q0 * row_stride, pitch, row_bytes, rows, hipMemcpyHostToDevice, stream);
        kernel_indices = staged, indices_stride = k, staged += listed->block * k;
    }
    /* the kernels' outputs share one stride: all staged (dense), or all the caller's */
    int const dense_outputs = call->stage_distances || call->stage_ends || call->stage_starts;
    if (dense_outputs) {
        kernel_distances = staged, staged += listed->block * k;
        if (call->ends) kernel_ends = staged, staged += listed->block * k;
        if (call->starts) kernel_starts = staged;
    }
    size_t const outputs_stride = dense_outputs ? k : row_stride;
    error = szs_listed_block_begin(listed, dealt, error);
    if (error == hipSuccess)
        error = (hipError_t)szs_hip_levenshtein_fuzzy_find(&listed->sides[0], &listed->sides[1], q0, listed->device_order, (uint32_t)dealt,
                                                           kernel_indices, indices_stride, k, kernel_distances, kernel_ends, outputs_stride,
                                                           widest, listed->flags, listed->device_counters, stream);
    if (error == hipSuccess && call->starts) /* behind the first launch on the same stream: it reads what that one wrote */
        error = (hipError_t)szs_hip_levenshtein_fuzzy_starts(&listed->sides[0], &listed->sides[1], q0, listed->device_order, (uint32_t)dealt,
                                                             kernel_indices, indices_stride, k, kernel_distances, kernel_ends, kernel_starts,
                                                             outputs_stride, widest, listed->flags, listed->device_counters, stream);
    error = szs_listed_block_end(listed, error);
    if (error == hipSuccess && dense_outputs)
        error = hipMemcpy2DAsync(call->distances + q0 * row_stride, pitch, kernel_distances, row_bytes, row_bytes, rows,
                                 call->stage_distances ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, stream);
    if (error == hipSuccess && dense_outputs && call->ends)
        error = hipMemcpy2DAsync(call->ends + q0 * row_stride, pitch, kernel_ends, row_bytes, row_bytes, rows,
                                 call->stage_ends ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, stream);
    if (error == hipSuccess && dense_outputs && call->starts)
        error = hipMemcpy2DAsync(call->starts + q0 * row_stride, pitch, kernel_starts, row_bytes, row_bytes, rows,
                                 call->stage_starts ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, stream);
    /* with starts: the cells and bytes of the reverse windows too */
    return szs_listed_block_finish(listed, error, hip_error, call->starts ? 2 : 1, longest,
                                   2 * 4 + 8 + (call->ends ? 8 : 0) + (call->starts ? 8 : 0), sz_unexpected_dimensions_k,
                                   fuzzy_find_long_query, error_message);
}

size_t szs_fuzzy_find_stage(szs_fuzzy_find_call_t *call) {
    call->stage_indices = call->indices && !szs_classify_pointer(call->indices).device_accessible;
    call->stage_distances = !szs_classify_pointer(call->distances).device_accessible;
    call->stage_ends = call->ends && !szs_classify_pointer(call->ends).device_accessible;
    call->stage_starts = call->starts && !szs_classify_pointer(call->starts).device_accessible;
    int const dense_outputs = call->stage_distances || call->stage_ends || call->stage_starts;
    return (size_t)call->stage_indices + (dense_outputs ? 1 + (call->ends != NULL) + (call->starts != NULL) : 0);
}

sz_status_t szs_fuzzy_find_prepare(szs_fuzzy_find_call_t *call, szs_input_t const *queries, szs_input_t const *candidates,
                                   char const *long_query, char const **error_message) {
    szs_listed_call_t *const listed = &call->listed;
    int usable = 0;
    sz_status_t status = szs_listed_prepare_queries(listed, queries, SZS_RERANK_LONGEST_QUERY, &usable, error_message);
    if (status != sz_success_k) return status;
    if (!usable) return szs_report(sz_status_unknown_k, error_message, "The queries are not strings the device can read");
    /* a query beyond the kernel's bit-vector fails the call here, before anything is launched */
    for (size_t q = 0; q < queries->count; ++q) {
        if (listed->query_lengths[q] != ~0u) continue;
        int const descends = !listed->refs_needed[0] && szs_tape_offset(queries, listed->offsets[0], q + 1) < szs_tape_offset(queries, listed->offsets[0], q);
        return szs_report(sz_unexpected_dimensions_k, error_message, descends ? "Tape offsets must ascend" : long_query);
    }
    status = szs_listed_prepare_candidates(listed, candidates, &usable, error_message);
    if (status != sz_success_k) return status;
    if (!usable) return szs_report(sz_status_unknown_k, error_message, "The candidates are not strings the device can read");
    return sz_success_k;
}

/** The one call path.  `starts` set: the starts are computed too.  `missing`: the message for a required output that is NULL, refused
 *  behind the checks of the dimensions, the engine and an empty batch; NULL when the entry has all it requires. */
static sz_status_t fuzzy_find_call(szs_engine_s *engine, szs_scope_s *scope, szs_input_t const *queries, szs_input_t const *candidates,
                                   size_t const *indices, size_t k, size_t *distances, size_t *starts, size_t *ends, size_t row_stride,
                                   char const *missing, char const **error_message) {
    double const started = szs_now_milliseconds();
    if (k < 1 || row_stride < k) return szs_report(sz_unexpected_dimensions_k, error_message, "k must be at least 1 and row_stride at least k");
    if (!engine || engine->magic != SZS_ENGINE_MAGIC || engine->family != szs_family_levenshtein_k || !engine->is_unit_cost)
        return szs_report(sz_status_unknown_k, error_message, "Fuzzy find needs an initialized unit-cost byte Levenshtein engine");
    if (!queries) return szs_report(sz_status_unknown_k, error_message, "Queries must not be null");
    if (!queries->count) return szs_report(sz_success_k, error_message, NULL);
    if (missing) return szs_report(sz_status_unknown_k, error_message, missing);
    szs_input_t const *const pool = candidates ? candidates : queries; /* the self form: the indices refer to the queries */
    size_t const q_count = queries->count, c_count = pool->count;
    if (!indices && k != c_count)
        return szs_report(sz_unexpected_dimensions_k, error_message, "Without indices k must be the number of candidates");
    if (k > (~(size_t)0 >> 4) / sizeof(uint64_t)) return szs_report(sz_overflow_risk_k, error_message, NULL);

    szs_fuzzy_find_call_t call;
    memset(&call, 0, sizeof(call));
    szs_listed_call_t *const listed = &call.listed;
    sz_status_t status = szs_listed_open(listed, engine, scope, k, row_stride, error_message);
    if (status != sz_success_k) return status;
    call.indices = (uint64_t const *)indices, call.distances = (uint64_t *)distances, call.ends = (uint64_t *)ends;
    call.starts = (uint64_t *)starts;

    /* indices the host can read: validated before anything is launched */
    if (indices && szs_classify_pointer(indices).host_readable && !szs_listed_indices_ok(call.indices, q_count, k, row_stride, c_count))
        return szs_report(sz_unexpected_dimensions_k, error_message, "An index is beyond the candidates");
    status = szs_listed_offsets(listed, queries, candidates, error_message);
    if (status != sz_success_k) return status;

    /* blocks of rows: the kernel's row list and - where the device cannot reach the caller's arrays - their dense copies in budget */
    size_t const staged_arrays = szs_fuzzy_find_stage(&call);
    size_t const block = listed->block = szs_listed_block_rows(q_count, k, staged_arrays != 0);

    size_t const no_extras[2] = {0, 0};
    void *extras[4];
    status = szs_listed_reserve(listed, queries, candidates, 1, no_extras, no_extras, staged_arrays, extras, error_message);
    if (status != sz_success_k) return status;

    status = szs_fuzzy_find_prepare(&call, queries, candidates, fuzzy_find_long_query, error_message);
    if (status != sz_success_k) return status;

    hipError_t error = hipSuccess;
    for (size_t q0 = 0; q0 < q_count && status == sz_success_k && error == hipSuccess; q0 += block)
        status = szs_fuzzy_find_block(&call, q0, q_count - q0 < block ? q_count - q0 : block, &error, error_message);
    return szs_listed_close(listed, status, error, started, error_message);
}

sz_status_t szs_engine_fuzzy_find(szs_engine_s *engine, szs_scope_s *scope, szs_input_t const *queries, szs_input_t const *candidates,
                                  size_t const *indices, size_t k, size_t *distances, size_t *ends, size_t row_stride,
                                  char const **error_message) {
    return fuzzy_find_call(engine, scope, queries, candidates, indices, k, distances, NULL, ends, row_stride,
                           distances ? NULL : "Distances must not be null", error_message);
}

sz_status_t szs_engine_fuzzy_find_spans(szs_engine_s *engine, szs_scope_s *scope, szs_input_t const *queries, szs_input_t const *candidates,
                                        size_t const *indices, size_t k, size_t *distances, size_t *starts, size_t *ends,
                                        size_t row_stride, char const **error_message) {
    char const *const missing = !distances ? "Distances must not be null" : !starts || !ends ? "Starts and ends must not be null" : NULL;
    return fuzzy_find_call(engine, scope, queries, candidates, indices, k, distances, starts, ends, row_stride, missing, error_message);
}
