/*
 *  within.c - every candidate of every query inside a score bound (szs_rocm_within*, include/stringzillas/stringzillas_rocm.h;
 *  DESIGN.md section 4.15): counts[q] = the hits among ALL candidates, and the leftmost `limit` of them - ascending candidate index -
 *  with their scores in row q of two (queries x limit) matrices, the slots behind them empty.
 *
 *  The call has top_k.c's loop: blocks of queries x tiles of candidates, every tile an ORDINARY engine call (szs_engine_cross) into
 *  the device scratch matrix, and behind it, on the scope's stream, the fold of hip/within.hip - a count pass and, with a `limit`, a
 *  store pass straight into the caller's rows; after the last tile one launch writes the counts and the empty slots.  Nothing is
 *  sorted and no allocation depends on the data.  The budget and every step but the scoring are selection.c's
 *  (selection_internal.h); no knob changes a result.
 */
#include "selection_internal.h"

sz_status_t szs_rocm_within_probe(sz_size_t queries_count, sz_size_t candidates_count, sz_size_t limit, sz_size_t *block, sz_size_t *tile,
                                  sz_size_t *segments, sz_size_t *segment_columns) {
    if (limit > SZS_WITHIN_MOST) return sz_unexpected_dimensions_k;
    szs_selection_within_plan_t const plan = szs_selection_within_plan(queries_count ? queries_count : 1, candidates_count, limit);
    if (block) *block = plan.cut.block;
    if (tile) *tile = plan.cut.tile;
    if (segments) *segments = plan.cut.segments;
    if (segment_columns) *segment_columns = plan.segment_columns;
    return sz_success_k;
}

sz_status_t szs_engine_within(szs_engine_s *engine, szs_scope_s *scope, szs_input_t const *queries, szs_input_t const *candidates,
                              sz_ssize_t bound, size_t limit, size_t *counts, size_t *indices, void *scores, size_t row_stride,
                              char const **error_message) {
    double const started = szs_now_milliseconds();
    if (limit > SZS_WITHIN_MOST || row_stride < limit)
        return szs_report(sz_unexpected_dimensions_k, error_message, "limit must be at most 65536 and row_stride at least limit");
    if (!engine || engine->magic != SZS_ENGINE_MAGIC || (unsigned)engine->family > szs_family_smith_waterman_k)
        return szs_report(sz_status_unknown_k, error_message, "Engine must be an initialized similarity engine");
    if (!queries) return szs_report(sz_status_unknown_k, error_message, "Queries must not be null");
    if (!queries->count) return szs_report(sz_success_k, error_message, NULL);
    if (!counts) return szs_report(sz_status_unknown_k, error_message, "Counts must not be null");
    if (limit && !indices) return szs_report(sz_status_unknown_k, error_message, "Indices must not be null");

    int device = 0;
    hipStream_t stream = NULL;
    sz_status_t status = szs_scope_bind_gpu(scope, &device, &stream, error_message);
    if (status != sz_success_k) return status;
    szs_engine_follow_device(engine, device);

    int const self = candidates == NULL;
    szs_input_t const *const pool = self ? queries : candidates;
    size_t const q_count = queries->count, c_count = pool->count;
    int const descending = engine->family == szs_family_needleman_wunsch_k || engine->family == szs_family_smith_waterman_k;
    int const reachable = descending || bound >= 0; /* no distance lies within a negative bound: nothing is scored */
    szs_selection_within_t selection = {.stream = stream, .device = device, .descending = descending, .bound = (uint64_t)bound,
                                        .limit = limit, .row_stride = row_stride, .counts = (uint64_t *)counts,
                                        .indices = (uint64_t *)indices, .scores = (uint64_t *)scores,
                                        .plan = szs_selection_within_plan(q_count, c_count, limit)};
    status = szs_selection_within_reserve(&selection, &engine->selection, error_message);
    if (status != sz_success_k) return status;
    size_t const block = selection.plan.cut.block, tile = selection.plan.cut.tile;

    szs_rocm_call_profile_t total;
    memset(&total, 0, sizeof(total));
    hipError_t error = hipSuccess;
    for (size_t q0 = 0; q0 < q_count && status == sz_success_k && error == hipSuccess; q0 += block) {
        size_t const rows = q_count - q0 < block ? q_count - q0 : block;
        szs_shifted_sequence_t query_wrapper, candidate_wrapper;
        szs_input_t const query_slice = szs_slice_input(queries, q0, rows, &query_wrapper);
        error = szs_selection_within_begin(&selection);
        for (size_t c0 = 0; c0 < c_count && reachable && error == hipSuccess; c0 += tile) {
            size_t const columns = c_count - c0 < tile ? c_count - c0 : tile;
            szs_input_t const candidate_slice = szs_slice_input(pool, c0, columns, &candidate_wrapper);
            status = szs_engine_cross(engine, scope, &query_slice, &candidate_slice, selection.cells, columns, error_message);
            if (status != sz_success_k) break;
            szs_selection_profile_add(&total, &engine->last_profile);
            error = szs_selection_within_fold(&selection, q0, rows, c0, columns, self);
            total.launches += szs_selection_within_fold_launches(&selection);
        }
        if (status != sz_success_k || error != hipSuccess) break;
        error = szs_selection_within_finish(&selection, q0, rows);
        total.launches += 1;
    }
    error = szs_selection_drain(selection.stream, error);
    if (status != sz_success_k) return status;
    if (error != hipSuccess) return szs_report_hip(error, error_message);
    szs_selection_profile_publish(engine, &total, c_count != 0 && reachable, started);
    return szs_report(sz_success_k, error_message, NULL);
}
