/*
 *  top_k.c - the k best candidates of every query (szs_rocm_top_k*, include/stringzillas/stringzillas_rocm.h).
 *
 *  The call is cut into blocks of queries x tiles of candidates.  Every tile is an ORDINARY engine call (szs_engine_cross) of the
 *  block's sub-tape of queries against the tile's sub-tape of candidates, written into a device scratch matrix; behind it, on the
 *  scope's stream, hip/top_k.hip folds the tile into each query's running list on the device.  The engine call of the next tile
 *  plans on the host while that fold runs, and its scoring launches queue behind it on the same stream.  After the last tile one
 *  launch writes the lists out, and one copy moves them to the caller's arrays when those are not device-accessible.  So every
 *  scoring tier serves top-k unchanged, and no knob changes a result: the lists only depend on the cells.  The budget and every
 *  step but the scoring are selection.c's (selection_internal.h), shared with the fingerprint and fuzzy searches; the sub-tapes of a
 *  tile and the sums of its profile are there too, shared with within.c.
 */
#include "selection_internal.h"

sz_status_t szs_engine_top_k(szs_engine_s *engine, szs_scope_s *scope, szs_input_t const *queries, szs_input_t const *candidates,
                             size_t k, size_t *indices, void *scores, size_t row_stride, char const **error_message) {
    double const started = szs_now_milliseconds();
    if (k < 1 || k > SZS_TOP_K_MOST || row_stride < k)
        return szs_report(sz_unexpected_dimensions_k, error_message, "k must be within [1, 1024] and row_stride at least k");
    if (!engine || engine->magic != SZS_ENGINE_MAGIC || (unsigned)engine->family > szs_family_smith_waterman_k)
        return szs_report(sz_status_unknown_k, error_message, "Engine must be an initialized similarity engine");
    if (!queries) return szs_report(sz_status_unknown_k, error_message, "Queries must not be null");
    if (!queries->count) return szs_report(sz_success_k, error_message, NULL);
    if (!indices) return szs_report(sz_status_unknown_k, error_message, "Indices must not be null");

    int device = 0;
    hipStream_t stream = NULL;
    sz_status_t status = szs_scope_bind_gpu(scope, &device, &stream, error_message);
    if (status != sz_success_k) return status;
    szs_engine_follow_device(engine, device);

    int const self = candidates == NULL;
    szs_input_t const *const pool = self ? queries : candidates;
    size_t const q_count = queries->count, c_count = pool->count;
    int const descending = engine->family == szs_family_needleman_wunsch_k || engine->family == szs_family_smith_waterman_k;
    szs_selection_t selection = {.stream = stream, .device = device, .k = k, .row_stride = row_stride, .descending = descending,
                                 .indices = (uint64_t *)indices, .scores = (uint64_t *)scores,
                                 .plan = szs_selection_plan(q_count, c_count, k, SIZE_MAX, SIZE_MAX)};
    status = szs_selection_reserve(&selection, &engine->selection, error_message);
    if (status != sz_success_k) return status;
    size_t const block = selection.plan.block, tile = selection.plan.tile;

    szs_rocm_call_profile_t total;
    memset(&total, 0, sizeof(total));
    hipError_t error = hipSuccess;
    for (size_t q0 = 0; q0 < q_count && status == sz_success_k && error == hipSuccess; q0 += block) {
        size_t const rows = q_count - q0 < block ? q_count - q0 : block;
        szs_shifted_sequence_t query_wrapper, candidate_wrapper;
        szs_input_t const query_slice = szs_slice_input(queries, q0, rows, &query_wrapper);
        error = szs_selection_block_begin(&selection, rows);
        for (size_t c0 = 0; c0 < c_count && error == hipSuccess; c0 += tile) {
            size_t const columns = c_count - c0 < tile ? c_count - c0 : tile;
            szs_input_t const candidate_slice = szs_slice_input(pool, c0, columns, &candidate_wrapper);
            status = szs_engine_cross(engine, scope, &query_slice, &candidate_slice, selection.cells, columns, error_message);
            if (status != sz_success_k) break;
            szs_selection_profile_add(&total, &engine->last_profile);
            error = szs_selection_fold(&selection, q0, rows, c0, columns, self);
            total.launches += szs_selection_fold_launches(&selection);
        }
        if (status != sz_success_k || error != hipSuccess) break;
        error = szs_selection_emit(&selection, q0, rows);
        total.launches += 1;
    }
    error = szs_selection_drain(selection.stream, error);
    if (status != sz_success_k) return status;
    if (error != hipSuccess) return szs_report_hip(error, error_message);
    szs_selection_profile_publish(engine, &total, c_count != 0, started);
    return szs_report(sz_success_k, error_message, NULL);
}
