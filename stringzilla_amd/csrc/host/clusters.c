/*
 *  clusters.c - the connected components of the graph "i ~ j iff the pair is a `within` hit" (szs_rocm_clusters*,
 *  include/stringzillas/stringzillas_rocm.h): labels[i] = the smallest index of the component of string i.
 *
 *  The call has within.c's loop in its self form: blocks of rows x tiles of columns of the SAME strings, every tile an ORDINARY
 *  engine call (szs_engine_cross) into the device scratch matrix, and behind it, on the scope's stream, the union launch of
 *  hip/clusters.hip into one forest of 32-bit parents; one launch before the first tile makes every string a root, one behind the
 *  last writes the labels and counts the roots.  No row is kept, so nothing truncates, and no allocation depends on the data.
 *
 *  THE TRIANGLE.  Where score(i, j) == score(j, i) - every Levenshtein engine, NW and SW with a symmetric substitution table - the
 *  tiles of a block start at the block's own first string: every pair i < j is scored once, as (row i, column j), and only the part
 *  of a block's own square below the diagonal is scored twice.  Otherwise the whole square is scored; the kernel joins the strings
 *  of a hit wherever it finds one, so "hit(i, j) or hit(j, i)" needs no code of its own.  The budget and every step but the scoring
 *  are selection.c's (selection_internal.h); no knob changes a result.
 */
#include "selection_internal.h"

sz_status_t szs_rocm_clusters_probe(sz_size_t count, int symmetric, sz_size_t *block, sz_size_t *tile, sz_size_t *tiles_scored,
                                    sz_size_t *pairs_scored) {
    if (count > SZS_CLUSTERS_MOST_STRINGS) return sz_unexpected_dimensions_k;
    szs_selection_within_plan_t const plan = szs_selection_clusters_plan(count, SIZE_MAX, SIZE_MAX);
    size_t tiles = 0, pairs = 0;
    szs_selection_clusters_work(&plan, count, symmetric != 0, &tiles, &pairs);
    if (block) *block = plan.cut.block;
    if (tile) *tile = plan.cut.tile;
    if (tiles_scored) *tiles_scored = tiles;
    if (pairs_scored) *pairs_scored = pairs;
    return sz_success_k;
}

/** score(i, j) == score(j, i) for every pair of strings: the gap costs are shared by both sides, so the substitution table decides -
 *  over the classes a byte can have, at most 32 x 32 compares. */
static int engine_is_symmetric(szs_engine_s const *engine) {
    if (engine->family != szs_family_needleman_wunsch_k && engine->family != szs_family_smith_waterman_k) return 1;
    uint32_t in_use = 0;
    for (int byte = 0; byte < 256; ++byte) in_use |= 1u << engine->byte_to_class[byte];
    for (int a = 0; a < 32; ++a)
        for (int b = 0; b < a; ++b)
            if (((in_use >> a) & 1u) && ((in_use >> b) & 1u) && engine->class_costs[a * 32 + b] != engine->class_costs[b * 32 + a]) return 0;
    return 1;
}

sz_status_t szs_engine_clusters(szs_engine_s *engine, szs_scope_s *scope, szs_input_t const *strings, sz_ssize_t bound, size_t *labels,
                                size_t *clusters_count, char const **error_message) {
    double const started = szs_now_milliseconds();
    if (strings && strings->count > SZS_CLUSTERS_MOST_STRINGS)
        return szs_report(sz_unexpected_dimensions_k, error_message, "At most 2^32 - 1 strings: the forest is 32-bit words");
    if (!engine || engine->magic != SZS_ENGINE_MAGIC || (unsigned)engine->family > szs_family_smith_waterman_k)
        return szs_report(sz_status_unknown_k, error_message, "Engine must be an initialized similarity engine");
    if (!strings) return szs_report(sz_status_unknown_k, error_message, "Strings must not be null");
    size_t const count = strings->count;
    if (!count) {
        if (clusters_count) *clusters_count = 0;
        return szs_report(sz_success_k, error_message, NULL);
    }
    if (!labels) return szs_report(sz_status_unknown_k, error_message, "Labels must not be null");

    int device = 0;
    hipStream_t stream = NULL;
    sz_status_t status = szs_scope_bind_gpu(scope, &device, &stream, error_message);
    if (status != sz_success_k) return status;
    szs_engine_follow_device(engine, device);

    int const descending = engine->family == szs_family_needleman_wunsch_k || engine->family == szs_family_smith_waterman_k;
    int const reachable = descending || bound >= 0; /* no distance lies within a negative bound: nothing is scored */
    int const symmetric = engine_is_symmetric(engine);
    szs_selection_clusters_t selection = {.stream = stream, .device = device, .descending = descending, .bound = (uint64_t)bound,
                                          .count = count, .labels = (uint64_t *)labels,
                                          .plan = szs_selection_clusters_plan(count, SIZE_MAX, SIZE_MAX)};
    status = szs_selection_clusters_reserve(&selection, &engine->selection, error_message);
    if (status != sz_success_k) return status;
    size_t const block = selection.plan.cut.block, tile = selection.plan.cut.tile;

    szs_rocm_call_profile_t total;
    memset(&total, 0, sizeof(total));
    uint64_t roots = 0;
    hipError_t error = szs_selection_clusters_begin(&selection);
    total.launches += 1;
    for (size_t q0 = 0; q0 < count && reachable && status == sz_success_k && error == hipSuccess; q0 += block) {
        size_t const rows = count - q0 < block ? count - q0 : block;
        szs_shifted_sequence_t row_wrapper, column_wrapper;
        szs_input_t const row_slice = szs_slice_input(strings, q0, rows, &row_wrapper);
        for (size_t c0 = symmetric ? q0 : 0; c0 < count && error == hipSuccess; c0 += tile) {
            size_t const columns = count - c0 < tile ? count - c0 : tile;
            szs_input_t const column_slice = szs_slice_input(strings, c0, columns, &column_wrapper);
            status = szs_engine_cross(engine, scope, &row_slice, &column_slice, selection.cells, columns, error_message);
            if (status != sz_success_k) break;
            szs_selection_profile_add(&total, &engine->last_profile);
            error = szs_selection_clusters_fold(&selection, q0, rows, c0, columns);
            total.launches += 1;
        }
    }
    if (status == sz_success_k && error == hipSuccess) {
        error = szs_selection_clusters_finish(&selection, &roots);
        total.launches += 1;
    }
    error = szs_selection_drain(selection.stream, error);
    if (status != sz_success_k) return status;
    if (error != hipSuccess) return szs_report_hip(error, error_message);
    if (clusters_count) *clusters_count = (size_t)roots;
    szs_selection_profile_publish(engine, &total, reachable, started);
    return szs_report(sz_success_k, error_message, NULL);
}
