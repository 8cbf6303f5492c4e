/*
 *  fuzzy_search.c - the k candidates that contain the best approximate match of every query (szs_rocm_fuzzy_search*,
 *  include/stringzillas/stringzillas_rocm.h): row q lists the k candidates with the smallest fuzzy-find
 *  distance of queries[q] - min over j of D[m][j], free start in the text - ascending, ties to the lower index.
 *
 *  The call has top_k.c's shape with hip/myers_fuzzy_tile.hip in place of the engine call: blocks of queries x tiles of candidates
 *  by the shared budget (selection_internal.h), every tile ONE scoring launch into the engine's selection scratch and, behind it on
 *  the scope's stream, the fold into the block's running lists; after the last tile the emit of indices and distances.  The strings reach the
 *  device as the listed-pairs calls bring theirs (listed_pairs.c): no sub-tapes, the kernel takes first rows and first columns.
 *  The tile kernel's grid is rows x segments of the tile's columns; the host picks the segment so that the launch fills the device.
 *
 *  `ends` and `starts` come from a WINNERS PASS: the cells of the scan stay one word and its tie rule top-k's, and once a block's index
 *  rows stand, fuzzy find's own block (fuzzy_find.c) runs on exactly those rows - Q x k pairs next to the tiles' Q x C - and writes
 *  the distances again, the same values, with the ends and starts that belong to them.
 */
#include "rerank_internal.h"
#include "selection_internal.h"

#define SZS_FUZZY_SEARCH_WAVES (256u * 4u * 5u) /* what the device holds of the tile kernel: 256 CUs x 4 SIMDs x 5 waves */
#define SZS_FUZZY_SEARCH_FILLS 4u               /* a tile's launch should fill it this many times over */
#define SZS_FUZZY_SEARCH_LANES 64u              /* a workgroup's candidates at a time: what a segment is a multiple of */

static char const fuzzy_search_long_query[] = "A query of more than 256 bytes: beyond what fuzzy search takes";

/** Candidates per workgroup of the tile kernel, on top of the shared plan: enough workgroups to fill the device several times over,
 *  each with at least 64 columns of its row. */
static size_t fuzzy_search_segment(szs_selection_plan_t const *plan) {
    size_t const wanted = (size_t)SZS_FUZZY_SEARCH_WAVES * SZS_FUZZY_SEARCH_FILLS;
    size_t const per_row = (wanted + plan->block - 1) / plan->block;
    size_t segment = (plan->tile + per_row - 1) / per_row;
    int const segment_knob = szs_tuning_get(szs_knob_fuzzy_search_segment_k);
    if (segment_knob > 0) segment = (size_t)segment_knob;
    segment = (segment + SZS_FUZZY_SEARCH_LANES - 1) / SZS_FUZZY_SEARCH_LANES * SZS_FUZZY_SEARCH_LANES;
    return segment < SZS_FUZZY_SEARCH_LANES ? SZS_FUZZY_SEARCH_LANES : segment;
}

sz_status_t szs_rocm_fuzzy_search_probe(sz_size_t queries_count, sz_size_t candidates_count, sz_size_t k, sz_size_t longest_query,
                                        sz_size_t *block, sz_size_t *tile, sz_size_t *segment, sz_size_t *workgroups) {
    if (k < 1 || k > SZS_TOP_K_MOST || longest_query > SZS_RERANK_LONGEST_QUERY) return sz_unexpected_dimensions_k;
    szs_selection_plan_t const plan = szs_selection_plan(queries_count ? queries_count : 1, candidates_count, k, SIZE_MAX, SIZE_MAX);
    size_t const rows = queries_count < plan.block ? queries_count : plan.block, tile_segment = fuzzy_search_segment(&plan);
    if (block) *block = plan.block;
    if (tile) *tile = plan.tile;
    if (segment) *segment = tile_segment;
    if (workgroups) *workgroups = candidates_count ? rows * ((plan.tile + tile_segment - 1) / tile_segment) : 0;
    return sz_success_k;
}

sz_status_t szs_engine_fuzzy_search(szs_engine_s *engine, szs_scope_s *scope, szs_input_t const *queries, szs_input_t const *candidates,
                                    size_t k, size_t *indices, size_t *distances, size_t *starts, size_t *ends, size_t row_stride,
                                    char const **error_message) {
    double const started = szs_now_milliseconds();
    if (k < 1 || k > SZS_TOP_K_MOST || row_stride < k)
        return szs_report(sz_unexpected_dimensions_k, error_message, "k must be within [1, 1024] and row_stride at least k");
    if (!engine || engine->magic != SZS_ENGINE_MAGIC || engine->family != szs_family_levenshtein_k || !engine->is_unit_cost)
        return szs_report(sz_status_unknown_k, error_message, "Fuzzy search needs an initialized unit-cost byte Levenshtein engine");
    if (!queries) return szs_report(sz_status_unknown_k, error_message, "Queries must not be null");
    if (!queries->count) return szs_report(sz_success_k, error_message, NULL);
    if (!indices || !distances) return szs_report(sz_status_unknown_k, error_message, "Indices and distances must not be null");
    if (starts && !ends) return szs_report(sz_status_unknown_k, error_message, "Starts need ends");

    int const self = candidates == NULL;
    size_t const q_count = queries->count, c_count = (self ? queries : candidates)->count;
    szs_fuzzy_find_call_t winners; /* the call's strings, flags and counters; with `ends`, the winners pass over the emitted rows */
    memset(&winners, 0, sizeof(winners));
    szs_listed_call_t *const listed = &winners.listed;
    sz_status_t status = szs_listed_open(listed, engine, scope, k, row_stride, error_message);
    if (status != sz_success_k) return status;
    hipStream_t const stream = listed->stream;
    status = szs_listed_offsets(listed, queries, candidates, error_message);
    if (status != sz_success_k) return status;
    winners.indices = (uint64_t const *)indices, winners.distances = (uint64_t *)distances;
    winners.ends = (uint64_t *)ends, winners.starts = (uint64_t *)starts;
    size_t const staged_arrays = ends ? szs_fuzzy_find_stage(&winners) : 0;
    listed->block = szs_listed_block_rows(q_count, k, staged_arrays != 0);
    size_t const no_extras[2] = {0, 0};
    void *extras[4];
    status = szs_listed_reserve(listed, queries, candidates, 1, no_extras, no_extras, staged_arrays, extras, error_message);
    if (status == sz_success_k) status = szs_fuzzy_find_prepare(&winners, queries, candidates, fuzzy_search_long_query, error_message);
    if (status != sz_success_k) return status;
    uint32_t longest = 0;
    for (size_t q = 0; q < q_count; ++q)
        if (listed->query_lengths[q] > longest) longest = listed->query_lengths[q];

    szs_selection_t selection = {.stream = stream, .device = listed->device, .k = k, .row_stride = row_stride, .descending = 0,
                                 .indices = (uint64_t *)indices, .scores = (uint64_t *)distances,
                                 .plan = szs_selection_plan(q_count, c_count, k, SIZE_MAX, SIZE_MAX)};
    status = szs_selection_reserve(&selection, &engine->selection, error_message);
    if (status != sz_success_k) return status;
    size_t const block = selection.plan.block, tile = selection.plan.tile, segment = fuzzy_search_segment(&selection.plan);

    hipError_t error = hipSuccess;
    for (size_t q0 = 0; q0 < q_count && status == sz_success_k && error == hipSuccess; q0 += block) {
        size_t const rows = q_count - q0 < block ? q_count - q0 : block;
        error = szs_selection_block_begin(&selection, rows);
        for (size_t c0 = 0; c0 < c_count && status == sz_success_k && error == hipSuccess; c0 += tile) {
            size_t const columns = c_count - c0 < tile ? c_count - c0 : tile;
            error = szs_listed_block_begin(listed, 0, error);
            if (error == hipSuccess)
                error = (hipError_t)szs_hip_levenshtein_fuzzy_tile(&listed->sides[0], &listed->sides[1], q0, (uint32_t)rows, c0,
                                                                   (uint32_t)columns, (uint32_t)segment, selection.cells, columns, listed->flags,
                                                                   listed->device_counters, stream);
            error = szs_listed_block_end(listed, error); /* the event pair: the scoring launch alone */
            if (error == hipSuccess) error = szs_selection_fold(&selection, q0, rows, c0, columns, self);
            /* per pair: an offset of the candidate's and the cell */
            status = szs_listed_block_finish(listed, error, &error, 1 + szs_selection_fold_launches(&selection), longest, 4 + 8,
                                             sz_unexpected_dimensions_k, fuzzy_search_long_query, error_message);
        }
        if (status != sz_success_k || error != hipSuccess) break;
        error = szs_selection_emit(&selection, q0, rows);
        listed->total.launches += 1;
        if (!ends || error != hipSuccess) continue;
        /* the winners pass: the index rows stand where the caller reads them, and fuzzy find's block reads them from there */
        error = hipStreamSynchronize(stream);
        double const scoring_milliseconds = listed->total.kernel_milliseconds; /* the profile's kernel time: the scoring launches */
        for (size_t w0 = q0; w0 < q0 + rows && status == sz_success_k && error == hipSuccess; w0 += listed->block)
            status = szs_fuzzy_find_block(&winners, w0, q0 + rows - w0 < listed->block ? q0 + rows - w0 : listed->block, &error, error_message);
        listed->total.kernel_milliseconds = scoring_milliseconds;
    }
    error = szs_selection_drain(selection.stream, error);
    if (status != sz_success_k) return status;
    if (error != hipSuccess) return szs_report_hip(error, error_message);
    engine->last_profile = listed->total; /* the sums over the call; every other field blank */
    engine->last_profile.host_milliseconds = szs_now_milliseconds() - started;
    return szs_report(sz_success_k, error_message, NULL);
}

/* ---- every candidate within a distance bound (szs_rocm_fuzzy_search_within*) ----------------------------------
 *
 *  The loop above with the bounded fold (selection_internal.h: hip/within.hip) in place of the sorting one: the same tile kernel,
 *  the same segment, and behind the last tile of a block the counts and the empty slots instead of the emit.  The winners pass runs
 *  over the (rows, limit) index rows as it does over the (rows, k) ones - an empty slot is the one fuzzy find skips.  A sibling, not
 *  a flag in the loop above: the two differ in every step but the scoring. */

sz_status_t szs_engine_fuzzy_search_within(szs_engine_s *engine, szs_scope_s *scope, szs_input_t const *queries, szs_input_t const *candidates,
                                           size_t max_distance, size_t limit, size_t *counts, size_t *indices, size_t *distances,
                                           size_t *starts, size_t *ends, size_t row_stride, char const **error_message) {
    double const started = szs_now_milliseconds();
    if (limit > SZS_WITHIN_MOST || row_stride < limit)
        return szs_report(sz_unexpected_dimensions_k, error_message, "limit must be at most 65536 and row_stride at least limit");
    if (!engine || engine->magic != SZS_ENGINE_MAGIC || engine->family != szs_family_levenshtein_k || !engine->is_unit_cost)
        return szs_report(sz_status_unknown_k, error_message, "Fuzzy search needs an initialized unit-cost byte Levenshtein engine");
    if (!queries) return szs_report(sz_status_unknown_k, error_message, "Queries must not be null");
    if (!queries->count) return szs_report(sz_success_k, error_message, NULL);
    if (!counts) return szs_report(sz_status_unknown_k, error_message, "Counts must not be null");
    if (limit && !indices) return szs_report(sz_status_unknown_k, error_message, "Indices must not be null");
    if (limit && ends && !distances) return szs_report(sz_status_unknown_k, error_message, "Ends need distances");
    if (limit && starts && !ends) return szs_report(sz_status_unknown_k, error_message, "Starts need ends");

    int const self = candidates == NULL, with_winners = limit && ends;
    size_t const q_count = queries->count, c_count = (self ? queries : candidates)->count;
    szs_fuzzy_find_call_t winners; /* the call's strings, flags and counters; with `ends`, the winners pass over the stored rows */
    memset(&winners, 0, sizeof(winners));
    szs_listed_call_t *const listed = &winners.listed;
    sz_status_t status = szs_listed_open(listed, engine, scope, limit, row_stride, error_message);
    if (status != sz_success_k) return status;
    hipStream_t const stream = listed->stream;
    status = szs_listed_offsets(listed, queries, candidates, error_message);
    if (status != sz_success_k) return status;
    winners.indices = (uint64_t const *)indices, winners.distances = (uint64_t *)distances;
    winners.ends = (uint64_t *)ends, winners.starts = (uint64_t *)starts;
    size_t const staged_arrays = with_winners ? szs_fuzzy_find_stage(&winners) : 0;
    listed->block = szs_listed_block_rows(q_count, limit ? limit : 1, staged_arrays != 0);
    size_t const no_extras[2] = {0, 0};
    void *extras[4];
    status = szs_listed_reserve(listed, queries, candidates, 1, no_extras, no_extras, staged_arrays, extras, error_message);
    if (status == sz_success_k) status = szs_fuzzy_find_prepare(&winners, queries, candidates, fuzzy_search_long_query, error_message);
    if (status != sz_success_k) return status;
    uint32_t longest = 0;
    for (size_t q = 0; q < q_count; ++q)
        if (listed->query_lengths[q] > longest) longest = listed->query_lengths[q];

    /* no distance exceeds the query's length: a bound beyond the longest query the kernels take is that length */
    szs_selection_within_t selection = {.stream = stream, .device = listed->device, .descending = 0,
                                        .bound = max_distance < SZS_RERANK_LONGEST_QUERY ? max_distance : SZS_RERANK_LONGEST_QUERY,
                                        .limit = limit, .row_stride = row_stride, .counts = (uint64_t *)counts,
                                        .indices = (uint64_t *)indices, .scores = (uint64_t *)distances,
                                        .plan = szs_selection_within_plan(q_count, c_count, limit)};
    status = szs_selection_within_reserve(&selection, &engine->selection, error_message);
    if (status != sz_success_k) return status;
    size_t const block = selection.plan.cut.block, tile = selection.plan.cut.tile, segment = fuzzy_search_segment(&selection.plan.cut);

    hipError_t error = hipSuccess;
    for (size_t q0 = 0; q0 < q_count && status == sz_success_k && error == hipSuccess; q0 += block) {
        size_t const rows = q_count - q0 < block ? q_count - q0 : block;
        error = szs_selection_within_begin(&selection);
        for (size_t c0 = 0; c0 < c_count && status == sz_success_k && error == hipSuccess; c0 += tile) {
            size_t const columns = c_count - c0 < tile ? c_count - c0 : tile;
            error = szs_listed_block_begin(listed, 0, error);
            if (error == hipSuccess)
                error = (hipError_t)szs_hip_levenshtein_fuzzy_tile(&listed->sides[0], &listed->sides[1], q0, (uint32_t)rows, c0,
                                                                   (uint32_t)columns, (uint32_t)segment, selection.cells, columns, listed->flags,
                                                                   listed->device_counters, stream);
            error = szs_listed_block_end(listed, error); /* the event pair: the scoring launch alone */
            if (error == hipSuccess) error = szs_selection_within_fold(&selection, q0, rows, c0, columns, self);
            /* per pair: an offset of the candidate's and the cell */
            status = szs_listed_block_finish(listed, error, &error, 1 + szs_selection_within_fold_launches(&selection), longest, 4 + 8,
                                             sz_unexpected_dimensions_k, fuzzy_search_long_query, error_message);
        }
        if (status != sz_success_k || error != hipSuccess) break;
        error = szs_selection_within_finish(&selection, q0, rows);
        listed->total.launches += 1;
        if (!with_winners || error != hipSuccess) continue;
        /* the winners pass: the index rows stand where the caller reads them, and fuzzy find's block reads them from there */
        error = hipStreamSynchronize(stream);
        double const scoring_milliseconds = listed->total.kernel_milliseconds; /* the profile's kernel time: the scoring launches */
        for (size_t w0 = q0; w0 < q0 + rows && status == sz_success_k && error == hipSuccess; w0 += listed->block)
            status = szs_fuzzy_find_block(&winners, w0, q0 + rows - w0 < listed->block ? q0 + rows - w0 : listed->block, &error, error_message);
        listed->total.kernel_milliseconds = scoring_milliseconds;
    }
    error = szs_selection_drain(selection.stream, error);
    if (status != sz_success_k) return status;
    if (error != hipSuccess) return szs_report_hip(error, error_message);
    engine->last_profile = listed->total; /* the sums over the call; every other field blank */
    engine->last_profile.host_milliseconds = szs_now_milliseconds() - started;
    return szs_report(sz_success_k, error_message, NULL);
}
