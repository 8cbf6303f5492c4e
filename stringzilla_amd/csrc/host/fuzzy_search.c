/*
 *  fuzzy_search.c - the k candidates that contain the best approximate match of every query (szs_rocm_fuzzy_search*,
 *  include/stringzillas/stringzillas_rocm.h): row q lists the k candidates with the smallest fuzzy-find
 *  distance of queries[q] - min over j of D[m][j], free start in the text - ascending, ties to the lower index.
 *
 *  The call has top_k.c's shape with hip/myers_fuzzy_tile.hip in place of the engine call: blocks of queries x tiles of candidates,
 *  every tile ONE scoring launch into the engine's top-k scratch and, behind it on the scope's stream, the scan of hip/top_k.hip that
 *  folds it into the block's running lists; after the last tile one launch emits indices and distances.  The strings reach the
 *  device as the listed-pairs calls bring theirs (listed_pairs.c): no sub-tapes, the kernel takes first rows and first columns.
 *  The tile kernel's grid is rows x segments of the tile's columns; the host picks the segment so that the launch fills the device.
 *
 *  `ends` and `starts` come from a WINNERS PASS: the cells of the scan stay one word and its tie rule top-k's, and once a block's index
 *  rows stand, fuzzy find's own block (fuzzy_find.c) runs on exactly those rows - Q x k pairs next to the tiles' Q x C - and writes
 *  the distances again, the same values, with the ends and starts that belong to them.
 */
#include "rerank_internal.h"

#define SZS_FUZZY_SEARCH_SCRATCH_CELLS ((size_t)16 << 20) /* as host/top_k.c: a tile the scan re-reads from the Infinity Cache */
#define SZS_FUZZY_SEARCH_LIST_BYTES ((size_t)128 << 20)   /* running lists of one block of queries */
#define SZS_FUZZY_SEARCH_MOST_STRINGS ((size_t)1 << 18)   /* per side of a tile */
#define SZS_FUZZY_SEARCH_SCAN_WORKGROUPS 2048u            /* as host/top_k.c: the scan's rows are split into segments below that */
#define SZS_FUZZY_SEARCH_WAVES (256u * 4u * 5u)           /* what the device holds of the tile kernel: 256 CUs x 4 SIMDs x 5 waves */
#define SZS_FUZZY_SEARCH_FILLS 4u                         /* a tile's launch should fill it this many times over */
#define SZS_FUZZY_SEARCH_LANES 64u                        /* a workgroup's candidates at a time: what a segment is a multiple of */

static char const fuzzy_search_long_query[] = "A query of more than 256 bytes: beyond what fuzzy search takes";

/** How a call is cut: queries per block, candidates per tile, candidates per workgroup of the tile kernel, segments per row of the scan. */
typedef struct {
    size_t block, tile, segment, scan_segments;
} szs_fuzzy_search_plan_t;

static szs_fuzzy_search_plan_t fuzzy_search_plan(size_t q_count, size_t c_count, size_t k) {
    szs_fuzzy_search_plan_t plan;
    size_t const list_bytes = 2 * szs_hip_top_k_width((uint32_t)k) * sizeof(uint64_t);
    /* top_k.c's budgets: a block's lists, and - with a long corpus - few enough rows that a tile keeps 4096 columns */
    size_t block = q_count < SZS_FUZZY_SEARCH_MOST_STRINGS ? q_count : SZS_FUZZY_SEARCH_MOST_STRINGS;
    if (block > SZS_FUZZY_SEARCH_LIST_BYTES / list_bytes) block = SZS_FUZZY_SEARCH_LIST_BYTES / list_bytes;
    size_t const wide = c_count < 4096 ? (c_count ? c_count : 1) : 4096;
    if (block > SZS_FUZZY_SEARCH_SCRATCH_CELLS / wide) block = SZS_FUZZY_SEARCH_SCRATCH_CELLS / wide;
    if (block < 1) block = 1;
    size_t tile = SZS_FUZZY_SEARCH_SCRATCH_CELLS / block;
    if (tile > SZS_FUZZY_SEARCH_MOST_STRINGS) tile = SZS_FUZZY_SEARCH_MOST_STRINGS;
    int const tile_knob = szs_tuning_get(szs_knob_top_k_tile_k);
    if (tile_knob > 0 && (size_t)tile_knob < tile) tile = (size_t)tile_knob;
    if (tile > c_count) tile = c_count ? c_count : 1;
    /* the tile kernel: enough workgroups to fill the device several times over, each with at least 64 columns of its row */
    size_t const wanted = (size_t)SZS_FUZZY_SEARCH_WAVES * SZS_FUZZY_SEARCH_FILLS;
    size_t const per_row = (wanted + block - 1) / block;
    size_t segment = (tile + per_row - 1) / per_row;
    int const segment_knob = szs_tuning_get(szs_knob_fuzzy_search_segment_k);
    if (segment_knob > 0) segment = (size_t)segment_knob;
    segment = (segment + SZS_FUZZY_SEARCH_LANES - 1) / SZS_FUZZY_SEARCH_LANES * SZS_FUZZY_SEARCH_LANES;
    if (segment < SZS_FUZZY_SEARCH_LANES) segment = SZS_FUZZY_SEARCH_LANES;
    /* the scan: top_k.c's segments per row */
    size_t scan_segments = (SZS_FUZZY_SEARCH_SCAN_WORKGROUPS + block - 1) / block;
    if (scan_segments > tile / 4096) scan_segments = tile / 4096;
    if (scan_segments < 1) scan_segments = 1;
    plan.block = block, plan.tile = tile, plan.segment = segment, plan.scan_segments = scan_segments;
    return plan;
}

sz_status_t szs_rocm_fuzzy_search_probe(sz_size_t queries_count, sz_size_t candidates_count, sz_size_t k, sz_size_t longest_query,
                                        sz_size_t *block, sz_size_t *tile, sz_size_t *segment, sz_size_t *workgroups) {
    if (k < 1 || k > SZS_TOP_K_MOST || longest_query > SZS_RERANK_LONGEST_QUERY) return sz_unexpected_dimensions_k;
    szs_fuzzy_search_plan_t const plan = fuzzy_search_plan(queries_count ? queries_count : 1, candidates_count, k);
    size_t const rows = queries_count < plan.block ? queries_count : plan.block;
    if (block) *block = plan.block;
    if (tile) *tile = plan.tile;
    if (segment) *segment = plan.segment;
    if (workgroups) *workgroups = candidates_count ? rows * ((plan.tile + plan.segment - 1) / plan.segment) : 0;
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

    szs_fuzzy_search_plan_t const plan = fuzzy_search_plan(q_count, c_count, k);
    size_t const block = plan.block, tile = plan.tile, segments = plan.scan_segments;
    size_t const width = szs_hip_top_k_width((uint32_t)k), list_bytes = 2 * width * sizeof(uint64_t);
    size_t const partial_bytes = segments > 1 ? block * segments * list_bytes : 0;
    int const device = listed->device;
    status = szs_buffer_reserve(&engine->device_top_k_scratch, szs_memory_device_k, device, block * tile * sizeof(uint64_t), error_message);
    if (status == sz_success_k)
        status = szs_buffer_reserve(&engine->device_top_k_lists, szs_memory_device_k, device, block * list_bytes + partial_bytes, error_message);
    /* outputs a kernel can write go straight there; others (plain host memory) are staged densely and copied in one piece */
    int const direct = szs_classify_pointer(indices).device_accessible && szs_classify_pointer(distances).device_accessible;
    if (status == sz_success_k && !direct)
        status = szs_buffer_reserve(&engine->device_top_k_out, szs_memory_device_k, device, 2 * block * k * sizeof(uint64_t), error_message);
    if (status != sz_success_k) return status;
    uint64_t *const lists = (uint64_t *)engine->device_top_k_lists.pointer;
    uint64_t *const partials = lists + block * 2 * width;
    uint64_t *const cells = (uint64_t *)engine->device_top_k_scratch.pointer;

    hipError_t error = hipSuccess;
    for (size_t q0 = 0; q0 < q_count && status == sz_success_k && error == hipSuccess; q0 += block) {
        size_t const rows = q_count - q0 < block ? q_count - q0 : block;
        error = hipMemsetAsync(lists, 0xFF, rows * list_bytes, stream); /* empty lists */
        for (size_t c0 = 0; c0 < c_count && status == sz_success_k && error == hipSuccess; c0 += tile) {
            size_t const columns = c_count - c0 < tile ? c_count - c0 : tile;
            error = szs_listed_block_begin(listed, 0, error);
            if (error == hipSuccess)
                error = (hipError_t)szs_hip_levenshtein_fuzzy_tile(&listed->sides[0], &listed->sides[1], q0, (uint32_t)rows, c0,
                                                                   (uint32_t)columns, (uint32_t)plan.segment, cells, columns, listed->flags,
                                                                   listed->device_counters, stream);
            error = szs_listed_block_end(listed, error); /* the event pair: the scoring launch alone */
            if (error == hipSuccess)
                error = (hipError_t)szs_hip_top_k_scan(cells, columns, (uint32_t)rows, (uint32_t)columns, c0, self ? q0 : ~(uint64_t)0, lists,
                                                       partials, (uint32_t)segments, (uint32_t)k, 0, stream);
            /* per pair: an offset of the candidate's and the cell */
            status = szs_listed_block_finish(listed, error, &error, segments > 1 ? 3 : 2, longest, 4 + 8, sz_unexpected_dimensions_k,
                                             fuzzy_search_long_query, error_message);
        }
        if (status != sz_success_k || error != hipSuccess) break;
        uint64_t *const block_indices = (uint64_t *)indices + q0 * row_stride, *const block_distances = (uint64_t *)distances + q0 * row_stride;
        if (direct) error = (hipError_t)szs_hip_top_k_emit(lists, (uint32_t)rows, (uint32_t)k, block_indices, block_distances, row_stride, 0, stream);
        else {
            uint64_t *const staged_indices = (uint64_t *)engine->device_top_k_out.pointer, *const staged_distances = staged_indices + rows * k;
            error = (hipError_t)szs_hip_top_k_emit(lists, (uint32_t)rows, (uint32_t)k, staged_indices, staged_distances, k, 0, stream);
            if (error == hipSuccess)
                error = hipMemcpy2DAsync(block_indices, row_stride * sizeof(uint64_t), staged_indices, k * sizeof(uint64_t),
                                         k * sizeof(uint64_t), rows, hipMemcpyDefault, stream);
            if (error == hipSuccess)
                error = hipMemcpy2DAsync(block_distances, row_stride * sizeof(uint64_t), staged_distances, k * sizeof(uint64_t),
                                         k * sizeof(uint64_t), rows, hipMemcpyDefault, stream);
        }
        listed->total.launches += 1;
        if (!ends || error != hipSuccess) continue;
        /* the winners pass: the index rows stand where the caller reads them, and fuzzy find's block reads them from there */
        error = hipStreamSynchronize(stream);
        double const scoring_milliseconds = listed->total.kernel_milliseconds; /* the profile's kernel time: the scoring launches */
        for (size_t w0 = q0; w0 < q0 + rows && status == sz_success_k && error == hipSuccess; w0 += listed->block)
            status = szs_fuzzy_find_block(&winners, w0, q0 + rows - w0 < listed->block ? q0 + rows - w0 : listed->block, &error, error_message);
        listed->total.kernel_milliseconds = scoring_milliseconds;
    }
    hipError_t const drained = hipStreamSynchronize(stream); /* synchronous, also when it fails */
    if (status != sz_success_k) return status;
    if (error == hipSuccess) error = drained;
    if (error != hipSuccess) return szs_report_hip(error, error_message);
    engine->last_profile = listed->total; /* the sums over the call; every other field blank */
    engine->last_profile.host_milliseconds = szs_now_milliseconds() - started;
    return szs_report(sz_success_k, error_message, NULL);
}
