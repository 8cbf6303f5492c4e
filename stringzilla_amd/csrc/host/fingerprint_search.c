/*
 *  fingerprint_search.c - what MinHash fingerprints are for: the equal dimensions of every (query, candidate) pair
 *  (szs_rocm_fingerprint_matches) and the k candidates with the most of them per query (szs_rocm_fingerprint_top_k);
 *  include/stringzillas/stringzillas_rocm.h, DESIGN.md section 4.7.  szs_rocm_fingerprint_clusters, at the end, is the search's
 *  loop over ONE side with the forest fold of hip/clusters.hip behind its tiles.
 *
 *  Both calls are cut into blocks of queries x tiles of candidates.  hip/fingerprint_matches.hip counts a tile; the matrix call
 *  writes it where the caller wants it, the search writes 8-byte cells into a device scratch matrix that hip/top_k.hip folds into
 *  each query's running list - the very selection the similarity engines use (host/selection.c), descending.  Hash matrices the device
 *  cannot read (plain host memory) are staged: the query block once per block, the candidate rows once per tile, so a corpus of
 *  any size passes through a bounded device buffer.  Everything runs on the scope's stream; both calls are synchronous.
 */
#include "selection_internal.h"

#define SZS_SEARCH_STAGE_BYTES ((size_t)256 << 20) /* per side: hashes staged from memory the device cannot read */

static size_t at_most(size_t value, size_t limit) { return value < limit ? value : limit; }
static size_t at_least_one(size_t value) { return value ? value : 1; }

/** What both calls check before anything is touched: the strides first, then the engine, then the strides against its dimensions. */
static sz_status_t vet(szs_fingerprints_s const *engine, sz_size_t query_hashes_stride, sz_u32_t const *candidate_hashes,
                       sz_size_t candidate_hashes_stride, char const **error_message) {
    if (query_hashes_stride % 4 || (candidate_hashes && candidate_hashes_stride % 4))
        return szs_report(sz_unexpected_dimensions_k, error_message, "Hash strides are in bytes and must be multiples of 4");
    if (!engine || engine->magic != SZS_FINGERPRINTS_MAGIC)
        return szs_report(sz_status_unknown_k, error_message, "Engine must be an initialized fingerprints engine");
    size_t const row_bytes = (size_t)engine->dimensions * sizeof(uint32_t);
    if (query_hashes_stride < row_bytes || (candidate_hashes && candidate_hashes_stride < row_bytes))
        return szs_report(sz_unexpected_dimensions_k, error_message, "Hash strides must be at least 4 * dimensions bytes");
    return sz_success_k;
}

/** One side of a call: where its rows are, and how a stretch of them reaches the device. */
typedef struct {
    char const *rows;
    size_t stride, count;
    int device_accessible;
    char *staging; /* dense rows of `row_bytes` in device memory, when not device-accessible */
} szs_hash_side_t;

/** Rows [first, first + count) for a kernel: in place, or copied into the side's staging area behind whatever still reads it. */
static hipError_t side_rows(szs_hash_side_t const *side, size_t first, size_t count, size_t row_bytes, hipStream_t stream,
                            uint32_t const **rows, uint64_t *stride) {
    if (side->device_accessible) {
        *rows = (uint32_t const *)(side->rows + first * side->stride), *stride = side->stride;
        return hipSuccess;
    }
    *rows = (uint32_t const *)side->staging, *stride = row_bytes;
    return hipMemcpy2DAsync(side->staging, row_bytes, side->rows + first * side->stride, side->stride, row_bytes, count, hipMemcpyDefault,
                            stream);
}

/** Reserves the staging areas of the sides that need one: [query block][candidate tile], each on a 256-byte boundary. */
static sz_status_t reserve_staging(szs_fingerprints_s *engine, int device, szs_hash_side_t *queries, size_t block, szs_hash_side_t *pool,
                                   size_t tile, size_t row_bytes, char const **error_message) {
    size_t const query_bytes = queries->device_accessible ? 0 : (block * row_bytes + 255) / 256 * 256;
    size_t const pool_bytes = pool->device_accessible ? 0 : tile * row_bytes;
    if (!(query_bytes + pool_bytes)) return sz_success_k;
    sz_status_t const status = szs_buffer_reserve(&engine->device_search_hashes, szs_memory_device_k, device, query_bytes + pool_bytes, error_message);
    if (status != sz_success_k) return status;
    queries->staging = (char *)engine->device_search_hashes.pointer;
    pool->staging = queries->staging + query_bytes;
    return sz_success_k;
}

sz_status_t szs_fingerprints_matches(szs_fingerprints_s *engine, szs_scope_s *scope, sz_u32_t const *query_hashes,
                                     sz_size_t query_hashes_stride, sz_size_t queries_count, sz_u32_t const *candidate_hashes,
                                     sz_size_t candidate_hashes_stride, sz_size_t candidates_count, sz_u32_t *counts,
                                     sz_size_t counts_stride, char const **error_message) {
    sz_status_t status = vet(engine, query_hashes_stride, candidate_hashes, candidate_hashes_stride, error_message);
    if (status != sz_success_k) return status;
    int const self = candidate_hashes == NULL;
    size_t const q_count = queries_count, c_count = self ? queries_count : candidates_count;
    if (!q_count || !c_count) return szs_report(sz_success_k, error_message, NULL);
    if (!query_hashes) return szs_report(sz_status_unknown_k, error_message, "Query hashes must not be null");
    if (!counts) return szs_report(sz_status_unknown_k, error_message, "Counts must not be null");
    if (counts_stride % 4 || counts_stride / sizeof(uint32_t) < c_count)
        return szs_report(sz_unexpected_dimensions_k, error_message, "The counts stride is in bytes: a multiple of 4, at least 4 * candidates");

    int device = 0;
    hipStream_t stream = NULL;
    status = szs_scope_bind_gpu(scope, &device, &stream, error_message);
    if (status != sz_success_k) return status;
    szs_fingerprints_follow_device(engine, device);

    uint32_t const dimensions = engine->dimensions;
    size_t const row_bytes = (size_t)dimensions * sizeof(uint32_t);
    szs_hash_side_t queries = {(char const *)query_hashes, query_hashes_stride, q_count, szs_classify_pointer(query_hashes).device_accessible, NULL};
    szs_hash_side_t pool = queries;
    if (!self) {
        pool.rows = (char const *)candidate_hashes, pool.stride = candidate_hashes_stride, pool.count = c_count;
        pool.device_accessible = szs_classify_pointer(candidate_hashes).device_accessible;
    }
    int const direct = szs_classify_pointer(counts).device_accessible;

    /* blocks of queries x tiles of candidates: within the kernel's grid, the staging areas and - for counts the device cannot
     * write - a dense scratch tile that is copied out in one piece */
    size_t block = at_most(q_count, (size_t)1 << 20), tile = at_most(c_count, (size_t)1 << 22);
    if (!queries.device_accessible) block = at_most(block, at_least_one(SZS_SEARCH_STAGE_BYTES / row_bytes));
    if (!pool.device_accessible) tile = at_most(tile, at_least_one(SZS_SEARCH_STAGE_BYTES / row_bytes));
    if (!direct) {
        block = at_most(block, 4096);
        tile = at_most(tile, 2 * SZS_SELECTION_SCRATCH_CELLS / block);
    }
    status = reserve_staging(engine, device, &queries, block, &pool, tile, row_bytes, error_message);
    if (status == sz_success_k && !direct)
        status = szs_buffer_reserve(&engine->selection.scratch, szs_memory_device_k, device, block * tile * sizeof(uint32_t), error_message);
    if (status != sz_success_k) return status;

    hipError_t error = hipSuccess;
    for (size_t q0 = 0; q0 < q_count && error == hipSuccess; q0 += block) {
        size_t const rows = at_most(q_count - q0, block);
        uint32_t const *query_rows = NULL, *pool_rows = NULL;
        uint64_t query_stride = 0, pool_stride = 0;
        error = side_rows(&queries, q0, rows, row_bytes, stream, &query_rows, &query_stride);
        for (size_t c0 = 0; c0 < c_count && error == hipSuccess; c0 += tile) {
            size_t const columns = at_most(c_count - c0, tile);
            error = side_rows(&pool, c0, columns, row_bytes, stream, &pool_rows, &pool_stride);
            if (error != hipSuccess) break;
            uint32_t *const target = direct ? (uint32_t *)((char *)counts + q0 * counts_stride) + c0 : (uint32_t *)engine->selection.scratch.pointer;
            size_t const target_stride = direct ? counts_stride : columns * sizeof(uint32_t);
            error = (hipError_t)szs_hip_fingerprint_matches_u32(query_rows, query_stride, (uint32_t)rows, pool_rows, pool_stride, (uint32_t)columns,
                                                                dimensions, target, target_stride, stream);
            if (error == hipSuccess && !direct)
                error = hipMemcpy2DAsync((char *)counts + q0 * counts_stride + c0 * sizeof(uint32_t), counts_stride, target, target_stride,
                                         columns * sizeof(uint32_t), rows, hipMemcpyDefault, stream);
        }
    }
    hipError_t const drained = hipStreamSynchronize(stream); /* synchronous, also when it fails */
    if (error == hipSuccess) error = drained;
    if (error != hipSuccess) return szs_report_hip(error, error_message);
    return szs_report(sz_success_k, error_message, NULL);
}

sz_status_t szs_fingerprints_top_k(szs_fingerprints_s *engine, szs_scope_s *scope, sz_u32_t const *query_hashes,
                                   sz_size_t query_hashes_stride, sz_size_t queries_count, sz_u32_t const *candidate_hashes,
                                   sz_size_t candidate_hashes_stride, sz_size_t candidates_count, sz_size_t k, sz_size_t *indices,
                                   sz_size_t *matches, sz_size_t row_stride, char const **error_message) {
    if (k < 1 || k > SZS_TOP_K_MOST || row_stride < k)
        return szs_report(sz_unexpected_dimensions_k, error_message, "k must be within [1, 1024] and row_stride at least k");
    sz_status_t status = vet(engine, query_hashes_stride, candidate_hashes, candidate_hashes_stride, error_message);
    if (status != sz_success_k) return status;
    if (!queries_count) return szs_report(sz_success_k, error_message, NULL);
    if (!query_hashes) return szs_report(sz_status_unknown_k, error_message, "Query hashes must not be null");
    if (!indices) return szs_report(sz_status_unknown_k, error_message, "Indices must not be null");

    int device = 0;
    hipStream_t stream = NULL;
    status = szs_scope_bind_gpu(scope, &device, &stream, error_message);
    if (status != sz_success_k) return status;
    szs_fingerprints_follow_device(engine, device);

    int const self = candidate_hashes == NULL;
    size_t const q_count = queries_count, c_count = self ? queries_count : candidates_count;
    uint32_t const dimensions = engine->dimensions;
    size_t const row_bytes = (size_t)dimensions * sizeof(uint32_t);
    szs_hash_side_t queries = {(char const *)query_hashes, query_hashes_stride, q_count, szs_classify_pointer(query_hashes).device_accessible, NULL};
    szs_hash_side_t pool = queries;
    if (!self) {
        pool.rows = (char const *)candidate_hashes, pool.stride = candidate_hashes_stride, pool.count = c_count;
        pool.device_accessible = szs_classify_pointer(candidate_hashes).device_accessible;
    }

    /* the shared budget, within the staging areas of hashes the device cannot read */
    size_t const most_staged = at_least_one(SZS_SEARCH_STAGE_BYTES / row_bytes);
    szs_selection_t selection = {.stream = stream, .device = device, .k = k, .row_stride = row_stride, .descending = 1 /* most matches first */,
                                 .indices = (uint64_t *)indices, .scores = (uint64_t *)matches,
                                 .plan = szs_selection_plan(q_count, c_count, k, queries.device_accessible ? SIZE_MAX : most_staged,
                                                            pool.device_accessible ? SIZE_MAX : most_staged)};
    size_t const block = selection.plan.block, tile = selection.plan.tile;
    status = reserve_staging(engine, device, &queries, block, &pool, tile, row_bytes, error_message);
    if (status == sz_success_k) status = szs_selection_reserve(&selection, &engine->selection, error_message);
    if (status != sz_success_k) return status;

    hipError_t error = hipSuccess;
    for (size_t q0 = 0; q0 < q_count && error == hipSuccess; q0 += block) {
        size_t const rows = at_most(q_count - q0, block);
        uint32_t const *query_rows = NULL, *pool_rows = NULL;
        uint64_t query_stride = 0, pool_stride = 0;
        error = side_rows(&queries, q0, rows, row_bytes, stream, &query_rows, &query_stride);
        if (error == hipSuccess) error = szs_selection_block_begin(&selection, rows);
        for (size_t c0 = 0; c0 < c_count && error == hipSuccess; c0 += tile) {
            size_t const columns = at_most(c_count - c0, tile);
            error = side_rows(&pool, c0, columns, row_bytes, stream, &pool_rows, &pool_stride);
            if (error == hipSuccess)
                error = (hipError_t)szs_hip_fingerprint_matches_u64(query_rows, query_stride, (uint32_t)rows, pool_rows, pool_stride,
                                                                    (uint32_t)columns, dimensions, selection.cells, columns, stream);
            if (error == hipSuccess) error = szs_selection_fold(&selection, q0, rows, c0, columns, self);
        }
        if (error == hipSuccess) error = szs_selection_emit(&selection, q0, rows);
    }
    error = szs_selection_drain(selection.stream, error);
    if (error != hipSuccess) return szs_report_hip(error, error_message);
    return szs_report(sz_success_k, error_message, NULL);
}

sz_status_t szs_fingerprints_clusters(szs_fingerprints_s *engine, szs_scope_s *scope, sz_u32_t const *hashes, sz_size_t hashes_stride,
                                      sz_size_t count, sz_size_t min_matches, sz_size_t *labels, sz_size_t *clusters_count,
                                      char const **error_message) {
    if (count > SZS_CLUSTERS_MOST_STRINGS)
        return szs_report(sz_unexpected_dimensions_k, error_message, "At most 2^32 - 1 fingerprints: the forest is 32-bit words");
    sz_status_t status = vet(engine, hashes_stride, NULL, 0, error_message);
    if (status != sz_success_k) return status;
    if (!count) {
        if (clusters_count) *clusters_count = 0;
        return szs_report(sz_success_k, error_message, NULL);
    }
    if (!hashes) return szs_report(sz_status_unknown_k, error_message, "Hashes must not be null");
    if (!labels) return szs_report(sz_status_unknown_k, error_message, "Labels must not be null");

    int device = 0;
    hipStream_t stream = NULL;
    status = szs_scope_bind_gpu(scope, &device, &stream, error_message);
    if (status != sz_success_k) return status;
    szs_fingerprints_follow_device(engine, device);

    uint32_t const dimensions = engine->dimensions;
    size_t const row_bytes = (size_t)dimensions * sizeof(uint32_t);
    int const reachable = min_matches <= dimensions; /* no pair shares more dimensions than there are: nothing is scored */
    szs_hash_side_t rows_side = {(char const *)hashes, hashes_stride, count, szs_classify_pointer(hashes).device_accessible, NULL};
    szs_hash_side_t columns_side = rows_side;

    /* the shared budget, within the staging areas of hashes the device cannot read; matches are symmetric: always the triangle */
    size_t const most_staged = rows_side.device_accessible ? SIZE_MAX : at_least_one(SZS_SEARCH_STAGE_BYTES / row_bytes);
    szs_selection_clusters_t selection = {.stream = stream, .device = device, .descending = 1 /* at least min_matches */,
                                          .bound = (uint64_t)min_matches, .count = count, .labels = (uint64_t *)labels,
                                          .plan = szs_selection_clusters_plan(count, most_staged, most_staged)};
    size_t const block = selection.plan.cut.block, tile = selection.plan.cut.tile;
    status = reserve_staging(engine, device, &rows_side, block, &columns_side, tile, row_bytes, error_message);
    if (status == sz_success_k) status = szs_selection_clusters_reserve(&selection, &engine->selection, error_message);
    if (status != sz_success_k) return status;

    uint64_t roots = 0;
    hipError_t error = szs_selection_clusters_begin(&selection);
    for (size_t q0 = 0; q0 < count && reachable && error == hipSuccess; q0 += block) {
        size_t const rows = at_most(count - q0, block);
        uint32_t const *row_hashes = NULL, *column_hashes = NULL;
        uint64_t row_stride = 0, column_stride = 0;
        error = side_rows(&rows_side, q0, rows, row_bytes, stream, &row_hashes, &row_stride);
        for (size_t c0 = q0; c0 < count && error == hipSuccess; c0 += tile) {
            size_t const columns = at_most(count - c0, tile);
            error = side_rows(&columns_side, c0, columns, row_bytes, stream, &column_hashes, &column_stride);
            if (error == hipSuccess)
                error = (hipError_t)szs_hip_fingerprint_matches_u64(row_hashes, row_stride, (uint32_t)rows, column_hashes, column_stride,
                                                                    (uint32_t)columns, dimensions, selection.cells, columns, stream);
            if (error == hipSuccess) error = szs_selection_clusters_fold(&selection, q0, rows, c0, columns);
        }
    }
    if (error == hipSuccess) error = szs_selection_clusters_finish(&selection, &roots);
    error = szs_selection_drain(selection.stream, error);
    if (error != hipSuccess) return szs_report_hip(error, error_message);
    if (clusters_count) *clusters_count = (size_t)roots;
    return szs_report(sz_success_k, error_message, NULL);
}
