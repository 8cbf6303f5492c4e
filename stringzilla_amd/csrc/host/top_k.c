/*
 *  top_k.c - the k best candidates of every query (szs_rocm_top_k*, include/stringzillas/stringzillas_rocm.h).
 *
 *  The call is cut into blocks of queries x tiles of candidates.  Every tile is an ORDINARY engine call (szs_engine_cross) of the
 *  block's sub-tape of queries against the tile's sub-tape of candidates, written into a device scratch matrix; behind it, on the
 *  scope's stream, hip/top_k.hip folds the tile into each query's running list on the device.  The engine call of the next tile
 *  plans on the host while that fold runs, and its scoring launches queue behind it on the same stream.  After the last tile one
 *  launch writes the lists out, and one copy moves them to the caller's arrays when those are not device-accessible.  So every
 *  scoring tier serves top-k unchanged, and no knob changes a result: the lists only depend on the cells.
 */
#include "szs_internal.h"

#include <string.h>
#include <time.h>

#define SZS_TOP_K_SCRATCH_CELLS ((size_t)16 << 20)  /* 128 MiB of 8-byte cells: a tile the fold re-reads from the Infinity Cache */
#define SZS_TOP_K_LIST_BYTES ((size_t)128 << 20)    /* running lists of one block of queries */
#define SZS_TOP_K_MOST_STRINGS ((size_t)1 << 18)    /* per side of a tile: tape calls stay device-planned (dispatch.c) */
#define SZS_TOP_K_WORKGROUPS 2048u                  /* the scan wants ~8 workgroups per CU: rows are split into segments below that */

static double now_milliseconds(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

/* ---- sub-sequences: strings [first, first + count) of a side ------------------------------------------------------------- */

typedef struct {
    sz_sequence_t sequence; /* first member: the handle of the wrapper is the wrapper itself */
    sz_sequence_t const *base;
    size_t first;
} szs_shifted_sequence_t;

static sz_cptr_t shifted_start(void const *handle, sz_sorted_idx_t i) {
    szs_shifted_sequence_t const *shifted = (szs_shifted_sequence_t const *)handle;
    return shifted->base->get_start(shifted->base->handle, shifted->first + i);
}
static sz_size_t shifted_length(void const *handle, sz_sorted_idx_t i) {
    szs_shifted_sequence_t const *shifted = (szs_shifted_sequence_t const *)handle;
    return shifted->base->get_length(shifted->base->handle, shifted->first + i);
}

static szs_input_t slice_input(szs_input_t const *input, size_t first, size_t count, szs_shifted_sequence_t *wrapper) {
    szs_input_t slice = *input;
    slice.count = count;
    if (input->kind == szs_input_sequence_k) {
        wrapper->base = input->sequence, wrapper->first = first;
        wrapper->sequence.handle = wrapper, wrapper->sequence.count = count;
        wrapper->sequence.get_start = shifted_start, wrapper->sequence.get_length = shifted_length;
        slice.sequence = &wrapper->sequence;
    }
    else
        slice.offsets = (char const *)input->offsets + first * (input->kind == szs_input_u32tape_k ? 4 : 8);
    return slice;
}

/* ---- the call ------------------------------------------------------------------------------------------------------------ */

sz_status_t szs_engine_top_k(szs_engine_s *engine, szs_scope_s *scope, szs_input_t const *queries, szs_input_t const *candidates,
                             size_t k, size_t *indices, void *scores, size_t row_stride, char const **error_message) {
    double const started = now_milliseconds();
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
    size_t const width = szs_hip_top_k_width((uint32_t)k), list_bytes = 2 * width * sizeof(uint64_t);

    /* blocks of queries: their lists within budget, and - with a long corpus - few enough rows that a tile keeps 4096 columns */
    size_t block = q_count < SZS_TOP_K_MOST_STRINGS ? q_count : SZS_TOP_K_MOST_STRINGS;
    if (block > SZS_TOP_K_LIST_BYTES / list_bytes) block = SZS_TOP_K_LIST_BYTES / list_bytes;
    size_t const wide = c_count < 4096 ? (c_count ? c_count : 1) : 4096;
    if (block > SZS_TOP_K_SCRATCH_CELLS / wide) block = SZS_TOP_K_SCRATCH_CELLS / wide;
    size_t tile = SZS_TOP_K_SCRATCH_CELLS / block;
    if (tile > SZS_TOP_K_MOST_STRINGS) tile = SZS_TOP_K_MOST_STRINGS;
    int const knob = szs_tuning_get(szs_knob_top_k_tile_k);
    if (knob > 0 && (size_t)knob < tile) tile = (size_t)knob;
    if (tile > c_count) tile = c_count ? c_count : 1;
    /* segments per row: enough workgroups for the whole GPU, each at least 4096 columns, their partial lists within budget */
    size_t segments = (SZS_TOP_K_WORKGROUPS + block - 1) / block;
    if (segments > tile / 4096) segments = tile / 4096;
    if (segments < 1) segments = 1;
    size_t const partial_bytes = segments > 1 ? block * segments * list_bytes : 0;

    status = szs_buffer_reserve(&engine->device_top_k_scratch, szs_memory_device_k, device, block * tile * sizeof(uint64_t), error_message);
    if (status == sz_success_k)
        status = szs_buffer_reserve(&engine->device_top_k_lists, szs_memory_device_k, device, block * list_bytes + partial_bytes, error_message);
    /* outputs a kernel can write go straight there; others (plain host memory) are staged densely and copied in one piece */
    int const direct = szs_classify_pointer(indices).device_accessible && (!scores || szs_classify_pointer(scores).device_accessible);
    if (status == sz_success_k && !direct)
        status = szs_buffer_reserve(&engine->device_top_k_out, szs_memory_device_k, device, 2 * block * k * sizeof(uint64_t), error_message);
    if (status != sz_success_k) return status;
    uint64_t *const lists = (uint64_t *)engine->device_top_k_lists.pointer;
    uint64_t *const partials = lists + block * 2 * width;
    uint64_t *const cells = (uint64_t *)engine->device_top_k_scratch.pointer;

    szs_rocm_call_profile_t total;
    memset(&total, 0, sizeof(total));
    hipError_t error = hipSuccess;
    for (size_t q0 = 0; q0 < q_count && status == sz_success_k && error == hipSuccess; q0 += block) {
        size_t const rows = q_count - q0 < block ? q_count - q0 : block;
        szs_shifted_sequence_t query_wrapper, candidate_wrapper;
        szs_input_t const query_slice = slice_input(queries, q0, rows, &query_wrapper);
        error = hipMemsetAsync(lists, 0xFF, rows * list_bytes, stream); /* empty lists */
        for (size_t c0 = 0; c0 < c_count && error == hipSuccess; c0 += tile) {
            size_t const columns = c_count - c0 < tile ? c_count - c0 : tile;
            szs_input_t const candidate_slice = slice_input(pool, c0, columns, &candidate_wrapper);
            status = szs_engine_cross(engine, scope, &query_slice, &candidate_slice, cells, columns, error_message);
            if (status != sz_success_k) break;
            szs_rocm_call_profile_t const *tile_profile = &engine->last_profile;
            total.kernel_milliseconds += tile_profile->kernel_milliseconds, total.cells += tile_profile->cells;
            total.pairs += tile_profile->pairs, total.algorithmic_bytes += tile_profile->algorithmic_bytes;
            total.unique_bytes += tile_profile->unique_bytes, total.launches += tile_profile->launches;
            if (tile_profile->longest_query > total.longest_query) total.longest_query = tile_profile->longest_query;
            if (tile_profile->longest_candidate > total.longest_candidate) total.longest_candidate = tile_profile->longest_candidate;
            error = (hipError_t)szs_hip_top_k_scan(cells, columns, (uint32_t)rows, (uint32_t)columns, c0, self ? q0 : ~(uint64_t)0, lists,
                                                   partials, (uint32_t)segments, (uint32_t)k, descending, stream);
            total.launches += segments > 1 ? 2 : 1;
        }
        if (status != sz_success_k || error != hipSuccess) break;
        if (direct)
            error = (hipError_t)szs_hip_top_k_emit(lists, (uint32_t)rows, (uint32_t)k, (uint64_t *)indices + q0 * row_stride,
                                                   scores ? (uint64_t *)scores + q0 * row_stride : NULL, row_stride, descending, stream);
        else {
            uint64_t *const staged_indices = (uint64_t *)engine->device_top_k_out.pointer, *const staged_scores = staged_indices + rows * k;
            error = (hipError_t)szs_hip_top_k_emit(lists, (uint32_t)rows, (uint32_t)k, staged_indices, staged_scores, k, descending, stream);
            if (error == hipSuccess)
                error = hipMemcpy2DAsync((uint64_t *)indices + q0 * row_stride, row_stride * sizeof(uint64_t), staged_indices,
                                         k * sizeof(uint64_t), k * sizeof(uint64_t), rows, hipMemcpyDefault, stream);
            if (error == hipSuccess && scores)
                error = hipMemcpy2DAsync((uint64_t *)scores + q0 * row_stride, row_stride * sizeof(uint64_t), staged_scores,
                                         k * sizeof(uint64_t), k * sizeof(uint64_t), rows, hipMemcpyDefault, stream);
        }
        total.launches += 1;
    }
    hipError_t const drained = hipStreamSynchronize(stream); /* synchronous, also when it fails */
    if (status != sz_success_k) return status;
    if (error == hipSuccess) error = drained;
    if (error != hipSuccess) return szs_report_hip(error, error_message);
    /* the profile of a top-k call: the last tile's, with the sums over all tiles (kernel time: the scoring launches) and the wall
     * time of the whole call */
    if (!c_count) memset(&engine->last_profile, 0, sizeof(engine->last_profile));
    engine->last_profile.kernel_milliseconds = total.kernel_milliseconds, engine->last_profile.cells = total.cells;
    engine->last_profile.pairs = total.pairs, engine->last_profile.algorithmic_bytes = total.algorithmic_bytes;
    engine->last_profile.unique_bytes = total.unique_bytes, engine->last_profile.launches = total.launches;
    engine->last_profile.longest_query = total.longest_query, engine->last_profile.longest_candidate = total.longest_candidate;
    engine->last_profile.host_milliseconds = now_milliseconds() - started;
    return szs_report(sz_success_k, error_message, NULL);
}
