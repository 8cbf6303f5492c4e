/* selection.c - the budget and the steps of a tiled selection (selection_internal.h). */
#include "selection_internal.h"

static size_t at_most(size_t value, size_t limit) { return value < limit ? value : limit; }

/** The cut both plans share; `most_rows_by_bytes`: the rows whose lists - or whose dense output - fit SZS_SELECTION_LIST_BYTES. */
static szs_selection_plan_t selection_cut(size_t q_count, size_t c_count, size_t most_rows_by_bytes, size_t most_block_rows,
                                          size_t most_tile_rows) {
    /* Every step but the last of `block` and of `tile` is a minimum, so the caller's caps may join in any order: the minimum of the
     * same terms is the same number.  `block` is at least 1 without a floor: the queries are, the lists allow 128 MiB / 16 KiB = 8192
     * rows (k = 1024) and the dense output 128 MiB / 1 MiB = 128 (limit = 65,536), the scratch 16 Mi / 4096 = 4096, and the caller's
     * cap is at least 1. */
    size_t const wide = c_count < 4096 ? (c_count ? c_count : 1) : 4096;
    size_t block = at_most(q_count, SZS_SELECTION_MOST_ROWS);
    block = at_most(block, most_rows_by_bytes);
    block = at_most(block, SZS_SELECTION_SCRATCH_CELLS / wide);
    block = at_most(block, most_block_rows);
    size_t tile = at_most(SZS_SELECTION_SCRATCH_CELLS / block, SZS_SELECTION_MOST_ROWS);
    tile = at_most(tile, most_tile_rows);
    int const knob = szs_tuning_get(szs_knob_top_k_tile_k);
    if (knob > 0) tile = at_most(tile, (size_t)knob);
    if (tile > c_count) tile = c_count ? c_count : 1;
    /* segments per row: enough workgroups for the whole GPU, each at least 4096 columns */
    size_t segments = at_most((SZS_SELECTION_WORKGROUPS + block - 1) / block, tile / 4096);
    return (szs_selection_plan_t){block, tile, segments ? segments : 1};
}

szs_selection_plan_t szs_selection_plan(size_t q_count, size_t c_count, size_t k, size_t most_block_rows, size_t most_tile_rows) {
    size_t const list_bytes = 2 * szs_hip_top_k_width((uint32_t)k) * sizeof(uint64_t);
    return selection_cut(q_count, c_count, SZS_SELECTION_LIST_BYTES / list_bytes, most_block_rows, most_tile_rows);
}

/** The segments of hip/within.hip's grid over `cut`: of a whole number of rounds, and as many as cover a full tile. */
static szs_selection_within_plan_t within_segments(szs_selection_plan_t cut) {
    size_t segment_columns = (cut.tile + cut.segments - 1) / cut.segments;
    segment_columns = (segment_columns + SZS_SELECTION_SEGMENT_QUANTUM - 1) / SZS_SELECTION_SEGMENT_QUANTUM * SZS_SELECTION_SEGMENT_QUANTUM;
    cut.segments = (cut.tile + segment_columns - 1) / segment_columns;
    return (szs_selection_within_plan_t){cut, segment_columns};
}

szs_selection_within_plan_t szs_selection_within_plan(size_t q_count, size_t c_count, size_t limit) {
    size_t const staged_row_bytes = 2 * limit * sizeof(uint64_t); /* indices and scores */
    return within_segments(selection_cut(q_count, c_count, limit ? SZS_SELECTION_LIST_BYTES / staged_row_bytes : SIZE_MAX, SIZE_MAX, SIZE_MAX));
}

szs_selection_within_plan_t szs_selection_clusters_plan(size_t count, size_t most_block_rows, size_t most_tile_rows) {
    return within_segments(selection_cut(count ? count : 1, count, SIZE_MAX, most_block_rows, most_tile_rows));
}

void szs_selection_clusters_work(szs_selection_within_plan_t const *plan, size_t count, int symmetric, size_t *tiles, size_t *pairs) {
    size_t const block = plan->cut.block, tile = plan->cut.tile;
    *tiles = *pairs = 0;
    for (size_t q0 = 0; q0 < count; q0 += block) {
        size_t const rows = at_most(count - q0, block), columns = symmetric ? count - q0 : count;
        *tiles += (columns + tile - 1) / tile, *pairs += rows * columns;
    }
}

void szs_selection_release(szs_selection_buffers_t *buffers) {
    szs_buffer_release(&buffers->scratch);
    szs_buffer_release(&buffers->lists);
    szs_buffer_release(&buffers->out);
}

sz_status_t szs_selection_reserve(szs_selection_t *call, szs_selection_buffers_t *buffers, char const **error_message) {
    size_t const block = call->plan.block, segments = call->plan.segments;
    call->width = szs_hip_top_k_width((uint32_t)call->k);
    size_t const list_bytes = 2 * call->width * sizeof(uint64_t);
    size_t const partial_bytes = segments > 1 ? block * segments * list_bytes : 0;
    sz_status_t status = szs_buffer_reserve(&buffers->scratch, szs_memory_device_k, call->device, block * call->plan.tile * sizeof(uint64_t), error_message);
    if (status == sz_success_k)
        status = szs_buffer_reserve(&buffers->lists, szs_memory_device_k, call->device, block * list_bytes + partial_bytes, error_message);
    /* outputs a kernel can write go straight there; others (plain host memory) are staged densely and copied in one piece */
    call->direct = szs_classify_pointer(call->indices).device_accessible && (!call->scores || szs_classify_pointer(call->scores).device_accessible);
    if (status == sz_success_k && !call->direct)
        status = szs_buffer_reserve(&buffers->out, szs_memory_device_k, call->device, 2 * block * call->k * sizeof(uint64_t), error_message);
    call->cells = (uint64_t *)buffers->scratch.pointer, call->lists = (uint64_t *)buffers->lists.pointer;
    call->partials = call->lists + block * 2 * call->width, call->staged = (uint64_t *)buffers->out.pointer;
    return status;
}

hipError_t szs_selection_block_begin(szs_selection_t const *call, size_t rows) {
    return hipMemsetAsync(call->lists, 0xFF, rows * 2 * call->width * sizeof(uint64_t), call->stream); /* empty lists */
}

hipError_t szs_selection_fold(szs_selection_t const *call, size_t q0, size_t rows, size_t c0, size_t columns, int self) {
    return (hipError_t)szs_hip_top_k_scan(call->cells, columns, (uint32_t)rows, (uint32_t)columns, c0, self ? q0 : ~(uint64_t)0, call->lists,
                                          call->partials, (uint32_t)call->plan.segments, (uint32_t)call->k, call->descending, call->stream);
}

hipError_t szs_selection_emit(szs_selection_t const *call, size_t q0, size_t rows) {
    size_t const k = call->k, row_stride = call->row_stride;
    uint64_t *const indices = call->indices + q0 * row_stride, *const scores = call->scores ? call->scores + q0 * row_stride : NULL;
    if (call->direct)
        return (hipError_t)szs_hip_top_k_emit(call->lists, (uint32_t)rows, (uint32_t)k, indices, scores, row_stride, call->descending, call->stream);
    uint64_t *const staged_indices = call->staged, *const staged_scores = staged_indices + rows * k;
    hipError_t error = (hipError_t)szs_hip_top_k_emit(call->lists, (uint32_t)rows, (uint32_t)k, staged_indices, staged_scores, k, call->descending, call->stream);
    if (error == hipSuccess)
        error = hipMemcpy2DAsync(indices, row_stride * sizeof(uint64_t), staged_indices, k * sizeof(uint64_t), k * sizeof(uint64_t), rows,
                                 hipMemcpyDefault, call->stream);
    if (error == hipSuccess && scores)
        error = hipMemcpy2DAsync(scores, row_stride * sizeof(uint64_t), staged_scores, k * sizeof(uint64_t), k * sizeof(uint64_t), rows,
                                 hipMemcpyDefault, call->stream);
    return error;
}

hipError_t szs_selection_drain(hipStream_t stream, hipError_t error) {
    hipError_t const drained = hipStreamSynchronize(stream);
    return error == hipSuccess ? drained : error;
}

/* ---- sub-sequences: strings [first, first + count) of a side ------------------------------------------------------------- */

static sz_cptr_t shifted_start(void const *handle, sz_sorted_idx_t i) {
    szs_shifted_sequence_t const *shifted = (szs_shifted_sequence_t const *)handle;
    return shifted->base->get_start(shifted->base->handle, shifted->first + i);
}
static sz_size_t shifted_length(void const *handle, sz_sorted_idx_t i) {
    szs_shifted_sequence_t const *shifted = (szs_shifted_sequence_t const *)handle;
    return shifted->base->get_length(shifted->base->handle, shifted->first + i);
}

szs_input_t szs_slice_input(szs_input_t const *input, size_t first, size_t count, szs_shifted_sequence_t *wrapper) {
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

void szs_selection_profile_add(szs_rocm_call_profile_t *total, szs_rocm_call_profile_t const *tile_profile) {
    total->kernel_milliseconds += tile_profile->kernel_milliseconds, total->cells += tile_profile->cells;
    total->pairs += tile_profile->pairs, total->algorithmic_bytes += tile_profile->algorithmic_bytes;
    total->unique_bytes += tile_profile->unique_bytes, total->launches += tile_profile->launches;
    if (tile_profile->longest_query > total->longest_query) total->longest_query = tile_profile->longest_query;
    if (tile_profile->longest_candidate > total->longest_candidate) total->longest_candidate = tile_profile->longest_candidate;
}

void szs_selection_profile_publish(szs_engine_s *engine, szs_rocm_call_profile_t const *total, int scored, double started) {
    if (!scored) memset(&engine->last_profile, 0, sizeof(engine->last_profile));
    engine->last_profile.kernel_milliseconds = total->kernel_milliseconds, engine->last_profile.cells = total->cells;
    engine->last_profile.pairs = total->pairs, engine->last_profile.algorithmic_bytes = total->algorithmic_bytes;
    engine->last_profile.unique_bytes = total->unique_bytes, engine->last_profile.launches = total->launches;
    engine->last_profile.longest_query = total->longest_query, engine->last_profile.longest_candidate = total->longest_candidate;
    engine->last_profile.host_milliseconds = szs_now_milliseconds() - started;
}

/* ---- the bounded fold (hip/within.hip) ---------------------------------------------------------------------------------------- */

sz_status_t szs_selection_within_reserve(szs_selection_within_t *call, szs_selection_buffers_t *buffers, char const **error_message) {
    size_t const block = call->plan.cut.block, segments = call->plan.cut.segments, limit = call->limit;
    /* outputs a kernel can write go straight there; others (plain host memory) are staged densely and copied in one piece */
    call->direct_counts = szs_classify_pointer(call->counts).device_accessible;
    call->direct = !limit || (szs_classify_pointer(call->indices).device_accessible &&
                              (!call->scores || szs_classify_pointer(call->scores).device_accessible));
    size_t const counts_bytes = call->direct_counts ? 0 : block * sizeof(uint64_t);
    size_t const rows_bytes = call->direct ? 0 : 2 * block * limit * sizeof(uint64_t);
    sz_status_t status = szs_buffer_reserve(&buffers->scratch, szs_memory_device_k, call->device,
                                            block * call->plan.cut.tile * sizeof(uint64_t), error_message);
    if (status == sz_success_k)
        status = szs_buffer_reserve(&buffers->lists, szs_memory_device_k, call->device,
                                    2 * block * sizeof(uint64_t) + block * segments * sizeof(uint32_t), error_message);
    if (status == sz_success_k && counts_bytes + rows_bytes)
        status = szs_buffer_reserve(&buffers->out, szs_memory_device_k, call->device, counts_bytes + rows_bytes, error_message);
    call->cells = (uint64_t *)buffers->scratch.pointer, call->running = (uint64_t *)buffers->lists.pointer;
    call->partials = (uint32_t *)(call->running + 2 * block);
    call->staged_counts = (uint64_t *)buffers->out.pointer, call->staged = call->staged_counts + counts_bytes / sizeof(uint64_t);
    call->folded = 0;
    return status;
}

hipError_t szs_selection_within_begin(szs_selection_within_t *call) {
    size_t const block = call->plan.cut.block;
    call->folded = 0;
    return hipMemsetAsync(call->running, 0, 2 * block * sizeof(uint64_t) + block * call->plan.cut.segments * sizeof(uint32_t), call->stream);
}

hipError_t szs_selection_within_fold(szs_selection_within_t *call, size_t q0, size_t rows, size_t c0, size_t columns, int self) {
    size_t const block = call->plan.cut.block, limit = call->limit;
    uint64_t *const running = call->running + (call->folded & 1) * block, *const running_next = call->running + (~call->folded & 1) * block;
    size_t const stride = call->direct ? call->row_stride : limit;
    uint64_t *const indices = !limit ? NULL : call->direct ? call->indices + q0 * stride : call->staged;
    uint64_t *const scores = !limit || !call->scores ? NULL : call->direct ? call->scores + q0 * stride : call->staged + rows * limit;
    if (limit) ++call->folded; /* the store pass moves the counts to the other half */
    return (hipError_t)szs_hip_within_fold(call->cells, columns, (uint32_t)rows, (uint32_t)columns, c0, self ? q0 : ~(uint64_t)0, call->bound,
                                           call->descending, (uint32_t)call->plan.cut.segments, (uint32_t)call->plan.segment_columns,
                                           call->partials, running, running_next, (uint32_t)limit, indices, scores, stride, call->stream);
}

hipError_t szs_selection_within_finish(szs_selection_within_t *call, size_t q0, size_t rows) {
    size_t const block = call->plan.cut.block, limit = call->limit, row_stride = call->row_stride;
    uint64_t *const counts = call->direct_counts ? call->counts + q0 : call->staged_counts;
    size_t const stride = call->direct ? row_stride : limit;
    uint64_t *const indices = !limit ? NULL : call->direct ? call->indices + q0 * stride : call->staged;
    uint64_t *const scores = !limit || !call->scores ? NULL : call->direct ? call->scores + q0 * stride : call->staged + rows * limit;
    /* without a limit no store pass has moved the partials into the running counts: the finish sums them */
    hipError_t error = (hipError_t)szs_hip_within_finish(call->running + (call->folded & 1) * block, call->partials,
                                                         limit ? 0 : (uint32_t)call->plan.cut.segments, (uint32_t)rows, (uint32_t)limit, counts,
                                                         indices, scores, stride, call->stream);
    if (error == hipSuccess && !call->direct_counts)
        error = hipMemcpyAsync(call->counts + q0, counts, rows * sizeof(uint64_t), hipMemcpyDefault, call->stream);
    if (error == hipSuccess && !call->direct)
        error = hipMemcpy2DAsync(call->indices + q0 * row_stride, row_stride * sizeof(uint64_t), indices, limit * sizeof(uint64_t),
                                 limit * sizeof(uint64_t), rows, hipMemcpyDefault, call->stream);
    if (error == hipSuccess && !call->direct && scores)
        error = hipMemcpy2DAsync(call->scores + q0 * row_stride, row_stride * sizeof(uint64_t), scores, limit * sizeof(uint64_t),
                                 limit * sizeof(uint64_t), rows, hipMemcpyDefault, call->stream);
    return error;
}

/* ---- the forest fold (hip/clusters.hip) --------------------------------------------------------------------------------------- */

sz_status_t szs_selection_clusters_reserve(szs_selection_clusters_t *call, szs_selection_buffers_t *buffers, char const **error_message) {
    size_t const count = call->count;
    /* labels a kernel can write go straight there; others (plain host memory) are staged and copied in one piece */
    call->direct = szs_classify_pointer(call->labels).device_accessible;
    sz_status_t status = szs_buffer_reserve(&buffers->scratch, szs_memory_device_k, call->device,
                                            call->plan.cut.block * call->plan.cut.tile * sizeof(uint64_t), error_message);
    if (status == sz_success_k)
        status = szs_buffer_reserve(&buffers->lists, szs_memory_device_k, call->device, sizeof(uint64_t) + count * sizeof(uint32_t), error_message);
    if (status == sz_success_k && !call->direct)
        status = szs_buffer_reserve(&buffers->out, szs_memory_device_k, call->device, count * sizeof(uint64_t), error_message);
    call->cells = (uint64_t *)buffers->scratch.pointer, call->roots = (uint64_t *)buffers->lists.pointer;
    call->parent = (uint32_t *)(call->roots + 1), call->staged = (uint64_t *)buffers->out.pointer;
    return status;
}

hipError_t szs_selection_clusters_begin(szs_selection_clusters_t const *call) {
    hipError_t const error = hipMemsetAsync(call->roots, 0, sizeof(uint64_t), call->stream);
    return error != hipSuccess ? error : (hipError_t)szs_hip_clusters_begin(call->parent, (uint32_t)call->count, call->stream);
}

hipError_t szs_selection_clusters_fold(szs_selection_clusters_t const *call, size_t q0, size_t rows, size_t c0, size_t columns) {
    return (hipError_t)szs_hip_clusters_union(call->cells, columns, (uint32_t)rows, (uint32_t)columns, q0, c0, call->bound, call->descending,
                                              (uint32_t)call->plan.cut.segments, (uint32_t)call->plan.segment_columns, call->parent,
                                              (uint32_t)call->count, call->stream);
}

hipError_t szs_selection_clusters_finish(szs_selection_clusters_t const *call, uint64_t *clusters_count) {
    uint64_t *const labels = call->direct ? call->labels : call->staged;
    hipError_t error = (hipError_t)szs_hip_clusters_finish(call->parent, (uint32_t)call->count, labels, call->roots, call->stream);
    if (error == hipSuccess && !call->direct)
        error = hipMemcpyAsync(call->labels, labels, call->count * sizeof(uint64_t), hipMemcpyDefault, call->stream);
    if (error == hipSuccess) error = hipMemcpyAsync(clusters_count, call->roots, sizeof(uint64_t), hipMemcpyDeviceToHost, call->stream);
    return error;
}
