/* selection.c - the budget and the steps of a tiled selection (selection_internal.h). */
#include "selection_internal.h"

static size_t at_most(size_t value, size_t limit) { return value < limit ? value : limit; }

szs_selection_plan_t szs_selection_plan(size_t q_count, size_t c_count, size_t k, size_t most_block_rows, size_t most_tile_rows) {
    size_t const list_bytes = 2 * szs_hip_top_k_width((uint32_t)k) * sizeof(uint64_t);
    /* Every step but the last of `block` and of `tile` is a minimum, so the caller's caps may join in any order: the minimum of the
     * same terms is the same number.  `block` is at least 1 without a floor: the queries are, the lists allow 128 MiB / 16 KiB = 8192
     * rows (k = 1024), the scratch 16 Mi / 4096 = 4096, and the caller's cap is at least 1. */
    size_t const wide = c_count < 4096 ? (c_count ? c_count : 1) : 4096;
    size_t block = at_most(q_count, SZS_SELECTION_MOST_ROWS);
    block = at_most(block, SZS_SELECTION_LIST_BYTES / list_bytes);
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

hipError_t szs_selection_drain(szs_selection_t const *call, hipError_t error) {
    hipError_t const drained = hipStreamSynchronize(call->stream);
    return error == hipSuccess ? drained : error;
}
