/*
 *  listed_pairs.c - the skeleton of a call over LISTED pairs (rerank_internal.h): what szs_rocm_rerank* (rerank.c) and
 *  szs_rocm_fuzzy_find* (fuzzy_find.c) do alike around their own kernels - blocks of at most 2^20 rows, every row of a block dealt
 *  by descending query length into launches that read the indices and write the outputs where they are when the device can reach
 *  them.  Indices the host can read are validated before anything is launched; indices only the device can read are checked by the
 *  kernels (`index < count` before every use, a flag in pinned memory).
 */
#include "rerank_internal.h"

sz_status_t szs_listed_open(szs_listed_call_t *call, szs_engine_s *engine, szs_scope_s *scope, size_t k, size_t row_stride,
                            char const **error_message) {
    memset(call, 0, sizeof(*call));
    sz_status_t const status = szs_scope_bind_gpu(scope, &call->device, &call->stream, error_message);
    if (status != sz_success_k) return status;
    szs_engine_follow_device(engine, call->device);
    if (engine->events_device != call->device) {
        hipError_t error = hipEventCreate(&engine->event_start);
        if (error == hipSuccess) error = hipEventCreate(&engine->event_stop);
        if (error != hipSuccess) return szs_report_hip(error, error_message);
        engine->events_device = call->device;
    }
    call->engine = engine, call->k = k, call->row_stride = row_stride;
    return sz_success_k;
}

int szs_listed_indices_ok(uint64_t const *indices, size_t rows, size_t k, size_t row_stride, size_t count) {
    for (size_t q = 0; q < rows; ++q)
        for (size_t r = 0; r < k; ++r) {
            uint64_t const index = indices[q * row_stride + r];
            if (index != SZS_RERANK_EMPTY && index >= count) return 0;
        }
    return 1;
}

static sz_status_t host_offsets_of(szs_input_t const *input, szs_buffer_t *copy, hipStream_t stream, void const **offsets,
                                   char const **error_message) {
    *offsets = input->offsets;
    if (input->kind == szs_input_sequence_k) return sz_success_k;
    if (!input->offsets) return szs_report(sz_status_unknown_k, error_message, "Tape offsets must not be null");
    if (szs_classify_pointer(input->offsets).host_readable) return sz_success_k;
    size_t const bytes = (input->count + 1) * (input->kind == szs_input_u32tape_k ? 4 : 8);
    sz_status_t const status = szs_buffer_reserve(copy, szs_memory_host_k, 0, bytes, error_message);
    if (status != sz_success_k) return status;
    hipError_t error = hipMemcpyAsync(copy->pointer, input->offsets, bytes, hipMemcpyDeviceToHost, stream);
    if (error == hipSuccess) error = hipStreamSynchronize(stream);
    if (error != hipSuccess) return szs_report_hip(error, error_message);
    *offsets = copy->pointer;
    return sz_success_k;
}

sz_status_t szs_listed_offsets(szs_listed_call_t *call, szs_input_t const *queries, szs_input_t const *candidates,
                               char const **error_message) {
    szs_engine_s *const engine = call->engine;
    sz_status_t status = host_offsets_of(queries, &engine->host_rerank_offsets[0], call->stream, &call->offsets[0], error_message);
    if (status == sz_success_k && candidates)
        status = host_offsets_of(candidates, &engine->host_rerank_offsets[1], call->stream, &call->offsets[1], error_message);
    if (!candidates) call->offsets[1] = call->offsets[0];
    return status;
}

size_t szs_listed_block_rows(size_t q_count, size_t k, int within_stage_budget) {
    size_t block = q_count < SZS_RERANK_MOST_ROWS ? q_count : SZS_RERANK_MOST_ROWS;
    if (within_stage_budget && block > SZS_RERANK_STAGE_BYTES / (k * sizeof(uint64_t))) block = SZS_RERANK_STAGE_BYTES / (k * sizeof(uint64_t));
    return block < 1 ? 1 : block;
}

/** One part of a scratch layout: `bytes` at `*end`, 16-byte aligned, each part behind the one before it. */
static size_t layout_part(size_t *end, size_t bytes) {
    size_t const at = *end;
    *end = at + ((bytes + 15) & ~(size_t)15);
    return at;
}

/** A side does not need refs when it is a tape whose offsets the device reads itself. */
static int side_needs_refs(szs_input_t const *input) {
    return input->kind == szs_input_sequence_k || !szs_classify_pointer(input->offsets).device_accessible;
}

sz_status_t szs_listed_reserve(szs_listed_call_t *call, szs_input_t const *queries, szs_input_t const *candidates, int kernels,
                               size_t const host_extra[2], size_t const pinned_extra[2], size_t staged_arrays, void *extras[4],
                               char const **error_message) {
    szs_engine_s *const engine = call->engine;
    size_t const q_count = queries->count, block = call->block;
    call->refs_needed[0] = kernels && side_needs_refs(queries), call->refs_needed[1] = kernels && candidates && side_needs_refs(candidates);
    call->refs_count[0] = call->refs_needed[0] ? q_count : 0, call->refs_count[1] = call->refs_needed[1] ? candidates->count : 0;
    size_t const gathered = call->refs_count[0] > call->refs_count[1] ? call->refs_count[0] : call->refs_count[1]; /* the larger side */
    size_t const refs_total = call->refs_count[0] + call->refs_count[1];                                           /* queries, then candidates */

    size_t end = 0;
    size_t const host_query_lengths = layout_part(&end, q_count * sizeof(uint32_t));
    size_t const host_addresses = layout_part(&end, gathered * sizeof(uint64_t));
    size_t const host_gathered_lengths = layout_part(&end, gathered * sizeof(uint32_t));
    size_t const host_extras[2] = {layout_part(&end, host_extra[0]), layout_part(&end, host_extra[1])};
    size_t const host_bytes = end;
    end = 0;
    size_t const pinned_flags = layout_part(&end, SZS_RERANK_FLAGS * sizeof(uint32_t)); /* the kernels' */
    size_t const pinned_landed = layout_part(&end, 3 * sizeof(uint64_t));               /* their counters, downloaded */
    size_t const pinned_extras[2] = {layout_part(&end, pinned_extra[0]), layout_part(&end, pinned_extra[1])};
    size_t const pinned_rows = layout_part(&end, block * sizeof(uint32_t));
    size_t const pinned_refs = layout_part(&end, refs_total * sizeof(szs_string_ref_t));
    size_t const pinned_bytes = end;
    end = 0;
    size_t const device_counters = layout_part(&end, 3 * sizeof(uint64_t));
    size_t const device_rows = layout_part(&end, block * sizeof(uint32_t));
    size_t const device_refs = layout_part(&end, refs_total * sizeof(szs_string_ref_t));
    size_t const device_bytes = end;

    sz_status_t status = szs_buffer_reserve(&engine->host_rerank, szs_memory_host_k, 0, host_bytes, error_message);
    if (status == sz_success_k) status = szs_buffer_reserve(&engine->pinned_rerank, szs_memory_pinned_k, call->device, pinned_bytes, error_message);
    if (status == sz_success_k && kernels)
        status = szs_buffer_reserve(&engine->device_rerank, szs_memory_device_k, call->device, device_bytes, error_message);
    if (status == sz_success_k && kernels && staged_arrays)
        status = szs_buffer_reserve(&engine->device_rerank_staged, szs_memory_device_k, call->device,
                                    staged_arrays * block * call->k * sizeof(uint64_t), error_message);
    if (status != sz_success_k) return status;
    char *const host = (char *)engine->host_rerank.pointer, *const pinned = (char *)engine->pinned_rerank.pointer;
    call->query_lengths = (uint32_t *)(host + host_query_lengths);
    call->addresses = (uint64_t *)(host + host_addresses), call->gathered_lengths = (uint32_t *)(host + host_gathered_lengths);
    call->flags = (uint32_t *)(pinned + pinned_flags), call->landed = (uint64_t *)(pinned + pinned_landed);
    call->order = (uint32_t *)(pinned + pinned_rows), call->pinned_refs = (szs_string_ref_t *)(pinned + pinned_refs);
    extras[0] = host + host_extras[0], extras[1] = host + host_extras[1];
    extras[2] = pinned + pinned_extras[0], extras[3] = pinned + pinned_extras[1];
    if (!kernels) return sz_success_k;
    char *const remote = (char *)engine->device_rerank.pointer;
    call->device_counters = (unsigned long long *)(remote + device_counters);
    call->device_order = (uint32_t *)(remote + device_rows), call->device_refs = (szs_string_ref_t *)(remote + device_refs);
    return sz_success_k;
}

/**
 *  Side `which` as the kernels read it: the tape itself, or refs in index order built on the host and uploaded.  `*usable` 0: the
 *  kernels cannot reach the side's strings (or its offsets are malformed).
 */
static sz_status_t kernel_side(szs_listed_call_t *call, int which, szs_input_t const *input, int *usable, char const **error_message) {
    szs_rerank_side_t *const side = &call->sides[which];
    void const *const offsets = call->offsets[which];
    memset(side, 0, sizeof(*side));
    side->count = input->count, *usable = 1;
    if (!call->refs_needed[which]) {
        side->offsets = input->offsets, side->base = (uint64_t)(uintptr_t)input->data, side->wide = input->kind == szs_input_u64tape_k;
        uint64_t const bytes = szs_tape_offset(input, offsets, input->count) - szs_tape_offset(input, offsets, 0);
        *usable = !bytes || szs_classify_pointer(input->data).device_accessible;
        return sz_success_k;
    }
    char const *ignored = NULL;
    uint64_t bytes = 0;
    if (szs_gather_strings(input, offsets, call->addresses, call->gathered_lengths, &bytes, NULL, &ignored) != sz_success_k) {
        *usable = 0;
        return sz_success_k;
    }
    size_t const first = which ? call->refs_count[0] : 0; /* the candidates' refs lie behind the queries' */
    szs_string_ref_t *const pinned_refs = call->pinned_refs + first, *const device_refs = call->device_refs + first;
    for (size_t i = 0; i < input->count; ++i)
        pinned_refs[i].address = call->addresses[i], pinned_refs[i].length = call->gathered_lengths[i], pinned_refs[i].index = (uint32_t)i;
    side->refs = device_refs;
    if (!input->count) return sz_success_k;
    hipError_t const error =
        hipMemcpyAsync(device_refs, pinned_refs, input->count * sizeof(szs_string_ref_t), hipMemcpyHostToDevice, call->stream);
    return error == hipSuccess ? sz_success_k : szs_report_hip(error, error_message);
}

sz_status_t szs_listed_prepare_queries(szs_listed_call_t *call, szs_input_t const *queries, uint32_t longest_query, int *usable,
                                       char const **error_message) {
    sz_status_t const status = kernel_side(call, 0, queries, usable, error_message);
    if (status != sz_success_k || !*usable) return status;
    /* the lengths of the queries: which rows a kernel takes, and the order it takes them in */
    for (size_t q = 0; q < queries->count; ++q) {
        uint64_t length = ~(uint64_t)0;
        if (call->refs_needed[0]) length = call->gathered_lengths[q];
        else {
            uint64_t const from = szs_tape_offset(queries, call->offsets[0], q), to = szs_tape_offset(queries, call->offsets[0], q + 1);
            if (to >= from) length = to - from;
        }
        call->query_lengths[q] = length <= longest_query ? (uint32_t)length : ~0u;
    }
    return sz_success_k;
}

sz_status_t szs_listed_prepare_candidates(szs_listed_call_t *call, szs_input_t const *candidates, int *usable, char const **error_message) {
    if (candidates) return kernel_side(call, 1, candidates, usable, error_message);
    call->sides[1] = call->sides[0], *usable = 1;
    return sz_success_k;
}

hipError_t szs_listed_block_begin(szs_listed_call_t *call, size_t dealt, hipError_t error) {
    memset(call->flags, 0, SZS_RERANK_FLAGS * sizeof(uint32_t));
    if (error == hipSuccess) error = hipMemsetAsync(call->device_counters, 0, 3 * sizeof(uint64_t), call->stream);
    if (error == hipSuccess && dealt) /* (none: a launch that takes no row list - the search's tile) */
        error = hipMemcpyAsync(call->device_order, call->order, dealt * sizeof(uint32_t), hipMemcpyHostToDevice, call->stream);
    if (error == hipSuccess) error = hipEventRecord(call->engine->event_start, call->stream);
    return error;
}

hipError_t szs_listed_block_end(szs_listed_call_t *call, hipError_t error) {
    if (error == hipSuccess) error = hipEventRecord(call->engine->event_stop, call->stream);
    if (error == hipSuccess)
        error = hipMemcpyAsync(call->landed, call->device_counters, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, call->stream);
    return error;
}

sz_status_t szs_listed_block_finish(szs_listed_call_t *call, hipError_t error, hipError_t *hip_error, unsigned launches, uint32_t longest,
                                    size_t bytes_per_pair, sz_status_t unfit_status, char const *unfit_message, char const **error_message) {
    hipError_t const drained = hipStreamSynchronize(call->stream);
    if (error == hipSuccess) error = drained;
    if (error != hipSuccess) {
        *hip_error = error;
        return sz_success_k;
    }
    if (call->flags[SZS_RERANK_FLAG_UNFIT]) return szs_report(unfit_status, error_message, unfit_message);
    if (call->flags[SZS_RERANK_FLAG_TAPE]) return szs_report(sz_unexpected_dimensions_k, error_message, "Tape offsets must ascend");
    if (call->flags[SZS_RERANK_FLAG_INDEX]) return szs_report(sz_unexpected_dimensions_k, error_message, "An index is beyond the candidates");
    float milliseconds = 0;
    if (hipEventElapsedTime(&milliseconds, call->engine->event_start, call->engine->event_stop) != hipSuccess) (void)hipGetLastError();
    szs_rocm_call_profile_t *const total = &call->total;
    total->kernel_milliseconds += milliseconds, total->launches += launches;
    total->pairs += call->landed[0], total->cells += call->landed[1];
    total->algorithmic_bytes += call->landed[2] + call->landed[0] * bytes_per_pair;
    if (longest > total->longest_query) total->longest_query = longest;
    return sz_success_k;
}

sz_status_t szs_listed_close(szs_listed_call_t *call, sz_status_t status, hipError_t error, double started, char const **error_message) {
    hipError_t const drained = hipStreamSynchronize(call->stream); /* synchronous, also when it fails */
    if (status != sz_success_k) return status;
    if (error == hipSuccess) error = drained;
    if (error != hipSuccess) return szs_report_hip(error, error_message);
    call->engine->last_profile = call->total; /* the sums over the call; every other field blank */
    call->engine->last_profile.host_milliseconds = szs_now_milliseconds() - started;
    return szs_report(sz_success_k, error_message, NULL);
}
