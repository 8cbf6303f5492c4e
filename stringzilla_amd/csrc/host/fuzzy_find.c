/*
 *  fuzzy_find.c - the best match of a query INSIDE each listed candidate (szs_rocm_fuzzy_find*, include/stringzillas/stringzillas_rocm.h;
 *  DESIGN.md section 4.9): distances[q][r] = the fewest edits that turn queries[q] into some substring of candidates[indices[q][r]],
 *  ends[q][r] = the smallest exclusive byte offset at which such a substring ends; szs_rocm_fuzzy_find_spans* add starts[q][r] = where
 *  the shortest such substring that ends there begins - a second launch (hip/myers_fuzzy_spans.hip) behind the first, on the same
 *  stream and inside the same event pair, and only in a call that asks for it.
 *
 *  The shape is rerank.c's kernel route alone (rerank_internal.h has what the two share): blocks of at most 2^20 rows, every row of a
 *  block in ONE launch of hip/myers_fuzzy_find.hip, dealt by descending query length; the kernel reads the indices and writes the
 *  outputs where they are when the device can reach them, else through a dense copy of the block - one 2-D copy per array.  There is
 *  no other route: no engine call computes a semi-global distance, so an engine that is not unit-cost byte Levenshtein, a query of
 *  more than SZS_RERANK_LONGEST_QUERY bytes and strings the device cannot read are refused.  Indices the host can read are validated
 *  before anything is launched; indices only the device can read are checked by the kernel (`index < count` before every use, a flag
 *  in pinned memory).  The scratch is the engine's rerank buffers (szs_internal.h): grow-only, released with the engine.
 */
#include "rerank_internal.h"

/** Byte offsets of every part of the engine's buffers: computed in ONE place, each part behind the one before it. */
typedef struct {
    /* engine->host_rerank */
    size_t host_query_lengths;    /* u32 x queries */
    size_t host_addresses;        /* u64 x gathered strings of the larger side */
    size_t host_gathered_lengths; /* u32 x the same */
    size_t host_bytes;
    /* engine->pinned_rerank */
    size_t pinned_flags;  /* u32 x SZS_RERANK_FLAGS: the kernel's */
    size_t pinned_landed; /* u64 x 3: the kernel's counters, downloaded */
    size_t pinned_rows;   /* u32 x block: the kernel's rows */
    size_t pinned_refs;   /* refs of the queries, then of the candidates */
    size_t pinned_bytes;
    /* engine->device_rerank */
    size_t device_counters; /* u64 x 3 */
    size_t device_rows;     /* u32 x block */
    size_t device_refs;     /* as pinned_refs */
    size_t device_bytes;
} szs_fuzzy_find_layout_t;

static szs_fuzzy_find_layout_t fuzzy_find_layout(size_t q_count, size_t gathered, size_t block, size_t refs_total) {
    szs_fuzzy_find_layout_t layout;
    size_t end = 0;
    layout.host_query_lengths = szs_layout_part(&end, q_count * sizeof(uint32_t));
    layout.host_addresses = szs_layout_part(&end, gathered * sizeof(uint64_t));
    layout.host_gathered_lengths = szs_layout_part(&end, gathered * sizeof(uint32_t));
    layout.host_bytes = end, end = 0;
    layout.pinned_flags = szs_layout_part(&end, SZS_RERANK_FLAGS * sizeof(uint32_t));
    layout.pinned_landed = szs_layout_part(&end, 3 * sizeof(uint64_t));
    layout.pinned_rows = szs_layout_part(&end, block * sizeof(uint32_t));
    layout.pinned_refs = szs_layout_part(&end, refs_total * sizeof(szs_string_ref_t));
    layout.pinned_bytes = end, end = 0;
    layout.device_counters = szs_layout_part(&end, 3 * sizeof(uint64_t));
    layout.device_rows = szs_layout_part(&end, block * sizeof(uint32_t));
    layout.device_refs = szs_layout_part(&end, refs_total * sizeof(szs_string_ref_t));
    layout.device_bytes = end;
    return layout;
}

/** What the blocks of one call share. */
typedef struct {
    szs_engine_s *engine;
    hipStream_t stream;
    size_t k, row_stride, block;
    uint64_t const *indices; /* NULL: the dense form */
    uint64_t *distances, *ends, *starts; /* `starts` NULL: the plain call - one launch a block */
    int stage_indices, stage_distances, stage_ends, stage_starts;
    szs_rerank_side_t sides[2];
    uint32_t *query_lengths, *flags, *order, *device_order;
    uint64_t *landed;
    unsigned long long *device_counters;
    szs_rocm_call_profile_t total;
} szs_fuzzy_find_call_t;

/** One block: stages what the device cannot reach, launches the kernel once over every row - and the kernel of the starts behind it,
 *  where the call asks for them - brings the outputs home, reads the flags. */
static sz_status_t fuzzy_find_block(szs_fuzzy_find_call_t *call, size_t q0, size_t rows, hipError_t *hip_error, char const **error_message) {
    szs_engine_s *const engine = call->engine;
    hipStream_t const stream = call->stream;
    size_t const k = call->k, row_stride = call->row_stride, row_bytes = k * sizeof(uint64_t), pitch = row_stride * sizeof(uint64_t);
    uint32_t longest = 0;
    size_t const dealt = szs_deal_short_rows(call->query_lengths + q0, rows, call->order, &longest); /* every row: the caller saw to it */
    unsigned const widest = longest ? (longest + 31) / 32 : 1;

    uint64_t *staged = (uint64_t *)engine->device_rerank_staged.pointer;
    uint64_t const *kernel_indices = call->indices ? call->indices + q0 * row_stride : NULL;
    uint64_t *kernel_distances = call->distances + q0 * row_stride, *kernel_ends = call->ends ? call->ends + q0 * row_stride : NULL;
    uint64_t *kernel_starts = call->starts ? call->starts + q0 * row_stride : NULL;
    size_t indices_stride = row_stride;
    hipError_t error = hipSuccess;
    if (call->stage_indices) {
        error = hipMemcpy2DAsync(staged, row_bytes, call->indices + q0 * row_stride, pitch, row_bytes, rows, hipMemcpyHostToDevice, stream);
        kernel_indices = staged, indices_stride = k, staged += call->block * k;
    }
    /* the kernels' outputs share one stride: all staged (dense), or all the caller's */
    int const dense_outputs = call->stage_distances || call->stage_ends || call->stage_starts;
    if (dense_outputs) {
        kernel_distances = staged, staged += call->block * k;
        if (call->ends) kernel_ends = staged, staged += call->block * k;
        if (call->starts) kernel_starts = staged;
    }
    size_t const outputs_stride = dense_outputs ? k : row_stride;
    memset(call->flags, 0, SZS_RERANK_FLAGS * sizeof(uint32_t));
    if (error == hipSuccess) error = hipMemsetAsync(call->device_counters, 0, 3 * sizeof(uint64_t), stream);
    if (error == hipSuccess) error = hipMemcpyAsync(call->device_order, call->order, dealt * sizeof(uint32_t), hipMemcpyHostToDevice, stream);
    if (error == hipSuccess) error = hipEventRecord(engine->event_start, stream);
    if (error == hipSuccess)
        error = (hipError_t)szs_hip_levenshtein_fuzzy_find(&call->sides[0], &call->sides[1], q0, call->device_order, (uint32_t)dealt,
                                                           kernel_indices, indices_stride, k, kernel_distances, kernel_ends, outputs_stride,
                                                           widest, call->flags, call->device_counters, stream);
    if (error == hipSuccess && call->starts) /* behind the first launch on the same stream: it reads what that one wrote */
        error = (hipError_t)szs_hip_levenshtein_fuzzy_starts(&call->sides[0], &call->sides[1], q0, call->device_order, (uint32_t)dealt,
                                                             kernel_indices, indices_stride, k, kernel_distances, kernel_ends, kernel_starts,
                                                             outputs_stride, widest, call->flags, call->device_counters, stream);
    if (error == hipSuccess) error = hipEventRecord(engine->event_stop, stream);
    if (error == hipSuccess) error = hipMemcpyAsync(call->landed, call->device_counters, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, stream);
    if (error == hipSuccess && dense_outputs)
        error = hipMemcpy2DAsync(call->distances + q0 * row_stride, pitch, kernel_distances, row_bytes, row_bytes, rows,
                                 call->stage_distances ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, stream);
    if (error == hipSuccess && dense_outputs && call->ends)
        error = hipMemcpy2DAsync(call->ends + q0 * row_stride, pitch, kernel_ends, row_bytes, row_bytes, rows,
                                 call->stage_ends ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, stream);
    if (error == hipSuccess && dense_outputs && call->starts)
        error = hipMemcpy2DAsync(call->starts + q0 * row_stride, pitch, kernel_starts, row_bytes, row_bytes, rows,
                                 call->stage_starts ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, stream);
    hipError_t const drained = hipStreamSynchronize(stream);
    if (error == hipSuccess) error = drained;
    if (error != hipSuccess) {
        *hip_error = error;
        return sz_success_k;
    }
    if (call->flags[SZS_RERANK_FLAG_UNFIT])
        return szs_report(sz_unexpected_dimensions_k, error_message, "A query of more than 256 bytes: beyond what fuzzy find takes");
    if (call->flags[SZS_RERANK_FLAG_TAPE]) return szs_report(sz_unexpected_dimensions_k, error_message, "Tape offsets must ascend");
    if (call->flags[SZS_RERANK_FLAG_INDEX]) return szs_report(sz_unexpected_dimensions_k, error_message, "An index is beyond the candidates");
    float milliseconds = 0;
    if (hipEventElapsedTime(&milliseconds, engine->event_start, engine->event_stop) != hipSuccess) (void)hipGetLastError();
    szs_rocm_call_profile_t *const total = &call->total;
    total->kernel_milliseconds += milliseconds, total->launches += call->starts ? 2 : 1;
    total->pairs += call->landed[0], total->cells += call->landed[1]; /* with starts: the cells and bytes of the reverse windows too */
    total->algorithmic_bytes += call->landed[2] + call->landed[0] * (2 * 4 + 8 + (call->ends ? 8 : 0) + (call->starts ? 8 : 0));
    if (longest > total->longest_query) total->longest_query = longest;
    return sz_success_k;
}

/** The one call path.  `starts` set: the starts are computed too.  `missing`: the message for a required output that is NULL, refused
 *  behind the checks of the dimensions, the engine and an empty batch; NULL when the entry has all it requires. */
static sz_status_t fuzzy_find_call(szs_engine_s *engine, szs_scope_s *scope, szs_input_t const *queries, szs_input_t const *candidates,
                                   size_t const *indices, size_t k, size_t *distances, size_t *starts, size_t *ends, size_t row_stride,
                                   char const *missing, char const **error_message) {
    double const started = szs_now_milliseconds();
    if (k < 1 || row_stride < k) return szs_report(sz_unexpected_dimensions_k, error_message, "k must be at least 1 and row_stride at least k");
    if (!engine || engine->magic != SZS_ENGINE_MAGIC || engine->family != szs_family_levenshtein_k || !engine->is_unit_cost)
        return szs_report(sz_status_unknown_k, error_message, "Fuzzy find needs an initialized unit-cost byte Levenshtein engine");
    if (!queries) return szs_report(sz_status_unknown_k, error_message, "Queries must not be null");
    if (!queries->count) return szs_report(sz_success_k, error_message, NULL);
    if (missing) return szs_report(sz_status_unknown_k, error_message, missing);
    szs_input_t const *const pool = candidates ? candidates : queries; /* the self form: the indices refer to the queries */
    size_t const q_count = queries->count, c_count = pool->count;
    if (!indices && k != c_count)
        return szs_report(sz_unexpected_dimensions_k, error_message, "Without indices k must be the number of candidates");
    if (k > (~(size_t)0 >> 4) / sizeof(uint64_t)) return szs_report(sz_overflow_risk_k, error_message, NULL);

    int device = 0;
    hipStream_t stream = NULL;
    sz_status_t status = szs_scope_bind_gpu(scope, &device, &stream, error_message);
    if (status != sz_success_k) return status;
    szs_engine_follow_device(engine, device);
    if (engine->events_device != device) {
        hipError_t error = hipEventCreate(&engine->event_start);
        if (error == hipSuccess) error = hipEventCreate(&engine->event_stop);
        if (error != hipSuccess) return szs_report_hip(error, error_message);
        engine->events_device = device;
    }

    szs_fuzzy_find_call_t call;
    memset(&call, 0, sizeof(call));
    call.engine = engine, call.stream = stream, call.k = k, call.row_stride = row_stride;
    call.indices = (uint64_t const *)indices, call.distances = (uint64_t *)distances, call.ends = (uint64_t *)ends;
    call.starts = (uint64_t *)starts;

    /* indices the host can read: validated before anything is launched */
    if (indices && szs_classify_pointer(indices).host_readable)
        for (size_t q = 0; q < q_count; ++q)
            for (size_t r = 0; r < k; ++r)
                if (szs_index_is_bad(call.indices[q * row_stride + r], c_count))
                    return szs_report(sz_unexpected_dimensions_k, error_message, "An index is beyond the candidates");

    void const *query_offsets = NULL, *pool_offsets = NULL;
    status = szs_host_offsets_of(queries, &engine->host_rerank_offsets[0], stream, &query_offsets, error_message);
    if (status == sz_success_k && candidates) status = szs_host_offsets_of(candidates, &engine->host_rerank_offsets[1], stream, &pool_offsets, error_message);
    if (status != sz_success_k) return status;
    if (!candidates) pool_offsets = query_offsets;

    /* blocks of rows: the kernel's row list and - where the device cannot reach the caller's arrays - their dense copies in budget */
    call.stage_indices = indices && !szs_classify_pointer(indices).device_accessible;
    call.stage_distances = !szs_classify_pointer(distances).device_accessible;
    call.stage_ends = ends && !szs_classify_pointer(ends).device_accessible;
    call.stage_starts = starts && !szs_classify_pointer(starts).device_accessible;
    int const dense_outputs = call.stage_distances || call.stage_ends || call.stage_starts;
    size_t const staged_arrays = (size_t)call.stage_indices + (dense_outputs ? 1 + (ends != NULL) + (starts != NULL) : 0);
    size_t block = q_count < SZS_RERANK_MOST_ROWS ? q_count : SZS_RERANK_MOST_ROWS;
    if (staged_arrays && block > SZS_RERANK_STAGE_BYTES / (k * sizeof(uint64_t))) block = SZS_RERANK_STAGE_BYTES / (k * sizeof(uint64_t));
    if (block < 1) block = 1;
    call.block = block;

    int const refs_needed[2] = {szs_side_needs_refs(queries), candidates && szs_side_needs_refs(candidates)};
    size_t const refs_count[2] = {refs_needed[0] ? q_count : 0, refs_needed[1] ? c_count : 0};
    size_t const gathered = refs_count[0] > refs_count[1] ? refs_count[0] : refs_count[1];
    szs_fuzzy_find_layout_t const layout = fuzzy_find_layout(q_count, gathered, block, refs_count[0] + refs_count[1]);
    status = szs_buffer_reserve(&engine->host_rerank, szs_memory_host_k, 0, layout.host_bytes, error_message);
    if (status == sz_success_k) status = szs_buffer_reserve(&engine->pinned_rerank, szs_memory_pinned_k, device, layout.pinned_bytes, error_message);
    if (status == sz_success_k) status = szs_buffer_reserve(&engine->device_rerank, szs_memory_device_k, device, layout.device_bytes, error_message);
    if (status == sz_success_k && staged_arrays)
        status = szs_buffer_reserve(&engine->device_rerank_staged, szs_memory_device_k, device, staged_arrays * block * k * sizeof(uint64_t),
                                    error_message);
    if (status != sz_success_k) return status;
    char *const host = (char *)engine->host_rerank.pointer, *const pinned = (char *)engine->pinned_rerank.pointer;
    char *const remote = (char *)engine->device_rerank.pointer;
    call.query_lengths = (uint32_t *)(host + layout.host_query_lengths);
    call.flags = (uint32_t *)(pinned + layout.pinned_flags), call.landed = (uint64_t *)(pinned + layout.pinned_landed);
    call.order = (uint32_t *)(pinned + layout.pinned_rows);
    call.device_counters = (unsigned long long *)(remote + layout.device_counters);
    call.device_order = (uint32_t *)(remote + layout.device_rows);
    szs_string_ref_t *const pinned_refs = (szs_string_ref_t *)(pinned + layout.pinned_refs);
    szs_string_ref_t *const device_refs = (szs_string_ref_t *)(remote + layout.device_refs);
    uint64_t *const addresses = (uint64_t *)(host + layout.host_addresses);
    uint32_t *const lengths = (uint32_t *)(host + layout.host_gathered_lengths);

    int usable = 0;
    status = szs_kernel_side(queries, query_offsets, refs_needed[0], addresses, lengths, pinned_refs, device_refs, stream, &call.sides[0], &usable,
                             error_message);
    if (status != sz_success_k) return status;
    if (!usable) return szs_report(sz_status_unknown_k, error_message, "The queries are not strings the device can read");
    /* the lengths of the queries: the order the kernel takes the rows in - and a query beyond its bit-vector fails the call here */
    for (size_t q = 0; q < q_count; ++q) {
        uint64_t length = 0;
        if (refs_needed[0]) length = lengths[q];
        else {
            uint64_t const from = szs_tape_offset(queries, query_offsets, q), to = szs_tape_offset(queries, query_offsets, q + 1);
            if (to < from) return szs_report(sz_unexpected_dimensions_k, error_message, "Tape offsets must ascend");
            length = to - from;
        }
        if (length > SZS_RERANK_LONGEST_QUERY)
            return szs_report(sz_unexpected_dimensions_k, error_message, "A query of more than 256 bytes: beyond what fuzzy find takes");
        call.query_lengths[q] = (uint32_t)length;
    }
    if (candidates) {
        status = szs_kernel_side(candidates, pool_offsets, refs_needed[1], addresses, lengths, pinned_refs + refs_count[0],
                                 device_refs + refs_count[0], stream, &call.sides[1], &usable, error_message);
        if (status != sz_success_k) return status;
        if (!usable) return szs_report(sz_status_unknown_k, error_message, "The candidates are not strings the device can read");
    }
    else call.sides[1] = call.sides[0];

    hipError_t error = hipSuccess;
    for (size_t q0 = 0; q0 < q_count && status == sz_success_k && error == hipSuccess; q0 += block)
        status = fuzzy_find_block(&call, q0, q_count - q0 < block ? q_count - q0 : block, &error, error_message);
    hipError_t const drained = hipStreamSynchronize(stream); /* synchronous, also when it fails */
    if (status != sz_success_k) return status;
    if (error == hipSuccess) error = drained;
    if (error != hipSuccess) return szs_report_hip(error, error_message);
    engine->last_profile = call.total; /* the sums over the call; every other field blank */
    engine->last_profile.host_milliseconds = szs_now_milliseconds() - started;
    return szs_report(sz_success_k, error_message, NULL);
}

sz_status_t szs_engine_fuzzy_find(szs_engine_s *engine, szs_scope_s *scope, szs_input_t const *queries, szs_input_t const *candidates,
                                  size_t const *indices, size_t k, size_t *distances, size_t *ends, size_t row_stride,
                                  char const **error_message) {
    return fuzzy_find_call(engine, scope, queries, candidates, indices, k, distances, NULL, ends, row_stride,
                           distances ? NULL : "Distances must not be null", error_message);
}

sz_status_t szs_engine_fuzzy_find_spans(szs_engine_s *engine, szs_scope_s *scope, szs_input_t const *queries, szs_input_t const *candidates,
                                        size_t const *indices, size_t k, size_t *distances, size_t *starts, size_t *ends,
                                        size_t row_stride, char const **error_message) {
    char const *const missing = !distances ? "Distances must not be null" : !starts || !ends ? "Starts and ends must not be null" : NULL;
    return fuzzy_find_call(engine, scope, queries, candidates, indices, k, distances, starts, ends, row_stride, missing, error_message);
}
