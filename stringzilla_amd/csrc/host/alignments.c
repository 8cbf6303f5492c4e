/*
 *  alignments.c - WHICH edits: the edit script of every listed pair (szs_rocm_alignments*, include/stringzillas/stringzillas_rocm.h;
 *  DESIGN.md section 4.14): per slot the distance of the query and candidate[start : end] (or the whole candidate), the length L of
 *  the canonical script and its L ops `= X I D` in a slot of `capacity` bytes.
 *
 *  The call is fuzzy_find.c's on the skeleton of listed_pairs.c (rerank_internal.h) around one kernel: blocks of at most 2^20 rows,
 *  every row of a block in ONE launch of hip/myers_alignments.hip, dealt by descending query length; the kernel reads the indices and
 *  the spans and writes the outputs where they are when the device can reach them, else through dense copies of the block.  `ops` is
 *  the wide array: a staged block's rows are bounded by k x max(8, capacity) bytes a row.  The kernel's trace lives in a grow-only
 *  engine buffer of as many workgroup regions as SZS_ALIGN_TRACE_BYTES holds, and the grid is sized by it: the memory does not grow
 *  with the call.  There is no other route: an engine that is not unit-cost byte Levenshtein, a query of more than
 *  SZS_RERANK_LONGEST_QUERY bytes, a span of more than SZS_ALIGN_LONGEST_SPAN bytes and strings the device cannot read are refused.
 */
#include "rerank_internal.h"

/* The trace a call may hold: the size of the MI355X's Infinity Cache - a choice, not a measurement.  Fewer regions mean fewer
 * workgroups in flight, each serving more rows; the `align_trace_kib` knob overrides it (tests make two workgroups serve many rows). */
#define SZS_ALIGN_TRACE_BYTES ((size_t)256 << 20)

static char const alignments_long_query[] = "A query of more than 256 bytes: beyond what alignments take";
static char const alignments_long_span[] = "A span of more than 512 bytes: beyond what alignments take";

/** What the blocks of one alignments call share. */
typedef struct {
    szs_listed_call_t listed;
    uint64_t const *indices, *starts, *ends; /* `indices` NULL: the dense form; `starts` and `ends` NULL: whole candidates */
    uint64_t *distances, *lengths;
    uint8_t *ops; /* NULL: `capacity` is 0 */
    size_t capacity;
    int stage_inputs, stage_outputs; /* the inputs share one stride, and so do the outputs: all dense copies, or all the caller's */
} alignments_call_t;

static hipMemcpyKind kind_towards_device(void const *pointer) {
    return szs_classify_pointer(pointer).device_accessible ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
}
static hipMemcpyKind kind_from_device(void const *pointer) {
    return szs_classify_pointer(pointer).device_accessible ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
}

/** The workgroups of a block of `dealt` rows - the regions the budget holds, at least one, no more than the block's runs of rows. */
static uint32_t alignments_workgroups(size_t dealt, size_t k, unsigned widest) {
    int const knob = szs_tuning_get(szs_knob_align_trace_kib_k);
    size_t const budget = knob > 0 ? (size_t)knob << 10 : SZS_ALIGN_TRACE_BYTES;
    size_t const groups = 64 / szs_hip_rerank_lanes(k), runs = (dealt + groups - 1) / groups;
    size_t workgroups = budget / SZS_ALIGN_REGION_BYTES(widest);
    if (workgroups > runs) workgroups = runs;
    return workgroups < 1 ? 1u : (uint32_t)workgroups;
}

/** One block: stages what the device cannot reach, launches the kernel once over every row, brings the outputs home, reads the flags. */
static sz_status_t alignments_block(alignments_call_t *call, size_t q0, size_t rows, hipError_t *hip_error, char const **error_message) {
    szs_listed_call_t *const listed = &call->listed;
    szs_engine_s *const engine = listed->engine;
    hipStream_t const stream = listed->stream;
    size_t const k = listed->k, row_stride = listed->row_stride, capacity = call->capacity;
    size_t const row_bytes = k * sizeof(uint64_t), pitch = row_stride * sizeof(uint64_t);
    uint32_t longest = 0;
    size_t const dealt = szs_deal_short_rows(listed->query_lengths + q0, rows, listed->order, &longest); /* every row: the caller saw to it */
    unsigned const widest = longest ? (longest + 31) / 32 : 1;

    uint32_t const workgroups = alignments_workgroups(dealt, k, widest);
    sz_status_t const status = szs_buffer_reserve(&engine->device_align_trace, szs_memory_device_k, listed->device,
                                                  workgroups * SZS_ALIGN_REGION_BYTES(widest), error_message);
    if (status != sz_success_k) return status;

    uint64_t *staged = (uint64_t *)engine->device_rerank_staged.pointer;
    uint64_t const *kernel_inputs[3] = {call->indices, call->starts, call->ends};
    hipError_t error = hipSuccess;
    for (int i = 0; i < 3; ++i) {
        if (!kernel_inputs[i]) continue;
        uint64_t const *const own = kernel_inputs[i] + q0 * row_stride;
        kernel_inputs[i] = own;
        if (!call->stage_inputs) continue;
        if (error == hipSuccess) error = hipMemcpy2DAsync(staged, row_bytes, own, pitch, row_bytes, rows, kind_towards_device(own), stream);
        kernel_inputs[i] = staged, staged += listed->block * k;
    }
    uint64_t *kernel_distances = call->distances + q0 * row_stride, *kernel_lengths = call->lengths + q0 * row_stride;
    uint8_t *kernel_ops = call->ops ? call->ops + q0 * row_stride * capacity : NULL;
    if (call->stage_outputs) {
        kernel_distances = staged, staged += listed->block * k;
        kernel_lengths = staged, staged += listed->block * k;
        if (call->ops) kernel_ops = (uint8_t *)staged;
    }
    size_t const inputs_stride = call->stage_inputs ? k : row_stride, outputs_stride = call->stage_outputs ? k : row_stride;
    error = szs_listed_block_begin(listed, dealt, error);
    if (error == hipSuccess)
        error = (hipError_t)szs_hip_levenshtein_alignments(&listed->sides[0], &listed->sides[1], q0, listed->device_order, (uint32_t)dealt,
                                                           kernel_inputs[0], kernel_inputs[1], kernel_inputs[2], inputs_stride, k,
                                                           kernel_distances, kernel_lengths, outputs_stride, kernel_ops, capacity, widest,
                                                           engine->device_align_trace.pointer, workgroups, listed->flags,
                                                           listed->device_counters, stream);
    error = szs_listed_block_end(listed, error);
    if (error == hipSuccess && call->stage_outputs)
        error = hipMemcpy2DAsync(call->distances + q0 * row_stride, pitch, kernel_distances, row_bytes, row_bytes, rows,
                                 kind_from_device(call->distances), stream);
    if (error == hipSuccess && call->stage_outputs)
        error = hipMemcpy2DAsync(call->lengths + q0 * row_stride, pitch, kernel_lengths, row_bytes, row_bytes, rows,
                                 kind_from_device(call->lengths), stream);
    if (error == hipSuccess && call->stage_outputs && call->ops)
        error = hipMemcpy2DAsync(call->ops + q0 * row_stride * capacity, row_stride * capacity, kernel_ops, k * capacity, k * capacity, rows,
                                 kind_from_device(call->ops), stream);
    /* per pair: two offsets, the index, the distance and the length, the span where the call gives one; the L ops are the kernel's count */
    return szs_listed_block_finish(listed, error, hip_error, 1, longest, 2 * 4 + 8 + 8 + 8 + (call->starts ? 16 : 0),
                                   sz_unexpected_dimensions_k, alignments_long_span, error_message);
}

sz_status_t szs_engine_alignments(szs_engine_s *engine, szs_scope_s *scope, szs_input_t const *queries, szs_input_t const *candidates,
                                  size_t const *indices, size_t k, size_t const *starts, size_t const *ends, size_t *distances,
                                  size_t *lengths, unsigned char *ops, size_t capacity, size_t row_stride, char const **error_message) {
    double const started = szs_now_milliseconds();
    if (k < 1 || row_stride < k) return szs_report(sz_unexpected_dimensions_k, error_message, "k must be at least 1 and row_stride at least k");
    if (!engine || engine->magic != SZS_ENGINE_MAGIC || engine->family != szs_family_levenshtein_k || !engine->is_unit_cost)
        return szs_report(sz_status_unknown_k, error_message, "Alignments need an initialized unit-cost byte Levenshtein engine");
    if (!queries) return szs_report(sz_status_unknown_k, error_message, "Queries must not be null");
    if (!queries->count) return szs_report(sz_success_k, error_message, NULL);
    if (!distances || !lengths) return szs_report(sz_status_unknown_k, error_message, "Distances and lengths must not be null");
    if (!starts != !ends) return szs_report(sz_status_unknown_k, error_message, "Starts and ends must both be given, or neither");
    if (!ops && capacity) return szs_report(sz_status_unknown_k, error_message, "Ops must not be null when the capacity is not zero");
    if (!ops) capacity = 0;
    else if (!capacity) ops = NULL; /* slots of no bytes: nothing to write */
    szs_input_t const *const pool = candidates ? candidates : queries; /* the self form: the indices refer to the queries */
    size_t const q_count = queries->count, c_count = pool->count;
    if (!indices && k != c_count)
        return szs_report(sz_unexpected_dimensions_k, error_message, "Without indices k must be the number of candidates");
    if (k > (~(size_t)0 >> 4) / sizeof(uint64_t) || (capacity && k > (~(size_t)0 >> 4) / capacity))
        return szs_report(sz_overflow_risk_k, error_message, NULL);

    alignments_call_t call;
    memset(&call, 0, sizeof(call));
    szs_listed_call_t *const listed = &call.listed;
    sz_status_t status = szs_listed_open(listed, engine, scope, k, row_stride, error_message);
    if (status != sz_success_k) return status;
    call.indices = (uint64_t const *)indices, call.starts = (uint64_t const *)starts, call.ends = (uint64_t const *)ends;
    call.distances = (uint64_t *)distances, call.lengths = (uint64_t *)lengths, call.ops = ops, call.capacity = capacity;

    /* indices the host can read: validated before anything is launched */
    if (indices && szs_classify_pointer(indices).host_readable && !szs_listed_indices_ok(call.indices, q_count, k, row_stride, c_count))
        return szs_report(sz_unexpected_dimensions_k, error_message, "An index is beyond the candidates");
    status = szs_listed_offsets(listed, queries, candidates, error_message);
    if (status != sz_success_k) return status;

    /* blocks of rows: the kernel's row list and - where the device cannot reach the caller's arrays - their dense copies in budget */
    size_t inputs = 0;
    uint64_t const *const given[3] = {call.indices, call.starts, call.ends};
    for (int i = 0; i < 3; ++i)
        if (given[i]) ++inputs, call.stage_inputs |= !szs_classify_pointer(given[i]).device_accessible;
    call.stage_outputs = !szs_classify_pointer(distances).device_accessible || !szs_classify_pointer(lengths).device_accessible ||
                         (ops && !szs_classify_pointer(ops).device_accessible);
    /* in dense arrays of k 8-byte cells a row: the inputs, the two cell outputs, and ceil(capacity / 8) of them for the ops */
    size_t const staged_arrays = (call.stage_inputs ? inputs : 0) + (call.stage_outputs ? 2 + (capacity + 7) / 8 : 0);
    size_t block = q_count < SZS_RERANK_MOST_ROWS ? q_count : SZS_RERANK_MOST_ROWS;
    size_t const widest_row = k * (capacity > 8 ? capacity : 8); /* the ops' row, or a cell array's */
    if (staged_arrays && block > SZS_RERANK_STAGE_BYTES / widest_row) block = SZS_RERANK_STAGE_BYTES / widest_row;
    if (block < 1) block = 1;
    listed->block = block;

    size_t const no_extras[2] = {0, 0};
    void *extras[4];
    status = szs_listed_reserve(listed, queries, candidates, 1, no_extras, no_extras, staged_arrays, extras, error_message);
    if (status != sz_success_k) return status;

    /* both sides as the kernel reads them; a query beyond its bit-vector fails the call here, before anything is launched */
    int usable = 0;
    status = szs_listed_prepare_queries(listed, queries, SZS_RERANK_LONGEST_QUERY, &usable, error_message);
    if (status != sz_success_k) return status;
    if (!usable) return szs_report(sz_status_unknown_k, error_message, "The queries are not strings the device can read");
    for (size_t q = 0; q < q_count; ++q) {
        if (listed->query_lengths[q] != ~0u) continue;
        int const descends = !listed->refs_needed[0] && szs_tape_offset(queries, listed->offsets[0], q + 1) < szs_tape_offset(queries, listed->offsets[0], q);
        return szs_report(sz_unexpected_dimensions_k, error_message, descends ? "Tape offsets must ascend" : alignments_long_query);
    }
    status = szs_listed_prepare_candidates(listed, candidates, &usable, error_message);
    if (status != sz_success_k) return status;
    if (!usable) return szs_report(sz_status_unknown_k, error_message, "The candidates are not strings the device can read");

    hipError_t error = hipSuccess;
    for (size_t q0 = 0; q0 < q_count && status == sz_success_k && error == hipSuccess; q0 += block)
        status = alignments_block(&call, q0, q_count - q0 < block ? q_count - q0 : block, &error, error_message);
    return szs_listed_close(listed, status, error, started, error_message);
}
