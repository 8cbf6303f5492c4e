/*
 *  rerank_internal.h - what the calls over LISTED pairs share on the host (rerank.c: szs_rocm_rerank*; fuzzy_find.c:
 *  szs_rocm_fuzzy_find*): the block and staging budgets, tape offsets where the host can read them, a side as the kernels read it
 *  (szs_rerank_side_t), the parts of a scratch layout, the deal of a block's rows by descending query length.
 */
#ifndef SZS_RERANK_INTERNAL_H_
#define SZS_RERANK_INTERNAL_H_

#include "szs_internal.h"

#include <string.h>
#include <time.h>

#define SZS_RERANK_STAGE_BYTES ((size_t)128 << 20) /* a block's dense copy of an array the device cannot reach */
#define SZS_RERANK_MOST_ROWS ((size_t)1 << 20)     /* rows of a block: bounds the kernel's row list */
#define SZS_RERANK_EMPTY (~(uint64_t)0)            /* SZ_SIZE_MAX: the empty slot top-k emits */

static inline double szs_now_milliseconds(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

static inline uint64_t szs_tape_offset(szs_input_t const *input, void const *offsets, size_t i) {
    return input->kind == szs_input_u32tape_k ? ((uint32_t const *)offsets)[i] : ((uint64_t const *)offsets)[i];
}

/** The offsets of a tape where the host can read them: as they are, or copied to the host - once per call. */
static inline sz_status_t szs_host_offsets_of(szs_input_t const *input, szs_buffer_t *copy, hipStream_t stream, void const **offsets,
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

static inline size_t szs_align16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

/** One part of a scratch layout: `bytes` at `*end`, each part behind the one before it. */
static inline size_t szs_layout_part(size_t *end, size_t bytes) {
    size_t const at = *end;
    *end = at + szs_align16(bytes);
    return at;
}

/** A side does not need refs when it is a tape whose offsets the device reads itself. */
static inline int szs_side_needs_refs(szs_input_t const *input) {
    return input->kind == szs_input_sequence_k || !szs_classify_pointer(input->offsets).device_accessible;
}

/**
 *  One side as the kernel reads it: the tape itself, or refs in index order built on the host and uploaded.  `*usable` 0: the kernel
 *  cannot reach the side's strings (or its offsets are malformed).
 */
static inline sz_status_t szs_kernel_side(szs_input_t const *input, void const *offsets, int needs_refs, uint64_t *addresses,
                                          uint32_t *lengths, szs_string_ref_t *pinned_refs, szs_string_ref_t *device_refs,
                                          hipStream_t stream, szs_rerank_side_t *side, int *usable, char const **error_message) {
    memset(side, 0, sizeof(*side));
    side->count = input->count, *usable = 1;
    if (!needs_refs) {
        side->offsets = input->offsets, side->base = (uint64_t)(uintptr_t)input->data, side->wide = input->kind == szs_input_u64tape_k;
        uint64_t const bytes = szs_tape_offset(input, offsets, input->count) - szs_tape_offset(input, offsets, 0);
        *usable = !bytes || szs_classify_pointer(input->data).device_accessible;
        return sz_success_k;
    }
    char const *ignored = NULL;
    uint64_t bytes = 0;
    if (szs_gather_strings(input, offsets, addresses, lengths, &bytes, NULL, &ignored) != sz_success_k) {
        *usable = 0;
        return sz_success_k;
    }
    for (size_t i = 0; i < input->count; ++i)
        pinned_refs[i].address = addresses[i], pinned_refs[i].length = lengths[i], pinned_refs[i].index = (uint32_t)i;
    side->refs = device_refs;
    if (!input->count) return sz_success_k;
    hipError_t const error = hipMemcpyAsync(device_refs, pinned_refs, input->count * sizeof(szs_string_ref_t), hipMemcpyHostToDevice, stream);
    return error == hipSuccess ? sz_success_k : szs_report_hip(error, error_message);
}

static inline int szs_index_is_bad(uint64_t index, size_t count) { return index != SZS_RERANK_EMPTY && index >= count; }

/**
 *  The rows of a block whose query has at most SZS_RERANK_LONGEST_QUERY bytes into `order`, longest query first (a counting sort of
 *  the lengths 256 ... 0): the rows of a wavefront then share a width.  `lengths`: the block's, ~0 where no kernel takes the row.
 */
static inline size_t szs_deal_short_rows(uint32_t const *lengths, size_t rows, uint32_t *order, uint32_t *longest) {
    uint32_t bins[SZS_RERANK_LONGEST_QUERY + 2];
    size_t dealt = 0;
    *longest = 0;
    memset(bins, 0, sizeof(bins));
    for (size_t r = 0; r < rows; ++r)
        if (lengths[r] <= SZS_RERANK_LONGEST_QUERY) ++bins[SZS_RERANK_LONGEST_QUERY - lengths[r] + 1], ++dealt;
    for (size_t b = 1; b < SZS_RERANK_LONGEST_QUERY + 2; ++b) bins[b] += bins[b - 1];
    for (size_t r = 0; r < rows; ++r) {
        if (lengths[r] > SZS_RERANK_LONGEST_QUERY) continue;
        order[bins[SZS_RERANK_LONGEST_QUERY - lengths[r]]++] = (uint32_t)r;
        if (lengths[r] > *longest) *longest = lengths[r];
    }
    return dealt;
}

#endif /* SZS_RERANK_INTERNAL_H_ */
