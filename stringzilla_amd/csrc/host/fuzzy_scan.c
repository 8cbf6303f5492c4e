/*
 *  fuzzy_scan.c - the best match of every query inside ONE long text (szs_rocm_fuzzy_scan*, include/stringzillas/stringzillas_rocm.h;
 *  DESIGN.md section 4.11): distances[q] = min over j of D[m][j] with a free start in the text, ends[q] = the smallest j that attains
 *  it, starts[q] = szs_rocm_fuzzy_find_spans' start - what szs_rocm_fuzzy_find(queries, [text]) returns in column 0, bit for bit.
 *
 *  The call is the skeleton of listed_pairs.c (rerank_internal.h) with the text as a one-string candidate side and k = 1: blocks of
 *  at most 2^20 rows, per block the scan (hip/myers_fuzzy_scan.hip: the text cut into pieces, the pieces dealt to lanes, an atomic
 *  minimum per row), its emit and - where the call asks for starts - fuzzy find's own reverse pass (hip/myers_fuzzy_spans.hip,
 *  unchanged) behind them, on one stream inside one event pair.  Outputs the device cannot reach are staged densely and copied home.
 *  The piece rule is ONE function, fuzzy_scan_cut, which the call and szs_rocm_fuzzy_scan_probe share.
 */
#include "rerank_internal.h"

#define SZS_FUZZY_SCAN_WAVES (256u * 4u * 5u) /* what the device holds of a 5-waves-a-SIMD kernel: 256 CUs x 4 SIMDs x 5 waves */
#define SZS_FUZZY_SCAN_FILLS 4u               /* a block's launch should fill it this many times over, as fuzzy search's does */
#define SZS_FUZZY_SCAN_LANES 64u              /* the pieces of a workgroup; what a piece's bytes are a multiple of */
#define SZS_FUZZY_SCAN_LEAST_PIECE 4096u      /* the warm-up of the longest query, 512 bytes, is at most an eighth of a lane's walk */
#define SZS_FUZZY_SCAN_MOST_WORKGROUPS ((uint64_t)0x7FFFFFFF)

static char const fuzzy_scan_long_query[] = "A query of more than 256 bytes: beyond what fuzzy scan takes";

/* (declared in rerank_internal.h: the bounded scans - fuzzy_scan_matches.c - cut their text by the same rule) */
fuzzy_scan_cut_t fuzzy_scan_cut(size_t rows, uint64_t n) {
    uint64_t const wanted = (uint64_t)SZS_FUZZY_SCAN_WAVES * SZS_FUZZY_SCAN_FILLS;
    uint64_t const chunks_wanted = (wanted + rows - 1) / rows, lanes_wanted = chunks_wanted * SZS_FUZZY_SCAN_LANES;
    uint64_t piece = (n + lanes_wanted - 1) / lanes_wanted;
    if (piece < SZS_FUZZY_SCAN_LEAST_PIECE) piece = SZS_FUZZY_SCAN_LEAST_PIECE;
    int const piece_knob = szs_tuning_get(szs_knob_fuzzy_scan_piece_k);
    if (piece_knob > 0) piece = (uint64_t)piece_knob;
    piece = (piece + SZS_FUZZY_SCAN_LANES - 1) / SZS_FUZZY_SCAN_LANES * SZS_FUZZY_SCAN_LANES;
    fuzzy_scan_cut_t cut = {piece, (n + piece - 1) / piece, 0};
    cut.chunks = (cut.pieces + SZS_FUZZY_SCAN_LANES - 1) / SZS_FUZZY_SCAN_LANES;
    return cut;
}

/** The rows of a block: listed_pairs.c's, and fewer where rows x chunks would pass the grid's 2^31 - 1 workgroups. */
static size_t fuzzy_scan_block_rows(size_t q_count, int within_stage_budget, uint64_t n, fuzzy_scan_cut_t *cut) {
    size_t block = szs_listed_block_rows(q_count, 1, within_stage_budget);
    *cut = fuzzy_scan_cut(block, n);
    if (cut->chunks && block > SZS_FUZZY_SCAN_MOST_WORKGROUPS / cut->chunks) block = (size_t)(SZS_FUZZY_SCAN_MOST_WORKGROUPS / cut->chunks);
    return block; /* at least 1: a text below 4 GiB has at most 2^26 pieces of 64 bytes, 2^20 chunks */
}

sz_status_t szs_rocm_fuzzy_scan_probe(sz_size_t queries_count, sz_size_t longest_query, sz_size_t text_length, sz_size_t *piece,
                                      sz_size_t *pieces, sz_size_t *workgroups, sz_size_t *walked_bytes_per_query) {
    if (longest_query > SZS_RERANK_LONGEST_QUERY || text_length > 0xFFFFFFFFull) return sz_unexpected_dimensions_k;
    fuzzy_scan_cut_t cut;
    size_t const block = fuzzy_scan_block_rows(queries_count ? queries_count : 1, 0, text_length, &cut);
    if (piece) *piece = cut.piece;
    if (pieces) *pieces = cut.pieces;
    if (workgroups) *workgroups = (queries_count < block ? queries_count : block) * cut.chunks;
    if (walked_bytes_per_query) {
        /* n + the warm-ups: min(p P, 2 m) over the pieces - p P for the `rising` pieces below 2 m / P, 2 m for the rest */
        uint64_t const warm = 2 * (uint64_t)longest_query, within = (warm + cut.piece - 1) / cut.piece;
        uint64_t const rising = within < cut.pieces ? within : cut.pieces;
        *walked_bytes_per_query = text_length + cut.piece * (rising * (rising ? rising - 1 : 0) / 2) + (cut.pieces - rising) * warm;
    }
    return sz_success_k;
}

/** What the blocks of one call share, next to fuzzy find's: the text, its cut, and the device's words. */
typedef struct {
    szs_fuzzy_find_call_t find; /* the text is candidate 0 of its `listed.sides[1]`; k = 1 and the strides are 1 */
    void const *text;
    uint64_t text_length;
    fuzzy_scan_cut_t cut;
    unsigned long long *keys; /* device: a block's rows */
    uint64_t *staged;         /* device: dense outputs of a block, where the device cannot reach the caller's */
} fuzzy_scan_call_t;

/** One block: the keys filled with ones, the scan, the emit, the starts where the call asks for them; what was staged goes home. */
static sz_status_t fuzzy_scan_block(fuzzy_scan_call_t *scan, size_t q0, size_t rows, hipError_t *hip_error, char const **error_message) {
    szs_fuzzy_find_call_t *const call = &scan->find;
    szs_listed_call_t *const listed = &call->listed;
    hipStream_t const stream = listed->stream;
    uint32_t longest = 0;
    size_t const dealt = szs_deal_short_rows(listed->query_lengths + q0, rows, listed->order, &longest); /* every row: the caller saw to it */
    unsigned const widest = longest ? (longest + 31) / 32 : 1;

    uint64_t *kernel_distances = call->distances + q0, *kernel_ends = call->ends ? call->ends + q0 : NULL;
    uint64_t *kernel_starts = call->starts ? call->starts + q0 : NULL;
    /* all staged (dense), or all the caller's */
    int const dense_outputs = call->stage_distances || call->stage_ends || call->stage_starts;
    if (dense_outputs) {
        kernel_distances = scan->staged;
        if (call->ends) kernel_ends = scan->staged + listed->block;
        if (call->starts) kernel_starts = scan->staged + 2 * listed->block;
    }
    size_t const bytes = rows * sizeof(uint64_t);
    hipError_t error = szs_listed_block_begin(listed, dealt, hipSuccess);
    if (error == hipSuccess) error = hipMemsetAsync(scan->keys, 0xFF, bytes, stream);
    if (error == hipSuccess)
        error = (hipError_t)szs_hip_levenshtein_fuzzy_scan(&listed->sides[0], q0, (uint32_t)rows, scan->text, scan->text_length,
                                                           scan->cut.piece, scan->keys, listed->flags, listed->device_counters, stream);
    if (error == hipSuccess)
        error = (hipError_t)szs_hip_levenshtein_fuzzy_scan_emit(&listed->sides[0], q0, (uint32_t)rows, scan->keys, kernel_distances,
                                                                kernel_ends, listed->flags, stream);
    if (error == hipSuccess && call->starts) /* fuzzy find's reverse pass: the dense form of one candidate, k = 1 */
        error = (hipError_t)szs_hip_levenshtein_fuzzy_starts(&listed->sides[0], &listed->sides[1], q0, listed->device_order, (uint32_t)dealt,
                                                             NULL, 1, 1, kernel_distances, kernel_ends, kernel_starts, 1, widest,
                                                             listed->flags, listed->device_counters, stream);
    error = szs_listed_block_end(listed, error);
    if (error == hipSuccess && dense_outputs)
        error = hipMemcpyAsync(call->distances + q0, kernel_distances, bytes,
                               call->stage_distances ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, stream);
    if (error == hipSuccess && dense_outputs && call->ends)
        error = hipMemcpyAsync(call->ends + q0, kernel_ends, bytes, call->stage_ends ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, stream);
    if (error == hipSuccess && dense_outputs && call->starts)
        error = hipMemcpyAsync(call->starts + q0, kernel_starts, bytes, call->stage_starts ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                               stream);
    return szs_listed_block_finish(listed, error, hip_error, (scan->text_length ? 2 : 1) + (call->starts ? 1 : 0), longest,
                                   2 * 4 + 8 + (call->ends ? 8 : 0) + (call->starts ? 8 : 0), sz_unexpected_dimensions_k,
                                   fuzzy_scan_long_query, error_message);
}

/** The one call path.  `missing`: the message for a required output that is NULL, refused behind the checks of the text's length,
 *  the engine and an empty batch; NULL when the entry has all it requires. */
static sz_status_t fuzzy_scan_call(szs_engine_s *engine, szs_scope_s *scope, szs_input_t const *queries, void const *text, size_t text_length,
                                   size_t *distances, size_t *starts, size_t *ends, char const *missing, char const **error_message) {
    double const started = szs_now_milliseconds();
    if ((uint64_t)text_length > 0xFFFFFFFFull) return szs_report(sz_unexpected_dimensions_k, error_message, "The text must have less than 4 GiB");
    if (!engine || engine->magic != SZS_ENGINE_MAGIC || engine->family != szs_family_levenshtein_k || !engine->is_unit_cost)
        return szs_report(sz_status_unknown_k, error_message, "Fuzzy scan needs an initialized unit-cost byte Levenshtein engine");
    if (!queries) return szs_report(sz_status_unknown_k, error_message, "Queries must not be null");
    if (!queries->count) return szs_report(sz_success_k, error_message, NULL);
    if (missing) return szs_report(sz_status_unknown_k, error_message, missing);
    if (!text && text_length) return szs_report(sz_status_unknown_k, error_message, "Text must not be null");
    size_t const q_count = queries->count;

    fuzzy_scan_call_t scan;
    memset(&scan, 0, sizeof(scan));
    szs_fuzzy_find_call_t *const call = &scan.find;
    szs_listed_call_t *const listed = &call->listed;
    sz_status_t status = szs_listed_open(listed, engine, scope, 1, 1, error_message);
    if (status != sz_success_k) return status;
    if (text_length && !szs_classify_pointer(text).device_accessible)
        return szs_report(sz_status_unknown_k, error_message, "The text is not memory the device can read");
    scan.text = text, scan.text_length = text_length;
    call->distances = (uint64_t *)distances, call->ends = (uint64_t *)ends, call->starts = (uint64_t *)starts;
    status = szs_listed_offsets(listed, queries, NULL, error_message);
    if (status != sz_success_k) return status;

    /* blocks of rows; the device's words: the text as a ref, a block's keys, dense copies of the outputs the device cannot reach */
    size_t const staged_arrays = szs_fuzzy_find_stage(call);
    size_t const block = listed->block = fuzzy_scan_block_rows(q_count, staged_arrays != 0, text_length, &scan.cut);
    size_t const no_extras[2] = {0, 0}, pinned_extras[2] = {sizeof(szs_string_ref_t), 0};
    void *extras[4];
    status = szs_listed_reserve(listed, queries, NULL, 1, no_extras, pinned_extras, 0, extras, error_message);
    if (status == sz_success_k)
        status = szs_buffer_reserve(&engine->device_rerank_staged, szs_memory_device_k, listed->device,
                                    sizeof(szs_string_ref_t) + (1 + staged_arrays) * block * sizeof(uint64_t), error_message);
    if (status != sz_success_k) return status;
    szs_string_ref_t *const pinned_text = (szs_string_ref_t *)extras[2], *const device_text = (szs_string_ref_t *)engine->device_rerank_staged.pointer;
    scan.keys = (unsigned long long *)(device_text + 1), scan.staged = (uint64_t *)scan.keys + block;

    /* a query beyond the kernel's bit-vector fails the call here, before anything is launched */
    status = szs_fuzzy_find_prepare(call, queries, NULL, fuzzy_scan_long_query, error_message);
    if (status != sz_success_k) return status;
    szs_rerank_side_t *const text_side = &listed->sides[1];
    memset(text_side, 0, sizeof(*text_side));
    pinned_text->address = (uint64_t)(uintptr_t)text, pinned_text->length = (uint32_t)text_length, pinned_text->index = 0;
    text_side->refs = device_text, text_side->count = 1;
    hipError_t error = hipMemcpyAsync(device_text, pinned_text, sizeof(*pinned_text), hipMemcpyHostToDevice, listed->stream);

    for (size_t q0 = 0; q0 < q_count && status == sz_success_k && error == hipSuccess; q0 += block)
        status = fuzzy_scan_block(&scan, q0, q_count - q0 < block ? q_count - q0 : block, &error, error_message);
    return szs_listed_close(listed, status, error, started, error_message);
}

sz_status_t szs_engine_fuzzy_scan(szs_engine_s *engine, szs_scope_s *scope, szs_input_t const *queries, void const *text, size_t text_length,
                                  size_t *distances, size_t *ends, char const **error_message) {
    return fuzzy_scan_call(engine, scope, queries, text, text_length, distances, NULL, ends, distances ? NULL : "Distances must not be null",
                           error_message);
}

sz_status_t szs_engine_fuzzy_scan_spans(szs_engine_s *engine, szs_scope_s *scope, szs_input_t const *queries, void const *text,
                                        size_t text_length, size_t *distances, size_t *starts, size_t *ends, char const **error_message) {
    char const *const missing = !distances ? "Distances must not be null" : !starts || !ends ? "Starts and ends must not be null" : NULL;
    return fuzzy_scan_call(engine, scope, queries, text, text_length, distances, starts, ends, missing, error_message);
}
