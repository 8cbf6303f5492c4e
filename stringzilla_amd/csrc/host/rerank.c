/*
 *  rerank.c - exact scores of LISTED candidates per query (szs_rocm_rerank*, include/stringzillas/stringzillas_rocm.h; DESIGN.md
 *  section 4.8): scores[q][r] = score(queries[q], candidates[indices[q][r]]), the cell the matrix call would put there.
 *
 *  Three routes inside one call, chosen per row (rerank_route_of):
 *    - the KERNEL route (hip/myers_rerank.hip): rows of a unit-cost byte Levenshtein engine whose query has at most 256 bytes.  All
 *      such rows of a block go into one launch, dealt by descending query length; the kernel reads the indices and writes the scores
 *      where they are when the device can reach them, else through a dense copy of the block;
 *    - the STRIPS route (hip/myers_rerank_strips.hip): rows of such an engine whose query has more than 256 and at most 65,536 bytes
 *      (SZS_RERANK_LONGEST_STRIPS_QUERY), candidates of any length that the parked scratch can hold (rerank_strips_grid).  All such
 *      rows of a block go into one launch of their own, dealt by descending word count of the query.  64 KiB is a design bound, not
 *      a measured one: above it one lane's serial chain of len(q) / 256 x len(c) columns is the wrong tool, and the engine's chained
 *      few-pairs tiers, which the row route reaches, are built for such pairs;
 *    - the ROW route: every other row - and every row with the `rerank` knob at 0, every long row with it at 1 - is one ordinary
 *      engine call (szs_engine_cross) of 1 x k' over a gathered sequence of the row's non-empty indices, scattered into the row on
 *      the host.
 *  Indices the host can read are validated before anything is launched; indices only the device can read are checked by the kernel
 *  (`index < count` before every use, a flag in pinned memory) - or, for the rows of the row route, downloaded and validated first.
 *
 *  szs_engine_rerank checks the arguments and walks the blocks on the skeleton of listed_pairs.c (rerank_internal.h: the preamble, the
 *  scratch, the sides, the bracket around a block's launches); per block:
 *  rerank_deal_rows and rerank_deal_strip_rows (which rows each kernel takes, longest query first), rerank_kernel_rows (staging, at
 *  most one launch of each kernel, the scores home), rerank_row (the row route).  The routes write disjoint rows of `scores`, so none
 *  depends on running before another.  szs_rocm_rerank_probe reports the routing of bare lengths through the same functions.
 */
#include "rerank_internal.h"

#define SZS_RERANK_PARKED_BYTES ((size_t)256 << 20) /* the parked deltas of the strips launch: a chosen budget (what top-k and the
                                                       fingerprint search give their staging), not a measurement */
#define SZS_RERANK_STRIPS_TABLES 5120u             /* 8 KB tables that 256 CUs x 160 KB of LDS hold: the most rows in flight */

enum { szs_rerank_route_row_k = 0, szs_rerank_route_kernel_k = 1, szs_rerank_route_strips_k = 2 };

/* ---- gathered sequences: strings picks[0 .. count) of a side, for the row route ------------------------------------------- */

typedef struct {
    sz_sequence_t sequence; /* first member: the handle of the wrapper is the wrapper itself */
    szs_input_t const *base;
    void const *offsets;    /* of a tape, where the host can read them */
    uint64_t const *picks;
} szs_gathered_sequence_t;

static sz_cptr_t gathered_start(void const *handle, sz_sorted_idx_t i) {
    szs_gathered_sequence_t const *gathered = (szs_gathered_sequence_t const *)handle;
    size_t const at = (size_t)gathered->picks[i];
    if (gathered->base->kind == szs_input_sequence_k) return gathered->base->sequence->get_start(gathered->base->sequence->handle, at);
    return gathered->base->data + szs_tape_offset(gathered->base, gathered->offsets, at);
}
static sz_size_t gathered_length(void const *handle, sz_sorted_idx_t i) {
    szs_gathered_sequence_t const *gathered = (szs_gathered_sequence_t const *)handle;
    size_t const at = (size_t)gathered->picks[i];
    if (gathered->base->kind == szs_input_sequence_k) return gathered->base->sequence->get_length(gathered->base->sequence->handle, at);
    uint64_t const from = szs_tape_offset(gathered->base, gathered->offsets, at), to = szs_tape_offset(gathered->base, gathered->offsets, at + 1);
    return to >= from ? to - from : SZS_RERANK_EMPTY; /* descending offsets: a length no call accepts */
}
static szs_input_t gather_input(szs_input_t const *base, void const *offsets, uint64_t const *picks, size_t count,
                                szs_gathered_sequence_t *wrapper) {
    wrapper->base = base, wrapper->offsets = offsets, wrapper->picks = picks;
    wrapper->sequence.handle = wrapper, wrapper->sequence.count = count;
    wrapper->sequence.get_start = gathered_start, wrapper->sequence.get_length = gathered_length;
    szs_input_t const input = {szs_input_sequence_k, count, NULL, NULL, &wrapper->sequence};
    return input;
}

static void add_profile(szs_rocm_call_profile_t *total, szs_rocm_call_profile_t const *part) {
    total->kernel_milliseconds += part->kernel_milliseconds, total->cells += part->cells, total->pairs += part->pairs;
    total->algorithmic_bytes += part->algorithmic_bytes, total->unique_bytes += part->unique_bytes, total->launches += part->launches;
    if (part->longest_query > total->longest_query) total->longest_query = part->longest_query;
    if (part->longest_candidate > total->longest_candidate) total->longest_candidate = part->longest_candidate;
}

/* ---- the call ------------------------------------------------------------------------------------------------------------ */

/** What the parts of one call share. */
typedef struct {
    szs_listed_call_t listed; /* query_lengths: filled with kernel_route, ~0 where no kernel takes the row */
    szs_scope_s *scope;
    szs_input_t const *queries, *pool; /* pool: the candidates, or the queries in the self form */
    uint64_t const *indices;
    uint64_t *scores;
    int scores_on_host, stage_indices, stage_scores;
    int kernel_route, strips_route; /* may rows take hip/myers_rerank.hip, and hip/myers_rerank_strips.hip */
    uint64_t longest_candidate;     /* strips_route: over the whole candidate side */
    uint64_t *picks, *row_cells, *row_image; /* the row route's: a row's non-empty indices, its scores as the engine call leaves
                                                them, the row as it is written */
    int engine_calls;
} szs_rerank_call_t;

/** Which kernels the rows of a call may take: by the engine (unit-cost byte Levenshtein) and the `rerank` knob. */
static void rerank_routes_enabled(int unit_cost_bytes, int *kernel_route, int *strips_route) {
    int const knob = szs_tuning_get(szs_knob_rerank_k);
    *kernel_route = knob != 0 && unit_cost_bytes;
    *strips_route = *kernel_route && knob != 1;
}

/** The route of a row whose query has `length` bytes (~0: more than any kernel takes, or unknown). */
static int rerank_route_of(int kernel_route, int strips_route, uint32_t length) {
    if (kernel_route && length <= SZS_RERANK_LONGEST_QUERY) return szs_rerank_route_kernel_k;
    if (strips_route && length != ~0u && length <= SZS_RERANK_LONGEST_STRIPS_QUERY) return szs_rerank_route_strips_k;
    return szs_rerank_route_row_k;
}

/**
 *  The persistent grid of the strips launch over `rows` rows of `k` slots and its parked scratch: one dword per 16 columns of the
 *  longest candidate for each of a workgroup's 64 lanes.  At most as many workgroups as rows need, as tables fit the device's LDS,
 *  and as keep the scratch within SZS_RERANK_PARKED_BYTES - fewer when one very long candidate asks for it; `workgroups` 0: even one
 *  workgroup's scratch is beyond the budget (a candidate of more than 16 MiB), the strips route is not taken.
 */
typedef struct {
    uint32_t workgroups, parked_dwords;
    size_t bytes;
} szs_rerank_strips_grid_t;

static szs_rerank_strips_grid_t rerank_strips_grid(size_t rows, size_t k, uint64_t longest_candidate) {
    szs_rerank_strips_grid_t grid = {0, 0, 0};
    uint64_t const dwords = longest_candidate ? (longest_candidate + 15) / 16 : 1;
    uint64_t const workgroup_bytes = dwords * 64 * sizeof(uint32_t);
    if (workgroup_bytes > SZS_RERANK_PARKED_BYTES) return grid;
    size_t const groups = 64 / szs_hip_rerank_lanes(k);
    size_t workgroups = (rows + groups - 1) / groups;
    if (workgroups > SZS_RERANK_STRIPS_TABLES / groups) workgroups = SZS_RERANK_STRIPS_TABLES / groups;
    if (workgroups > SZS_RERANK_PARKED_BYTES / workgroup_bytes) workgroups = SZS_RERANK_PARKED_BYTES / workgroup_bytes;
    if (workgroups < 1) workgroups = 1;
    grid.workgroups = (uint32_t)workgroups, grid.parked_dwords = (uint32_t)dwords, grid.bytes = workgroups * (size_t)workgroup_bytes;
    return grid;
}

static int row_route(szs_rerank_call_t const *call, size_t query) {
    return call->kernel_route ? rerank_route_of(call->kernel_route, call->strips_route, call->listed.query_lengths[query]) : szs_rerank_route_row_k;
}

/** The short kernel's rows of block [q0, q0 + rows) into `order`, longest query first (a counting sort of the lengths 256 ... 0). */
static size_t rerank_deal_rows(szs_rerank_call_t const *call, size_t q0, size_t rows, uint32_t *order, uint32_t *longest) {
    *longest = 0;
    if (!call->kernel_route) return 0;
    return szs_deal_short_rows(call->listed.query_lengths + q0, rows, order, longest);
}

/**
 *  The strips kernel's rows of the block into `order`, most words first (a counting sort of the word counts 2048 ... 9): the rows of
 *  a wavefront then share a strip count, and mostly a strip width.
 */
static size_t rerank_deal_strip_rows(szs_rerank_call_t const *call, size_t q0, size_t rows, uint32_t *order, uint32_t *longest) {
    enum { most_words = SZS_RERANK_LONGEST_STRIPS_QUERY / 32 };
    *longest = 0;
    if (!call->strips_route) return 0;
    uint32_t bins[most_words + 2];
    size_t strip_rows = 0;
    memset(bins, 0, sizeof(bins));
    for (size_t r = 0; r < rows; ++r)
        if (row_route(call, q0 + r) == szs_rerank_route_strips_k)
            ++bins[most_words - SZS_RERANK_WORDS_OF(call->listed.query_lengths[q0 + r]) + 1], ++strip_rows;
    for (size_t b = 1; b < most_words + 2; ++b) bins[b] += bins[b - 1];
    for (size_t r = 0; r < rows; ++r) {
        if (row_route(call, q0 + r) != szs_rerank_route_strips_k) continue;
        uint32_t const length = call->listed.query_lengths[q0 + r];
        order[bins[most_words - SZS_RERANK_WORDS_OF(length)]++] = (uint32_t)r;
        if (length > *longest) *longest = length;
    }
    return strip_rows;
}

/**
 *  The two kernel routes of one block: stages what the device cannot reach, launches each kernel at most once - the short rows are
 *  order[0 .. short_rows), the strips rows follow them - brings the scores home, reads the flags.  Staged scores go home by RUNS of
 *  consecutive rows of either kernel - one 2-D copy when the kernels took the whole block - so the rows of the row route are never
 *  written from here.
 */
static sz_status_t rerank_kernel_rows(szs_rerank_call_t *call, size_t q0, size_t rows, size_t short_rows, uint32_t longest_short,
                                      size_t strip_rows, uint32_t longest_strips, hipError_t *hip_error, char const **error_message) {
    szs_listed_call_t *const listed = &call->listed;
    szs_engine_s *const engine = listed->engine;
    hipStream_t const stream = listed->stream;
    size_t const k = listed->k, row_stride = listed->row_stride, row_bytes = k * sizeof(uint64_t);
    szs_rerank_strips_grid_t const grid = rerank_strips_grid(strip_rows, k, call->longest_candidate);
    if (strip_rows) {
        sz_status_t const status = szs_buffer_reserve(&engine->device_rerank_parked, szs_memory_device_k, listed->device, grid.bytes, error_message);
        if (status != sz_success_k) return status;
    }
    uint64_t *const staged = (uint64_t *)engine->device_rerank_staged.pointer;
    uint64_t const *kernel_indices = call->indices + q0 * row_stride;
    uint64_t *kernel_scores = call->scores + q0 * row_stride;
    size_t kernel_indices_stride = row_stride, kernel_scores_stride = row_stride;
    unsigned const widest = longest_short ? (longest_short + 31) / 32 : 1;
    uint32_t const longest = longest_short > longest_strips ? longest_short : longest_strips;
    hipError_t error = hipSuccess;
    if (call->stage_indices) {
        error = hipMemcpy2DAsync(staged, row_bytes, call->indices + q0 * row_stride, row_stride * sizeof(uint64_t), row_bytes, rows,
                                 hipMemcpyHostToDevice, stream);
        kernel_indices = staged, kernel_indices_stride = k;
    }
    if (call->stage_scores) kernel_scores = staged + (call->stage_indices ? listed->block * k : 0), kernel_scores_stride = k;
    error = szs_listed_block_begin(listed, short_rows + strip_rows, error);
    if (error == hipSuccess && short_rows)
        error = (hipError_t)szs_hip_levenshtein_rerank(&listed->sides[0], &listed->sides[1], q0, listed->device_order, (uint32_t)short_rows,
                                                       kernel_indices, kernel_indices_stride, k, kernel_scores, kernel_scores_stride, widest,
                                                       listed->flags, listed->device_counters, stream);
    if (error == hipSuccess && strip_rows)
        error = (hipError_t)szs_hip_levenshtein_rerank_strips(&listed->sides[0], &listed->sides[1], q0, listed->device_order + short_rows,
                                                              (uint32_t)strip_rows, kernel_indices, kernel_indices_stride, k, kernel_scores,
                                                              kernel_scores_stride, grid.workgroups,
                                                              (uint32_t *)engine->device_rerank_parked.pointer, grid.parked_dwords,
                                                              listed->flags, listed->device_counters, stream);
    error = szs_listed_block_end(listed, error);
    for (size_t r = 0; r < rows && error == hipSuccess && call->stage_scores;) {
        if (row_route(call, q0 + r) == szs_rerank_route_row_k) {
            ++r;
            continue;
        }
        size_t run = r + 1;
        while (run < rows && row_route(call, q0 + run) != szs_rerank_route_row_k) ++run;
        error = hipMemcpy2DAsync(call->scores + (q0 + r) * row_stride, row_stride * sizeof(uint64_t), kernel_scores + r * k, row_bytes, row_bytes,
                                 run - r, hipMemcpyDeviceToHost, stream);
        r = run;
    }
    return szs_listed_block_finish(listed, error, hip_error, (short_rows != 0) + (strip_rows != 0), longest, 2 * 4 + 8, sz_status_unknown_k,
                                   "A query or a candidate beyond what the rerank kernels were sized for", error_message);
}

/** The row route of one row: one engine call of 1 x k' over the row's non-empty indices, scattered into the row. */
static sz_status_t rerank_row(szs_rerank_call_t *call, size_t query, uint64_t const *row_indices, hipError_t *hip_error,
                              char const **error_message) {
    szs_engine_s *const engine = call->listed.engine;
    size_t const k = call->listed.k;
    size_t listed = 0;
    for (size_t i = 0; i < k; ++i)
        if (row_indices[i] != SZS_RERANK_EMPTY) call->picks[listed++] = row_indices[i];
    if (listed) {
        uint64_t const query_pick = query;
        szs_gathered_sequence_t query_wrapper, candidate_wrapper;
        szs_input_t const one = gather_input(call->queries, call->listed.offsets[0], &query_pick, 1, &query_wrapper);
        szs_input_t const few = gather_input(call->pool, call->listed.offsets[1], call->picks, listed, &candidate_wrapper);
        sz_status_t const status = szs_engine_cross(engine, call->scope, &one, &few, call->row_cells, listed, error_message); /* synchronous */
        if (status != sz_success_k) return status;
        add_profile(&call->listed.total, &engine->last_profile), ++call->engine_calls;
    }
    for (size_t i = 0, next = 0; i < k; ++i) call->row_image[i] = row_indices[i] != SZS_RERANK_EMPTY ? call->row_cells[next++] : 0;
    uint64_t *const row_scores = call->scores + query * call->listed.row_stride;
    if (call->scores_on_host) memcpy(row_scores, call->row_image, k * sizeof(uint64_t));
    else { /* (the image is free again once this copy has run: nothing writes it before the next synchronisation) */
        hipError_t error = hipMemcpyAsync(row_scores, call->row_image, k * sizeof(uint64_t), hipMemcpyHostToDevice, call->listed.stream);
        if (error == hipSuccess) error = hipStreamSynchronize(call->listed.stream);
        *hip_error = error;
    }
    return sz_success_k;
}

sz_status_t szs_engine_rerank(szs_engine_s *engine, szs_scope_s *scope, szs_input_t const *queries, szs_input_t const *candidates,
                              size_t const *indices, size_t k, void *scores, size_t row_stride, char const **error_message) {
    double const started = szs_now_milliseconds();
    if (k < 1 || row_stride < k) return szs_report(sz_unexpected_dimensions_k, error_message, "k must be at least 1 and row_stride at least k");
    if (!engine || engine->magic != SZS_ENGINE_MAGIC || (unsigned)engine->family > szs_family_smith_waterman_k)
        return szs_report(sz_status_unknown_k, error_message, "Engine must be an initialized similarity engine");
    if (!queries) return szs_report(sz_status_unknown_k, error_message, "Queries must not be null");
    if (!queries->count) return szs_report(sz_success_k, error_message, NULL);
    if (!indices) return szs_report(sz_status_unknown_k, error_message, "Indices must not be null");
    if (!scores) return szs_report(sz_status_unknown_k, error_message, "Scores must not be null");
    if (k > (~(size_t)0 >> 4) / sizeof(uint64_t)) return szs_report(sz_overflow_risk_k, error_message, NULL);

    szs_rerank_call_t call;
    memset(&call, 0, sizeof(call));
    szs_listed_call_t *const listed = &call.listed;
    sz_status_t status = szs_listed_open(listed, engine, scope, k, row_stride, error_message);
    if (status != sz_success_k) return status;
    hipStream_t const stream = listed->stream;
    call.scope = scope, call.queries = queries;
    call.pool = candidates ? candidates : queries; /* the self form: the indices refer to the queries */
    call.indices = (uint64_t const *)indices, call.scores = (uint64_t *)scores;
    size_t const q_count = queries->count, c_count = call.pool->count;
    szs_pointer_traits_t const index_traits = szs_classify_pointer(indices), score_traits = szs_classify_pointer(scores);
    call.scores_on_host = score_traits.host_readable;

    /* indices the host can read: validated before anything is launched */
    if (index_traits.host_readable && !szs_listed_indices_ok(call.indices, q_count, k, row_stride, c_count))
        return szs_report(sz_unexpected_dimensions_k, error_message, "An index is beyond the candidates");
    status = szs_listed_offsets(listed, queries, candidates, error_message);
    if (status != sz_success_k) return status;

    /* blocks of rows: the kernel's row list and - where the device cannot reach the caller's arrays, or the host the indices that
       the row route needs - their dense copies in budget */
    call.stage_indices = !index_traits.device_accessible, call.stage_scores = !score_traits.device_accessible;
    size_t const block = listed->block =
        szs_listed_block_rows(q_count, k, call.stage_indices || call.stage_scores || !index_traits.host_readable);

    rerank_routes_enabled(engine->family == szs_family_levenshtein_k && engine->is_unit_cost, &call.kernel_route, &call.strips_route);
    /* the row route's parts of the scratch: a block of indices only the device can read (else empty) and a row's picks on the host,
       a row's cells and its image in pinned memory */
    size_t const host_extra[2] = {index_traits.host_readable ? 0 : block * k * sizeof(uint64_t), k * sizeof(uint64_t)};
    size_t const pinned_extra[2] = {k * sizeof(uint64_t), k * sizeof(uint64_t)};
    void *extras[4];
    status = szs_listed_reserve(listed, queries, candidates, call.kernel_route, host_extra, pinned_extra,
                                (size_t)call.stage_indices + (size_t)call.stage_scores, extras, error_message);
    if (status != sz_success_k) return status;
    uint64_t *const downloaded = (uint64_t *)extras[0];
    call.picks = (uint64_t *)extras[1], call.row_cells = (uint64_t *)extras[2], call.row_image = (uint64_t *)extras[3];

    if (call.kernel_route) {
        /* a side the kernels cannot read: every row takes the row route */
        int usable = 0;
        status = szs_listed_prepare_queries(listed, queries, SZS_RERANK_LONGEST_STRIPS_QUERY, &usable, error_message);
        if (status != sz_success_k) return status;
        if (!usable) call.kernel_route = 0;
        if (call.kernel_route) {
            status = szs_listed_prepare_candidates(listed, candidates, &usable, error_message);
            if (status != sz_success_k) return status;
            if (!usable) call.kernel_route = 0;
        }
        /* the strips route: sized by the longest string of the candidate side - looked for only when a row would take it */
        int wanted = 0;
        for (size_t q = 0; q < q_count && call.kernel_route && call.strips_route && !wanted; ++q)
            wanted = row_route(&call, q) == szs_rerank_route_strips_k;
        if (!call.kernel_route || !wanted) call.strips_route = 0;
        else {
            int const pool_side = candidates ? 1 : 0;
            for (size_t i = 0; i < c_count; ++i) {
                uint64_t length = 0;
                if (listed->refs_needed[pool_side]) length = listed->gathered_lengths[i]; /* the side gathered last: the candidates', or the queries' own */
                else {
                    uint64_t const from = szs_tape_offset(call.pool, listed->offsets[1], i), to = szs_tape_offset(call.pool, listed->offsets[1], i + 1);
                    length = to >= from ? to - from : 0; /* (descending offsets: the kernel reports them) */
                }
                if (length > call.longest_candidate) call.longest_candidate = length;
            }
            if (!rerank_strips_grid(1, k, call.longest_candidate).workgroups) call.strips_route = 0; /* those rows: the row route */
        }
    }

    hipError_t error = hipSuccess;
    for (size_t q0 = 0; q0 < q_count && status == sz_success_k && error == hipSuccess; q0 += block) {
        size_t const rows = q_count - q0 < block ? q_count - q0 : block;
        uint32_t longest_short = 0, longest_strips = 0;
        size_t const short_rows = rerank_deal_rows(&call, q0, rows, listed->order, &longest_short);
        size_t const strip_rows = rerank_deal_strip_rows(&call, q0, rows, listed->order + short_rows, &longest_strips);
        size_t const kernel_rows = short_rows + strip_rows;

        /* the rows of the row route need their indices on the host: downloaded and validated before anything is launched */
        uint64_t const *host_indices = call.indices + q0 * row_stride;
        size_t host_indices_stride = row_stride;
        if (!index_traits.host_readable && kernel_rows < rows) {
            error = hipMemcpy2DAsync(downloaded, k * sizeof(uint64_t), call.indices + q0 * row_stride, row_stride * sizeof(uint64_t),
                                     k * sizeof(uint64_t), rows, hipMemcpyDeviceToHost, stream);
            if (error == hipSuccess) error = hipStreamSynchronize(stream);
            if (error != hipSuccess) break;
            if (!szs_listed_indices_ok(downloaded, rows, k, k, c_count))
                status = szs_report(sz_unexpected_dimensions_k, error_message, "An index is beyond the candidates");
            if (status != sz_success_k) break;
            host_indices = downloaded, host_indices_stride = k;
        }

        if (kernel_rows)
            status = rerank_kernel_rows(&call, q0, rows, short_rows, longest_short, strip_rows, longest_strips, &error, error_message);
        for (size_t r = 0; r < rows && kernel_rows < rows && status == sz_success_k && error == hipSuccess; ++r)
            if (row_route(&call, q0 + r) == szs_rerank_route_row_k) status = rerank_row(&call, q0 + r, host_indices + r * host_indices_stride, &error, error_message);
    }
    hipError_t const drained = hipStreamSynchronize(stream); /* synchronous, also when it fails */
    if (status != sz_success_k) return status;
    if (error == hipSuccess) error = drained;
    if (error != hipSuccess) return szs_report_hip(error, error_message);
    /* the profile of a rerank call: the last engine call's (none: blank), with the sums over the launch and every engine call */
    if (!call.engine_calls) memset(&engine->last_profile, 0, sizeof(engine->last_profile));
    szs_rocm_call_profile_t const *const total = &listed->total;
    engine->last_profile.kernel_milliseconds = total->kernel_milliseconds, engine->last_profile.cells = total->cells;
    engine->last_profile.pairs = total->pairs, engine->last_profile.algorithmic_bytes = total->algorithmic_bytes;
    engine->last_profile.unique_bytes = total->unique_bytes, engine->last_profile.launches = total->launches;
    engine->last_profile.longest_query = total->longest_query, engine->last_profile.longest_candidate = total->longest_candidate;
    engine->last_profile.host_milliseconds = szs_now_milliseconds() - started;
    return szs_report(sz_success_k, error_message, NULL);
}

/* ---- the exported probe ----------------------------------------------------------------------------------------------------- */

sz_status_t szs_rocm_rerank_probe(int unit_cost, int runes, sz_u32_t const *query_lengths, sz_size_t queries_count, sz_size_t k,
                                  sz_size_t longest_candidate, sz_u8_t *routes, sz_u32_t *strips, sz_u32_t *strip_words,
                                  sz_size_t *scratch_bytes) {
    if (k < 1 || (queries_count && !query_lengths)) return sz_unexpected_dimensions_k;
    int kernel_route = 0, strips_route = 0;
    rerank_routes_enabled(unit_cost && !runes, &kernel_route, &strips_route);
    if (!rerank_strips_grid(1, k, longest_candidate).workgroups) strips_route = 0;
    size_t strip_rows = 0;
    for (size_t q = 0; q < queries_count; ++q) {
        int const route = rerank_route_of(kernel_route, strips_route, query_lengths[q]);
        uint32_t const words = SZS_RERANK_WORDS_OF(query_lengths[q]);
        strip_rows += route == szs_rerank_route_strips_k;
        if (routes) routes[q] = (sz_u8_t)route;
        /* the short kernel: one bit-vector of the query's own words - what the strips rule gives up to 8 words; the row route: none */
        if (strips) strips[q] = route == szs_rerank_route_row_k ? 0 : SZS_RERANK_STRIPS_OF(words);
        if (strip_words) strip_words[q] = route == szs_rerank_route_row_k ? 0 : SZS_RERANK_STRIP_WORDS_OF(words);
    }
    if (scratch_bytes) *scratch_bytes = strip_rows ? rerank_strips_grid(strip_rows, k, longest_candidate).bytes : 0;
    return sz_success_k;
}
