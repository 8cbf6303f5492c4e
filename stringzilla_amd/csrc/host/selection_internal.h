/*
 *  selection_internal.h - what the calls that keep the k best candidates of every query share on the host (top_k.c: szs_rocm_top_k*;
 *  fingerprint_search.c: szs_rocm_fingerprint_top_k; fuzzy_search.c: szs_rocm_fuzzy_search*): the budget that
 *  cuts a call into blocks of queries x tiles of candidates, and the steps around hip/top_k.hip (selection.c) - reserve, begin a
 *  block, fold a tile, emit a block, drain.  Policy stays with the callers: the checks, the loops, how a tile is scored, the profile.
 *  Every step enqueues on the call's stream and returns; only the drain waits.
 */
#ifndef SZS_SELECTION_INTERNAL_H_
#define SZS_SELECTION_INTERNAL_H_

#include "szs_internal.h"

#define SZS_SELECTION_SCRATCH_CELLS ((size_t)16 << 20) /* 128 MiB of 8-byte cells: a tile the fold re-reads from the Infinity Cache */
#define SZS_SELECTION_LIST_BYTES ((size_t)128 << 20)   /* running lists of one block of queries */
#define SZS_SELECTION_MOST_ROWS ((size_t)1 << 18)      /* per side of a tile: tape calls stay device-planned (dispatch.c) */
#define SZS_SELECTION_WORKGROUPS 2048u                 /* the scan wants ~8 workgroups per CU: rows are split into segments below that */

/** How a call is cut: queries per block, candidates per tile, segments per row of the scan. */
typedef struct {
    size_t block, tile, segments;
} szs_selection_plan_t;

/**
 *  The budget of a call of `q_count` >= 1 queries: blocks whose lists fit SZS_SELECTION_LIST_BYTES and - with a long corpus - of few
 *  enough rows that a tile keeps 4096 columns; tiles whose cells fit the scratch matrix, at most the `top_k_tile` knob; segments so
 *  that the scan fills the GPU, each of at least 4096 columns.  `most_block_rows` and `most_tile_rows`: the caller's own caps
 *  (SIZE_MAX: none), at least 1.
 */
szs_selection_plan_t szs_selection_plan(size_t q_count, size_t c_count, size_t k, size_t most_block_rows, size_t most_tile_rows);

/** One call: the caller fills the first group, szs_selection_reserve the second. */
typedef struct {
    hipStream_t stream;
    int device, descending;
    size_t k, row_stride;
    szs_selection_plan_t plan;
    uint64_t *indices, *scores; /* the caller's arrays, rows `row_stride` apart; `scores` may be NULL */

    size_t width; /* of a list: szs_hip_top_k_width(k) */
    int direct;   /* the emit kernel writes the caller's arrays itself */
    uint64_t *cells, *lists, *partials, *staged;
} szs_selection_t;

/** Reserves a block x tile of cells, a block's lists with the segments' partial lists behind them, and - when a kernel cannot write
 *  the caller's arrays (plain host memory) - a block's dense output. */
sz_status_t szs_selection_reserve(szs_selection_t *call, szs_selection_buffers_t *buffers, char const **error_message);
/** Empties the lists of a block of `rows` queries. */
hipError_t szs_selection_block_begin(szs_selection_t const *call, size_t rows);
/** Folds the scored tile `cells[r * columns + c]` - queries q0 + r, candidates c0 + c - into the block's lists; `self`: query q0 + r
 *  skips candidate q0 + r. */
hipError_t szs_selection_fold(szs_selection_t const *call, size_t q0, size_t rows, size_t c0, size_t columns, int self);
/** The launches of one fold: the scan, and with segments the merge of their partial lists. */
static inline unsigned szs_selection_fold_launches(szs_selection_t const *call) { return call->plan.segments > 1 ? 2 : 1; }
/** Rows [q0, q0 + rows) of the caller's arrays from the block's lists: one launch, and for staged output one copy per array. */
hipError_t szs_selection_emit(szs_selection_t const *call, size_t q0, size_t rows);
/** Waits for the stream - the calls are synchronous, also when they fail - and returns `error`, or what the wait met. */
hipError_t szs_selection_drain(szs_selection_t const *call, hipError_t error);

#endif /* SZS_SELECTION_INTERNAL_H_ */
