/*
 *  selection_internal.h - what the calls that keep the k best candidates of every query share on the host (top_k.c: szs_rocm_top_k*;
 *  fingerprint_search.c: szs_rocm_fingerprint_top_k; fuzzy_search.c: szs_rocm_fuzzy_search*): the budget that
 *  cuts a call into blocks of queries x tiles of candidates, and the steps around hip/top_k.hip (selection.c) - reserve, begin a
 *  block, fold a tile, emit a block, drain.  Policy stays with the callers: the checks, the loops, how a tile is scored, the profile.
 *  Every step enqueues on the call's stream and returns; only the drain waits.  The calls that keep EVERY candidate inside a bound
 *  (within.c: szs_rocm_within*; fuzzy_search.c: szs_rocm_fuzzy_search_within*) share the budget, the buffers
 *  and the drain, and have steps of their own around hip/within.hip below; so do the calls that group ONE set of strings by those
 *  hits (clusters.c: szs_rocm_clusters*; fingerprint_search.c: szs_rocm_fingerprint_clusters), around
 *  hip/clusters.hip.
 */
#ifndef SZS_SELECTION_INTERNAL_H_
#define SZS_SELECTION_INTERNAL_H_

#include "szs_internal.h"

#include <string.h>

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
/** Waits for the call's stream - the calls are synchronous, also when they fail - and returns `error`, or what the wait met. */
hipError_t szs_selection_drain(hipStream_t stream, hipError_t error);

/* ---- what the calls whose tiles are ordinary engine calls share (top_k.c, within.c) ------------------------------------------------ */

/** Strings [first, first + count) of a sequence: the wrapper a slice of an sz_sequence_t input points into. */
typedef struct {
    sz_sequence_t sequence; /* first member: the handle of the wrapper is the wrapper itself */
    sz_sequence_t const *base;
    size_t first;
} szs_shifted_sequence_t;

/** Strings [first, first + count) of a side as an input of its own: a tape's offsets shifted, a sequence behind `wrapper`. */
szs_input_t szs_slice_input(szs_input_t const *input, size_t first, size_t count, szs_shifted_sequence_t *wrapper);
/** Adds a tile's profile - the engine call that scored it - to the sums of the call. */
void szs_selection_profile_add(szs_rocm_call_profile_t *total, szs_rocm_call_profile_t const *tile_profile);
/** The profile of a tiled call: the last tile's (`scored` 0, no tile: blank), with the sums over all tiles - kernel time: the scoring
 *  launches - and the wall time of the whole call since `started`. */
void szs_selection_profile_publish(szs_engine_s *engine, szs_rocm_call_profile_t const *total, int scored, double started);

/* ---- the second fold: every candidate inside a bound (hip/within.hip; within.c: szs_rocm_within*; fuzzy_search.c:
 *      szs_rocm_fuzzy_search_within*).  The same tiles, buffers and drain; no lists - a running count a row,
 *      and the leftmost `limit` hits straight into the caller's rows. ------------------------------------------------------------- */

#define SZS_SELECTION_SEGMENT_QUANTUM 1024u /* columns: what a workgroup of hip/within.hip walks in one round */

/** How a bounded call is cut: `cut.segments` workgroups a row, each `segment_columns` columns of a tile. */
typedef struct {
    szs_selection_plan_t cut;
    size_t segment_columns;
} szs_selection_within_plan_t;

/**
 *  The budget of a bounded call of `q_count` >= 1 queries: szs_selection_plan's, but the block is bounded by the dense copy of its
 *  output - 2 x block x limit x 8 bytes within SZS_SELECTION_LIST_BYTES - instead of by list bytes (`limit` 0: by neither).  Segments
 *  by the same rule - enough workgroups for the whole GPU, each at least 4096 columns - of a whole number of rounds, and as many as
 *  cover a full tile; a narrower last tile leaves the ones behind it idle.
 */
szs_selection_within_plan_t szs_selection_within_plan(size_t q_count, size_t c_count, size_t limit);

/** One call: the caller fills the first group, szs_selection_within_reserve the second, the steps count `folded`. */
typedef struct {
    hipStream_t stream;
    int device, descending;
    uint64_t bound; /* as the kernel compares it: unsigned <=, or - `descending` - signed >= */
    size_t limit, row_stride;
    szs_selection_within_plan_t plan;
    uint64_t *counts, *indices, *scores; /* the caller's: a vector, and rows `row_stride` apart; `limit` 0: the rows are not looked at */

    int direct, direct_counts; /* the kernels write the caller's rows / counts themselves */
    uint64_t *cells, *running, *staged_counts, *staged;
    uint32_t *partials;
    size_t folded; /* tiles of the current block whose hits the running counts hold: which half of `running` is current */
} szs_selection_within_t;

/** Reserves a block x tile of cells, two running counts and `cut.segments` partial counts a row, and - for what a kernel cannot
 *  write (plain host memory) - a block's dense counts and rows. */
sz_status_t szs_selection_within_reserve(szs_selection_within_t *call, szs_selection_buffers_t *buffers, char const **error_message);
/** Zeroes the counts of a block. */
hipError_t szs_selection_within_begin(szs_selection_within_t *call);
/** Folds the scored tile `cells[r * columns + c]` - szs_selection_fold's contract - into the block's counts and rows. */
hipError_t szs_selection_within_fold(szs_selection_within_t *call, size_t q0, size_t rows, size_t c0, size_t columns, int self);
/** The launches of one fold: the count pass, and with a `limit` the store pass. */
static inline unsigned szs_selection_within_fold_launches(szs_selection_within_t const *call) { return call->limit ? 2 : 1; }
/** Rows [q0, q0 + rows) of the caller's counts, and the empty pairs behind the hits of every row: one launch, and one copy per
 *  staged array. */
hipError_t szs_selection_within_finish(szs_selection_within_t *call, size_t q0, size_t rows);

/* ---- the third fold: the connected components of the hits (hip/clusters.hip; clusters.c: szs_rocm_clusters*; fingerprint_search.c:
 *      szs_rocm_fingerprint_clusters).  The same tiles - both sides the SAME strings -, buffers and drain; no
 *      rows and no counts - one forest of `count` 32-bit parents for the whole call, and a label a string behind the last tile. ---- */

#define SZS_CLUSTERS_MOST_STRINGS ((size_t)0xFFFFFFFFu) /* the forest is 32-bit words: a choice, not a measurement */

/** The budget of a call over `count` strings: szs_selection_within_plan(count, count, 0) within the caller's caps (SIZE_MAX: none). */
szs_selection_within_plan_t szs_selection_clusters_plan(size_t count, size_t most_block_rows, size_t most_tile_rows);

/** What a call over `count` strings scores, cut as `plan` cuts it: with `symmetric` the tiles of a block of rows start at the
 *  block's own first string - every pair i < j once, as (row i, column j), plus the block's own square below the diagonal -
 *  otherwise at 0, the whole square. */
void szs_selection_clusters_work(szs_selection_within_plan_t const *plan, size_t count, int symmetric, size_t *tiles, size_t *pairs);

/** One call: the caller fills the first group, szs_selection_clusters_reserve the second. */
typedef struct {
    hipStream_t stream;
    int device, descending;
    uint64_t bound; /* as the kernel compares it */
    size_t count;
    szs_selection_within_plan_t plan;
    uint64_t *labels; /* the caller's: `count` cells */

    int direct; /* the finish kernel writes the caller's labels itself */
    uint64_t *cells, *roots, *staged;
    uint32_t *parent;
} szs_selection_clusters_t;

/** Reserves a block x tile of cells, the forest - 4 bytes a string - with the 8-byte count of its roots, and - for labels a kernel
 *  cannot write (plain host memory) - 8 bytes a string of staging. */
sz_status_t szs_selection_clusters_reserve(szs_selection_clusters_t *call, szs_selection_buffers_t *buffers, char const **error_message);
/** Every string a root, no root counted: one launch. */
hipError_t szs_selection_clusters_begin(szs_selection_clusters_t const *call);
/** Joins the strings of every hit of the scored tile `cells[r * columns + c]` - strings q0 + r and c0 + c: one launch. */
hipError_t szs_selection_clusters_fold(szs_selection_clusters_t const *call, size_t q0, size_t rows, size_t c0, size_t columns);
/** The caller's labels and `*clusters_count`, a word the HOST can write: one launch, and a copy for each. */
hipError_t szs_selection_clusters_finish(szs_selection_clusters_t const *call, uint64_t *clusters_count);

#endif /* SZS_SELECTION_INTERNAL_H_ */
