/*
 *  stringzillas_rocm.h - ADDITIVE entry points of the ROCm build.  Nothing here changes a reference signature;
 *  a caller that only knows <stringzillas/stringzillas.h> never needs this header.
 *
 *  - szs_rocm_last_call_profile : device-event kernel time and work counters of the last engine call - the
 *    counterpart of the reference's `cuda_status_t::elapsed_milliseconds` / "Kernel GCUPS"
 *    (/root/reference/include/stringzillas/types.cuh:280-298,482-534; bench/similarities.cuh:303-308).
 *  - szs_rocm_last_pairing, szs_rocm_pair_rule_probe : which two queries shared a workgroup of the short launch that plans itself
 *    (csrc/hip/pair_rule.h) - what the last call's sorter chose, and the same choice on bare lengths without a GPU.
 *  - szs_rocm_corner_cut_probe  : the text columns in which the short Myers bodies skip an end word of the bit-vector
 *    (csrc/hip/corner_cut.h), on bare lengths without a GPU.
 *  - szs_rocm_shard_rows        : longest-processing-time assignment of query rows to N GPUs;
 *    the reference has no multi-GPU path at all (one engine call = one device, stringzillas.h:137).
 *  - szs_rocm_rerank_probe, szs_rocm_plan_probe, szs_rocm_orientation_probe, szs_rocm_team_orientation_probe, szs_rocm_launch_order_probe,
 *    szs_rocm_queue_probe : expose
 *    the host planner - refs, tier and orientation, lanes per item, launch shapes and order - so that it is unit-tested
 *    without a GPU (tests/test_host_logic.py).
 *  - szs_rocm_node_*            : one cross-product over the N GPUs of a host, in C (csrc/host/node.c).
 *  - szs_rocm_tuning_set        : the tuning / testing knobs.
 *  - szs_rocm_top_k*            : the k best candidates of every query, without the queries x candidates matrix (csrc/host/top_k.c).
 *  - szs_rocm_within*           : EVERY candidate of every query inside a score bound - the full count and the leftmost `limit` hits
 *    in fixed (queries x limit) rows (csrc/host/within.c); szs_rocm_fuzzy_search_within* answers the same for approximate substring
 *    matches (csrc/host/fuzzy_search.c), and szs_rocm_within_probe reports how either call would be cut.
 *  - szs_rocm_clusters*         : the connected components of those hits among ONE set of strings, a label per string - the groups of a
 *    deduplication, from a lock-free union-find on the device (csrc/host/clusters.c); szs_rocm_fingerprint_clusters groups MinHash
 *    fingerprints the same way, and szs_rocm_clusters_probe reports what a call would score.
 *  - szs_rocm_rerank*           : exact scores of LISTED candidates per query - what verifies the hits of a coarse search (top-k's own
 *    `indices`, a fingerprint search, any outside candidate generator) without a queries x candidates matrix (csrc/host/rerank.c).
 *  - szs_rocm_fuzzy_find*       : the best match of a query INSIDE each listed candidate - fewest edits to some substring, and where it
 *    ends - for a snippet in a document, a primer in a read, a misspelled name in a record (csrc/host/fuzzy_find.c).
 *  - szs_rocm_fuzzy_find_spans* : the same call with the whole span: where that best match starts as well.
 *  - szs_rocm_alignments*       : WHICH edits - per listed pair the edit script `= X I D` of the query against the candidate, or
 *    against the span of it that szs_rocm_fuzzy_find_spans* or szs_rocm_fuzzy_scan_occurrences* found: what differs between a snippet
 *    and the place it was found, the mismatches of a primer, the correction of a name (csrc/host/alignments.c).
 *  - szs_rocm_fuzzy_search*     : the k candidates of a corpus that contain the best such match per query, without the matrix
 *    (csrc/host/fuzzy_search.c); szs_rocm_fuzzy_search_probe reports how a call would be cut.
 *  - szs_rocm_fuzzy_scan*       : the best match of every query inside ONE long text, the text cut over the device's lanes
 *    (csrc/host/fuzzy_scan.c); szs_rocm_fuzzy_scan_spans* add the starts, szs_rocm_fuzzy_scan_probe reports the cut.
 *  - szs_rocm_fuzzy_scan_matches* : every end within a distance bound in that text, per query the count and the leftmost `limit`
 *    hits (csrc/host/fuzzy_scan_matches.c).
 *  - szs_rocm_fuzzy_scan_occurrences* : one span per occurrence in that text - the first column of every valley floor of the DP's
 *    bottom row within the bound, with its distance and where the match starts (csrc/host/fuzzy_scan_occurrences.c).
 *  - szs_rocm_fingerprint_matches, szs_rocm_fingerprint_top_k : what the MinHash fingerprints of szs_fingerprints_* are for - the
 *    equal dimensions of every pair of fingerprints (divided by `dimensions`: the Jaccard estimate) and the k candidates with the
 *    most of them per query, for near-duplicate search at `dimensions` compares per pair (csrc/host/fingerprint_search.c).
 */
#ifndef STRINGZILLAS_ROCM_H_
#define STRINGZILLAS_ROCM_H_

#include "stringzillas.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct szs_rocm_call_profile_t {
    double kernel_milliseconds;   /* hipEvent pair around the scoring launches, on the scope's stream */
    double host_milliseconds;     /* wall time of the whole C-ABI call, planning and copies included */
    sz_u64_t cells;               /* sum over scored pairs of len(query) * len(candidate): the GCUPS numerator */
    sz_u64_t pairs;               /* scored pairs (lower triangle only in symmetric mode) */
    sz_u64_t algorithmic_bytes;   /* sum over pairs of len(q) + len(c) + 2 * 4 + 8   */
    sz_u64_t unique_bytes;        /* bytes of both tapes + offsets + the results matrix, each counted once */
    sz_u32_t launches;            /* kernel launches issued */
    sz_u32_t longest_query;
    sz_u32_t longest_candidate;
    sz_u32_t tier;                /* 0: one pair per lane (lev_myers.hip, weighted*.hip); 1: systolic.hip; 2: myers_chain.hip */
    sz_u32_t transposed;          /* 1: the planner swapped the sides (candidates on workgroups, queries on lanes) */
    sz_u32_t cell_bits;           /* width of the DP cells of the last launch: 16 (weighted_packed.hip), 32, 64 (wide.hip), or 0 (bit-parallel) */
    sz_u32_t planner;             /* 0: planned on the host; 1: on the device (hip/planner.hip); 2: on the device, launches speculated;
                                     3: the plan of the previous call of the same tapes, re-used behind a guard;
                                     4: planned INSIDE the scoring launch (its first two workgroups sort the sides; hip/lev_myers.hip);
                                     5: not planned at all - the tiny-token kernel scores straight from the tapes (hip/myers_tiny.hip) */
    sz_u32_t team;                /* 0, or lanes * 10000 + registers * 100 + wavefronts per SIMD of the team tier (weighted_teams.hip) */
    sz_u32_t team_wide;           /* team tier: 0 cells ordered as half-float patterns (three-input maxima), 1 as unsigned integers */
    sz_u32_t streams;             /* streams the launches of the call were dealt over: 1 ... 8, never more than the `queues` knob */
    sz_u32_t queue_items;         /* 0, or the work items of the ONE persistent launch that scored every bit-parallel width of the call (myers_queue.hip) */
    sz_u32_t queue_tiles;         /* ... and the (query slice) x (candidate column) tiles its queue was ordered by */
} szs_rocm_call_profile_t;

/** Copies the profile of the most recent call made through `engine` (any of the four engine handle types). */
SZ_API_RUNTIME sz_status_t szs_rocm_last_call_profile(void *engine, szs_rocm_call_profile_t *profile);

/**
 *  The pairing rule of the most recent call made through `engine`: which two queries shared a workgroup of the short launch that
 *  plans itself (planner mode 4).  Queries ranked by descending length, slots = ceil(Q / 2), n = Q - slots: 0 - slot s < n scored
 *  ranks s and slots + s; delta + 1 - ranks s and slots + ((n - 1 - s + delta) mod n).  0 also when the call took another way.
 */
SZ_API_RUNTIME sz_u32_t szs_rocm_last_pairing(void *engine);

/**
 *  The same choice on bare lengths (any order), without a GPU.  `*rule` in: SZS_ROCM_PAIR_RULE_CHOOSE - choose as the launch
 *  does (rule 0 and sixteen evenly spaced shifts delta = k n / 16; the fewest words win, ties to rule 0, then to the smallest
 *  shift; more than 1024 queries, or one beyond 256 bytes: rule 0) - or a rule <= n to evaluate.  `*rule` out: the rule;
 *  `total_words` (optional): the bit-vector words per text column, summed over the slots; `slot_pairs_out` (optional, 2 x slots
 *  entries): the descending ranks of every slot's two queries, 0xFFFFFFFF where a slot has no second one.
 */
#define SZS_ROCM_PAIR_RULE_CHOOSE 0xFFFFFFFFu
SZ_API_RUNTIME sz_status_t szs_rocm_pair_rule_probe(sz_u32_t const *lengths, sz_size_t count, sz_u32_t *rule, sz_u64_t *total_words,
                                                    sz_u32_t *slot_pairs_out);

/**
 *  Which text columns of the short Myers bodies may leave an end word of the bit-vector untouched (csrc/hip/corner_cut.h), on bare
 *  lengths, without a GPU: a vector of `words` words holding a query of `first_length` bytes and - unless `second_length` is
 *  SZS_ROCM_NO_SECOND_QUERY - two separator rows and a second query above it, against the texts of one wavefront, the shortest of
 *  `n_short` and the longest of `n_long` bytes.  Columns counted from 0: those below `*head_until` may skip the top word, those from
 *  `*late_from` on the bottom word (SZS_ROCM_CORNER_CUT_NEVER: none does).  Fewer than three words: 0 and never.
 */
#define SZS_ROCM_NO_SECOND_QUERY 0xFFFFFFFFu
#define SZS_ROCM_CORNER_CUT_NEVER 0xFFFFFFFFu
SZ_API_RUNTIME sz_status_t szs_rocm_corner_cut_probe(sz_u32_t first_length, sz_u32_t second_length, sz_u32_t words, sz_u32_t n_short,
                                                     sz_u32_t n_long, sz_u32_t *head_until, sz_u32_t *late_from);

/**
 *  Deals `rows` query rows to `shards` devices so that the summed `row_weights` per shard are as equal as the
 *  longest-processing-time heuristic makes them (sort descending, always give to the lightest shard).
 *  `shard_of_row[i]` receives the shard of row i; `shard_loads` (optional) the resulting per-shard weight sums.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_shard_rows(sz_size_t const *row_weights, sz_size_t rows, sz_size_t shards,
                                               sz_u32_t *shard_of_row, sz_u64_t *shard_loads);

/**
 *  Deals the rows of a SYMMETRIC call's lower triangle to `shards` devices as contiguous bands of equal weight - row i weighs
 *  (len_i + 1) x sum_{j <= i} (len_j + 1), its cells - band g = rows [band_first[g], band_first[g + 1]);
 *  `band_first` holds shards + 1 entries, `band_weights` (optional) the weights dealt.  A band is its rows against every string
 *  before it (a rectangle) plus the triangle of its own rows: two ordinary calls of a single-GPU engine.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_shard_triangle(sz_size_t const *lengths, sz_size_t rows, sz_size_t shards, sz_size_t *band_first,
                                                   sz_u64_t *band_weights);

/**
 *  The k best candidates of every query, in one call, without materialising the queries x candidates matrix: the call is scored
 *  tile by tile (ordinary engine calls into device scratch) and every tile is folded into per-query lists on the device.
 *
 *  `engine`: a Levenshtein, Levenshtein UTF-8, Needleman-Wunsch or Smith-Waterman engine; any other handle is refused and nothing
 *  is written.  Row q receives `indices[q * row_stride + r]` and, when `scores` is not NULL, `scores[q * row_stride + r]` for
 *  r < k: 8-byte cells of the engine's own type (`sz_size_t` distances, `sz_ssize_t` scores).  Cells [k, row_stride) are left
 *  untouched.  Distances rank ascending, NW / SW scores descending; equal scores go to the LOWER candidate index.
 *
 *  `candidates` NULL: SELF-SEARCH - the queries against themselves, each query's own index excluded (duplicates at other indices
 *  count).  Unlike the matrix calls, where NULL means the symmetric matrix with its diagonal.
 *
 *  A row with fewer than k candidates (C < k, or C - 1 < k in self-search) is completed with index SZ_SIZE_MAX and score 0.
 *  1 <= k <= 1024 and row_stride >= k, else sz_unexpected_dimensions_k.  Zero queries: success, nothing written; zero candidates:
 *  every row is completed that way.  Candidate counts beyond 2^32 are fine.  Inputs and outputs may live in host, pinned, unified
 *  or device memory, as for the matrix calls.  Synchronous, also when it fails.  The `top_k_tile` knob caps the candidates of a tile.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_top_k(void *engine, szs_device_scope_t device, sz_sequence_t const *queries,
                                          sz_sequence_t const *candidates, sz_size_t k, sz_size_t *indices, void *scores,
                                          sz_size_t row_stride, char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_top_k_u32tape(void *engine, szs_device_scope_t device, sz_sequence_u32tape_t const *queries,
                                                  sz_sequence_u32tape_t const *candidates, sz_size_t k, sz_size_t *indices,
                                                  void *scores, sz_size_t row_stride, char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_top_k_u64tape(void *engine, szs_device_scope_t device, sz_sequence_u64tape_t const *queries,
                                                  sz_sequence_u64tape_t const *candidates, sz_size_t k, sz_size_t *indices,
                                                  void *scores, sz_size_t row_stride, char const **error_message);

/**
 *  WITHIN: every candidate of every query inside a score bound - "everything at least this close", where szs_rocm_top_k answers
 *  "the k best" - in one call, without materialising the queries x candidates matrix and without an output that grows with the data:
 *      counts[q]                     = the number of hits of query q among ALL candidates (it may exceed `limit`),
 *      indices[q * row_stride + i]   = the candidate of its i-th hit in ASCENDING candidate index, and - `scores` not NULL -
 *      scores[q * row_stride + i]    = the score of that pair, an 8-byte cell of the engine's own type,   for i < min(counts[q], limit);
 *  slots [min(counts[q], limit), limit) hold index SZ_SIZE_MAX and score 0 - szs_rocm_top_k's empty pair, the slot that
 *  szs_rocm_rerank, szs_rocm_fuzzy_find and szs_rocm_alignments skip, so the rows feed them directly - and cells [limit, row_stride)
 *  are left untouched.  `limit` 0 writes `counts` only: `indices` and `scores` may then be NULL and are not looked at.
 *
 *  `engine`: any engine szs_rocm_top_k takes - Levenshtein over bytes or UTF-8 at any costs, Needleman-Wunsch, Smith-Waterman.  A
 *  DISTANCE engine hits iff bound >= 0 and score <= bound (a negative bound: no hits, and nothing is scored); NW and SW hit iff the
 *  signed score >= bound.  `candidates` NULL: SELF-SEARCH, each query's own index excluded (duplicates at other indices count).
 *
 *  Refused before anything is launched, with nothing written, in this order: limit > 65,536 or row_stride < limit
 *  (sz_unexpected_dimensions_k; the cap is a choice, not a measurement - `counts` is the full number whatever the limit); an engine that
 *  is none of the above; NULL queries (zero queries: success, nothing is looked at); NULL `counts`; with limit > 0 a NULL `indices`
 *  (each sz_status_unknown_k).  Zero candidates: counts of 0 and empty rows.  Candidate counts beyond 2^32 are fine.  Inputs and outputs
 *  may live in host, pinned, unified or device memory; plain host outputs are staged densely - 2 x block x limit x 8 bytes within 128 MiB
 *  bound the queries of a block - and copied in one 2-D copy per array.  Synchronous, also when it fails.
 *
 *  The call scores szs_rocm_top_k's tiles (ordinary engine calls into device scratch) and folds each with csrc/hip/within.hip: a
 *  count pass, a store pass - not launched with limit 0 - and after the last tile one launch for the counts and the empty slots.  No
 *  atomic decides a slot: the bytes written depend on the strings, the bound and the limit alone.  The `top_k_tile` knob caps the
 *  candidates of a tile.  szs_rocm_last_call_profile: pairs and cells of the scoring launches; launches = scoring, count, store and
 *  finish launches; kernel time = the scoring launches.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_within(void *engine, szs_device_scope_t device, sz_sequence_t const *queries,
                                           sz_sequence_t const *candidates, sz_ssize_t bound, sz_size_t limit, sz_size_t *counts,
                                           sz_size_t *indices, void *scores, sz_size_t row_stride, char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_within_u32tape(void *engine, szs_device_scope_t device, sz_sequence_u32tape_t const *queries,
                                                   sz_sequence_u32tape_t const *candidates, sz_ssize_t bound, sz_size_t limit,
                                                   sz_size_t *counts, sz_size_t *indices, void *scores, sz_size_t row_stride,
                                                   char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_within_u64tape(void *engine, szs_device_scope_t device, sz_sequence_u64tape_t const *queries,
                                                   sz_sequence_u64tape_t const *candidates, sz_ssize_t bound, sz_size_t limit,
                                                   sz_size_t *counts, sz_size_t *indices, void *scores, sz_size_t row_stride,
                                                   char const **error_message);

/**
 *  How szs_rocm_within and szs_rocm_fuzzy_search_within would cut a call of these counts - host only, no GPU: the queries of a block,
 *  the candidates of a tile, the workgroups that share a row of the fold (`segments`) and the columns of each (`segment_columns`, a
 *  multiple of 1024; segments x segment_columns >= tile).  The `top_k_tile` knob applies as it does to the calls.  Outputs are optional.
 *  limit > 65,536: sz_unexpected_dimensions_k.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_within_probe(sz_size_t queries_count, sz_size_t candidates_count, sz_size_t limit, sz_size_t *block,
                                                 sz_size_t *tile, sz_size_t *segments, sz_size_t *segment_columns);

/**
 *  CLUSTERS: the connected components of the graph "i ~ j iff the pair is a szs_rocm_within hit", as one label per string - the groups
 *  a deduplication wants, where szs_rocm_within returns rows of neighbours that truncate at `limit`.  For n strings and a bound:
 *      hit(i, j), i != j   = szs_rocm_within's predicate on the score of query i against candidate j: a DISTANCE engine hits iff
 *                            bound >= 0 and score <= bound, compared unsigned; NW and SW hit iff the signed score >= bound;
 *      i ~ j               iff hit(i, j) or hit(j, i): the graph is undirected;
 *      labels[i]           = the SMALLEST index in the connected component of i, so labels[labels[i]] == labels[i]; a string with no
 *                            neighbour labels itself; duplicates of one string are ordinary hits (distance 0) and share a component;
 *      *clusters_count     = the number of i with labels[i] == i (`clusters_count` may be NULL).
 *  The result is a function of the strings, the engine and the bound alone: no knob, tile size or arrival order changes a byte -
 *  atomics build the forest, the minimum-index label is what makes their order invisible.  A negative bound on a distance engine
 *  gives labels 0 .. n-1, and nothing is scored.  n == 0 succeeds with nothing written except *clusters_count = 0.
 *
 *  `engine`: any engine szs_rocm_within takes.  `labels`: n 8-byte cells in host, pinned, unified or device memory; plain host memory
 *  is staged - n x 8 bytes, not data-dependent.  Refused before anything is launched, with nothing written, in this order: more than
 *  2^32 - 1 strings (sz_unexpected_dimensions_k; a choice, not a measurement - the forest is 32-bit words, and the square of that
 *  count is beyond any call); an engine that is none of the above; NULL strings; with n > 0 NULL `labels` (each sz_status_unknown_k).
 *  Synchronous, also when it fails.
 *
 *  The call scores szs_rocm_within's self-form tiles (ordinary engine calls into device scratch) and folds each with
 *  csrc/hip/clusters.hip: a lock-free union-find over n 32-bit parents, hooking the larger root under the smaller.  Where the engine
 *  is symmetric in its two sides - every Levenshtein engine; NW and SW iff their substitution table is symmetric over the classes in
 *  use - the tiles of a block of rows start at the block's own first string, so every pair i < j is scored once; otherwise the whole
 *  square is scored.  The `top_k_tile` knob caps the columns of a tile.  szs_rocm_last_call_profile: pairs and cells are the sums
 *  over the scoring launches, so the triangle shows there; launches = scoring, begin, union and finish launches; kernel time = the
 *  scoring launches.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_clusters(void *engine, szs_device_scope_t device, sz_sequence_t const *strings, sz_ssize_t bound,
                                             sz_size_t *labels, sz_size_t *clusters_count, char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_clusters_u32tape(void *engine, szs_device_scope_t device, sz_sequence_u32tape_t const *strings,
                                                     sz_ssize_t bound, sz_size_t *labels, sz_size_t *clusters_count,
                                                     char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_clusters_u64tape(void *engine, szs_device_scope_t device, sz_sequence_u64tape_t const *strings,
                                                     sz_ssize_t bound, sz_size_t *labels, sz_size_t *clusters_count,
                                                     char const **error_message);

/**
 *  The same components over MinHash fingerprints: rows i != j of an (n x dimensions) hash matrix hit iff at least `min_matches` of
 *  their dimensions are equal (szs_rocm_fingerprint_matches' count).  `hashes_stride` in bytes, as for szs_rocm_fingerprint_top_k;
 *  hashes in plain host memory are staged tile by tile.  min_matches == 0 makes every pair a hit - one cluster; min_matches beyond
 *  the dimensions none, and nothing is scored.  Refused in this order: more than 2^32 - 1 rows; a stride that is no multiple of 4, an
 *  engine that is no fingerprints engine, a stride below 4 x dimensions; then - n == 0 succeeds as above - NULL `hashes`, NULL `labels`.
 *  Matches are symmetric: always the triangle.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_fingerprint_clusters(void *engine, szs_device_scope_t device, sz_u32_t const *hashes,
                                                         sz_size_t hashes_stride, sz_size_t count, sz_size_t min_matches,
                                                         sz_size_t *labels, sz_size_t *clusters_count, char const **error_message);

/**
 *  How szs_rocm_clusters would cut a call over `count` strings - host only, no GPU: the rows of a block, the columns of a tile, and
 *  the tiles and pairs it would score - with `symmetric` the triangle (per block of rows, rows x (count - first row of the block)),
 *  otherwise the square.  The `top_k_tile` knob applies as it does to the call.  Outputs are optional.  count > 2^32 - 1:
 *  sz_unexpected_dimensions_k.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_clusters_probe(sz_size_t count, int symmetric, sz_size_t *block, sz_size_t *tile,
                                                   sz_size_t *tiles_scored, sz_size_t *pairs_scored);

/**
 *  Rerank: the exact scores of the candidates an index row LISTS per query, in one call -
 *      scores[q * row_stride + r] = score(queries[q], candidates[indices[q * row_stride + r]])   for r < k,
 *  8-byte cells of the engine's own type (`sz_size_t` distances, `sz_ssize_t` scores): exactly the value the matrix call would put
 *  in that cell.  `indices` and `scores` share `row_stride`, in 8-byte cells - the layout szs_rocm_top_k* and
 *  szs_rocm_fingerprint_top_k write, so their `indices` output is this call's input unchanged.
 *
 *  `engine`: a Levenshtein, Levenshtein UTF-8, Needleman-Wunsch or Smith-Waterman engine; any other handle is refused and nothing
 *  is written.  An index equal to SZ_SIZE_MAX is the empty slot those calls emit: its score cell receives 0 and no string is
 *  touched.  Any other index >= the candidates' count fails the whole call with sz_unexpected_dimensions_k, and no string or offset
 *  is ever read through it: indices the host can read are validated before anything is launched, indices only the device can read
 *  are checked by the kernel before every use.  After a failed call the contents of `scores` are unspecified.  Duplicate indices
 *  within a row, and the same candidate in many rows, are fine.
 *
 *  `candidates` NULL: the indices refer to `queries` themselves - the self-search form of top-k; no index is excluded.
 *
 *  k >= 1, with no upper bound, and row_stride >= k, else sz_unexpected_dimensions_k; score cells [k, row_stride) are left
 *  untouched.  Zero queries: success, nothing written.  `indices` and `scores` must not be NULL.  Both may live in host, pinned,
 *  unified or device memory, as may the strings' offsets.  The call runs on the scope's stream and is synchronous, also when it fails.
 *
 *  Rows of a unit-cost byte Levenshtein engine whose query has at most 256 bytes are scored by ONE launch of a kernel made for this
 *  shape (a group of lanes and a match table per row, one listed candidate per lane: csrc/hip/myers_rerank.hip); rows whose query
 *  has more than 256 and at most 65,536 bytes - documents - by ONE launch of its twin that walks the query as strips of up to 256
 *  rows (csrc/hip/myers_rerank_strips.hip); every other row is an ordinary 1 x k engine call of its own.  64 KiB is a design bound,
 *  not a measured one: beyond it one lane's serial chain over the strips is the wrong tool and the engine's chained tiers for few
 *  long pairs, which the engine call reaches, are built for such rows.  One call may mix all three; the `rerank` knob at 0 sends
 *  every row down the last route, at 1 every row of more than 256 bytes.
 *  szs_rocm_last_call_profile reports the sums over the call: pairs (non-empty slots), cells, kernel time, launches, wall time.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_rerank(void *engine, szs_device_scope_t device, sz_sequence_t const *queries,
                                           sz_sequence_t const *candidates, sz_size_t const *indices, sz_size_t k, void *scores,
                                           sz_size_t row_stride, char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_rerank_u32tape(void *engine, szs_device_scope_t device, sz_sequence_u32tape_t const *queries,
                                                   sz_sequence_u32tape_t const *candidates, sz_size_t const *indices, sz_size_t k,
                                                   void *scores, sz_size_t row_stride, char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_rerank_u64tape(void *engine, szs_device_scope_t device, sz_sequence_u64tape_t const *queries,
                                                   sz_sequence_u64tape_t const *candidates, sz_size_t const *indices, sz_size_t k,
                                                   void *scores, sz_size_t row_stride, char const **error_message);

/**
 *  Fuzzy substring search: where inside a candidate does something close to the query occur, and how close?  For a query q of m
 *  bytes and a candidate c of n bytes let D be the unit-cost DP with a FREE START in the text: D[0][j] = 0, D[i][0] = i,
 *  D[i][j] = min(D[i-1][j-1] + (q[i-1] != c[j-1]), D[i-1][j] + 1, D[i][j-1] + 1).  Per pair the call writes
 *      distances[q * row_stride + r] = min over j in [0, n] of D[m][j]  - the fewest edits that turn q into SOME substring of c: at
 *                                      most m, and at most the global distance;
 *      ends[q * row_stride + r]      = the smallest j that attains it   - the exclusive byte offset in c at which the leftmost-ending
 *                                      best match ends; 0: the empty substring (distance m).
 *  Start offsets are szs_rocm_fuzzy_find_spans' (below).  `ends` may be NULL, `distances` may not.
 *
 *  Rows and slots are szs_rocm_rerank's: `indices`, `distances` and `ends` share `row_stride`, in 8-byte cells; slot r of row q pairs
 *  queries[q] with candidates[indices[q * row_stride + r]] for r < k; cells [k, row_stride) are left untouched; k >= 1 and
 *  row_stride >= k, else sz_unexpected_dimensions_k.  An index of SZ_SIZE_MAX is an empty slot: distance 0, end 0, no string
 *  touched.  Any other index >= the candidates' count fails the whole call with sz_unexpected_dimensions_k and addresses nothing:
 *  indices the host can read are validated before anything is launched, indices only the device can read are checked by the kernel
 *  before every use.  After a failed call the contents of the outputs are unspecified.
 *  `indices` NULL is the DENSE form - every query in every candidate, without a queries x candidates index matrix: slot r is
 *  candidate r, and k must equal the candidates' count, else sz_unexpected_dimensions_k.
 *  `candidates` NULL: the indices refer to `queries` themselves; no index is excluded.
 *
 *  TWO LIMITS.  (1) `engine` must be a unit-cost BYTE Levenshtein engine (szs_levenshtein_distances_init with match 0, mismatch 1,
 *  open 1, extend 1): any other engine - other costs, UTF-8 codepoints, Needleman-Wunsch, Smith-Waterman - and a blank or NULL one is
 *  refused with sz_status_unknown_k and a message, and nothing is written.  (2) Every query has at most 256 bytes: a longer one fails
 *  the whole call with sz_unexpected_dimensions_k.  Candidates may have any length below 4 GiB.  There is no slower route behind
 *  either limit: no engine call computes this distance.
 *
 *  Zero queries: success, nothing written.  `indices`, the outputs and the strings' offsets may live in host, pinned, unified or
 *  device memory; the strings themselves must be readable by the device.  The call runs on the scope's stream and is synchronous,
 *  also when it fails.  All rows of up to 2^20 queries are ONE launch (csrc/hip/myers_fuzzy_find.hip).
 *  szs_rocm_last_call_profile reports the sums over the call: pairs (non-empty slots), cells (m x n over them), kernel time,
 *  launches, wall time.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_find(void *engine, szs_device_scope_t device, sz_sequence_t const *queries,
                                               sz_sequence_t const *candidates, sz_size_t const *indices, sz_size_t k,
                                               sz_size_t *distances, sz_size_t *ends, sz_size_t row_stride, char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_find_u32tape(void *engine, szs_device_scope_t device, sz_sequence_u32tape_t const *queries,
                                                       sz_sequence_u32tape_t const *candidates, sz_size_t const *indices, sz_size_t k,
                                                       sz_size_t *distances, sz_size_t *ends, sz_size_t row_stride,
                                                       char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_find_u64tape(void *engine, szs_device_scope_t device, sz_sequence_u64tape_t const *queries,
                                                       sz_sequence_u64tape_t const *candidates, sz_size_t const *indices, sz_size_t k,
                                                       sz_size_t *distances, sz_size_t *ends, sz_size_t row_stride,
                                                       char const **error_message);

/**
 *  Fuzzy find with SPANS: szs_rocm_fuzzy_find and, per pair, where the match starts - candidate[start : end] is the snippet to
 *  highlight, the primer to cut out, the misspelled name to extract.  `distances` and `ends` are exactly szs_rocm_fuzzy_find's, and
 *
 *      starts[q * row_stride + r] = end - t*,  t* = the smallest t in [0, min(end, m + distance)] for which the global unit-cost
 *                                   distance of q and c[end - t : end] equals `distance`
 *
 *  - the SHORTEST best match that ends at `end`.  Such a t exists (D[m][end] is the minimum over every start of that distance), none
 *  gives less, and any t that attains `distance` has |t - m| <= distance: the span is at most m + distance <= 2 m bytes long.
 *  end = 0 (nothing of the query occurs, or it is empty) gives start = 0; an empty slot gives (0, 0, 0).
 *
 *  All three outputs are required: a NULL one is refused with sz_status_unknown_k and nothing is written.  They share `row_stride`
 *  with `indices`.  Every other rule - rows and slots, the dense and the self form, the two limits, refusals, memory kinds, what a
 *  failed call leaves behind - is szs_rocm_fuzzy_find's.  A block of rows is TWO launches on the scope's stream: the forward kernel,
 *  unchanged, and behind it a reverse pass over at most m + distance bytes per pair (csrc/hip/myers_fuzzy_spans.hip).
 *  szs_rocm_last_call_profile reports launches = 2 per block, pairs as before, and cells = m x n + m x min(end, m + distance) over
 *  the non-empty slots.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_find_spans(void *engine, szs_device_scope_t device, sz_sequence_t const *queries,
                                                     sz_sequence_t const *candidates, sz_size_t const *indices, sz_size_t k,
                                                     sz_size_t *distances, sz_size_t *starts, sz_size_t *ends, sz_size_t row_stride,
                                                     char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_find_spans_u32tape(void *engine, szs_device_scope_t device,
                                                             sz_sequence_u32tape_t const *queries,
                                                             sz_sequence_u32tape_t const *candidates, sz_size_t const *indices,
                                                             sz_size_t k, sz_size_t *distances, sz_size_t *starts, sz_size_t *ends,
                                                             sz_size_t row_stride, char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_find_spans_u64tape(void *engine, szs_device_scope_t device,
                                                             sz_sequence_u64tape_t const *queries,
                                                             sz_sequence_u64tape_t const *candidates, sz_size_t const *indices,
                                                             sz_size_t k, sz_size_t *distances, sz_size_t *starts, sz_size_t *ends,
                                                             sz_size_t row_stride, char const **error_message);

/**
 *  ALIGNMENTS: which edits.  For slot (q, r) let c = candidates[indices[q * row_stride + r]] of n bytes, s = c[start : end] of t bytes
 *  where `starts` and `ends` are given (start = starts[q * row_stride + r], end likewise), else s = c, and m = len(queries[q]).  S is
 *  the unit-cost SUFFIX DP of q and s:
 *      S[m][j] = t - j,  S[i][t] = m - i,  S[i][j] = min(S[i+1][j+1] + (q[i] != s[j]), S[i+1][j] + 1, S[i][j+1] + 1).
 *  The CANONICAL script is the walk from (0, 0) to (m, t) that takes, at (i, j), the first of these that holds:
 *      1. i < m, j < t and S[i+1][j+1] + (q[i] != s[j]) == S[i][j]:  '=' if the bytes are equal, else 'X' - one byte of each string;
 *      2. i < m and S[i+1][j] + 1 == S[i][j]:                        'I' - a byte of the query alone;
 *      3. otherwise:                                                 'D' - a byte of the candidate alone.
 *  The letters are those of extended CIGAR with the query as the read.  Per slot the call writes
 *      distances[q * row_stride + r] = S[0][0] = lev(q, s);
 *      lengths[q * row_stride + r]   = L, the number of ops: max(m, t) <= L <= m + t;
 *      ops[(q * row_stride + r) * capacity + 0 .. L)       = the script in forward order, the ASCII bytes `= X I D`;
 *      ops[(q * row_stride + r) * capacity + L .. capacity) = 0.
 *  L > capacity: `lengths` still holds L, all `capacity` bytes of the slot are zero and the call succeeds - the rule `counts` and
 *  `limit` follow in the scans.  `capacity` 0 with `ops` NULL returns distances and lengths only; `ops` NULL with a capacity above 0
 *  is refused (sz_status_unknown_k).  `distances` and `lengths` are required.  `starts` and `ends` are both NULL or both given: exactly
 *  one is refused with sz_status_unknown_k.
 *
 *  Everything else is szs_rocm_fuzzy_find_spans': rows and slots (`indices`, `starts`, `ends`, `distances` and `lengths` share
 *  `row_stride`, in cells; `ops` has `capacity` bytes per cell of that layout), k >= 1 and row_stride >= k, cells and `ops` slots at
 *  [k, row_stride) left untouched, the dense form (`indices` NULL, k = the candidates' count), the self form (`candidates` NULL), index
 *  validation on the host where it can read the indices and in the kernel before every use otherwise, the memory kinds of every
 *  array, a synchronous call on the scope's stream.  An EMPTY slot is an index of SZ_SIZE_MAX or - with spans - start = end =
 *  SZ_SIZE_MAX: distance 0, length 0, zero ops, no string touched; so the (rows, limit) matrices of
 *  szs_rocm_fuzzy_scan_occurrences go straight in over [text] with an all-zero index matrix.
 *
 *  LIMITS, each refused as szs_rocm_fuzzy_find refuses its own.  The engine is not a unit-cost byte Levenshtein engine:
 *  sz_status_unknown_k, nothing written.  A query above 256 bytes: sz_unexpected_dimensions_k, before anything is launched.  A span -
 *  or, without spans, a whole candidate - above 512 bytes: sz_unexpected_dimensions_k; 512 is a design bound, m + distance <= 512 is
 *  all a span from this library can be.  `starts` and `ends` are values the kernel reads from memory the caller owns:
 *  start <= end <= n is checked before they address anything, else the call fails with sz_unexpected_dimensions_k.
 *
 *  All rows of up to 2^20 queries are ONE launch (csrc/hip/myers_alignments.hip): the pass of the spans over the reversed strings
 *  with every column's trace kept, then one walk per pair.  The trace lives in an engine buffer that does not grow with the call - at
 *  most 256 MiB of workgroup regions, each reused for every row its workgroup serves (the `align_trace_kib` knob: another budget).
 *  szs_rocm_last_call_profile reports pairs (non-empty slots), cells (m x t over them), launches = 1 per block, and bytes that
 *  include the L ops of every pair.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_alignments(void *engine, szs_device_scope_t device, sz_sequence_t const *queries,
                                               sz_sequence_t const *candidates, sz_size_t const *indices, sz_size_t k,
                                               sz_size_t const *starts, sz_size_t const *ends, sz_size_t *distances, sz_size_t *lengths,
                                               sz_u8_t *ops, sz_size_t capacity, sz_size_t row_stride, char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_alignments_u32tape(void *engine, szs_device_scope_t device, sz_sequence_u32tape_t const *queries,
                                                       sz_sequence_u32tape_t const *candidates, sz_size_t const *indices, sz_size_t k,
                                                       sz_size_t const *starts, sz_size_t const *ends, sz_size_t *distances,
                                                       sz_size_t *lengths, sz_u8_t *ops, sz_size_t capacity, sz_size_t row_stride,
                                                       char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_alignments_u64tape(void *engine, szs_device_scope_t device, sz_sequence_u64tape_t const *queries,
                                                       sz_sequence_u64tape_t const *candidates, sz_size_t const *indices, sz_size_t k,
                                                       sz_size_t const *starts, sz_size_t const *ends, sz_size_t *distances,
                                                       sz_size_t *lengths, sz_u8_t *ops, sz_size_t capacity, sz_size_t row_stride,
                                                       char const **error_message);

/**
 *  Fuzzy SEARCH: which candidates of a corpus contain something close to the query?  Row q receives the k candidates with the
 *  smallest szs_rocm_fuzzy_find distance of queries[q] - min over j of D[m][j], free start in the text - in ascending order, ties
 *  to the LOWER candidate index (szs_rocm_top_k's rule, from the same scan):
 *      indices[q * row_stride + i], distances[q * row_stride + i] for i < k, and - where the arrays are given -
 *      ends[q * row_stride + i], starts[q * row_stride + i]: exactly what szs_rocm_fuzzy_find / szs_rocm_fuzzy_find_spans return for
 *      the pair (q, indices[q * row_stride + i]), bit for bit.
 *  Cells [k, row_stride) are left untouched.  No queries x candidates matrix is written anywhere the caller sees: the call scores
 *  tiles of (a block of queries) x (up to 2^18 candidates) into device scratch with csrc/hip/myers_fuzzy_tile.hip - one workgroup
 *  per (query, segment of the tile's candidates), so a few queries over a large corpus fill the device - and folds every tile into
 *  per-query lists with csrc/hip/top_k.hip.  `ends` and `starts` come from a winners pass: szs_rocm_fuzzy_find's kernels on the
 *  k listed candidates of every row; a call without `ends` launches none.
 *
 *  `candidates` NULL: SELF-SEARCH - the queries in each other, each query's own index excluded.  A row with fewer than k candidates
 *  (none at all; the self-search of one query) is completed with index SZ_SIZE_MAX, distance 0, end 0, start 0.  A query of no
 *  bytes has distance 0 and end 0 in every candidate: its row lists candidates 0 ... k - 1.
 *
 *  1 <= k <= 1024 and row_stride >= k, else sz_unexpected_dimensions_k - checked first.  `engine` must be a unit-cost BYTE
 *  Levenshtein engine, as for szs_rocm_fuzzy_find: any other, a blank or a NULL one is refused with sz_status_unknown_k.  Zero
 *  queries: success, nothing is looked at.  `indices` and `distances` are required, `ends` is optional, `starts` requires `ends`: a
 *  missing one is refused with sz_status_unknown_k.  A query of more than 256 bytes fails the whole call with
 *  sz_unexpected_dimensions_k before anything is launched.  Nothing is written on a refusal.  The outputs may live in device,
 *  pinned, unified or plain host memory (staged densely, one 2-D copy per array), the strings' offsets likewise; the strings
 *  themselves must be readable by the device.  Synchronous, also when it fails.
 *
 *  Knobs, none of which changes a result: `top_k_tile` caps the candidates of a tile, `fuzzy_search_segment` sets the candidates one
 *  workgroup scores for its row (rounded up to a multiple of 64; automatic: enough workgroups to fill the device four times over).
 *  szs_rocm_last_call_profile: pairs and cells of every scored (query, candidate) - the self column included - plus the winners
 *  pass's; launches = scoring, scan / fold, emit and winners-pass launches; kernel time = the scoring launches.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_search(void *engine, szs_device_scope_t device, sz_sequence_t const *queries,
                                                 sz_sequence_t const *candidates, sz_size_t k, sz_size_t *indices, sz_size_t *distances,
                                                 sz_size_t *starts, sz_size_t *ends, sz_size_t row_stride, char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_search_u32tape(void *engine, szs_device_scope_t device, sz_sequence_u32tape_t const *queries,
                                                         sz_sequence_u32tape_t const *candidates, sz_size_t k, sz_size_t *indices,
                                                         sz_size_t *distances, sz_size_t *starts, sz_size_t *ends, sz_size_t row_stride,
                                                         char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_search_u64tape(void *engine, szs_device_scope_t device, sz_sequence_u64tape_t const *queries,
                                                         sz_sequence_u64tape_t const *candidates, sz_size_t k, sz_size_t *indices,
                                                         sz_size_t *distances, sz_size_t *starts, sz_size_t *ends, sz_size_t row_stride,
                                                         char const **error_message);

/**
 *  How szs_rocm_fuzzy_search would cut a call of these counts - host only, no GPU: the queries of a block, the candidates of a tile,
 *  the candidates one workgroup of the tile kernel scores for its row (`segment`, a multiple of 64) and the workgroups of the first
 *  tile's launch = rows of the block x ceil(tile / segment).  The knobs apply as they do to the call.  Outputs are optional.
 *  k outside [1, 1024] or `longest_query` above 256: sz_unexpected_dimensions_k.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_search_probe(sz_size_t queries_count, sz_size_t candidates_count, sz_size_t k,
                                                       sz_size_t longest_query, sz_size_t *block, sz_size_t *tile, sz_size_t *segment,
                                                       sz_size_t *workgroups);

/**
 *  Fuzzy search WITHIN a bound: every candidate that contains something within `max_distance` edits of the query.  A hit of query q is
 *  a candidate whose szs_rocm_fuzzy_find distance - min over j of D[m][j] - is <= max_distance:
 *      counts[q]                   = the number of hits among ALL candidates (it may exceed `limit`),
 *      indices[q * row_stride + i] = the candidate of the i-th hit in ASCENDING candidate index, for i < min(counts[q], limit), and -
 *      where the arrays are given - distances[...], ends[...], starts[...]: exactly what szs_rocm_fuzzy_find /
 *      szs_rocm_fuzzy_find_spans return for the rows of `indices`, bit for bit;
 *  slots [min(counts[q], limit), limit) hold (SZ_SIZE_MAX, 0, 0, 0), cells [limit, row_stride) are left untouched, and `limit` 0 writes
 *  `counts` only - no other array is looked at.  `max_distance` is any sz_size_t: no distance exceeds the query's length, so the
 *  kernels receive min(max_distance, 256).  A query of no bytes hits every candidate.  `candidates` NULL: SELF-SEARCH, the own index
 *  excluded.
 *
 *  Engines, query lengths and statuses are szs_rocm_fuzzy_search's - a unit-cost BYTE Levenshtein engine, queries of at most 256 bytes
 *  (a longer one fails the whole call with sz_unexpected_dimensions_k before anything is launched) - and the refusals come in its
 *  order, with nothing written: limit > 65,536 or row_stride < limit (sz_unexpected_dimensions_k; the cap is a choice, not a
 *  measurement); the engine; NULL queries (zero queries: success); NULL `counts`; with limit > 0 a NULL `indices`, `ends` without
 *  `distances`, `starts` without `ends` (each sz_status_unknown_k).  Synchronous, also when it fails.
 *
 *  The call is szs_rocm_fuzzy_search's with the fold of csrc/hip/within.hip in place of the sorting one: the same tile kernel, the
 *  same knobs (`top_k_tile`, `fuzzy_search_segment`), none of which changes a result; `ends` and `starts` come from the same winners
 *  pass over the (queries x limit) index rows, and a call without `ends` or with limit 0 launches none.  szs_rocm_last_call_profile:
 *  pairs and cells of every scored (query, candidate) plus the winners pass's (every slot of a row that holds a hit); launches =
 *  scoring, count, store, finish and winners-pass launches; kernel time = the scoring launches.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_search_within(void *engine, szs_device_scope_t device, sz_sequence_t const *queries,
                                                        sz_sequence_t const *candidates, sz_size_t max_distance, sz_size_t limit,
                                                        sz_size_t *counts, sz_size_t *indices, sz_size_t *distances, sz_size_t *starts,
                                                        sz_size_t *ends, sz_size_t row_stride, char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_search_within_u32tape(void *engine, szs_device_scope_t device,
                                                                sz_sequence_u32tape_t const *queries,
                                                                sz_sequence_u32tape_t const *candidates, sz_size_t max_distance,
                                                                sz_size_t limit, sz_size_t *counts, sz_size_t *indices,
                                                                sz_size_t *distances, sz_size_t *starts, sz_size_t *ends,
                                                                sz_size_t row_stride, char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_search_within_u64tape(void *engine, szs_device_scope_t device,
                                                                sz_sequence_u64tape_t const *queries,
                                                                sz_sequence_u64tape_t const *candidates, sz_size_t max_distance,
                                                                sz_size_t limit, sz_size_t *counts, sz_size_t *indices,
                                                                sz_size_t *distances, sz_size_t *starts, sz_size_t *ends,
                                                                sz_size_t row_stride, char const **error_message);

/**
 *  Fuzzy SCAN: many short patterns in ONE long text - a chromosome, a book, a log file, a concatenated corpus.  For every query q
 *  of m bytes and the text c of n = `text_length` bytes, with D szs_rocm_fuzzy_find's unit-cost DP with a free start in the text:
 *      distances[q] = min over j in [0, n] of D[m][j];
 *      ends[q]      = the smallest j that attains it;
 *      starts[q]    = szs_rocm_fuzzy_find_spans' start for that pair (szs_rocm_fuzzy_scan_spans*).
 *  These are exactly the values szs_rocm_fuzzy_find(queries, [text]) / szs_rocm_fuzzy_find_spans return in column 0, bit for bit -
 *  but that call walks the whole text on one lane per query, a serial chain of n columns, and this one fills the device.  The
 *  outputs are vectors of `queries.count` 8-byte cells, no row stride.  `ends` may be NULL; the spans twins require all three.
 *  A query of no bytes gives (0, 0, 0); an empty text gives (m, 0, 0).
 *
 *  HOW, and why it is exact (csrc/hip/myers_fuzzy_scan.hip, csrc/host/fuzzy_scan.c).  The text is cut into
 *  pieces of P bytes; piece p owns columns (p P, min(n, (p + 1) P)].  The lane that takes it walks from s = max(0, p P - 2 m) - a
 *  warm-up of min(p P, 2 m) bytes ahead of its own - follows (best, leftmost end) over every column it walks and reports
 *  (best, s + end); the answer is the lexicographic minimum of (distance, end) over the pieces, by one 64-bit atomic minimum per
 *  (query, 64 pieces).  (1) A DP that starts at s chooses among fewer starts: every value it sees is >= the true D[m][j], no piece
 *  reports too little.  (2) For j - s >= 2 m, or s = 0, the value is exact: the start that attains D[m][j] lies within
 *  m + D[m][j] <= 2 m bytes of j - so the piece that owns the true leftmost best end j* reports exactly (d, j*).  (3) Any other
 *  piece that reports d at a column e has d >= D[m][e] >= d: e is a true best end too, and e >= j*.  Where nothing occurs piece 0
 *  reports (m, 0) and every other piece (m, s > 0).  The starts are szs_rocm_fuzzy_find_spans' reverse pass, unchanged, over at most
 *  m + distance bytes back from `end`.
 *
 *  LIMITS.  (1) `engine` must be a unit-cost BYTE Levenshtein engine, as for szs_rocm_fuzzy_find.  (2) Every query has at most 256
 *  bytes.  (3) The text has less than 4 GiB: the kernels' lengths and ends are 32-bit, as candidates' are.  (4) The text must be
 *  readable by the device (device, pinned or unified memory); the queries likewise.  The outputs may live in device, pinned, unified
 *  or plain host memory (staged densely and copied home).
 *
 *  Refusals, in this order, before any launch and with nothing written: `text_length` >= 2^32 - sz_unexpected_dimensions_k; an engine
 *  that is NULL, blank or not unit-cost byte Levenshtein - sz_status_unknown_k; NULL `queries` - sz_status_unknown_k; zero queries -
 *  success, nothing is looked at; a NULL `distances`, or (the spans twins) a NULL `starts` or `ends` - sz_status_unknown_k; a NULL
 *  `text` with `text_length` > 0, or a text the device cannot read - sz_status_unknown_k; a query of more than 256 bytes -
 *  sz_unexpected_dimensions_k.  Synchronous, also when it fails.
 *
 *  Blocks of at most 2^20 queries; per block the scan, its emit and - with starts - the reverse pass, on the scope's stream.  The
 *  piece: P = ceil(n / (64 x ceil(20480 / rows))), rounded up to a multiple of 64 and at least 4096 - enough wavefronts to fill the
 *  device four times over, and the warm-up of the longest query at most an eighth of a lane's walk.  The `fuzzy_scan_piece` knob
 *  sets P (rounded up to a multiple of 64); like every knob it changes no result.  szs_rocm_last_call_profile: pairs = the queries
 *  of at least one byte (none for an empty text), cells = m x the bytes walked, warm-ups included, plus the reverse windows',
 *  launches = 2 per block (3 with starts; the scan is not launched for an empty text), kernel time = the event pair around them.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_scan(void *engine, szs_device_scope_t device, sz_sequence_t const *queries, void const *text,
                                               sz_size_t text_length, sz_size_t *distances, sz_size_t *ends, char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_scan_u32tape(void *engine, szs_device_scope_t device, sz_sequence_u32tape_t const *queries,
                                                       void const *text, sz_size_t text_length, sz_size_t *distances, sz_size_t *ends,
                                                       char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_scan_u64tape(void *engine, szs_device_scope_t device, sz_sequence_u64tape_t const *queries,
                                                       void const *text, sz_size_t text_length, sz_size_t *distances, sz_size_t *ends,
                                                       char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_scan_spans(void *engine, szs_device_scope_t device, sz_sequence_t const *queries, void const *text,
                                                     sz_size_t text_length, sz_size_t *distances, sz_size_t *starts, sz_size_t *ends,
                                                     char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_scan_spans_u32tape(void *engine, szs_device_scope_t device, sz_sequence_u32tape_t const *queries,
                                                             void const *text, sz_size_t text_length, sz_size_t *distances,
                                                             sz_size_t *starts, sz_size_t *ends, char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_scan_spans_u64tape(void *engine, szs_device_scope_t device, sz_sequence_u64tape_t const *queries,
                                                             void const *text, sz_size_t text_length, sz_size_t *distances,
                                                             sz_size_t *starts, sz_size_t *ends, char const **error_message);

/**
 *  How szs_rocm_fuzzy_scan would cut a text of `text_length` bytes for `queries_count` queries - host only, no GPU: the bytes of a
 *  piece (a multiple of 64), the pieces, the workgroups of the first block's scan = its rows x ceil(pieces / 64), and the bytes a
 *  query of `longest_query` bytes walks: text_length + the sum over the pieces p of min(p x piece, 2 x longest_query).  The
 *  `fuzzy_scan_piece` knob applies as it does to the call.  Outputs are optional.  `longest_query` above 256 or `text_length` >= 2^32:
 *  sz_unexpected_dimensions_k.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_scan_probe(sz_size_t queries_count, sz_size_t longest_query, sz_size_t text_length,
                                                     sz_size_t *piece, sz_size_t *pieces, sz_size_t *workgroups,
                                                     sz_size_t *walked_bytes_per_query);

/**
 *  Fuzzy scan MATCHES: where EVERY occurrence of a pattern lies in one long text, up to `max_distance` errors - fuzzy grep, all
 *  primer sites, every misspelling of a name.  For every query q of m >= 1 bytes and the text of n = `text_length` bytes, with D
 *  szs_rocm_fuzzy_find's unit-cost DP with a free start in the text, a HIT is a column j in [1, n] with D[m][j] <= max_distance
 *  (column 0, the empty match, never is):
 *      counts[q]                = the hits in the whole text - it may exceed `limit`;
 *      ends[q * limit + i]      = the i-th hit in ascending j, for i < min(counts[q], limit): the exclusive byte offset at which the
 *                                 match ends, as szs_rocm_fuzzy_scan reports ends;
 *      distances[q * limit + i] = D[m][j] of that hit;
 *  and every slot from min(counts[q], limit) to limit - 1 of both matrices holds 2^64 - 1, the empty slot (as szs_rocm_rerank's
 *  indices).  `counts` is a vector of `queries.count` 8-byte cells, `distances` and `ends` are dense `queries.count` x `limit`
 *  matrices of 8-byte cells: no strides.  A query of no bytes has count 0 and a row of empty slots; so has any query against an empty
 *  text.  `max_distance` is any sz_size_t: D[m][j] <= m, so a bound of m or more makes every column 1 ... n a hit (the kernels
 *  receive min(max_distance, 256)).  `limit` 0 is the counting form: only `counts` is written, `distances` and `ends` are not looked
 *  at and may be NULL.  `limit` above 2^24 is refused - a choice, not a measurement: one row of outputs is then 256 MiB.
 *
 *  HOW, and why it is exact (csrc/hip/myers_fuzzy_matches.hip, csrc/host/fuzzy_scan_matches.c).  The text
 *  is cut exactly as szs_rocm_fuzzy_scan cuts it: piece p owns columns (p P, min(n, (p + 1) P)] and its lane walks from
 *  s = p P - min(p P, 2 m).  (1) A DP that starts at s chooses among fewer starts: its value L[j] >= D[m][j], no column is reported
 *  that is not a hit.  (2) For an owned column j - s > 2 m or s = 0, and the start that attains D[m][j] lies within
 *  m + D[m][j] <= 2 m bytes of j: L[j] = D[m][j], every hit is reported with its exact distance, by the one piece that owns it.
 *  (3) A lane counts and reports owned columns only; its warm-up belongs to the piece before.  (A warm-up of m, enough for the
 *  minimum of szs_rocm_fuzzy_scan, is NOT enough here.)  Two passes over the same bytes with the same arithmetic: the first counts
 *  the hits per piece, prefix sums turn the counts into slots, the second stores the hits whose slot is below `limit`.  Every cell
 *  has one writer: no allocation depends on the data, and the same call gives the same bytes every time.
 *
 *  LIMITS are szs_rocm_fuzzy_scan's: a unit-cost BYTE Levenshtein engine, queries of at most 256 bytes, a text below 4 GiB that the
 *  device can read.  The outputs may live in device, pinned, unified or plain host memory (staged densely and copied home).
 *
 *  Refusals, in this order, before any launch and with nothing written: `text_length` >= 2^32 - sz_unexpected_dimensions_k;
 *  `limit` > 2^24 - sz_unexpected_dimensions_k; an engine that is NULL, blank or not unit-cost byte Levenshtein - sz_status_unknown_k;
 *  NULL `queries` - sz_status_unknown_k; zero queries - success, nothing is looked at; a NULL `counts` - sz_status_unknown_k; with
 *  `limit` > 0 a NULL `distances` or `ends` - sz_status_unknown_k; a NULL `text` with `text_length` > 0, or a text the device cannot
 *  read - sz_status_unknown_k; a query of more than 256 bytes - sz_unexpected_dimensions_k.  Synchronous, also when it fails.
 *
 *  Blocks of at most 2^20 queries - fewer where a staged block of outputs would pass 128 MiB an array, where rows x chunks of 64
 *  pieces would pass 2^31 - 1 workgroups, or where the block's scratch (65 dwords per row and chunk, in the engine's staging
 *  buffer) would pass 256 MiB; that figure too is a choice.  Per block the count, the offsets and - with `limit` > 0 - two fills and
 *  the write, on the scope's stream.  The piece and the `fuzzy_scan_piece` knob are szs_rocm_fuzzy_scan's, and
 *  szs_rocm_fuzzy_scan_probe reports them.  szs_rocm_last_call_profile: pairs = the queries of at least one byte (none for an empty
 *  text), cells = m x the bytes walked by both passes, warm-ups included, launches = 2 per block with `limit` 0, else 3 (0 for an
 *  empty text), kernel time = the event pair around them.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_scan_matches(void *engine, szs_device_scope_t device, sz_sequence_t const *queries, void const *text,
                                                       sz_size_t text_length, sz_size_t max_distance, sz_size_t limit, sz_size_t *counts,
                                                       sz_size_t *distances, sz_size_t *ends, char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_scan_matches_u32tape(void *engine, szs_device_scope_t device, sz_sequence_u32tape_t const *queries,
                                                               void const *text, sz_size_t text_length, sz_size_t max_distance,
                                                               sz_size_t limit, sz_size_t *counts, sz_size_t *distances, sz_size_t *ends,
                                                               char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_scan_matches_u64tape(void *engine, szs_device_scope_t device, sz_sequence_u64tape_t const *queries,
                                                               void const *text, sz_size_t text_length, sz_size_t max_distance,
                                                               sz_size_t limit, sz_size_t *counts, sz_size_t *distances, sz_size_t *ends,
                                                               char const **error_message);

/**
 *  Fuzzy scan OCCURRENCES: one span per occurrence instead of every end column - what to highlight, what to cut out.  A real
 *  occurrence shows up in szs_rocm_fuzzy_scan_matches as a cluster of adjacent hits j - 1, j, j + 1, ...; this call reports one end
 *  per cluster and where the match that ends there starts.  m, n, D and `max_distance` mean exactly what they mean there (D[m][0] = m).
 *  Column j in [1, n] is an OCCURRENCE END of query q iff all three hold:
 *      (1) D[m][j] <= max_distance;   (2) D[m][j] < D[m][j - 1];   (3) j == n or D[m][j] <= D[m][j + 1]
 *  - the first column of a valley floor of the bottom row, within the bound.  A plateau reports its leftmost column only (the
 *  leftmost-ending convention of szs_rocm_fuzzy_find); a step down that keeps descending is not reported; (2) and (3) look at the
 *  neighbours whether or not those are within the bound.  The spans of different occurrences MAY OVERLAP: a non-overlapping selection
 *  is not promised and is left to the caller.
 *      counts[q]                = the occurrence ends in the whole text - it may exceed `limit`;
 *      ends[q * limit + i]      = the i-th of them in ascending j, for i < min(counts[q], limit);
 *      distances[q * limit + i] = D[m][j] of it;
 *      starts[q * limit + i]    = j - t*, t* the smallest t <= min(j, m + D[m][j]) with lev(query, text[j - t : j]) == D[m][j] - the
 *                                 definition of szs_rocm_fuzzy_find_spans; such a t exists because D[m][j] is the minimum over all
 *                                 starts, and |t - m| <= D[m][j] for any t that attains it;
 *  and every slot from min(counts[q], limit) to limit - 1 of the three matrices holds 2^64 - 1.  Shapes, the empty query, the empty
 *  text, any `max_distance` and the `limit` are szs_rocm_fuzzy_scan_matches'.  `limit` 0 counts only: the matrices are not looked at
 *  and may be NULL.  `starts` may be NULL with any `limit`: no reverse pass is launched.
 *
 *  Three facts (tests/test_fuzzy_scan_occurrences_model.py; tests/test_gpu_fuzzy_scan_occurrences.py).  (a) Every occurrence end is
 *  a hit of szs_rocm_fuzzy_scan_matches for the same bound, with the same distance: (1) is that call's condition.  (b) If the best
 *  distance d* of szs_rocm_fuzzy_scan satisfies d* <= max_distance and d* < m, its (d*, end) is an occurrence, and the leftmost one
 *  of minimum distance: the leftmost global minimum of the bottom row is below everything to its left - D[m][0] = m > d* included, so
 *  it is not column 0 - which is (2), and at most everything to its right, which is (3).  (c) A query that matches nothing better
 *  than m everywhere has no occurrence, even at max_distance >= m: the bottom row never goes below D[m][0] = m and never above it.
 *
 *  HOW (csrc/hip/myers_fuzzy_occurrences.hip, csrc/host/fuzzy_scan_occurrences.c).  The cut, the warm-up of
 *  min(p P, 2 m) bytes and the two passes over a fixed capacity are szs_rocm_fuzzy_scan_matches'.  Proof sketch of the rule under the
 *  cut: a lane whose piece is not the last walks one column behind its last owned column, (p + 1) P + 1, which is exact as owned
 *  columns are (it lies further from the lane's start s); the left neighbour of the first owned column, p P, is 2 m columns into the
 *  walk or s = 0, and the start that attains D[m][p P] lies within m + D <= 2 m bytes of it, at or behind s.  So a lane sees the exact
 *  bottom row on its owned columns and one column to each side, and decides column c - 1 at column c; the lane of the last piece
 *  decides column n behind its walk.  The starts are szs_rocm_fuzzy_find_spans' reverse pass over every filled slot: the reversed
 *  query over at most m + D <= 512 bytes that end at `end`.  No atomics on outputs, one writer a slot, the same bytes every call.
 *
 *  LIMITS, refusals and their order, the memory kinds of the outputs, blocks (also: rows x ceil(limit / 64) within 2^31 - 1
 *  workgroups) and the `fuzzy_scan_piece` knob are szs_rocm_fuzzy_scan_matches'; the messages name this call.
 *  szs_rocm_last_call_profile: pairs as there; cells = m x the bytes walked by every pass that ran - warm-ups, tail columns and the
 *  windows of the reverse pass included; launches = 2 per block with `limit` 0, 3 with a limit and no `starts`, 4 with `starts` (0
 *  for an empty text).
 */
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_scan_occurrences(void *engine, szs_device_scope_t device, sz_sequence_t const *queries,
                                                           void const *text, sz_size_t text_length, sz_size_t max_distance, sz_size_t limit,
                                                           sz_size_t *counts, sz_size_t *distances, sz_size_t *starts, sz_size_t *ends,
                                                           char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_scan_occurrences_u32tape(void *engine, szs_device_scope_t device,
                                                                   sz_sequence_u32tape_t const *queries, void const *text,
                                                                   sz_size_t text_length, sz_size_t max_distance, sz_size_t limit,
                                                                   sz_size_t *counts, sz_size_t *distances, sz_size_t *starts,
                                                                   sz_size_t *ends, char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_fuzzy_scan_occurrences_u64tape(void *engine, szs_device_scope_t device,
                                                                   sz_sequence_u64tape_t const *queries, void const *text,
                                                                   sz_size_t text_length, sz_size_t max_distance, sz_size_t limit,
                                                                   sz_size_t *counts, sz_size_t *distances, sz_size_t *starts,
                                                                   sz_size_t *ends, char const **error_message);

/**
 *  Fingerprint search: consumes the `min_hashes` matrices that `szs_fingerprints_*` produce.  `engine` is a fingerprints engine
 *  - it supplies `dimensions` and owns the device scratch; any other handle is refused and nothing is written.  Hash matrices are
 *  row-major `sz_u32_t` with a row stride in BYTES, a multiple of 4 and at least 4 * dimensions, exactly as `szs_fingerprints_*`
 *  state them (else sz_unexpected_dimensions_k); they may live in device, unified, pinned or plain host memory - what the device
 *  cannot read is staged a block of queries and a tile of candidates at a time, so a corpus larger than device memory is fine.
 *
 *  The comparison is plain equality of the 32-bit hashes: two 0xFFFFFFFF entries (a text shorter than the window) count as equal.
 *  The Jaccard estimate of a pair is its count divided by `dimensions`; the division is left to the caller.
 *
 *  szs_rocm_fingerprint_matches: counts[q * counts_stride (bytes) + c * 4] receives the number of equal dimensions of query q and
 *  candidate c.  `counts_stride` is a multiple of 4, at least 4 * candidates.  `candidate_hashes` NULL: queries x queries, diagonal
 *  included (= dimensions); `candidates_count` is then ignored.  Zero queries or zero candidates: success, nothing written.
 *
 *  szs_rocm_fingerprint_top_k: the k candidates with the MOST equal dimensions per query, without the matrix.  `k`, `row_stride`,
 *  `indices` and `matches` follow szs_rocm_top_k: 1 <= k <= 1024 and row_stride >= k (in 8-byte cells), else
 *  sz_unexpected_dimensions_k; `matches` may be NULL; cells [k, row_stride) are left untouched; equal counts go to the LOWER
 *  candidate index; a row with fewer than k candidates is completed with index SZ_SIZE_MAX and count 0; zero queries: success,
 *  nothing written; zero candidates: every row is completed that way; candidate counts beyond 2^32 are fine.  `candidate_hashes`
 *  NULL: SELF-SEARCH - each query's own index is excluded, identical fingerprints at other indices count.  The `top_k_tile` knob
 *  caps the candidates of a tile here too.
 *
 *  Both calls run on the scope's stream and are synchronous, also when they fail.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_fingerprint_matches(szs_fingerprints_t engine, szs_device_scope_t device,
                                                        sz_u32_t const *query_hashes, sz_size_t query_hashes_stride,
                                                        sz_size_t queries_count, sz_u32_t const *candidate_hashes,
                                                        sz_size_t candidate_hashes_stride, sz_size_t candidates_count,
                                                        sz_u32_t *counts, sz_size_t counts_stride, char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_fingerprint_top_k(szs_fingerprints_t engine, szs_device_scope_t device,
                                                      sz_u32_t const *query_hashes, sz_size_t query_hashes_stride,
                                                      sz_size_t queries_count, sz_u32_t const *candidate_hashes,
                                                      sz_size_t candidate_hashes_stride, sz_size_t candidates_count, sz_size_t k,
                                                      sz_size_t *indices, sz_size_t *matches, sz_size_t row_stride,
                                                      char const **error_message);

/**
 *  The routing of a rerank call over queries of these lengths (bytes) with `k` slots per row, against a candidate side whose
 *  longest string has `longest_candidate` bytes - no GPU involved, and the functions the call itself runs (csrc/host/rerank.c).
 *  `unit_cost`: the engine is unit-cost Levenshtein; `runes`: it counts codepoints.  Outputs (all optional): routes[q] - 0 an engine
 *  call of the row's own, 1 the kernel of csrc/hip/myers_rerank.hip, 2 the strips kernel of csrc/hip/myers_rerank_strips.hip;
 *  strips[q] and strip_words[q] - how many strips the query is walked in and their width in 32-bit words (one strip of the query's
 *  own width on route 1, zeros on route 0; rows that share a wavefront run at the shape of its longest query);
 *  `*scratch_bytes` - the parked deltas the strips launch of these rows would allocate (0: no row takes it).  The `rerank` knob
 *  applies as it does to the call.  k >= 1, else sz_unexpected_dimensions_k.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_rerank_probe(int unit_cost, int runes, sz_u32_t const *query_lengths, sz_size_t queries_count,
                                                 sz_size_t k, sz_size_t longest_candidate, sz_u8_t *routes, sz_u32_t *strips,
                                                 sz_u32_t *strip_words, sz_size_t *scratch_bytes);

/**
 *  Runs the host planner on bare length arrays.  Outputs (all optional):
 *    candidate_order[c]  - candidate indices by ascending length (stable);
 *    query_order[q]      - query indices grouped by kernel variant;
 *    query_variant[q]    - the variant (Myers: 32-bit words rounded to an instantiated kernel; 0 = weighted kernel)
 *                          of the query at planned position q;
 *    cells               - sum of len(q) * len(c) over live pairs.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_plan_probe(int unit_cost, int symmetric, sz_u32_t const *query_lengths,
                                               sz_size_t queries_count, sz_u32_t const *candidate_lengths,
                                               sz_size_t candidates_count, sz_u32_t *candidate_order,
                                               sz_u32_t *query_order, sz_u32_t *query_variant, sz_u64_t *cells);

/**
 *  Runs the planner's tier / orientation decision on bare length arrays (no GPU needed): `*tier` receives 0 (one pair per
 *  lane) or 1 (systolic: one pair per chain of wavefronts), `*transposed` whether the sides are swapped so that the
 *  candidates take the workgroup / band role.  `unit_cost`: the engine is unit-cost Levenshtein (bit-parallel kernels
 *  exist); `uniform`: any Levenshtein engine; `candidate_lengths` is ignored for symmetric calls.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_orientation_probe(int unit_cost, int affine, int uniform, int symmetric,
                                                      sz_u32_t const *query_lengths, sz_size_t queries_count,
                                                      sz_u32_t const *candidate_lengths, sz_size_t candidates_count,
                                                      int *tier, int *transposed);

/**
 *  The same decision for a class-table engine whose DP values fit 16 bits - the calls the team tier (hip/weighted_teams.hip)
 *  may take: `*lanes` receives the lanes per (pair of queries, candidate) the planner deals, 16 or 4, or 0 for the
 *  one-pair-per-lane kernel (also when `*tier` is not 0).
 */
SZ_API_RUNTIME sz_status_t szs_rocm_team_orientation_probe(int affine, int symmetric, sz_u32_t const *query_lengths,
                                                           sz_size_t queries_count, sz_u32_t const *candidate_lengths,
                                                           sz_size_t candidates_count, int *tier, int *transposed, sz_u32_t *lanes);

/**
 *  The launches of a unit-cost Levenshtein call over queries of these lengths (bytes, or runes with `runes` != 0) against
 *  `candidates_count` candidates, in the order they leave the host - longest pair first, the short launch last
 *  (DESIGN.md section 4.1): per launch the width group's variant (8: the short kernel; 10 ... 64 words; 0: longer queries),
 *  the words of the kernel that takes it and the lanes per pair (0: one).  `*launches` receives the number of groups; at
 *  most `capacity` entries are written.  No GPU involved.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_launch_order_probe(int runes, sz_u32_t const *query_lengths, sz_size_t queries_count,
                                                       sz_size_t candidates_count, sz_u32_t *variants, sz_u32_t *words, sz_u32_t *lanes,
                                                       sz_size_t capacity, sz_size_t *launches);

/**
 *  The work queue of the ONE persistent launch that scores every bit-vector width of a unit-cost byte call
 *  (hip/myers_queue.hip; host/plan.c: szs_plan_queue), planned from bare length arrays - no GPU involved.  Queries are taken
 *  longest first, candidates shortest first (szs_rocm_plan_probe gives both orders).  `alphabet` 0: byte strings; A: lengths
 *  count codepoints of a batch renumbered 1 ... A (hip/utf8.hip), whose tables have A + 1 rows - `*items_total` 0 when such an
 *  alphabet leaves some query no table (the per-width launches score those calls).  `tiles` receives 10 values per tile, in
 *  queue order: items of all tiles before it, first query and queries of its slice, first and one-past-last candidate of its
 *  column, candidates per work item, words per lane (0: the query's own width on one lane), lanes per pair, queries per
 *  work item G and flags (1: sparse tables).  With `groups` = ceil(queries / G), work item j of a tile scores the queries of group `j % groups` against the
 *  candidates of block `j / groups`, blocks cut from the column's end.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_queue_probe(int symmetric, sz_u32_t alphabet, sz_u32_t const *query_lengths, sz_size_t queries_count,
                                                sz_u32_t const *candidate_lengths, sz_size_t candidates_count, sz_u32_t *tiles,
                                                sz_size_t capacity, sz_size_t *tiles_count, sz_u64_t *items_total);

/* ---- one cross-product over the N GPUs of a host (csrc/host/node.c) ------------------------------
 *
 *  The reference's C-ABI is one device per call (stringzillas.h:137) and has no multi-GPU path; what its threading rules
 *  allow - N scopes and N engines on N host threads - is packaged here: query ROWS are dealt to the GPUs by LPT on their
 *  lengths, both tapes are replicated to every GPU once per call (peer-to-peer over xGMI when they live on a GPU), one host
 *  thread per GPU runs the ordinary single-GPU engine on `its rows x all candidates`, and every result row is copied to its
 *  place in the caller's matrix.  Scores are bit-identical to the single-GPU engines': they ARE the single-GPU engines.
 */
#define SZS_ROCM_NODE_MOST_GPUS 16

typedef void *szs_rocm_node_t;        /* a set of GPUs of this host */
typedef void *szs_rocm_node_engine_t; /* one cost model, instantiated on every GPU of a node */

typedef struct szs_rocm_node_stats_t {
    sz_size_t gpus;
    double wall_milliseconds;                             /* the whole call */
    double busy_milliseconds[SZS_ROCM_NODE_MOST_GPUS];    /* per GPU: replication + scoring + placing its rows */
    double kernel_milliseconds[SZS_ROCM_NODE_MOST_GPUS];  /* per GPU: the scoring kernels alone (hipEvent pair) */
    sz_u64_t cells[SZS_ROCM_NODE_MOST_GPUS];              /* per GPU: DP cells scored */
    sz_u64_t row_weights[SZS_ROCM_NODE_MOST_GPUS];        /* per GPU: sum of (len(query) + 1) over its rows - what LPT balances */
    sz_u32_t rows[SZS_ROCM_NODE_MOST_GPUS];               /* per GPU: query rows dealt to it */
    sz_u32_t peer_copies[SZS_ROCM_NODE_MOST_GPUS];        /* per GPU: tape replicas that came straight from another GPU's memory (peer access over xGMI) */
    sz_u32_t staged_copies[SZS_ROCM_NODE_MOST_GPUS];      /* per GPU: replicas staged through pinned host memory (no peer access to the source GPU), or from host memory */
    sz_u32_t peer_pairs;                                  /* ordered pairs of the node's GPUs with peer access enabled (szs_rocm_node_init) */
    sz_u32_t symmetric;                                   /* 1: the call sharded the lower triangle (bands of rows) and mirrored it */
} szs_rocm_node_stats_t;

/** `gpu_devices` NULL or `count` 0: every visible GPU.  `*node` receives the handle. */
SZ_API_RUNTIME sz_status_t szs_rocm_node_init(sz_size_t const *gpu_devices, sz_size_t count, szs_rocm_node_t *node,
                                              char const **error_message);
SZ_API_RUNTIME sz_size_t szs_rocm_node_size(szs_rocm_node_t node);
/** Engines created from the node keep it alive until they are freed themselves.  The handle must not be used after this call:
 *  a second free is recognised (and ignored) only while such engines still exist - afterwards the memory is gone. */
SZ_API_RUNTIME void szs_rocm_node_free(szs_rocm_node_t node);

/** Engines of a node: same arguments and meaning as `szs_*_init` (stringzillas.h), `*engine` must be NULL on entry. */
SZ_API_RUNTIME sz_status_t szs_rocm_node_levenshtein_distances_init(szs_rocm_node_t node, sz_error_cost_t match,
                                                                    sz_error_cost_t mismatch, sz_error_cost_t open,
                                                                    sz_error_cost_t extend, szs_rocm_node_engine_t *engine,
                                                                    char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_node_levenshtein_distances_utf8_init(szs_rocm_node_t node, sz_error_cost_t match,
                                                                         sz_error_cost_t mismatch, sz_error_cost_t open,
                                                                         sz_error_cost_t extend, szs_rocm_node_engine_t *engine,
                                                                         char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_node_needleman_wunsch_scores_init(szs_rocm_node_t node, sz_u8_t const *byte_to_class,
                                                                      sz_error_cost_t const *class_substitution_costs,
                                                                      sz_error_cost_t open, sz_error_cost_t extend,
                                                                      szs_rocm_node_engine_t *engine, char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_node_smith_waterman_scores_init(szs_rocm_node_t node, sz_u8_t const *byte_to_class,
                                                                    sz_error_cost_t const *class_substitution_costs,
                                                                    sz_error_cost_t open, sz_error_cost_t extend,
                                                                    szs_rocm_node_engine_t *engine, char const **error_message);
SZ_API_RUNTIME void szs_rocm_node_engine_free(szs_rocm_node_engine_t engine);

/**
 *  Scores all `queries x candidates` into `results[q * stride + c]`, 8-byte cells.  `candidates` NULL: queries against themselves
 *  - the lower triangle is scored ONCE, in bands of rows of equal weight (szs_rocm_shard_triangle), and mirrored, as the
 *  single-GPU engines do (serial.hpp:3169-3182).  8-byte
 *  cells (`sz_size_t` distances / `sz_ssize_t` scores).  Tapes may live in host, pinned, unified or any GPU's memory;
 *  so may `results`.  Synchronous.  `stats` (optional) receives the per-GPU timing the multi-GPU configs ask to report.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_node_scores_u32tape(szs_rocm_node_engine_t engine, sz_sequence_u32tape_t const *queries,
                                                        sz_sequence_u32tape_t const *candidates, void *results,
                                                        sz_size_t results_row_stride, szs_rocm_node_stats_t *stats,
                                                        char const **error_message);
SZ_API_RUNTIME sz_status_t szs_rocm_node_scores_u64tape(szs_rocm_node_engine_t engine, sz_sequence_u64tape_t const *queries,
                                                        sz_sequence_u64tape_t const *candidates, void *results,
                                                        sz_size_t results_row_stride, szs_rocm_node_stats_t *stats,
                                                        char const **error_message);

/**
 *  Tuning / testing knobs (csrc/host/tuning.c).  The library reads the `SZS_ROCM_*` environment variables ONCE, when it
 *  is loaded; afterwards a knob changes only through this call.  `knob` is one of "tier" (lanes | systolic | chain),
 *  "swap" (0 | 1), "packed" (0), "rune_ids" (n), "chain_waves" (4 | 8 | 16), "trace" (0 | 1), "cells" (64),
 *  "planner" (host | device), "speculate" (0), "streams" (0: one stream), "reuse" (0: never re-use a plan),
 *  "split" (0 | 2 | 4 | 8: lanes per pair of the bit-parallel widths of 16 words and more), "alphabet" (0 | 1: never / always renumber the runes
 *  of a codepoint batch on the device), "merge" (n: candidate blocks per workgroup of the short bit-parallel kernels),
 *  "team" (0: never | lanes * 10000 + registers * 100 + waves: that shape of the team tier of the 16-bit weighted scorers),
 *  "queue" (0: never | 1: every unit-cost byte call - the one persistent launch of hip/myers_queue.hip; automatic: calls of two or
 *  more bit-vector widths whose lengths are skewed), "queue_words" (4 | 8 | 12 | 16: the most words of a pattern one lane holds
 *  there), "queue_rounds" (n: candidates per work item in rounds of eight wavefronts), "queue_priority" (0 | 1: wave priorities by
 *  chain length inside that launch; automatic: byte calls and short codepoint calls), "fused" (0: never plan a short unit-cost
 *  call inside its own scoring launch), "tiny" (0: never | 1: every unit-cost byte call of strings up to 255 bytes of which
 *  few are beyond 16 - the tiny-token launch of hip/myers_tiny.hip | 2: the same, and blocks full of longer strings are scored there
 *  too, slowly, instead of refused (testing); automatic: batches of tiny tokens on both sides),
 *  "top_k_tile" (n: the most candidates per scored tile of a top-k call),
 *  "rerank" (0: every row of a rerank call as an engine call of its own | 1: rows whose query has at most 256 bytes in one launch of
 *  hip/myers_rerank.hip, longer rows as engine calls; automatic: those, and rows whose query has at most 64 KiB in one launch of
 *  hip/myers_rerank_strips.hip),
 *  "fuzzy_search_segment" (n: the candidates one workgroup of hip/myers_fuzzy_tile.hip scores for its row in a fuzzy search, rounded
 *  up to a multiple of 64; automatic: enough workgroups to fill the device four times over),
 *  "fuzzy_scan_piece" (n: the bytes of the text one lane of hip/myers_fuzzy_scan.hip owns in a fuzzy scan, rounded up to a multiple
 *  of 64; automatic: enough wavefronts to fill the device four times over, at least 4096 bytes),
 *  "align_trace_kib" (n: the KiB of trace memory an alignments call may hold, at least one workgroup's region; 0 or automatic:
 *  256 MiB),
 *  "queues" (see below), "roctx" (1: the host phases of every call - plan, decide, enqueue, wait - as roctx ranges for a
 *  `rocprofv3 --marker-trace` timeline; the marker library is looked up at run time, never linked),
 *  "cpu_requests" (strict | gpu: serve capability
 *  masks without the GPU bit and CPU device scopes with the GPU engines on device 0 instead of refusing them) - or its
 *  environment spelling ("SZS_ROCM_TIER" ...); `value` NULL, "" or "auto" restores the automatic choice.  No knob changes a
 *  result: they pick among kernels that compute the same scores.
 *
 *  "queues" (n): hardware queues the process has.  The launches of a mixed-length batch fan out over at most that many
 *  streams; the HIP runtime gives a process GPU_MAX_HW_QUEUES of them, 4 by default, fixed when HIP initialises.  The library
 *  never writes the environment: it reads GPU_MAX_HW_QUEUES once, when it is loaded, and an application that wants the wide
 *  fan-out (a latency-bound share of a batch: 2.0 ms on twelve queues, 3.0 on four) exports GPU_MAX_HW_QUEUES=12
 *  itself before its first HIP call.  `szs_rocm_call_profile_t.streams` says what a call really used.
 */
SZ_API_RUNTIME sz_status_t szs_rocm_tuning_set(char const *knob, char const *value);

/** The `team` shapes this build holds (lanes * 10000 + registers * 100 + wavefronts per SIMD), 0 past the last one. */
SZ_API_RUNTIME sz_u32_t szs_rocm_team_shape(sz_size_t index);

#ifdef __cplusplus
}
#endif
#endif /* STRINGZILLAS_ROCM_H_ */
