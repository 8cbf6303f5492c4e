/*
 *  engines.c - the `extern "C"` engine entry points: init / call (sequence, u32tape, u64tape) / free for the four
 *  similarity families and for the fingerprint engines, and the ROCm profile accessor.
 *
 *  ROCm counterpart of c/stringzillas/{levenshtein,needleman_wunsch,smith_waterman,fingerprints}.cuh.
 *  The capability ladder of the reference (levenshtein.cuh:107-200) collapses to one rung here: this build ships
 *  GPU engines only, so `capabilities` must contain sz_cap_cuda_k.
 */
#include "szs_internal.h"
#include "../hip/pair_rule.h"
#include "../hip/corner_cut.h"

#include <stdlib.h>
#include <string.h>

void szs_engine_release(szs_engine_s *engine); /* dispatch.c */

static unsigned magnitude_of(int value) { return (unsigned)(value < 0 ? -value : value); }

static sz_status_t engine_new(szs_family_t family, sz_capability_t capabilities, void **out, szs_engine_s **created,
                              char const **error_message) {
    if (!out) return szs_report(sz_status_unknown_k, error_message, "Engine must not be null");
    if (*out) return szs_report(sz_status_unknown_k, error_message, "Engine must be uninitialized");
    /* Strict by default; with the `cpu_requests` knob set to "gpu" a mask without the GPU bit is served by the only engines
     * this build has (host/tuning.c) - the results are the same numbers, computed on the GPU. */
    if ((capabilities & sz_cap_cuda_k) == 0 && szs_tuning_get(szs_knob_cpu_requests_k) != 1)
        return szs_report(sz_missing_gpu_k, error_message,
                          "The ROCm build ships GPU engines only: request sz_cap_cuda_k (e.g. from a GPU device scope)");
    if ((szs_capabilities() & sz_cap_cuda_k) == 0) return szs_report(sz_missing_gpu_k, error_message, NULL);
    szs_engine_s *engine = (szs_engine_s *)calloc(1, sizeof(szs_engine_s));
    if (!engine) return szs_report(sz_bad_alloc_k, error_message, NULL);
    engine->magic = SZS_ENGINE_MAGIC;
    engine->family = family;
    engine->device = -1, engine->events_device = -1, engine->model_uploaded_device = -1, engine->aux_device = -1;
    *created = engine;
    *out = engine;
    return szs_report(sz_success_k, error_message, NULL);
}

static void engine_free(void *handle) {
    szs_engine_s *engine = (szs_engine_s *)handle;
    if (!engine || engine->magic != SZS_ENGINE_MAGIC) return;
    szs_engine_release(engine);
    engine->magic = 0;
    free(engine);
}

static sz_status_t levenshtein_init(szs_family_t family, sz_error_cost_t match, sz_error_cost_t mismatch,
                                    sz_error_cost_t open, sz_error_cost_t extend, sz_capability_t capabilities,
                                    void **out, char const **error_message) {
    szs_engine_s *engine = NULL;
    sz_status_t const status = engine_new(family, capabilities, out, &engine, error_message);
    if (status != sz_success_k) return status;
    engine->match = match, engine->mismatch = mismatch, engine->open = open, engine->extend = extend;
    engine->is_linear = open == extend;                                               /* levenshtein.cuh:117 */
    engine->is_unit_cost = match == 0 && mismatch == 1 && open == 1 && extend == 1;   /* serial.hpp:118-120 */
    unsigned magnitude = magnitude_of(match);
    if (magnitude_of(mismatch) > magnitude) magnitude = magnitude_of(mismatch);
    if (magnitude_of(open) > magnitude) magnitude = magnitude_of(open);
    if (magnitude_of(extend) > magnitude) magnitude = magnitude_of(extend);
    engine->magnitude = magnitude;
    return sz_success_k;
}

static sz_status_t scores_init(szs_family_t family, sz_u8_t const *byte_to_class, sz_error_cost_t const *class_costs,
                               sz_error_cost_t open, sz_error_cost_t extend, sz_capability_t capabilities, void **out,
                               char const **error_message) {
    if (!byte_to_class || !class_costs)
        return szs_report(sz_status_unknown_k, error_message, "Substitution tables must not be null");
    szs_engine_s *engine = NULL;
    sz_status_t const status = engine_new(family, capabilities, out, &engine, error_message);
    if (status != sz_success_k) return status;
    memcpy(engine->byte_to_class, byte_to_class, 256); /* needleman_wunsch.cuh:99-118: both tables are copied */
    memcpy(engine->class_costs, class_costs, 32 * 32);
    for (int i = 0; i < 256; ++i) engine->byte_to_class[i] &= 31; /* a class is one of 32 */
    engine->open = open, engine->extend = extend;
    engine->is_linear = open == extend;
    unsigned magnitude = magnitude_of(open) > magnitude_of(extend) ? magnitude_of(open) : magnitude_of(extend);
    for (int i = 0; i < 32 * 32; ++i)
        if (magnitude_of(class_costs[i]) > magnitude) magnitude = magnitude_of(class_costs[i]);
    engine->magnitude = magnitude;
    return sz_success_k;
}

static szs_input_t input_from_sequence(sz_sequence_t const *sequence) {
    szs_input_t input = {szs_input_sequence_k, sequence->count, NULL, NULL, sequence};
    return input;
}
static szs_input_t input_from_u32tape(sz_sequence_u32tape_t const *tape) {
    szs_input_t input = {szs_input_u32tape_k, tape->count, tape->data, tape->offsets, NULL};
    return input;
}
static szs_input_t input_from_u64tape(sz_sequence_u64tape_t const *tape) {
    szs_input_t input = {szs_input_u64tape_k, tape->count, tape->data, tape->offsets, NULL};
    return input;
}

#define SZS_CROSS_BODY(MAKE_INPUT)                                                                                     \
    if (!queries) return szs_report(sz_status_unknown_k, error_message, "Queries must not be null");                   \
    szs_input_t const query_input = MAKE_INPUT(queries);                                                               \
    szs_input_t candidate_input;                                                                                       \
    if (candidates) candidate_input = MAKE_INPUT(candidates);                                                          \
    return szs_engine_cross((szs_engine_s *)engine, (szs_scope_s *)device, &query_input,                               \
                            candidates ? &candidate_input : NULL, results, results_row_stride, error_message);

/* ---- Levenshtein, bytes (stringzillas.h:197-254) -------------------------------------------------------------------- */

sz_status_t szs_levenshtein_distances_init(sz_error_cost_t match, sz_error_cost_t mismatch, sz_error_cost_t open,
                                           sz_error_cost_t extend, sz_memory_allocator_t const *alloc,
                                           sz_capability_t capabilities, szs_levenshtein_distances_t *engine,
                                           char const **error_message) {
    (void)alloc; /* accepted and ignored, as in the reference (levenshtein.cuh:112) */
    return levenshtein_init(szs_family_levenshtein_k, match, mismatch, open, extend, capabilities, engine, error_message);
}
sz_status_t szs_levenshtein_distances(szs_levenshtein_distances_t engine, szs_device_scope_t device,
                                      sz_sequence_t const *queries, sz_sequence_t const *candidates, sz_size_t *results,
                                      sz_size_t results_row_stride, char const **error_message) {
    SZS_CROSS_BODY(input_from_sequence)
}
sz_status_t szs_levenshtein_distances_u32tape(szs_levenshtein_distances_t engine, szs_device_scope_t device,
                                              sz_sequence_u32tape_t const *queries,
                                              sz_sequence_u32tape_t const *candidates, sz_size_t *results,
                                              sz_size_t results_row_stride, char const **error_message) {
    SZS_CROSS_BODY(input_from_u32tape)
}
sz_status_t szs_levenshtein_distances_u64tape(szs_levenshtein_distances_t engine, szs_device_scope_t device,
                                              sz_sequence_u64tape_t const *queries,
                                              sz_sequence_u64tape_t const *candidates, sz_size_t *results,
                                              sz_size_t results_row_stride, char const **error_message) {
    SZS_CROSS_BODY(input_from_u64tape)
}
void szs_levenshtein_distances_free(szs_levenshtein_distances_t engine) { engine_free(engine); }

/* ---- Levenshtein, UTF-8 codepoints (stringzillas.h:271-328) - a "next" row of SURVEY.md section 8f ----------------- */

sz_status_t szs_levenshtein_distances_utf8_init(sz_error_cost_t match, sz_error_cost_t mismatch, sz_error_cost_t open,
                                                sz_error_cost_t extend, sz_memory_allocator_t const *alloc,
                                                sz_capability_t capabilities, szs_levenshtein_distances_utf8_t *engine,
                                                char const **error_message) {
    (void)alloc;
    return levenshtein_init(szs_family_levenshtein_utf8_k, match, mismatch, open, extend, capabilities, engine,
                            error_message);
}
sz_status_t szs_levenshtein_distances_utf8(szs_levenshtein_distances_utf8_t engine, szs_device_scope_t device,
                                           sz_sequence_t const *queries, sz_sequence_t const *candidates,
                                           sz_size_t *results, sz_size_t results_row_stride,
                                           char const **error_message) {
    SZS_CROSS_BODY(input_from_sequence)
}
sz_status_t szs_levenshtein_distances_utf8_u32tape(szs_levenshtein_distances_utf8_t engine, szs_device_scope_t device,
                                                   sz_sequence_u32tape_t const *queries,
                                                   sz_sequence_u32tape_t const *candidates, sz_size_t *results,
                                                   sz_size_t results_row_stride, char const **error_message) {
    SZS_CROSS_BODY(input_from_u32tape)
}
sz_status_t szs_levenshtein_distances_utf8_u64tape(szs_levenshtein_distances_utf8_t engine, szs_device_scope_t device,
                                                   sz_sequence_u64tape_t const *queries,
                                                   sz_sequence_u64tape_t const *candidates, sz_size_t *results,
                                                   sz_size_t results_row_stride, char const **error_message) {
    SZS_CROSS_BODY(input_from_u64tape)
}
void szs_levenshtein_distances_utf8_free(szs_levenshtein_distances_utf8_t engine) { engine_free(engine); }

/* ---- Needleman-Wunsch (stringzillas.h:355-413) ----------------------------------------------------------------------- */

sz_status_t szs_needleman_wunsch_scores_init(sz_u8_t const *byte_to_class, sz_error_cost_t const *class_substitution_costs,
                                             sz_error_cost_t open, sz_error_cost_t extend,
                                             sz_memory_allocator_t const *alloc, sz_capability_t capabilities,
                                             szs_needleman_wunsch_scores_t *engine, char const **error_message) {
    (void)alloc;
    return scores_init(szs_family_needleman_wunsch_k, byte_to_class, class_substitution_costs, open, extend,
                       capabilities, engine, error_message);
}
sz_status_t szs_needleman_wunsch_scores(szs_needleman_wunsch_scores_t engine, szs_device_scope_t device,
                                        sz_sequence_t const *queries, sz_sequence_t const *candidates,
                                        sz_ssize_t *results, sz_size_t results_row_stride, char const **error_message) {
    SZS_CROSS_BODY(input_from_sequence)
}
sz_status_t szs_needleman_wunsch_scores_u32tape(szs_needleman_wunsch_scores_t engine, szs_device_scope_t device,
                                                sz_sequence_u32tape_t const *queries,
                                                sz_sequence_u32tape_t const *candidates, sz_ssize_t *results,
                                                sz_size_t results_row_stride, char const **error_message) {
    SZS_CROSS_BODY(input_from_u32tape)
}
sz_status_t szs_needleman_wunsch_scores_u64tape(szs_needleman_wunsch_scores_t engine, szs_device_scope_t device,
                                                sz_sequence_u64tape_t const *queries,
                                                sz_sequence_u64tape_t const *candidates, sz_ssize_t *results,
                                                sz_size_t results_row_stride, char const **error_message) {
    SZS_CROSS_BODY(input_from_u64tape)
}
void szs_needleman_wunsch_scores_free(szs_needleman_wunsch_scores_t engine) { engine_free(engine); }

/* ---- Smith-Waterman (stringzillas.h:430-488) ------------------------------------------------------------------------- */

sz_status_t szs_smith_waterman_scores_init(sz_u8_t const *byte_to_class, sz_error_cost_t const *class_substitution_costs,
                                           sz_error_cost_t open, sz_error_cost_t extend,
                                           sz_memory_allocator_t const *alloc, sz_capability_t capabilities,
                                           szs_smith_waterman_scores_t *engine, char const **error_message) {
    (void)alloc;
    return scores_init(szs_family_smith_waterman_k, byte_to_class, class_substitution_costs, open, extend, capabilities,
                       engine, error_message);
}
sz_status_t szs_smith_waterman_scores(szs_smith_waterman_scores_t engine, szs_device_scope_t device,
                                      sz_sequence_t const *queries, sz_sequence_t const *candidates, sz_ssize_t *results,
                                      sz_size_t results_row_stride, char const **error_message) {
    SZS_CROSS_BODY(input_from_sequence)
}
sz_status_t szs_smith_waterman_scores_u32tape(szs_smith_waterman_scores_t engine, szs_device_scope_t device,
                                              sz_sequence_u32tape_t const *queries,
                                              sz_sequence_u32tape_t const *candidates, sz_ssize_t *results,
                                              sz_size_t results_row_stride, char const **error_message) {
    SZS_CROSS_BODY(input_from_u32tape)
}
sz_status_t szs_smith_waterman_scores_u64tape(szs_smith_waterman_scores_t engine, szs_device_scope_t device,
                                              sz_sequence_u64tape_t const *queries,
                                              sz_sequence_u64tape_t const *candidates, sz_ssize_t *results,
                                              sz_size_t results_row_stride, char const **error_message) {
    SZS_CROSS_BODY(input_from_u64tape)
}
void szs_smith_waterman_scores_free(szs_smith_waterman_scores_t engine) { engine_free(engine); }

/* ---- fingerprints (stringzillas.h:532-596): host/fingerprint_engines.c + hip/fingerprints.hip -------------------------------- */

sz_status_t szs_fingerprints_init(sz_size_t dimensions, sz_size_t alphabet_size, sz_size_t const *window_widths,
                                  sz_size_t window_widths_count, sz_u64_t seed, sz_memory_allocator_t const *alloc,
                                  sz_capability_t capabilities, szs_fingerprints_t *engine, char const **error_message) {
    (void)alloc; /* accepted and ignored, as in the reference (fingerprints.cuh:38) */
    return szs_fingerprints_create(dimensions, alphabet_size, window_widths, window_widths_count, seed, capabilities, engine,
                                   error_message);
}
sz_status_t szs_fingerprints_sequence(szs_fingerprints_t engine, szs_device_scope_t device, sz_sequence_t const *texts,
                                      sz_u32_t *min_hashes, sz_size_t min_hashes_stride, sz_u32_t *min_counts,
                                      sz_size_t min_counts_stride, char const **error_message) {
    if (!texts) return szs_report(sz_status_unknown_k, error_message, "Input texts cannot be null");
    szs_input_t const input = input_from_sequence(texts);
    return szs_fingerprints_call((szs_fingerprints_s *)engine, (szs_scope_s *)device, &input, min_hashes, min_hashes_stride,
                                 min_counts, min_counts_stride, error_message);
}
sz_status_t szs_fingerprints_u64tape(szs_fingerprints_t engine, szs_device_scope_t device,
                                     sz_sequence_u64tape_t const *texts, sz_u32_t *min_hashes,
                                     sz_size_t min_hashes_stride, sz_u32_t *min_counts, sz_size_t min_counts_stride,
                                     char const **error_message) {
    if (!texts) return szs_report(sz_status_unknown_k, error_message, "Input texts cannot be null");
    szs_input_t const input = input_from_u64tape(texts);
    return szs_fingerprints_call((szs_fingerprints_s *)engine, (szs_scope_s *)device, &input, min_hashes, min_hashes_stride,
                                 min_counts, min_counts_stride, error_message);
}
sz_status_t szs_fingerprints_u32tape(szs_fingerprints_t engine, szs_device_scope_t device,
                                     sz_sequence_u32tape_t const *texts, sz_u32_t *min_hashes,
                                     sz_size_t min_hashes_stride, sz_u32_t *min_counts, sz_size_t min_counts_stride,
                                     char const **error_message) {
    if (!texts) return szs_report(sz_status_unknown_k, error_message, "Input texts cannot be null");
    szs_input_t const input = input_from_u32tape(texts);
    return szs_fingerprints_call((szs_fingerprints_s *)engine, (szs_scope_s *)device, &input, min_hashes, min_hashes_stride,
                                 min_counts, min_counts_stride, error_message);
}
void szs_fingerprints_free(szs_fingerprints_t engine) { szs_fingerprints_destroy((szs_fingerprints_s *)engine); }

/* ---- ROCm extension --------------------------------------------------------------------------------------------------- */

sz_status_t szs_rocm_last_call_profile(void *handle, szs_rocm_call_profile_t *profile) {
    szs_engine_s *engine = (szs_engine_s *)handle;
    if (!engine || engine->magic != SZS_ENGINE_MAGIC || !profile) return sz_status_unknown_k;
    *profile = engine->last_profile;
    return sz_success_k;
}

sz_u32_t szs_rocm_last_pairing(void *handle) {
    szs_engine_s const *engine = (szs_engine_s const *)handle;
    return engine && engine->magic == SZS_ENGINE_MAGIC ? engine->last_pairing : 0u;
}

static int descending_lengths(void const *a, void const *b) {
    sz_u32_t const x = *(sz_u32_t const *)a, y = *(sz_u32_t const *)b;
    return x < y ? 1 : x > y ? -1 : 0;
}

/* The choice of fused_sort_side (hip/lev_myers.hip) on bare lengths, through the same header. */
sz_status_t szs_rocm_pair_rule_probe(sz_u32_t const *lengths, sz_size_t count, sz_u32_t *rule, sz_u64_t *total_words, sz_u32_t *slot_pairs_out) {
    if (!rule || (count && !lengths) || count > 0x7FFFFFFFull) return sz_status_unknown_k;
    unsigned const queries = (unsigned)count, slots = szs_pair_slots(queries), seconds = szs_pair_seconds(queries);
    if (*rule != SZS_ROCM_PAIR_RULE_CHOOSE && *rule > seconds) return sz_unexpected_dimensions_k;
    sz_u32_t *const ranked = (sz_u32_t *)malloc((count ? count : 1) * sizeof(sz_u32_t));
    if (!ranked) return sz_bad_alloc_k;
    int blank = 0; /* a query beyond the short kernel: the sorter writes every length as 0 and the host plans the call another way */
    for (unsigned i = 0; i < queries; ++i) ranked[i] = lengths[i], blank |= lengths[i] > 32u * SZS_MYERS_SHORT_WORDS;
    if (blank) memset(ranked, 0, count * sizeof(sz_u32_t));
    qsort(ranked, count, sizeof(sz_u32_t), descending_lengths);
    sz_u64_t alone = 0; /* the middle query of an odd count: the same under every rule */
    for (unsigned slot = seconds; slot < slots; ++slot) alone += szs_pair_words_alone(ranked[slot]);
    unsigned chosen = *rule == SZS_ROCM_PAIR_RULE_CHOOSE ? 0u : *rule;
    sz_u64_t fewest = 0;
    for (unsigned k = 0; k < (*rule == SZS_ROCM_PAIR_RULE_CHOOSE ? SZS_PAIR_RULE_CANDIDATES : 1u); ++k) {
        unsigned const candidate = *rule == SZS_ROCM_PAIR_RULE_CHOOSE ? szs_pair_rule_candidate(k, seconds) : *rule;
        if (k && (!seconds || queries > SZS_FUSED_MOST_STRINGS)) break; /* larger sides are not staged in LDS: rule 0 */
        sz_u64_t words = alone;
        for (unsigned slot = 0; slot < seconds; ++slot)
            words += szs_pair_slot_words(ranked[slot], ranked[szs_pair_second_rank(candidate, slot, slots, seconds)]);
        if (!k || words < fewest) fewest = words, chosen = candidate;
    }
    *rule = chosen;
    if (total_words) *total_words = fewest;
    if (slot_pairs_out)
        for (unsigned slot = 0; slot < slots; ++slot)
            slot_pairs_out[2 * slot] = slot,
                               slot_pairs_out[2 * slot + 1] = slot < seconds ? szs_pair_second_rank(chosen, slot, slots, seconds) : 0xFFFFFFFFu;
    free(ranked);
    return sz_success_k;
}

/* The phase bounds of myers_workgroup (hip/lev_myers.hip) on bare lengths, through the same header. */
sz_status_t szs_rocm_corner_cut_probe(sz_u32_t first_length, sz_u32_t second_length, sz_u32_t words, sz_u32_t n_short, sz_u32_t n_long,
                                      sz_u32_t *head_until, sz_u32_t *late_from) {
    int const paired = second_length != SZS_ROCM_NO_SECOND_QUERY;
    if (!head_until || !late_from || n_short > n_long) return sz_status_unknown_k;
    if ((sz_u64_t)first_length + (paired ? (sz_u64_t)second_length + 2u : 0u) > 32ull * words) return sz_unexpected_dimensions_k;
    unsigned head = 0, late = 0;
    szs_corner_cut(first_length, paired ? second_length : 0u, paired, words, n_short, n_long, &head, &late);
    *head_until = head, *late_from = late;
    return sz_success_k;
}

/* ---- top-k (host/top_k.c) --------------------------------------------------------------------------------------------- */

#define SZS_TOP_K_BODY(MAKE_INPUT)                                                                                     \
    if (k < 1 || k > SZS_TOP_K_MOST || row_stride < k || !queries)                                                     \
        return szs_engine_top_k((szs_engine_s *)engine, (szs_scope_s *)device, NULL, NULL, k, indices, scores,         \
                                row_stride, error_message);                                                            \
    szs_input_t const query_input = MAKE_INPUT(queries);                                                               \
    szs_input_t candidate_input;                                                                                       \
    if (candidates) candidate_input = MAKE_INPUT(candidates);                                                          \
    return szs_engine_top_k((szs_engine_s *)engine, (szs_scope_s *)device, &query_input,                               \
                            candidates ? &candidate_input : NULL, k, indices, scores, row_stride, error_message);

sz_status_t szs_rocm_top_k(void *engine, szs_device_scope_t device, sz_sequence_t const *queries, sz_sequence_t const *candidates,
                           sz_size_t k, sz_size_t *indices, void *scores, sz_size_t row_stride, char const **error_message) {
    SZS_TOP_K_BODY(input_from_sequence)
}
sz_status_t szs_rocm_top_k_u32tape(void *engine, szs_device_scope_t device, sz_sequence_u32tape_t const *queries,
                                   sz_sequence_u32tape_t const *candidates, sz_size_t k, sz_size_t *indices, void *scores,
                                   sz_size_t row_stride, char const **error_message) {
    SZS_TOP_K_BODY(input_from_u32tape)
}
sz_status_t szs_rocm_top_k_u64tape(void *engine, szs_device_scope_t device, sz_sequence_u64tape_t const *queries,
                                   sz_sequence_u64tape_t const *candidates, sz_size_t k, sz_size_t *indices, void *scores,
                                   sz_size_t row_stride, char const **error_message) {
    SZS_TOP_K_BODY(input_from_u64tape)
}

/* ---- within (host/within.c) ------------------------------------------------------------------------------------------- */

#define SZS_WITHIN_BODY(MAKE_INPUT)                                                                                    \
    if (limit > SZS_WITHIN_MOST || row_stride < limit || !queries)                                                     \
        return szs_engine_within((szs_engine_s *)engine, (szs_scope_s *)device, NULL, NULL, bound, limit, counts,      \
                                 indices, scores, row_stride, error_message);                                          \
    szs_input_t const query_input = MAKE_INPUT(queries);                                                               \
    szs_input_t candidate_input;                                                                                       \
    if (candidates) candidate_input = MAKE_INPUT(candidates);                                                          \
    return szs_engine_within((szs_engine_s *)engine, (szs_scope_s *)device, &query_input,                              \
                             candidates ? &candidate_input : NULL, bound, limit, counts, indices, scores, row_stride,  \
                             error_message);

sz_status_t szs_rocm_within(void *engine, szs_device_scope_t device, sz_sequence_t const *queries, sz_sequence_t const *candidates,
                            sz_ssize_t bound, sz_size_t limit, sz_size_t *counts, sz_size_t *indices, void *scores, sz_size_t row_stride,
                            char const **error_message) {
    SZS_WITHIN_BODY(input_from_sequence)
}
sz_status_t szs_rocm_within_u32tape(void *engine, szs_device_scope_t device, sz_sequence_u32tape_t const *queries,
                                    sz_sequence_u32tape_t const *candidates, sz_ssize_t bound, sz_size_t limit, sz_size_t *counts,
                                    sz_size_t *indices, void *scores, sz_size_t row_stride, char const **error_message) {
    SZS_WITHIN_BODY(input_from_u32tape)
}
sz_status_t szs_rocm_within_u64tape(void *engine, szs_device_scope_t device, sz_sequence_u64tape_t const *queries,
                                    sz_sequence_u64tape_t const *candidates, sz_ssize_t bound, sz_size_t limit, sz_size_t *counts,
                                    sz_size_t *indices, void *scores, sz_size_t row_stride, char const **error_message) {
    SZS_WITHIN_BODY(input_from_u64tape)
}

/* ---- clusters (host/clusters.c) --------------------------------------------------------------------------------------- */

#define SZS_CLUSTERS_BODY(MAKE_INPUT)                                                                                  \
    szs_input_t input;                                                                                                 \
    if (strings) input = MAKE_INPUT(strings);                                                                          \
    return szs_engine_clusters((szs_engine_s *)engine, (szs_scope_s *)device, strings ? &input : NULL, bound, labels,  \
                               clusters_count, error_message);

sz_status_t szs_rocm_clusters(void *engine, szs_device_scope_t device, sz_sequence_t const *strings, sz_ssize_t bound, sz_size_t *labels,
                              sz_size_t *clusters_count, char const **error_message) {
    SZS_CLUSTERS_BODY(input_from_sequence)
}
sz_status_t szs_rocm_clusters_u32tape(void *engine, szs_device_scope_t device, sz_sequence_u32tape_t const *strings, sz_ssize_t bound,
                                      sz_size_t *labels, sz_size_t *clusters_count, char const **error_message) {
    SZS_CLUSTERS_BODY(input_from_u32tape)
}
sz_status_t szs_rocm_clusters_u64tape(void *engine, szs_device_scope_t device, sz_sequence_u64tape_t const *strings, sz_ssize_t bound,
                                      sz_size_t *labels, sz_size_t *clusters_count, char const **error_message) {
    SZS_CLUSTERS_BODY(input_from_u64tape)
}

/* ---- rerank (host/rerank.c) ------------------------------------------------------------------------------------------- */

#define SZS_RERANK_BODY(MAKE_INPUT)                                                                                    \
    if (k < 1 || row_stride < k || !queries)                                                                           \
        return szs_engine_rerank((szs_engine_s *)engine, (szs_scope_s *)device, NULL, NULL, indices, k, scores,        \
                                 row_stride, error_message);                                                           \
    szs_input_t const query_input = MAKE_INPUT(queries);                                                               \
    szs_input_t candidate_input;                                                                                       \
    if (candidates) candidate_input = MAKE_INPUT(candidates);                                                          \
    return szs_engine_rerank((szs_engine_s *)engine, (szs_scope_s *)device, &query_input,                              \
                             candidates ? &candidate_input : NULL, indices, k, scores, row_stride, error_message);

sz_status_t szs_rocm_rerank(void *engine, szs_device_scope_t device, sz_sequence_t const *queries, sz_sequence_t const *candidates,
                            sz_size_t const *indices, sz_size_t k, void *scores, sz_size_t row_stride, char const **error_message) {
    SZS_RERANK_BODY(input_from_sequence)
}
sz_status_t szs_rocm_rerank_u32tape(void *engine, szs_device_scope_t device, sz_sequence_u32tape_t const *queries,
                                    sz_sequence_u32tape_t const *candidates, sz_size_t const *indices, sz_size_t k, void *scores,
                                    sz_size_t row_stride, char const **error_message) {
    SZS_RERANK_BODY(input_from_u32tape)
}
sz_status_t szs_rocm_rerank_u64tape(void *engine, szs_device_scope_t device, sz_sequence_u64tape_t const *queries,
                                    sz_sequence_u64tape_t const *candidates, sz_size_t const *indices, sz_size_t k, void *scores,
                                    sz_size_t row_stride, char const **error_message) {
    SZS_RERANK_BODY(input_from_u64tape)
}

/* ---- fuzzy find (host/fuzzy_find.c) ----------------------------------------------------------------------------------- */

#define SZS_FUZZY_FIND_BODY(MAKE_INPUT)                                                                                \
    if (k < 1 || row_stride < k || !queries)                                                                           \
        return szs_engine_fuzzy_find((szs_engine_s *)engine, (szs_scope_s *)device, NULL, NULL, indices, k, distances, \
                                     ends, row_stride, error_message);                                                 \
    szs_input_t const query_input = MAKE_INPUT(queries);                                                               \
    szs_input_t candidate_input;                                                                                       \
    if (candidates) candidate_input = MAKE_INPUT(candidates);                                                          \
    return szs_engine_fuzzy_find((szs_engine_s *)engine, (szs_scope_s *)device, &query_input,                          \
                                 candidates ? &candidate_input : NULL, indices, k, distances, ends, row_stride,        \
                                 error_message);

sz_status_t szs_rocm_fuzzy_find(void *engine, szs_device_scope_t device, sz_sequence_t const *queries, sz_sequence_t const *candidates,
                                sz_size_t const *indices, sz_size_t k, sz_size_t *distances, sz_size_t *ends, sz_size_t row_stride,
                                char const **error_message) {
    SZS_FUZZY_FIND_BODY(input_from_sequence)
}
sz_status_t szs_rocm_fuzzy_find_u32tape(void *engine, szs_device_scope_t device, sz_sequence_u32tape_t const *queries,
                                        sz_sequence_u32tape_t const *candidates, sz_size_t const *indices, sz_size_t k,
                                        sz_size_t *distances, sz_size_t *ends, sz_size_t row_stride, char const **error_message) {
    SZS_FUZZY_FIND_BODY(input_from_u32tape)
}
sz_status_t szs_rocm_fuzzy_find_u64tape(void *engine, szs_device_scope_t device, sz_sequence_u64tape_t const *queries,
                                        sz_sequence_u64tape_t const *candidates, sz_size_t const *indices, sz_size_t k,
                                        sz_size_t *distances, sz_size_t *ends, sz_size_t row_stride, char const **error_message) {
    SZS_FUZZY_FIND_BODY(input_from_u64tape)
}

#define SZS_FUZZY_FIND_SPANS_BODY(MAKE_INPUT)                                                                                \
    if (k < 1 || row_stride < k || !queries)                                                                                 \
        return szs_engine_fuzzy_find_spans((szs_engine_s *)engine, (szs_scope_s *)device, NULL, NULL, indices, k, distances, \
                                           starts, ends, row_stride, error_message);                                         \
    szs_input_t const query_input = MAKE_INPUT(queries);                                                                     \
    szs_input_t candidate_input;                                                                                             \
    if (candidates) candidate_input = MAKE_INPUT(candidates);                                                                \
    return szs_engine_fuzzy_find_spans((szs_engine_s *)engine, (szs_scope_s *)device, &query_input,                          \
                                       candidates ? &candidate_input : NULL, indices, k, distances, starts, ends,            \
                                       row_stride, error_message);

sz_status_t szs_rocm_fuzzy_find_spans(void *engine, szs_device_scope_t device, sz_sequence_t const *queries,
                                      sz_sequence_t const *candidates, sz_size_t const *indices, sz_size_t k, sz_size_t *distances,
                                      sz_size_t *starts, sz_size_t *ends, sz_size_t row_stride, char const **error_message) {
    SZS_FUZZY_FIND_SPANS_BODY(input_from_sequence)
}
sz_status_t szs_rocm_fuzzy_find_spans_u32tape(void *engine, szs_device_scope_t device, sz_sequence_u32tape_t const *queries,
                                              sz_sequence_u32tape_t const *candidates, sz_size_t const *indices, sz_size_t k,
                                              sz_size_t *distances, sz_size_t *starts, sz_size_t *ends, sz_size_t row_stride,
                                              char const **error_message) {
    SZS_FUZZY_FIND_SPANS_BODY(input_from_u32tape)
}
sz_status_t szs_rocm_fuzzy_find_spans_u64tape(void *engine, szs_device_scope_t device, sz_sequence_u64tape_t const *queries,
                                              sz_sequence_u64tape_t const *candidates, sz_size_t const *indices, sz_size_t k,
                                              sz_size_t *distances, sz_size_t *starts, sz_size_t *ends, sz_size_t row_stride,
                                              char const **error_message) {
    SZS_FUZZY_FIND_SPANS_BODY(input_from_u64tape)
}

/* ---- alignments (host/alignments.c) ----------------------------------------------------------------------------------- */

#define SZS_ALIGNMENTS_BODY(MAKE_INPUT)                                                                                \
    if (k < 1 || row_stride < k || !queries)                                                                           \
        return szs_engine_alignments((szs_engine_s *)engine, (szs_scope_s *)device, NULL, NULL, indices, k, starts,    \
                                     ends, distances, lengths, ops, capacity, row_stride, error_message);              \
    szs_input_t const query_input = MAKE_INPUT(queries);                                                               \
    szs_input_t candidate_input;                                                                                       \
    if (candidates) candidate_input = MAKE_INPUT(candidates);                                                          \
    return szs_engine_alignments((szs_engine_s *)engine, (szs_scope_s *)device, &query_input,                          \
                                 candidates ? &candidate_input : NULL, indices, k, starts, ends, distances, lengths,   \
                                 ops, capacity, row_stride, error_message);

sz_status_t szs_rocm_alignments(void *engine, szs_device_scope_t device, sz_sequence_t const *queries, sz_sequence_t const *candidates,
                                sz_size_t const *indices, sz_size_t k, sz_size_t const *starts, sz_size_t const *ends, sz_size_t *distances,
                                sz_size_t *lengths, sz_u8_t *ops, sz_size_t capacity, sz_size_t row_stride, char const **error_message) {
    SZS_ALIGNMENTS_BODY(input_from_sequence)
}
sz_status_t szs_rocm_alignments_u32tape(void *engine, szs_device_scope_t device, sz_sequence_u32tape_t const *queries,
                                        sz_sequence_u32tape_t const *candidates, sz_size_t const *indices, sz_size_t k,
                                        sz_size_t const *starts, sz_size_t const *ends, sz_size_t *distances, sz_size_t *lengths,
                                        sz_u8_t *ops, sz_size_t capacity, sz_size_t row_stride, char const **error_message) {
    SZS_ALIGNMENTS_BODY(input_from_u32tape)
}
sz_status_t szs_rocm_alignments_u64tape(void *engine, szs_device_scope_t device, sz_sequence_u64tape_t const *queries,
                                        sz_sequence_u64tape_t const *candidates, sz_size_t const *indices, sz_size_t k,
                                        sz_size_t const *starts, sz_size_t const *ends, sz_size_t *distances, sz_size_t *lengths,
                                        sz_u8_t *ops, sz_size_t capacity, sz_size_t row_stride, char const **error_message) {
    SZS_ALIGNMENTS_BODY(input_from_u64tape)
}

/* ---- fuzzy search (host/fuzzy_search.c) ------------------------------------------------------------------------------- */

#define SZS_FUZZY_SEARCH_BODY(MAKE_INPUT)                                                                              \
    if (k < 1 || k > SZS_TOP_K_MOST || row_stride < k || !queries)                                                     \
        return szs_engine_fuzzy_search((szs_engine_s *)engine, (szs_scope_s *)device, NULL, NULL, k, indices,          \
                                       distances, starts, ends, row_stride, error_message);                            \
    szs_input_t const query_input = MAKE_INPUT(queries);                                                               \
    szs_input_t candidate_input;                                                                                       \
    if (candidates) candidate_input = MAKE_INPUT(candidates);                                                          \
    return szs_engine_fuzzy_search((szs_engine_s *)engine, (szs_scope_s *)device, &query_input,                        \
                                   candidates ? &candidate_input : NULL, k, indices, distances, starts, ends,          \
                                   row_stride, error_message);

sz_status_t szs_rocm_fuzzy_search(void *engine, szs_device_scope_t device, sz_sequence_t const *queries, sz_sequence_t const *candidates,
                                  sz_size_t k, sz_size_t *indices, sz_size_t *distances, sz_size_t *starts, sz_size_t *ends,
                                  sz_size_t row_stride, char const **error_message) {
    SZS_FUZZY_SEARCH_BODY(input_from_sequence)
}
sz_status_t szs_rocm_fuzzy_search_u32tape(void *engine, szs_device_scope_t device, sz_sequence_u32tape_t const *queries,
                                          sz_sequence_u32tape_t const *candidates, sz_size_t k, sz_size_t *indices, sz_size_t *distances,
                                          sz_size_t *starts, sz_size_t *ends, sz_size_t row_stride, char const **error_message) {
    SZS_FUZZY_SEARCH_BODY(input_from_u32tape)
}
sz_status_t szs_rocm_fuzzy_search_u64tape(void *engine, szs_device_scope_t device, sz_sequence_u64tape_t const *queries,
                                          sz_sequence_u64tape_t const *candidates, sz_size_t k, sz_size_t *indices, sz_size_t *distances,
                                          sz_size_t *starts, sz_size_t *ends, sz_size_t row_stride, char const **error_message) {
    SZS_FUZZY_SEARCH_BODY(input_from_u64tape)
}

#define SZS_FUZZY_SEARCH_WITHIN_BODY(MAKE_INPUT)                                                                       \
    if (limit > SZS_WITHIN_MOST || row_stride < limit || !queries)                                                     \
        return szs_engine_fuzzy_search_within((szs_engine_s *)engine, (szs_scope_s *)device, NULL, NULL, max_distance, \
                                              limit, counts, indices, distances, starts, ends, row_stride,             \
                                              error_message);                                                          \
    szs_input_t const query_input = MAKE_INPUT(queries);                                                               \
    szs_input_t candidate_input;                                                                                       \
    if (candidates) candidate_input = MAKE_INPUT(candidates);                                                          \
    return szs_engine_fuzzy_search_within((szs_engine_s *)engine, (szs_scope_s *)device, &query_input,                 \
                                          candidates ? &candidate_input : NULL, max_distance, limit, counts, indices,  \
                                          distances, starts, ends, row_stride, error_message);

sz_status_t szs_rocm_fuzzy_search_within(void *engine, szs_device_scope_t device, sz_sequence_t const *queries,
                                         sz_sequence_t const *candidates, sz_size_t max_distance, sz_size_t limit, sz_size_t *counts,
                                         sz_size_t *indices, sz_size_t *distances, sz_size_t *starts, sz_size_t *ends,
                                         sz_size_t row_stride, char const **error_message) {
    SZS_FUZZY_SEARCH_WITHIN_BODY(input_from_sequence)
}
sz_status_t szs_rocm_fuzzy_search_within_u32tape(void *engine, szs_device_scope_t device, sz_sequence_u32tape_t const *queries,
                                                 sz_sequence_u32tape_t const *candidates, sz_size_t max_distance, sz_size_t limit,
                                                 sz_size_t *counts, sz_size_t *indices, sz_size_t *distances, sz_size_t *starts,
                                                 sz_size_t *ends, sz_size_t row_stride, char const **error_message) {
    SZS_FUZZY_SEARCH_WITHIN_BODY(input_from_u32tape)
}
sz_status_t szs_rocm_fuzzy_search_within_u64tape(void *engine, szs_device_scope_t device, sz_sequence_u64tape_t const *queries,
                                                 sz_sequence_u64tape_t const *candidates, sz_size_t max_distance, sz_size_t limit,
                                                 sz_size_t *counts, sz_size_t *indices, sz_size_t *distances, sz_size_t *starts,
                                                 sz_size_t *ends, sz_size_t row_stride, char const **error_message) {
    SZS_FUZZY_SEARCH_WITHIN_BODY(input_from_u64tape)
}

/* ---- fuzzy scan (host/fuzzy_scan.c) ----------------------------------------------------------------------------------- */

#define SZS_FUZZY_SCAN_BODY(MAKE_INPUT)                                                                                \
    szs_input_t query_input;                                                                                           \
    if (queries) query_input = MAKE_INPUT(queries);                                                                    \
    return szs_engine_fuzzy_scan((szs_engine_s *)engine, (szs_scope_s *)device, queries ? &query_input : NULL, text,   \
                                 text_length, distances, ends, error_message);

sz_status_t szs_rocm_fuzzy_scan(void *engine, szs_device_scope_t device, sz_sequence_t const *queries, void const *text,
                                sz_size_t text_length, sz_size_t *distances, sz_size_t *ends, char const **error_message) {
    SZS_FUZZY_SCAN_BODY(input_from_sequence)
}
sz_status_t szs_rocm_fuzzy_scan_u32tape(void *engine, szs_device_scope_t device, sz_sequence_u32tape_t const *queries, void const *text,
                                        sz_size_t text_length, sz_size_t *distances, sz_size_t *ends, char const **error_message) {
    SZS_FUZZY_SCAN_BODY(input_from_u32tape)
}
sz_status_t szs_rocm_fuzzy_scan_u64tape(void *engine, szs_device_scope_t device, sz_sequence_u64tape_t const *queries, void const *text,
                                        sz_size_t text_length, sz_size_t *distances, sz_size_t *ends, char const **error_message) {
    SZS_FUZZY_SCAN_BODY(input_from_u64tape)
}

#define SZS_FUZZY_SCAN_SPANS_BODY(MAKE_INPUT)                                                                                \
    szs_input_t query_input;                                                                                                 \
    if (queries) query_input = MAKE_INPUT(queries);                                                                          \
    return szs_engine_fuzzy_scan_spans((szs_engine_s *)engine, (szs_scope_s *)device, queries ? &query_input : NULL, text,   \
                                       text_length, distances, starts, ends, error_message);

sz_status_t szs_rocm_fuzzy_scan_spans(void *engine, szs_device_scope_t device, sz_sequence_t const *queries, void const *text,
                                      sz_size_t text_length, sz_size_t *distances, sz_size_t *starts, sz_size_t *ends,
                                      char const **error_message) {
    SZS_FUZZY_SCAN_SPANS_BODY(input_from_sequence)
}
sz_status_t szs_rocm_fuzzy_scan_spans_u32tape(void *engine, szs_device_scope_t device, sz_sequence_u32tape_t const *queries,
                                              void const *text, sz_size_t text_length, sz_size_t *distances, sz_size_t *starts,
                                              sz_size_t *ends, char const **error_message) {
    SZS_FUZZY_SCAN_SPANS_BODY(input_from_u32tape)
}
sz_status_t szs_rocm_fuzzy_scan_spans_u64tape(void *engine, szs_device_scope_t device, sz_sequence_u64tape_t const *queries,
                                              void const *text, sz_size_t text_length, sz_size_t *distances, sz_size_t *starts,
                                              sz_size_t *ends, char const **error_message) {
    SZS_FUZZY_SCAN_SPANS_BODY(input_from_u64tape)
}

/* ---- fuzzy scan matches (host/fuzzy_scan_matches.c) ------------------------------------------------------------------- */

#define SZS_FUZZY_SCAN_MATCHES_BODY(MAKE_INPUT)                                                                                \
    szs_input_t query_input;                                                                                                   \
    if (queries) query_input = MAKE_INPUT(queries);                                                                            \
    return szs_engine_fuzzy_scan_matches((szs_engine_s *)engine, (szs_scope_s *)device, queries ? &query_input : NULL, text,   \
                                         text_length, max_distance, limit, counts, distances, ends, error_message);

sz_status_t szs_rocm_fuzzy_scan_matches(void *engine, szs_device_scope_t device, sz_sequence_t const *queries, void const *text,
                                        sz_size_t text_length, sz_size_t max_distance, sz_size_t limit, sz_size_t *counts,
                                        sz_size_t *distances, sz_size_t *ends, char const **error_message) {
    SZS_FUZZY_SCAN_MATCHES_BODY(input_from_sequence)
}
sz_status_t szs_rocm_fuzzy_scan_matches_u32tape(void *engine, szs_device_scope_t device, sz_sequence_u32tape_t const *queries,
                                                void const *text, sz_size_t text_length, sz_size_t max_distance, sz_size_t limit,
                                                sz_size_t *counts, sz_size_t *distances, sz_size_t *ends, char const **error_message) {
    SZS_FUZZY_SCAN_MATCHES_BODY(input_from_u32tape)
}
sz_status_t szs_rocm_fuzzy_scan_matches_u64tape(void *engine, szs_device_scope_t device, sz_sequence_u64tape_t const *queries,
                                                void const *text, sz_size_t text_length, sz_size_t max_distance, sz_size_t limit,
                                                sz_size_t *counts, sz_size_t *distances, sz_size_t *ends, char const **error_message) {
    SZS_FUZZY_SCAN_MATCHES_BODY(input_from_u64tape)
}

/* ---- fuzzy scan occurrences (host/fuzzy_scan_matches.c) ----------------------------------------------------------- */

#define SZS_FUZZY_SCAN_OCCURRENCES_BODY(MAKE_INPUT)                                                                                \
    szs_input_t query_input;                                                                                                       \
    if (queries) query_input = MAKE_INPUT(queries);                                                                                \
    return szs_engine_fuzzy_scan_occurrences((szs_engine_s *)engine, (szs_scope_s *)device, queries ? &query_input : NULL, text,   \
                                             text_length, max_distance, limit, counts, distances, starts, ends, error_message);

sz_status_t szs_rocm_fuzzy_scan_occurrences(void *engine, szs_device_scope_t device, sz_sequence_t const *queries, void const *text,
                                            sz_size_t text_length, sz_size_t max_distance, sz_size_t limit, sz_size_t *counts,
                                            sz_size_t *distances, sz_size_t *starts, sz_size_t *ends, char const **error_message) {
    SZS_FUZZY_SCAN_OCCURRENCES_BODY(input_from_sequence)
}
sz_status_t szs_rocm_fuzzy_scan_occurrences_u32tape(void *engine, szs_device_scope_t device, sz_sequence_u32tape_t const *queries,
                                                    void const *text, sz_size_t text_length, sz_size_t max_distance, sz_size_t limit,
                                                    sz_size_t *counts, sz_size_t *distances, sz_size_t *starts, sz_size_t *ends,
                                                    char const **error_message) {
    SZS_FUZZY_SCAN_OCCURRENCES_BODY(input_from_u32tape)
}
sz_status_t szs_rocm_fuzzy_scan_occurrences_u64tape(void *engine, szs_device_scope_t device, sz_sequence_u64tape_t const *queries,
                                                    void const *text, sz_size_t text_length, sz_size_t max_distance, sz_size_t limit,
                                                    sz_size_t *counts, sz_size_t *distances, sz_size_t *starts, sz_size_t *ends,
                                                    char const **error_message) {
    SZS_FUZZY_SCAN_OCCURRENCES_BODY(input_from_u64tape)
}

/* ---- fingerprint search (host/fingerprint_search.c) ------------------------------------------------------------------- */

sz_status_t szs_rocm_fingerprint_matches(szs_fingerprints_t engine, szs_device_scope_t device, sz_u32_t const *query_hashes,
                                         sz_size_t query_hashes_stride, sz_size_t queries_count, sz_u32_t const *candidate_hashes,
                                         sz_size_t candidate_hashes_stride, sz_size_t candidates_count, sz_u32_t *counts,
                                         sz_size_t counts_stride, char const **error_message) {
    return szs_fingerprints_matches((szs_fingerprints_s *)engine, (szs_scope_s *)device, query_hashes, query_hashes_stride, queries_count,
                                    candidate_hashes, candidate_hashes_stride, candidates_count, counts, counts_stride, error_message);
}
sz_status_t szs_rocm_fingerprint_top_k(szs_fingerprints_t engine, szs_device_scope_t device, sz_u32_t const *query_hashes,
                                       sz_size_t query_hashes_stride, sz_size_t queries_count, sz_u32_t const *candidate_hashes,
                                       sz_size_t candidate_hashes_stride, sz_size_t candidates_count, sz_size_t k, sz_size_t *indices,
                                       sz_size_t *matches, sz_size_t row_stride, char const **error_message) {
    return szs_fingerprints_top_k((szs_fingerprints_s *)engine, (szs_scope_s *)device, query_hashes, query_hashes_stride, queries_count,
                                  candidate_hashes, candidate_hashes_stride, candidates_count, k, indices, matches, row_stride,
                                  error_message);
}
sz_status_t szs_rocm_fingerprint_clusters(void *engine, szs_device_scope_t device, sz_u32_t const *hashes, sz_size_t hashes_stride,
                                          sz_size_t count, sz_size_t min_matches, sz_size_t *labels, sz_size_t *clusters_count,
                                          char const **error_message) {
    return szs_fingerprints_clusters((szs_fingerprints_s *)engine, (szs_scope_s *)device, hashes, hashes_stride, count, min_matches, labels,
                                     clusters_count, error_message);
}
