/*
 *  fuzzy_scan_occurrences_args_probe - the argument paths of szs_rocm_fuzzy_scan_occurrences* (csrc/host/fuzzy_scan_occurrences.c) that
 *  end before a GPU is needed, from a C program of its own, against the header's prototypes: tests/test_fuzzy_scan_occurrences_host.py
 *  builds and runs it, and linked against a host built with -DSTRINGZILLAS_ROCM_SANITIZE=ON it lets AddressSanitizer and
 *  UndefinedBehaviorSanitizer watch the same paths on any machine.  Exit status 0 and "fuzzy_scan_occurrences_args_probe: ok" when
 *  every call answered as the header says: the refusals in its order, nothing written.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../stringzilla_amd/csrc/host/szs_internal.h"

#define UNTOUCHED 0x5A5A5A5A5A5A5A5Aull
#define LIMIT 3

static int failures = 0;

static void expect(int condition, char const *what, int line) {
    if (condition) return;
    fprintf(stderr, "fuzzy_scan_occurrences_args_probe: line %d: %s\n", line, what);
    ++failures;
}
#define EXPECT(condition) expect((condition), #condition, __LINE__)

static char const bytes[] = "abcabd";
static sz_u32_t const offsets32[] = {0, 3, 6};
static sz_u64_t const offsets64[] = {0, 3, 6};

static sz_cptr_t member_start(void const *handle, sz_sorted_idx_t i) { return (void)handle, bytes + offsets32[i]; }
static sz_size_t member_length(void const *handle, sz_sorted_idx_t i) { return (void)handle, offsets32[i + 1] - offsets32[i]; }

/** One call of entry `form` (0: sz_sequence_t, 1: u32tape, 2: u64tape) over `count` of the two strings; `count` < 0: NULL queries. */
static sz_status_t call(int form, void *engine, int count, void const *text, sz_size_t text_length, sz_size_t max_distance, sz_size_t limit,
                        sz_size_t *counts, sz_size_t *distances, sz_size_t *starts, sz_size_t *ends, char const **message) {
    *message = NULL;
    sz_sequence_t sequence;
    memset(&sequence, 0, sizeof(sequence));
    sequence.count = count < 0 ? 0 : (sz_size_t)count, sequence.get_start = member_start, sequence.get_length = member_length;
    sz_sequence_u32tape_t tape32 = {bytes, offsets32, sequence.count};
    sz_sequence_u64tape_t tape64 = {bytes, offsets64, sequence.count};
    int const null_queries = count < 0;
    switch (form) {
    case 0:
        return szs_rocm_fuzzy_scan_occurrences(engine, NULL, null_queries ? NULL : &sequence, text, text_length, max_distance, limit, counts,
                                               distances, starts, ends, message);
    case 1:
        return szs_rocm_fuzzy_scan_occurrences_u32tape(engine, NULL, null_queries ? NULL : &tape32, text, text_length, max_distance, limit,
                                                       counts, distances, starts, ends, message);
    default:
        return szs_rocm_fuzzy_scan_occurrences_u64tape(engine, NULL, null_queries ? NULL : &tape64, text, text_length, max_distance, limit,
                                                       counts, distances, starts, ends, message);
    }
}

static int untouched(sz_size_t const *cells, size_t count) {
    for (size_t i = 0; i < count; ++i)
        if (cells[i] != UNTOUCHED) return 0;
    return 1;
}

int main(void) {
    /* memory that passes for an engine up to the point where a GPU would be needed */
    szs_engine_s *unit = (szs_engine_s *)calloc(1, sizeof(szs_engine_s)), *weighted = (szs_engine_s *)calloc(1, sizeof(szs_engine_s));
    szs_engine_s *blank = (szs_engine_s *)calloc(1, sizeof(szs_engine_s)), *runes = (szs_engine_s *)calloc(1, sizeof(szs_engine_s));
    szs_engine_s *global = (szs_engine_s *)calloc(1, sizeof(szs_engine_s)), *local = (szs_engine_s *)calloc(1, sizeof(szs_engine_s));
    if (!unit || !weighted || !blank || !runes || !global || !local) return 2;
    unit->magic = weighted->magic = runes->magic = global->magic = local->magic = SZS_ENGINE_MAGIC;
    unit->family = weighted->family = szs_family_levenshtein_k, runes->family = szs_family_levenshtein_utf8_k;
    global->family = szs_family_needleman_wunsch_k, local->family = szs_family_smith_waterman_k;
    unit->is_unit_cost = runes->is_unit_cost = global->is_unit_cost = local->is_unit_cost = 1, weighted->is_unit_cost = 0;
    static char const text[] = "xxabcxx";
    sz_size_t const four_gib = (sz_size_t)1 << 32, most = (sz_size_t)1 << 24;

    for (int form = 0; form < 3; ++form) {
        sz_size_t counts[2], distances[2 * LIMIT], starts[2 * LIMIT], ends[2 * LIMIT];
        char const *message = NULL;
        for (size_t i = 0; i < 2; ++i) counts[i] = UNTOUCHED;
        for (size_t i = 0; i < 2 * LIMIT; ++i) distances[i] = starts[i] = ends[i] = UNTOUCHED;

        /* 1: the text's length, before the limit and the engine are looked at */
        EXPECT(call(form, NULL, 2, NULL, four_gib, 1, most + 1, counts, distances, starts, ends, &message) == sz_unexpected_dimensions_k &&
               message && strstr(message, "4 GiB"));
        EXPECT(call(form, unit, 0, NULL, four_gib, 1, LIMIT, NULL, NULL, NULL, NULL, &message) == sz_unexpected_dimensions_k);
        /* 2: the limit, before the engine */
        EXPECT(call(form, NULL, 2, text, 7, 1, most + 1, counts, distances, starts, ends, &message) == sz_unexpected_dimensions_k && message &&
               strstr(message, "2^24"));
        EXPECT(call(form, unit, 0, text, 7, 1, ~(sz_size_t)0, NULL, NULL, NULL, NULL, &message) == sz_unexpected_dimensions_k);
        EXPECT(call(form, NULL, 2, text, 7, 1, most, counts, distances, starts, ends, &message) == sz_status_unknown_k); /* 2^24: the engine */
        /* 3: the engine, before the queries */
        void *const refused[] = {NULL, blank, weighted, runes, global, local};
        for (size_t e = 0; e < sizeof(refused) / sizeof(refused[0]); ++e) {
            EXPECT(call(form, refused[e], 2, text, 7, 1, LIMIT, counts, distances, starts, ends, &message) == sz_status_unknown_k && message);
            EXPECT(call(form, refused[e], 0, text, 7, 1, LIMIT, counts, distances, starts, ends, &message) == sz_status_unknown_k && message);
            EXPECT(call(form, refused[e], -1, text, 7, 1, LIMIT, counts, distances, starts, ends, &message) == sz_status_unknown_k && message &&
                   strstr(message, "engine"));
        }
        /* 4, 5: NULL queries; zero queries succeed with every pointer NULL */
        EXPECT(call(form, unit, -1, text, 7, 1, LIMIT, NULL, NULL, NULL, NULL, &message) == sz_status_unknown_k && message &&
               strstr(message, "Queries"));
        EXPECT(call(form, unit, 0, NULL, 7, 1, LIMIT, NULL, NULL, NULL, NULL, &message) == sz_success_k);
        EXPECT(call(form, unit, 0, text, 7, 1, LIMIT, counts, distances, starts, ends, &message) == sz_success_k);
        /* 6: the counts, before the matrices and the text */
        EXPECT(call(form, unit, 2, NULL, 7, 1, LIMIT, NULL, NULL, NULL, NULL, &message) == sz_status_unknown_k && message &&
               strstr(message, "Counts"));
        EXPECT(call(form, unit, 2, NULL, 7, 1, 0, NULL, NULL, NULL, NULL, &message) == sz_status_unknown_k && message && strstr(message, "Counts"));
        /* 7: with a limit, distances and ends - before the text; the starts are optional */
        EXPECT(call(form, unit, 2, NULL, 7, 1, LIMIT, counts, NULL, starts, ends, &message) == sz_status_unknown_k && message &&
               strstr(message, "Distances and ends"));
        EXPECT(call(form, unit, 2, NULL, 7, 1, LIMIT, counts, distances, starts, NULL, &message) == sz_status_unknown_k && message &&
               strstr(message, "Distances and ends"));
        /* 8: a NULL text of 7 bytes - with and without starts; the counting form passes the outputs' check with NULL matrices */
        EXPECT(call(form, unit, 2, NULL, 7, 1, LIMIT, counts, distances, starts, ends, &message) == sz_status_unknown_k && message &&
               strstr(message, "Text"));
        EXPECT(call(form, unit, 2, NULL, 7, 1, LIMIT, counts, distances, NULL, ends, &message) == sz_status_unknown_k && message &&
               strstr(message, "Text"));
        EXPECT(call(form, unit, 2, NULL, 7, 1, 0, counts, NULL, NULL, NULL, &message) == sz_status_unknown_k && message && strstr(message, "Text"));
        EXPECT(call(form, unit, 2, NULL, 7, ~(sz_size_t)0, 0, counts, NULL, NULL, NULL, &message) == sz_status_unknown_k && message &&
               strstr(message, "Text")); /* any bound is taken */
        EXPECT(untouched(counts, 2) && untouched(distances, 2 * LIMIT) && untouched(starts, 2 * LIMIT) && untouched(ends, 2 * LIMIT));
    }

    free(unit), free(weighted), free(blank), free(runes), free(global), free(local);
    if (failures) return 1;
    puts("fuzzy_scan_occurrences_args_probe: ok");
    return 0;
}
