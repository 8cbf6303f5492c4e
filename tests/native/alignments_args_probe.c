/*
 *  alignments_args_probe - the argument paths of szs_rocm_alignments* (csrc/host/alignments.c) that end before a GPU is needed, from
 *  a C program of its own, against the header's prototypes: tests/test_alignments_host.py builds and runs it, and built against the
 *  sanitized host it lets AddressSanitizer and UndefinedBehaviorSanitizer watch them on any machine -
 *      make -C stringzilla_amd/csrc asan && make -C tests/native bin/alignments_args_probe_asan && tests/native/bin/alignments_args_probe_asan
 *  (the Makefile's pattern rule for `bin/%_asan`).  Exit status 0 and "alignments_args_probe: ok" when every call answered as the
 *  header says.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../stringzilla_amd/csrc/host/szs_internal.h"

#define UNTOUCHED 0x5A5A5A5A5A5A5A5Aull
#define CAPACITY 8

static int failures = 0;

static void expect(int condition, char const *what, int line) {
    if (condition) return;
    fprintf(stderr, "alignments_args_probe: line %d: %s\n", line, what);
    ++failures;
}
#define EXPECT(condition) expect((condition), #condition, __LINE__)

static char const bytes[] = "abcabd";
static sz_u32_t const offsets32[] = {0, 3, 6};
static sz_u64_t const offsets64[] = {0, 3, 6};

static sz_cptr_t member_start(void const *handle, sz_sorted_idx_t i) { return (void)handle, bytes + offsets32[i]; }
static sz_size_t member_length(void const *handle, sz_sorted_idx_t i) { return (void)handle, offsets32[i + 1] - offsets32[i]; }

/** What a call takes besides the strings. */
typedef struct {
    sz_size_t const *indices, *starts, *ends;
    sz_size_t *distances, *lengths;
    sz_u8_t *ops;
    sz_size_t capacity;
} arrays_t;

/** One call of entry `form` (0: sz_sequence_t, 1: u32tape, 2: u64tape) over `count` of the two strings, queries = candidates. */
static sz_status_t call(int form, void *engine, sz_size_t count, sz_size_t k, arrays_t const *a, sz_size_t row_stride, char const **message) {
    *message = NULL;
    if (form == 0) {
        sz_sequence_t sequence;
        memset(&sequence, 0, sizeof(sequence));
        sequence.count = count, sequence.get_start = member_start, sequence.get_length = member_length;
        return szs_rocm_alignments(engine, NULL, &sequence, &sequence, a->indices, k, a->starts, a->ends, a->distances, a->lengths, a->ops,
                                   a->capacity, row_stride, message);
    }
    if (form == 1) {
        sz_sequence_u32tape_t tape = {bytes, offsets32, count};
        return szs_rocm_alignments_u32tape(engine, NULL, &tape, &tape, a->indices, k, a->starts, a->ends, a->distances, a->lengths, a->ops,
                                           a->capacity, row_stride, message);
    }
    sz_sequence_u64tape_t tape = {bytes, offsets64, count};
    return szs_rocm_alignments_u64tape(engine, NULL, &tape, &tape, a->indices, k, a->starts, a->ends, a->distances, a->lengths, a->ops,
                                       a->capacity, row_stride, message);
}

static int untouched(void const *cells, size_t count) {
    for (size_t i = 0; i < count; ++i)
        if (((unsigned char const *)cells)[i] != 0x5A) return 0;
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

    for (int form = 0; form < 3; ++form) {
        sz_size_t indices[6] = {0, 1, 0, 1, 0, 1}, starts[6] = {0, 0, 0, 0, 0, 0}, ends[6] = {3, 3, 3, 3, 3, 3}, distances[6], lengths[6];
        sz_u8_t ops[6 * CAPACITY];
        char const *message = NULL;
        memset(distances, 0x5A, sizeof(distances)), memset(lengths, 0x5A, sizeof(lengths)), memset(ops, 0x5A, sizeof(ops));
        arrays_t const all = {indices, starts, ends, distances, lengths, ops, CAPACITY};
        arrays_t const whole = {indices, NULL, NULL, distances, lengths, ops, CAPACITY}; /* no spans: the whole candidates */
        arrays_t const none = {NULL, NULL, NULL, NULL, NULL, NULL, 0};

        void *const refused[] = {NULL, blank, weighted, runes, global, local}; /* no engine, no magic, other costs, other families */
        for (size_t e = 0; e < sizeof(refused) / sizeof(refused[0]); ++e) {
            EXPECT(call(form, refused[e], 2, 2, &all, 3, &message) == sz_status_unknown_k && message);
            EXPECT(call(form, refused[e], 2, 2, &whole, 3, &message) == sz_status_unknown_k && message);
            EXPECT(call(form, refused[e], 0, 2, &all, 3, &message) == sz_status_unknown_k && message);
            EXPECT(call(form, refused[e], 2, 0, &all, 4, &message) == sz_unexpected_dimensions_k); /* k first */
        }
        EXPECT(call(form, unit, 2, 4, &all, 3, &message) == sz_unexpected_dimensions_k);
        EXPECT(call(form, unit, 2, 2, &all, 1, &message) == sz_unexpected_dimensions_k);
        EXPECT(call(form, unit, 2, 0, &none, 4, &message) == sz_unexpected_dimensions_k); /* before the outputs are looked at */
        arrays_t dense = all;
        dense.indices = NULL;
        EXPECT(call(form, unit, 2, 1, &dense, 3, &message) == sz_unexpected_dimensions_k && message); /* dense: k = 2 */
        EXPECT(call(form, unit, 2, 3, &dense, 3, &message) == sz_unexpected_dimensions_k && message);
        EXPECT(call(form, unit, 0, 2, &all, 3, &message) == sz_success_k);
        EXPECT(call(form, unit, 0, 2, &none, 3, &message) == sz_success_k); /* zero queries: nothing is looked at */

        arrays_t missing = all; /* each required output NULL */
        missing.distances = NULL;
        EXPECT(call(form, unit, 2, 2, &missing, 3, &message) == sz_status_unknown_k && message);
        missing = all, missing.lengths = NULL;
        EXPECT(call(form, unit, 2, 2, &missing, 3, &message) == sz_status_unknown_k && message);
        missing = all, missing.ops = NULL; /* ... and `ops` wherever the capacity is not zero */
        EXPECT(call(form, unit, 2, 2, &missing, 3, &message) == sz_status_unknown_k && message);
        missing = all, missing.starts = NULL; /* exactly one of the spans' arrays */
        EXPECT(call(form, unit, 2, 2, &missing, 3, &message) == sz_status_unknown_k && message);
        missing = all, missing.ends = NULL;
        EXPECT(call(form, unit, 2, 2, &missing, 3, &message) == sz_status_unknown_k && message);
        EXPECT(untouched(distances, sizeof(distances)) && untouched(lengths, sizeof(lengths)) && untouched(ops, sizeof(ops)));
    }
    free(unit), free(weighted), free(blank), free(runes), free(global), free(local);
    if (failures) return 1;
    puts("alignments_args_probe: ok");
    return 0;
}
