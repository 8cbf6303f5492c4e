/*
 *  ways_planned.c - device-planned calls of either family: the ways to a call's plan (see dispatch_internal.h).
 */
#include "dispatch_internal.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* ---- device-planned calls: the ways to a call's plan, tried cheapest first ----------------------------------------------------
 *
 *  (round 6: one function per way - rounds 2 to 5 grew them inside one function of 380 lines.)  Each returns the call's status,
 *  or SZS_WAY_NOT_TAKEN: this call is not one for this way (or turned out not to be: nothing real was scored) - try the next.
 *
 *  Codepoint calls take the same ways, without the host reading a single offset (round 2 planned these calls on the host: offsets
 *  downloaded, strings gathered and re-addressed in O(Q + C) host loops, a wait between transcoding and planning - a third of the
 *  wall time of a batch of short words).  One stream, one wait:
 *      transcode both tapes (hip/utf8.hip: rune starts follow from the byte offsets alone, no scan) -> renumber the runes
 *      -> plan on RUNE counts (hip/planner.hip) -> wait -> decide -> launch.
 *  The UTF-32 buffer is sized by the previous calls; a batch that needs more says so (`needed`) and is transcoded again.
 *  An ASCII corpus goes to the byte engines (serial.hpp:2809-2813, applied per call).
 */

typedef struct planned_call_t {
    szs_call_t *call;
    szs_engine_s *engine;
    szs_decision_t *remembered;  /* the engine's previous device-planned call */
    szs_plan_side_t q_side, c_side; /* the caller's sides (the same one twice for a symmetric call) */
    szs_pinned_words_t volatile *words; /* pinned: where the device planner reports */
    int use_myers, knobs_automatic, uniform_bytes;
    unsigned myers_words;
    void const *key_data[2], *key_offsets[2]; /* what "the same tapes" means */
    int key_wide[2];
    szs_plan_summary_t seen; /* the summary of THIS call's tapes, once a planner has reported */
    int have_summary;        /* ... by a speculated plan whose launches did not hold: the refs on the device are blank */
    /* codepoint calls: the transcoding pass's staging in engine->device_transcode - [rune starts, u64][rune counts, u32]
     * [any_multibyte, distinct runes, alphabet overflow, pad][needed, u64] - and the copy of its flags that the planner's wait brings */
    int runes, renumber;
    uint64_t *starts;
    uint32_t *counts, *device_flags;
    uint32_t volatile *flags; /* pinned: 4 flags, then `needed` */
} planned_call_t;

#define SZS_TRANSCODE_FLAGS_BYTES (4 * sizeof(uint32_t) + sizeof(uint64_t))

/** The planner's sides: the caller's tapes - a codepoint call's as the runes the transcoding writes to the UTF-32 buffer (rebuilt
 *  when that buffer moves) - and their refs in engine->device_plan_refs. */
static void build_sides(planned_call_t *way) {
    szs_call_t const *call = way->call;
    uint32_t const q_count = call->q_count, c_count = call->c_count;
    szs_string_ref_t *const base = (szs_string_ref_t *)way->engine->device_plan_refs.pointer;
    uint64_t const runes = (uint64_t)(uintptr_t)way->engine->device_runes.pointer;
    szs_plan_side_t const q_side = {call->queries->offsets, way->runes ? runes : (uint64_t)(uintptr_t)call->queries->data, q_count,
                                    call->queries->kind == szs_input_u64tape_k, base, base + q_count, way->counts, way->starts};
    way->q_side = way->c_side = q_side;
    if (!call->symmetric) {
        szs_plan_side_t const other = {call->candidates->offsets, way->runes ? runes : (uint64_t)(uintptr_t)call->candidates->data, c_count,
                                       call->candidates->kind == szs_input_u64tape_k, base + 2 * (size_t)q_count,
                                       base + 2 * (size_t)q_count + c_count, way->runes ? way->counts + q_count : NULL,
                                       way->runes ? way->starts + q_count : NULL};
        way->c_side = other;
    }
}

/** Both tapes into the engine's UTF-32 buffer and, with `renumber`, their runes into ids: launches only, no wait. */
static hipError_t enqueue_transcoding(planned_call_t const *way) {
    szs_call_t const *call = way->call;
    szs_engine_s *engine = way->engine;
    int const symmetric = call->symmetric;
    uint32_t const q_count = call->q_count, c_count = symmetric ? 0u : call->c_count;
    uint32_t *const runes = (uint32_t *)engine->device_runes.pointer;
    hipError_t error = hipMemsetAsync(way->device_flags, 0, SZS_TRANSCODE_FLAGS_BYTES, call->stream);
    if (error == hipSuccess)
        error = (hipError_t)szs_hip_utf8_transcode_tapes(call->queries->data, call->queries->offsets, q_count, call->queries->kind == szs_input_u64tape_k,
                                                         symmetric ? NULL : call->candidates->data, symmetric ? NULL : call->candidates->offsets, c_count,
                                                         !symmetric && call->candidates->kind == szs_input_u64tape_k,
                                                         engine->device_runes.capacity / sizeof(uint32_t), runes, way->starts, way->counts, way->device_flags,
                                                         (uint64_t *)(way->device_flags + 4), way->renumber ? engine->device_alphabet.pointer : NULL, call->stream);
    if (error == hipSuccess && way->renumber)
        error = (hipError_t)szs_hip_alphabet_rename(q_count + c_count, way->starts, way->counts, runes, way->device_flags, engine->device_alphabet.pointer, 1,
                                                    SZS_ALPHABET_MOST, way->device_flags + 1, call->stream);
    return error;
}

/** The planner, behind the transcoding of a codepoint call (whose flags are copied back behind it): launches only, no wait.
 *  `expected` gets the plan's sequence. */
static hipError_t enqueue_plan(planned_call_t *way, szs_plan_expectation_t *expected) {
    szs_call_t const *call = way->call;
    expected->sequence = ++way->engine->plan_sequence;
    way->remembered->refs_current = 0; /* the planner is about to overwrite the refs */
    hipError_t error = way->runes ? enqueue_transcoding(way) : hipSuccess;
    if (error == hipSuccess)
        error = (hipError_t)szs_hip_plan(&way->q_side, call->symmetric ? NULL : &way->c_side, way->myers_words, expected,
                                         (szs_plan_summary_t *)&way->words->summary, szs_device_words(way->engine)->verdicts, call->stream);
    if (error == hipSuccess && way->runes)
        error = hipMemcpyAsync((void *)way->flags, way->device_flags, SZS_TRANSCODE_FLAGS_BYTES, hipMemcpyDeviceToHost, call->stream);
    return error;
}

/** The narrow buffer of a codepoint call's tiny tokens (cross_tiny).  `needed` counts every string's BYTE span rounded up
 *  (hip/utf8.hip: transcode_tape_t::span): it bounds the bytes of both tapes. */
static sz_status_t reserve_narrow(szs_engine_s *engine, int device, char const **error_message) {
    size_t const before = engine->device_narrow.capacity;
    sz_status_t const status = szs_buffer_reserve(&engine->device_narrow, szs_memory_device_k, device,
                                                  (size_t)(engine->runes_needed + engine->runes_needed / 4) + 64 + SZS_NARROW_WORKSPACE, error_message);
    if (engine->device_narrow.capacity != before) engine->narrow_zeroed = NULL; /* (a new buffer, wherever it lies) */
    return status;
}

/** The profile of a call that was scored before its statistics were known (speculated, or planned inside its launch), and what the
 *  next call may count on: the refs on the device describe these tapes; a batch of tiny tokens goes to their kernel next time. */
static void complete_from_summary(planned_call_t *way, szs_plan_summary_t const *seen) {
    szs_engine_s *engine = way->engine;
    int const symmetric = way->call->symmetric;
    uint32_t const q_count = way->call->q_count, c_count = way->call->c_count;
    szs_rocm_call_profile_t *profile = &engine->last_profile;
    profile->cells = symmetric ? seen->symmetric_cells : seen->side[0].symbols * seen->side[1].symbols;
    profile->algorithmic_bytes = (symmetric ? ((uint64_t)q_count + 1) * seen->side[0].symbols
                                            : (uint64_t)c_count * seen->side[0].symbols + (uint64_t)q_count * seen->side[1].symbols) + profile->pairs * 16;
    profile->unique_bytes += seen->side[0].symbols + (symmetric ? 0 : seen->side[1].symbols);
    profile->longest_query = seen->side[0].longest, profile->longest_candidate = seen->side[1].longest;
    if (way->runes) engine->runes_needed = *(uint64_t const volatile *)(way->flags + 4);
    szs_call_stamp_refs(way->remembered, way->key_data, way->key_offsets, way->key_wide, seen);
    /* words scored on the shape of an earlier batch (sentences before them, or words the tiny-token launch was not tried on): the next
     * call of these counts goes to that launch (cross_tiny).  A codepoint batch must not be all ASCII, and it counts a refusal down
     * here where a byte batch does not (kept as it was). */
    if ((!way->runes || way->flags[0]) && szs_tiny_shaped(engine, symmetric, &seen->side[0], &seen->side[1]) &&
        !szs_tiny_recently_refused(engine, q_count, c_count, way->runes)) {
        if (!way->runes) szs_tiny_note(&engine->tiny[0], 1, q_count, c_count);
        else if (reserve_narrow(engine, way->call->device, NULL) == sz_success_k) szs_tiny_note(&engine->tiny[1], 1, q_count, c_count);
    }
}

/** The launches of decision `d` over the refs of this call's sides (the kernel's queries longest first, its candidates shortest first;
 *  `guard`: refs of an earlier call, or NULL), the wait and the profile of plan mode `planner`.  `*stalled`: run it again on lanes. */
static sz_status_t score(planned_call_t *way, szs_decision_t const *d, szs_ref_guard_t const *guard, uint32_t planner, uint64_t query_symbols,
                         uint64_t candidate_symbols, int *stalled) {
    szs_call_t *call = way->call;
    szs_engine_s *engine = way->engine;
    uint32_t launches = 0, cell_bits = 0;
    sz_status_t enqueue_status = sz_success_k;
    hipError_t error = hipEventRecord(engine->event_start, call->stream);
    if (error == hipSuccess)
        error = szs_call_enqueue(engine, d, call->device, d->transposed ? way->c_side.descending : way->q_side.descending,
                                 d->transposed ? way->q_side.ascending : way->c_side.ascending, call->device_results, call->device_stride, call->stream,
                                 guard, &launches, &cell_bits, &enqueue_status, call->error_message);
    engine->last_profile.planner = planner;
    *stalled = 0;
    return szs_call_finish(call, d, error, enqueue_status, launches, cell_bits, query_symbols, candidate_symbols, stalled);
}

/**
 *  Way 3 (bytes) - the same tapes again: the refs planned for them are still on the device, no planner at all.  Every workgroup and
 *  lane of the byte kernels checks its ref against the offsets as they are NOW before it touches a string (hip/kernels.h:
 *  szs_ref_guard_t), so a tape that was rewritten in place, freed or reallocated costs one re-plan, never a wrong score or a stray
 *  read.  Only launches whose kernels carry the guard take this way: unit-cost byte queries of up to 256 bytes - ONE launch of
 *  ~0.2 ms, where 25 us of planning matter (with longer queries the guarded launches were slower than planning: 128 x 128 x 1 KB
 *  over eight lanes per pair 0.67 ms behind the guard, 0.50 ms planned - profiles/r03).
 */
static sz_status_t planned_on_the_same_tapes(planned_call_t *way) {
    szs_call_t *call = way->call;
    szs_engine_s *engine = way->engine;
    szs_decision_t *const remembered = way->remembered;
    int const symmetric = call->symmetric;
    if (!(remembered->valid && remembered->refs_current && way->knobs_automatic && szs_tuning_get(szs_knob_reuse_k) != 0 &&
          remembered->tier == SZS_TIER_LANES && remembered->use_myers && !remembered->runes && !remembered->wide_cells &&
          !szs_decision_has_variant_zero(remembered) && remembered->plan.groups_count == 1 &&
          remembered->plan.groups[0].variant == SZS_MYERS_SHORT_WORDS && remembered->q_count == call->q_count && remembered->c_count == call->c_count &&
          remembered->symmetric == symmetric && remembered->key_data[0] == way->key_data[0] && remembered->key_data[1] == way->key_data[1] &&
          remembered->key_offsets[0] == way->key_offsets[0] && remembered->key_offsets[1] == way->key_offsets[1] &&
          remembered->key_wide[0] == way->key_wide[0] && remembered->key_wide[1] == way->key_wide[1]))
        return SZS_WAY_NOT_TAKEN;
    szs_decision_t const *d = remembered;
    uint32_t volatile *const stale = &way->words->stale;
    szs_ref_guard_t guard;
    memset(&guard, 0, sizeof(guard));
    guard.enabled = 1, guard.sequence = ++engine->plan_sequence, guard.stale = (uint32_t *)stale;
    for (int role = 0; role < 2; ++role) { /* kernel roles: 0 = its queries, 1 = its candidates */
        szs_plan_side_t const *side = (role == 0) == (d->transposed == 0) ? &way->q_side : &way->c_side;
        if (symmetric) side = &way->q_side;
        guard.side[role].offsets = side->offsets, guard.side[role].base = side->base;
        guard.side[role].wide = side->wide, guard.side[role].count = side->count;
    }
    *stale = 0;
    sz_status_t status = szs_call_prepare(engine, d, call->device, call->stream, call->error_message);
    if (status != sz_success_k) return status;
    szs_call_phase(call, 2);
    int stalled;
    status = score(way, d, &guard, 3, d->summary.side[0].symbols, d->summary.side[1].symbols, &stalled);
    if (status != sz_success_k) return status;
    if (*stale != guard.sequence) return sz_success_k; /* every ref still described its string: scored */
    remembered->refs_current = 0;                      /* the tapes changed under the same pointers: plan them afresh */
    return SZS_WAY_NOT_TAKEN;
}

/**
 *  Way 4 (bytes) - the planner INSIDE the scoring launch (round 5; hip/kernels.h: szs_fused_plan_t).  The previous call of this engine
 *  was ONE launch of the short unit-cost byte kernel and this one has the same counts: the launch goes out alone - its first two
 *  workgroups sort the two sides (what hip/planner.hip does in a launch of its own) while the others wait for the refs.  No planner
 *  launch, no kernel boundary: config 2's fresh-batch call 202 -> ~190 us.  Round 6: symmetric calls too (one side, sorted once,
 *  serves both roles) and sides of up to 16,384 strings (counted and placed in two walks over their offsets).  A batch that does not
 *  fit after all (a query beyond 256 bytes, malformed offsets) is scored as empty strings; a launch whose waiting workgroups ran out
 *  of polls scored only part of the matrix: either way the call goes on to the next way.
 */
static sz_status_t planned_inside_the_launch(planned_call_t *way) {
    szs_call_t *call = way->call;
    szs_engine_s *engine = way->engine;
    szs_decision_t *const remembered = way->remembered;
    int const symmetric = call->symmetric;
    int const knob = szs_tuning_get(szs_knob_fused_k);
    if (!(remembered->valid && !remembered->runes && remembered->tier == SZS_TIER_LANES && remembered->use_myers && !remembered->wide_cells &&
          !remembered->use_queue && szs_decision_is_one_launch(remembered) && remembered->plan.groups[0].variant == SZS_MYERS_SHORT_WORDS &&
          remembered->q_count == call->q_count && remembered->c_count == call->c_count && remembered->symmetric == symmetric &&
          call->q_count <= SZS_FUSED_MOST_STRINGS_TWO_PASSES && call->c_count <= SZS_FUSED_MOST_STRINGS_TWO_PASSES && way->knobs_automatic &&
          !way->uniform_bytes && knob != 0 && (!engine->fused_gave_up || knob == 2)))
        return SZS_WAY_NOT_TAKEN;
    szs_decision_t const *d = remembered;
    szs_fused_side_report_t volatile *const reports = way->words->fused_reports;
    uint32_t volatile *const gave_up = &way->words->fused_gave_up;
    szs_fused_plan_t fused;
    memset(&fused, 0, sizeof(fused));
    fused.side[0] = d->transposed ? way->c_side : way->q_side, fused.side[1] = d->transposed ? way->q_side : way->c_side;
    if (!++engine->plan_sequence) ++engine->plan_sequence; /* never 0: the ready words start there */
    fused.sequence = engine->plan_sequence;
    fused.ready = szs_device_words(engine)->ready, fused.report = (szs_fused_side_report_t *)reports;
    *gave_up = 0;
    fused.gave_up = (uint32_t *)gave_up, fused.poll_budget = SZS_FUSED_POLL_BUDGET;
    if (knob == 2) fused.withhold = 1, fused.poll_budget = 64; /* testing: nobody is ever told */
    sz_status_t status = szs_call_prepare(engine, d, call->device, call->stream, call->error_message); /* buffers of the previous call: nothing to allocate */
    if (status != sz_success_k) return status;
    szs_call_phase(call, 2);
    remembered->refs_current = 0; /* the launch is about to overwrite the refs */
    /* (Measured and not kept: the launch stamping the event pair itself - hipExtLaunchKernel with a start and a stop event, no
     * records around it.  The kernel's own time reads 177.0 us instead of 180.9, but the call takes 200.7 us instead of 193.7.) */
    hipError_t error = hipEventRecord(engine->event_start, call->stream);
    uint32_t launches = 0;
    if (error == hipSuccess) {
        error = (hipError_t)szs_hip_levenshtein_myers_fused(&fused, (uint64_t *)call->device_results, call->device_stride, d->layout, call->stream);
        launches = error == hipSuccess;
    }
    engine->last_streams = 1;
    int stalled = 0;
    engine->last_profile.planner = 4;
    status = szs_call_finish(call, d, error, sz_success_k, launches, 0, 0, 0, &stalled);
    if (status != sz_success_k) return status;
    szs_fused_side_report_t sides[2];
    memcpy(sides, (void const *)reports, sizeof(sides));
    if (*gave_up == fused.sequence) { /* a workgroup ran out of polls: whatever the reports say, not every cell was scored - the ready
                                         words are zeroed before anything waits on them again, and this engine does not try again */
        engine->fused_gave_up = 1, engine->fused_zeroed = NULL;
        return SZS_WAY_NOT_TAKEN;
    }
    if (!(sides[0].sequence == fused.sequence && !sides[0].status && !sides[0].blank &&
          (symmetric || (sides[1].sequence == fused.sequence && !sides[1].status && !sides[1].blank))))
        return SZS_WAY_NOT_TAKEN; /* not this shape after all: nothing real was scored */
    engine->last_pairing = sides[0].pairing; /* of the KERNEL's query side */
    /* scored; the profile and the remembered plan take this batch's figures (caller roles again; a symmetric call has one side) */
    szs_fused_side_report_t const *const of_queries = &sides[!symmetric && d->transposed ? 1 : 0];
    szs_fused_side_report_t const *const of_candidates = symmetric ? of_queries : &sides[d->transposed ? 0 : 1];
    if (call->trace)
        for (int s = 0; s < (symmetric ? 1 : 2); ++s)
            fprintf(stderr, "fused sorter %d (10 ns ticks since it began): offsets loaded %u, positions %u, refs written %u, published %u; began %d ticks after sorter 0; pairing rule %u\n",
                    s, sides[s].ticks[1], sides[s].ticks[2], sides[s].ticks[3], sides[s].ticks[4], (int)(sides[s].ticks[0] - sides[0].ticks[0]), sides[s].pairing);
    szs_plan_summary_t seen_here = remembered->summary;
    seen_here.status = 0, seen_here.speculation_held = 1, seen_here.sequence = fused.sequence;
    seen_here.side[0] = of_queries->stats, seen_here.side[1] = of_candidates->stats;
    memcpy(seen_here.rank_lengths[0], of_queries->rank_lengths, sizeof(seen_here.rank_lengths[0]));
    memcpy(seen_here.rank_lengths[1], of_candidates->rank_lengths, sizeof(seen_here.rank_lengths[1]));
    /* the lower triangle of a symmetric call: sum over i of len_i x (sum over j <= i of len_j) = ((sum len)^2 + sum len^2) / 2 */
    seen_here.symmetric_cells = symmetric ? (seen_here.side[0].symbols * seen_here.side[0].symbols + of_queries->squares) / 2 : 0;
    remembered->longest[0] = seen_here.side[0].longest, remembered->longest[1] = seen_here.side[1].longest;
    complete_from_summary(way, &seen_here);
    return szs_report(sz_success_k, call->error_message, NULL);
}

/**
 *  Way 2 - speculate: launches shaped like the previous call go in right behind the planner, which validates the shape and blanks
 *  the refs of a side that does not have it.  (Round 3: only calls of ONE launch.  The launches of a mixed-length batch leave the
 *  host one after the other, longest pairs first, and reach the device in that order; enqueued behind the planner they are all
 *  released by the same event and the device takes them as it likes - the short launch's thousands of workgroups first, the long
 *  pairs late.  Config 5: 9.68 ms speculated, 9.60 planned-and-waited-for; an eighth of it 1.95 / 1.85; codepoints 8.4 / 7.1.)
 *  A codepoint batch is also transcoded and renumbered behind the same wait, and must fit two more conditions that only the device
 *  can check: no more runes than the buffer holds, no more distinct ones than the tables have rows (4096 x 4096 words of prose: the
 *  planning half was as long as the scoring - profiles/r03/real_text.jsonl).
 *  Leaves `way->seen` / `way->have_summary` when the planner reported on a byte batch but the shape did not hold.
 */
static sz_status_t planned_and_speculated(planned_call_t *way) {
    szs_call_t *call = way->call;
    szs_engine_s *engine = way->engine;
    szs_decision_t *const remembered = way->remembered;
    int const symmetric = call->symmetric;
    if (!(remembered->valid && remembered->runes == way->runes && remembered->tier == SZS_TIER_LANES && remembered->q_count == call->q_count &&
          remembered->c_count == call->c_count && remembered->symmetric == symmetric && way->knobs_automatic && !way->uniform_bytes &&
          szs_decision_is_one_launch(remembered) && (remembered->use_myers || !way->runes) && (!remembered->alphabet || way->renumber)))
        return SZS_WAY_NOT_TAKEN;
    szs_decision_t const *d = remembered;
    szs_plan_expectation_t expected = {0};
    expected.enabled = 1, expected.query_side = (uint32_t)d->transposed;
    expected.longest[0] = d->longest[0], expected.longest[1] = d->longest[1];
    memcpy(expected.variant_counts, d->variant_counts, sizeof(expected.variant_counts));
    if (way->runes) {
        expected.runes_needed = (uint64_t const *)(way->device_flags + 4), expected.runes_capacity = engine->device_runes.capacity / sizeof(uint32_t);
        expected.alphabet_flags = way->device_flags, expected.alphabet = d->alphabet;
    }
    sz_status_t status = szs_call_prepare(engine, d, call->device, call->stream, call->error_message); /* buffers of the previous call: nothing to allocate */
    if (status != sz_success_k) return status;
    szs_call_phase(call, 2);
    hipError_t error = enqueue_plan(way, &expected);
    if (error != hipSuccess) {
        (void)hipStreamSynchronize(call->stream);
        return szs_report_hip(error, call->error_message); /* no scoring launch has been enqueued */
    }
    /* the summary is read after the wait; the profile's statistics are filled in from it afterwards */
    int stalled;
    status = score(way, d, NULL, 2, 0, 0, &stalled);
    if (status != sz_success_k) return status;
    memcpy(&way->seen, (void const *)&way->words->summary, sizeof(way->seen));
    int const reported = way->seen.sequence == expected.sequence;
    way->have_summary = reported && !way->runes; /* (a codepoint batch is transcoded again: its runes may not have fit the buffer) */
    if (!(reported && !way->seen.status && way->seen.speculation_held))
        return SZS_WAY_NOT_TAKEN; /* another shape, more runes, a richer alphabet or malformed offsets: the refs were blanked, nothing real was scored */
    complete_from_summary(way, &way->seen); /* the batch had the remembered shape and has been scored */
    return szs_report(sz_success_k, call->error_message, NULL);
}

/** The size of the direct tables the codepoint kernels are launched with for a batch of `distinct` renumbered runes: some
 *  room above it, so that the NEXT batch of the stream - launched on this one's shape before anyone has counted its runes -
 *  still fits when it holds a few more (a table row is 4 bytes of LDS). */
static uint32_t alphabet_with_room(uint32_t distinct) {
    uint32_t const roomy = distinct + distinct / 8 + 8;
    return roomy < SZS_ALPHABET_MOST ? roomy : SZS_ALPHABET_MOST;
}

/** Way 1 - plan on the device, wait for the summary, decide, launch (and, for a batch of tiny tokens, their launch instead). */
static sz_status_t planned_and_waited_for(planned_call_t *way) {
    szs_call_t *call = way->call;
    szs_engine_s *engine = way->engine;
    szs_decision_t *const remembered = way->remembered;
    hipStream_t const stream = call->stream;
    int const symmetric = call->symmetric;
    char const **error_message = call->error_message;
    szs_plan_summary_t *const seen = &way->seen;
    sz_status_t status;
    hipError_t error;
    if (!way->have_summary)
        for (int round = 0;; ++round) { /* a codepoint call's second round: its runes outgrew the UTF-32 buffer */
            uint64_t const capacity = engine->device_runes.capacity / sizeof(uint32_t);
            szs_plan_expectation_t none = {0};
            error = enqueue_plan(way, &none);
            hipError_t const drained = hipStreamSynchronize(stream); /* THE wait of the planning half; also on failure */
            if (error == hipSuccess) error = drained;
            if (error != hipSuccess) return szs_report_hip(error, error_message);
            memcpy(seen, (void const *)&way->words->summary, sizeof(*seen));
            if (seen->sequence != none.sequence) return szs_report(sz_status_unknown_k, error_message, "The device planner did not report");
            if (!way->runes || (seen->status & (SZS_PLAN_STATUS_DESCENDING | SZS_PLAN_STATUS_OVERFLOW))) break; /* (reported below) */
            uint64_t const needed = *(uint64_t const volatile *)(way->flags + 4);
            engine->runes_needed = needed;
            if (needed <= capacity) break;
            if (round) return szs_report(sz_status_unknown_k, error_message, "The UTF-32 buffer did not settle");
            status = szs_buffer_reserve(&engine->device_runes, szs_memory_device_k, call->device, (size_t)(needed + needed / 4 + 4) * sizeof(uint32_t), error_message);
            if (status != sz_success_k) return status; /* grown: transcode again, every string fits now */
            build_sides(way);
        }
    if (seen->status & SZS_PLAN_STATUS_DESCENDING) return szs_report(sz_unexpected_dimensions_k, error_message, "Tape offsets must ascend");
    if (seen->status & SZS_PLAN_STATUS_OVERFLOW) return szs_report(sz_overflow_risk_k, error_message, NULL);
    if (way->runes) {
        if (remembered->runes) remembered->valid = 0; /* whatever happens below, the next call is not launched on an older codepoint shape */
        if (!way->flags[0]) return SZS_RUNES_ARE_BYTES;
    }
    if (seen->status & SZS_PLAN_STATUS_UNSORTED) return SZS_NOT_DEVICE_PLANNABLE; /* strings beyond the planner's histogram */
    if (way->uniform_bytes) { /* the scan has landed (the planner's wait covered it): number the bytes that occur 0 ... A - 1 */
        uint32_t volatile const *const presence = way->words->presence;
        uint32_t classes = 0;
        for (unsigned byte = 0; byte < 256; ++byte)
            engine->uniform_byte_to_class[byte] = (presence[byte / 32] >> (byte % 32)) & 1u ? (uint8_t)classes++ : 0;
        engine->uniform_classes = classes ? classes : 1; /* a batch of empty strings: one class nobody belongs to */
    }
    szs_call_phase(call, 1);

    /* the summary (in RUNES for a codepoint call) says tiny tokens, and the kernel did not refuse the previous batch of these counts: no
     * refs needed after all.  A codepoint call's narrow strings get a buffer of their own - should that launch refuse the batch, the
     * UTF-32 arrays are scored below.  (Only a byte call looks at the tier, swap and queue knobs here.) */
    if ((way->runes || (szs_tuning_get(szs_knob_tier_k) < 0 && szs_tuning_get(szs_knob_swap_k) < 0 && szs_tuning_get(szs_knob_queue_k) < 0)) &&
        szs_tiny_shaped(engine, symmetric, &seen->side[0], &seen->side[1]) && !szs_tiny_recently_refused(engine, call->q_count, call->c_count, 1)) {
        if (way->runes && (status = reserve_narrow(engine, call->device, error_message)) != sz_success_k) return status;
        status = szs_cross_tiny(call, 1, seen, way->runes);
        if (status != SZS_TINY_NOT_TAKEN) return status;
    }
    uint32_t alphabet = 0; /* a renumbered codepoint batch: the arrays hold ids 1 ... distinct, the kernels index direct tables with them */
    if (way->renumber) {
        uint32_t const distinct = way->flags[1], overflowed = way->flags[2];
        if (distinct && distinct <= SZS_ALPHABET_MOST && !overflowed) alphabet = alphabet_with_room(distinct);
    }

    for (int attempt = 0; attempt < 2; ++attempt) { /* second round: a stalled band chain is re-run on the lanes tier */
        szs_decision_t d;
        uint64_t const cells = symmetric ? seen->symmetric_cells : seen->side[0].symbols * seen->side[1].symbols;
        status = szs_call_decide(engine, symmetric, way->runes, attempt > 0, &seen->side[0], &seen->side[1], seen->variant_counts[0], seen->variant_counts[1],
                        seen->rank_lengths, cells, &d, error_message);
        if (status != sz_success_k) return status;
        d.alphabet = alphabet;
        szs_call_decide_queue(engine, &d, seen->rank_lengths);
        status = szs_call_prepare(engine, &d, call->device, stream, error_message);
        if (status != sz_success_k) return status;
        szs_call_phase(call, 2);
        if (way->have_summary) { /* the refs on the device are blank (failed speculation): write the real ones */
            szs_plan_expectation_t none = {0};
            error = enqueue_plan(way, &none);
            if (error != hipSuccess) return szs_report_hip(error, error_message);
            way->have_summary = 0;
        }
        int stalled;
        status = score(way, &d, NULL, 1, seen->side[0].symbols, seen->side[1].symbols, &stalled);
        if (status != sz_success_k) return status;
        if (!stalled) {
            /* the next call of this shape goes in speculatively - or, a byte call on the same tapes, without a planner (a codepoint
             * plan is stamped too: ways 3 and 4 look at byte plans only) */
            *remembered = d;
            szs_call_stamp_refs(remembered, way->key_data, way->key_offsets, way->key_wide, seen);
            return sz_success_k;
        }
    }
    return szs_report(sz_status_unknown_k, error_message, "Systolic pipeline stalled");
}

/** A non-unit-cost Levenshtein call: which bytes occur in this batch?  One pass over both tapes, enqueued ahead of the planner and
 *  read after the planner's own wait; the team tier keys its profile by the classes the host numbers from it (szs_call_decide).
 *  Such a call is not speculated: its launch depends on what the scan finds. */
static sz_status_t enqueue_byte_presence(planned_call_t *way) {
    szs_call_t const *call = way->call;
    szs_engine_s *engine = way->engine;
    hipStream_t const stream = call->stream;
    way->uniform_bytes = (engine->family == szs_family_levenshtein_k || engine->family == szs_family_levenshtein_utf8_k) && !engine->is_unit_cost &&
                         szs_tuning_get(szs_knob_packed_k) != 0 && szs_tuning_get(szs_knob_team_k) != 0;
    engine->uniform_classes = 0;
    if (!way->uniform_bytes) return sz_success_k;
    sz_status_t const status = szs_buffer_reserve(&engine->device_presence, szs_memory_device_k, call->device, 8 * sizeof(uint32_t), call->error_message);
    if (status != sz_success_k) return status;
    uint32_t *const presence = (uint32_t *)engine->device_presence.pointer;
    hipError_t error = hipMemsetAsync(presence, 0, 8 * sizeof(uint32_t), stream);
    if (error == hipSuccess)
        error = (hipError_t)szs_hip_byte_presence(call->queries->data, call->queries->offsets, call->q_count, (int)way->q_side.wide, presence, stream);
    if (error == hipSuccess && !call->symmetric)
        error = (hipError_t)szs_hip_byte_presence(call->candidates->data, call->candidates->offsets, call->c_count, (int)way->c_side.wide, presence, stream);
    if (error == hipSuccess) error = hipMemcpyAsync((void *)way->words->presence, presence, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    if (error != hipSuccess) {
        (void)hipStreamSynchronize(stream);
        return szs_report_hip(error, call->error_message);
    }
    return sz_success_k;
}

sz_status_t szs_cross_device_planned(szs_call_t *call, int runes) {
    szs_engine_s *engine = call->engine;
    int const device = call->device, symmetric = call->symmetric;
    uint32_t const q_count = call->q_count, c_count = call->c_count;
    char const **error_message = call->error_message;
    size_t const strings = (size_t)q_count + (symmetric ? 0 : c_count);

    void *const refs_before = engine->device_plan_refs.pointer;
    sz_status_t status = szs_buffer_reserve(&engine->device_plan_refs, szs_memory_device_k, device, 2 * strings * sizeof(szs_string_ref_t), error_message);
    /* The refs of the previous call live in that buffer.  If the reserve moved it (or failed), the remembered plan describes
     * memory that is gone: forget it HERE, before any way below could re-use it behind nothing but the in-kernel guard. */
    if (engine->remembered && (status != sz_success_k || engine->device_plan_refs.pointer != refs_before))
        engine->remembered->refs_current = 0, engine->remembered->valid = 0;
    if (status != sz_success_k) return status;
    if (!engine->remembered) {
        engine->remembered = (szs_decision_t *)calloc(1, sizeof(szs_decision_t));
        if (!engine->remembered) return szs_report(sz_bad_alloc_k, error_message, NULL);
    }
    planned_call_t way;
    memset(&way, 0, sizeof(way));
    way.call = call, way.engine = engine, way.remembered = engine->remembered, way.runes = runes;
    if (runes) {
        /* the transcoding's staging (planned_call_t), which also holds the word per string of a batch of tiny tokens (cross_tiny) */
        size_t const counts_at = strings * sizeof(uint64_t), flags_at = (counts_at + strings * sizeof(uint32_t) + 7) & ~(size_t)7;
        status = szs_buffer_reserve(&engine->device_transcode, szs_memory_device_k, device, flags_at + SZS_TRANSCODE_FLAGS_BYTES, error_message);
        if (status == sz_success_k) status = szs_buffer_reserve(&engine->pinned_transcode, szs_memory_pinned_k, device, 64, error_message);
        if (status == sz_success_k && engine->device_runes.capacity < ((size_t)1 << 20))
            status = szs_buffer_reserve(&engine->device_runes, szs_memory_device_k, device, (size_t)1 << 20, error_message);
        /* Renumbering the runes (hip/utf8.hip) is four more operations ahead of the planner - ~60 us and a pass over every rune,
         * ~15 ps each - and makes the scoring kernels ~15 % faster (one LDS read per column instead of a hash probe, ~3 fs per
         * cell): worth it when the CELLS of the call outweigh its runes.  4096 x 4096 words of prose (6e8 cells): 0.39 ms
         * renumbered, 0.31 not; config 5u (4.4e11 cells): 7.1 against 8.4 ms, an eighth of it 1.82 / 2.16.  The host has not read
         * an offset, so it goes by the PREVIOUS call of this engine - a stream of batches settles at once. */
        int const alphabet_knob = szs_tuning_get(szs_knob_alphabet_k);
        way.renumber = alphabet_knob == 0  ? 0
                       : alphabet_knob > 0 ? 1
                                           : engine->cells_before >= 20000000000ull + 5000ull * engine->runes_needed && engine->runes_needed > 0;
        if (status == sz_success_k && way.renumber)
            status = szs_buffer_reserve(&engine->device_alphabet, szs_memory_device_k, device, szs_hip_alphabet_workspace_bytes(), error_message);
        if (status != sz_success_k) return status;
        char *const staging = (char *)engine->device_transcode.pointer;
        way.starts = (uint64_t *)staging, way.counts = (uint32_t *)(staging + counts_at), way.device_flags = (uint32_t *)(staging + flags_at);
        way.flags = (uint32_t volatile *)engine->pinned_transcode.pointer;
    }
    status = szs_call_place_results(call);
    if (status != sz_success_k) return status;
    status = szs_call_reserve_device_words(engine, device, call->stream, error_message);
    if (status != sz_success_k) return status;
    way.words = szs_pinned_words(engine);
    /* (the codepoint family gets here as bytes with an ASCII corpus: its runes are its bytes) */
    way.use_myers = engine->is_unit_cost && (engine->family == szs_family_levenshtein_k || engine->family == szs_family_levenshtein_utf8_k);
    way.myers_words = way.use_myers ? SZS_MYERS_MAX_WORDS : 0;
    build_sides(&way);
    way.key_data[0] = call->queries->data, way.key_data[1] = symmetric ? call->queries->data : call->candidates->data;
    way.key_offsets[0] = call->queries->offsets, way.key_offsets[1] = symmetric ? call->queries->offsets : call->candidates->offsets;
    way.key_wide[0] = (int)way.q_side.wide, way.key_wide[1] = (int)way.c_side.wide;
    /* (a pinned `queue` knob makes one-group calls queue launches: those are planned and waited for) */
    way.knobs_automatic = szs_tuning_get(szs_knob_speculate_k) != 0 && szs_tuning_get(szs_knob_tier_k) < 0 && szs_tuning_get(szs_knob_swap_k) < 0 &&
                          szs_tuning_get(szs_knob_cells_k) < 0 && szs_tuning_get(szs_knob_packed_k) < 0 && szs_tuning_get(szs_knob_team_k) < 0 &&
                          szs_tuning_get(szs_knob_queue_k) < 0 && (!runes || szs_tuning_get(szs_knob_rune_ids_k) < 0);
    szs_call_phase(call, 0);

    /* ---- way 5, tiny tokens (hip/myers_tiny.hip): the previous call of these counts was scored straight from the tapes - so is this
     * one, with no planner at all; the kernel says when a query does not fit it.  A codepoint call is narrowed to byte strings first
     * (cross_tiny) instead of being transcoded, renumbered and planned; a batch that is something else says so itself (a string beyond
     * 255 runes, too many long ones, an alphabet beyond the table) and is scored below.  It also goes by the byte record: ASCII words,
     * which this engine hands to the byte kernels after transcoding and planning them to find that out - narrowed, an ASCII batch is
     * its own bytes, 13 us instead of that front end.  (The families look at different knobs here.) */
    szs_tiny_memory_t const *const bytes_before = &engine->tiny[0], *const runes_before = &engine->tiny[1];
    int const words_before = (bytes_before->valid && szs_tiny_counts_match(bytes_before, q_count, c_count)) ||
                             (runes && runes_before->valid && szs_tiny_counts_match(runes_before, q_count, c_count));
    if (words_before && way.use_myers && szs_tuning_get(szs_knob_tiny_k) != 0 && szs_tuning_get(szs_knob_speculate_k) != 0 &&
        szs_tuning_get(szs_knob_tier_k) < 0 && (runes ? engine->runes_needed != 0 : szs_tuning_get(szs_knob_swap_k) < 0 && szs_tuning_get(szs_knob_queue_k) < 0)) {
        if (runes && (status = reserve_narrow(engine, device, error_message)) != sz_success_k) return status;
        status = szs_cross_tiny(call, 5, NULL, runes);
        if (status != SZS_TINY_NOT_TAKEN) return status;
    }

    if (!runes) { /* the ways that re-use a byte plan */
        status = planned_on_the_same_tapes(&way); /* way 3 */
        if (status != SZS_WAY_NOT_TAKEN) return status;
        status = enqueue_byte_presence(&way);
        if (status != sz_success_k) return status;
        status = planned_inside_the_launch(&way); /* way 4 */
        if (status != SZS_WAY_NOT_TAKEN) return status;
    }
    status = planned_and_speculated(&way); /* way 2 */
    if (status != SZS_WAY_NOT_TAKEN) return status;
    return planned_and_waited_for(&way); /* way 1 */
}
