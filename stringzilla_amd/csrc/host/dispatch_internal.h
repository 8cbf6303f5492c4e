/*
 *  dispatch_internal.h - what the translation units of ONE ENGINE CALL share (round 6: dispatch.c had grown to 2,150 lines).
 *
 *      dispatch.c       the call itself: inputs, buffers, the decision (tier, orientation, cell width), the launch sequence, the wait
 *                       and the profile; host-planned calls; which way a call goes
 *      ways_planned.c   device-planned calls of either family: the ways to a call's plan (speculated, waited for; tiny tokens; for
 *                       bytes also the same tapes and the plan inside the launch), codepoint calls transcoded and planned on rune counts
 *      ways_tiny.c      the tiny-token launch of either family (hip/myers_tiny.hip, hip/utf8.hip: utf8_narrow_kernel)
 *
 *  Nothing here is exported (csrc/exports.map).
 */
#ifndef SZS_DISPATCH_INTERNAL_H_
#define SZS_DISPATCH_INTERNAL_H_

#include "szs_internal.h"

typedef struct szs_call_t {
    szs_engine_s *engine;
    int device;
    hipStream_t stream;
    szs_input_t const *queries, *candidates;
    int symmetric;
    uint32_t q_count, c_count;
    void *results;
    size_t results_row_stride;
    int direct; /* kernels write the caller's matrix in place */
    void *device_results;
    size_t device_stride;
    double started, phase_started, phases[6];
    int trace;
    int ranges; /* roctx ranges currently open for this call: 0, 1 (the call) or 2 (the call and a phase) */
    char const **error_message;
} szs_call_t;

/** engine->pinned_summary: the words the device leaves for the host during a call.  The offsets are fixed (the asserts below): a
 *  field that grows into the next one fails the build. */
#define SZS_PINNED_WORDS_BYTES 2048u
typedef struct szs_pinned_words_t {
    szs_plan_summary_t summary;                 /* the device planner's (hip/planner.hip) */
    uint8_t unused_0[16];
    unsigned long long plan_timestamps[8];      /* SZS_PLAN_TIMESTAMPS builds: the planner's phases */
    uint64_t stall_flag;                        /* a chained tier's, copied from its control block (szs_call_finish) */
    uint8_t unused_1[248];
    uint32_t stale;                             /* same tapes: a guarded ref met offsets that changed (szs_ref_guard_t) */
    uint8_t unused_2[124];
    uint32_t presence[8];                       /* the bytes that occur in a batch of a non-unit Levenshtein engine */
    uint8_t unused_3[32];
    uint32_t queue_unfit;                       /* the one-launch kernel met a query it has no table for */
    uint8_t unused_4[12];
    unsigned long long tiny_symbols[2];         /* the tiny-token launch: both sides' totals of symbols ... */
    uint32_t tiny_unfit;                        /* ... and its refusal */
    uint8_t unused_5[28];
    szs_fused_side_report_t fused_reports[2];   /* the launch that plans itself (szs_fused_plan_t) ... */
    uint32_t fused_gave_up;                     /* ... and a workgroup of it that ran out of polls */
} szs_pinned_words_t;
_Static_assert(offsetof(szs_pinned_words_t, plan_timestamps) == SZS_PLAN_TIMESTAMPS_AT, "the planner's summary runs into its timestamps");
_Static_assert(offsetof(szs_pinned_words_t, stall_flag) == 512, "pinned words moved");
_Static_assert(offsetof(szs_pinned_words_t, stale) == 768, "pinned words moved");
_Static_assert(offsetof(szs_pinned_words_t, presence) == 896, "pinned words moved");
_Static_assert(offsetof(szs_pinned_words_t, queue_unfit) == 960, "pinned words moved");
_Static_assert(offsetof(szs_pinned_words_t, tiny_symbols) == 976, "pinned words moved");
_Static_assert(offsetof(szs_pinned_words_t, tiny_unfit) == 992, "pinned words moved");
_Static_assert(offsetof(szs_pinned_words_t, fused_reports) == 1024, "pinned words moved");
_Static_assert(sizeof(szs_pinned_words_t) <= SZS_PINNED_WORDS_BYTES, "the pinned words outgrew their page");

/** engine->device_fused: device memory, zeroed when allocated and after a failed call, never by a launch (szs_call_reserve_device_words). */
typedef struct szs_device_words_t {
    uint32_t ready[48];   /* the launch that plans itself: ready[0] and ready[32], one word a side (szs_fused_plan_t); ready[0 .. 1] are
                             ONE 64-bit word - the sequence below, the query side's pairing rule above */
    uint32_t verdicts[8]; /* the two-workgroup planner's (szs_hip_plan) */
    uint32_t unused[8];
} szs_device_words_t;
_Static_assert(offsetof(szs_device_words_t, verdicts) == 48 * sizeof(uint32_t) && sizeof(szs_device_words_t) == 256, "device words moved");
_Static_assert(offsetof(szs_device_words_t, ready) % 8 == 0, "the query side's ready word is read as 64 bits");

static inline szs_pinned_words_t volatile *szs_pinned_words(szs_engine_s const *engine) {
    return (szs_pinned_words_t volatile *)engine->pinned_summary.pointer;
}
static inline szs_device_words_t *szs_device_words(szs_engine_s const *engine) { return (szs_device_words_t *)engine->device_fused.pointer; }

/* the tiny-token memory of one family (szs_engine_s::tiny) */
static inline void szs_tiny_note(szs_tiny_memory_t *memory, int valid, uint32_t q_count, uint32_t c_count) {
    memory->valid = valid, memory->q_count = q_count, memory->c_count = c_count;
}
static inline void szs_tiny_forget(szs_tiny_memory_t *memory) { memory->valid = 0; }
static inline int szs_tiny_counts_match(szs_tiny_memory_t const *memory, uint32_t q_count, uint32_t c_count) {
    return memory->q_count == q_count && memory->c_count == c_count;
}

/* internal statuses: how a way says "not me" */
#define SZS_NOT_DEVICE_PLANNABLE ((sz_status_t)1) /* internal: take the host-planned path instead */
#define SZS_TINY_NOT_TAKEN ((sz_status_t)3) /* internal: score the call the ordinary way */
#define SZS_WAY_NOT_TAKEN ((sz_status_t)4)
#define SZS_RUNES_ARE_BYTES ((sz_status_t)2) /* internal: the corpus is ASCII - the byte engines compute the same distances */

/* dispatch.c */
sz_status_t szs_call_decide(szs_engine_s const *engine, int symmetric, int runes, int force_lanes, szs_side_stats_t const *q_stats, szs_side_stats_t const *c_stats, uint32_t const *q_variants, uint32_t const *c_variants, uint32_t const (*ranks)[SZS_PLAN_RANK_SAMPLES + 1] /* the caller's sides, or NULL: not known yet */, uint64_t cells, szs_decision_t *d, char const **error_message);
void szs_call_decide_queue(szs_engine_s const *engine, szs_decision_t *d, uint32_t const (*ranks)[SZS_PLAN_RANK_SAMPLES + 1]);
int szs_decision_has_variant_zero(szs_decision_t const *d);
int szs_decision_is_one_launch(szs_decision_t const *d);
sz_status_t szs_call_prepare(szs_engine_s *engine, szs_decision_t const *d, int device, hipStream_t stream, char const **error_message);
hipError_t szs_call_enqueue(szs_engine_s *engine, szs_decision_t const *d, int device, szs_string_ref_t const *query_refs, szs_string_ref_t const *candidate_refs, void *device_results, size_t device_stride, hipStream_t stream, szs_ref_guard_t const *guard /* refs of an earlier call: validate in the kernels; else NULL */, uint32_t *launches, uint32_t *cell_bits, sz_status_t *status, char const **error_message);
void szs_call_phase(szs_call_t *call, int index);
sz_status_t szs_call_finish(szs_call_t *call, szs_decision_t const *d, hipError_t error, sz_status_t status, uint32_t launches, uint32_t cell_bits, uint64_t query_symbols, uint64_t candidate_symbols, int *stalled);
sz_status_t szs_call_place_results(szs_call_t *call);
void szs_call_stamp_refs(szs_decision_t *remembered, void const *const data[2], void const *const offsets[2], int const wide[2], szs_plan_summary_t const *summary);
sz_status_t szs_call_reserve_device_words(szs_engine_s *engine, int device, hipStream_t stream, char const **error_message);

/* ways_tiny.c */
int szs_tiny_shaped(szs_engine_s const *engine, int symmetric, szs_side_stats_t const *queries, szs_side_stats_t const *candidates);
int szs_tiny_recently_refused(szs_engine_s *engine, uint32_t q_count, uint32_t c_count, int count_down);
sz_status_t szs_cross_tiny(szs_call_t *call, uint32_t planner_mode, szs_plan_summary_t const *seen /* or NULL */, int runes);
/* ways_planned.c: `runes` - a codepoint call (transcoded, planned on rune counts; SZS_RUNES_ARE_BYTES: score it as bytes instead) */
sz_status_t szs_cross_device_planned(szs_call_t *call, int runes);

#endif /* SZS_DISPATCH_INTERNAL_H_ */
