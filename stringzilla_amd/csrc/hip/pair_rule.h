/*
 *  pair_rule.h - which two queries share a workgroup of the short launch that plans itself (hip/lev_myers.hip), in plain C
 *  that the sorting workgroup, the scoring workgroups and the host (szs_rocm_pair_rule_probe) all compile: one text, one rule.
 *
 *  The Q queries of a call are ranked by DESCENDING length; slots = ceil(Q / 2) workgroup slots take one query each from the
 *  longer half (rank s) and n = Q - slots of them a second one from the shorter half:
 *
 *      rule 0          slot s < n takes ranks s and slots + s                              (longest with median: sums fall with s)
 *      rule delta + 1  slot s < n takes ranks s and slots + ((n - 1 - s + delta) mod n)    (longest with shortest, shifted by delta)
 *
 *  A slot s >= n (the middle query of an odd count) has no second query.  For every rule s -> second is a bijection of [0, n)
 *  onto [slots, Q): every rank sits in exactly one slot.  A pair shares ONE bit-vector of ceil((a + b + 2) / 32) words when that
 *  is no wider than the two apart and at most SZS_PAIR_WORDS_MOST; else the two run one after the other.  The rows a vector
 *  holds beyond a + b + 2 are idle, so the sorter evaluates rule 0 and SZS_PAIR_RULE_SHIFTS evenly spaced shifts and publishes the
 *  rule with the fewest words over all slots (ties: rule 0, then the smallest shift).
 *
 *  Includes nothing; the includer may define SZS_PAIR_RULE_FN (the device: `__host__ __device__ static inline`).
 */
#ifndef SZS_PAIR_RULE_H_
#define SZS_PAIR_RULE_H_

#ifndef SZS_PAIR_RULE_FN
#define SZS_PAIR_RULE_FN static inline
#endif

#define SZS_PAIR_WORDS_MOST 10u  /* the widest bit-vector of two queries */
#define SZS_PAIR_RULE_SHIFTS 16u /* candidate shifts: delta_k = k n / 16, k = 0 ... 15 */
#define SZS_PAIR_RULE_CANDIDATES (SZS_PAIR_RULE_SHIFTS + 1u)

/** Words of one query alone (an empty one still takes a word). */
SZS_PAIR_RULE_FN unsigned szs_pair_words_alone(unsigned length) { return length ? (length + 31u) / 32u : 1u; }

/** Words of the two lengths in one vector: their rows and a separator row behind each. */
SZS_PAIR_RULE_FN unsigned szs_pair_words_shared(unsigned a, unsigned b) { return (a + b + 2u + 31u) / 32u; }

/** Do the two share a vector?  (`shared`, `words_a`, `words_b`: the three figures above.) */
SZS_PAIR_RULE_FN int szs_pair_shares(unsigned shared, unsigned words_a, unsigned words_b) {
    return shared <= words_a + words_b && shared <= SZS_PAIR_WORDS_MOST;
}

/** Words per text column a slot of the two lengths costs. */
SZS_PAIR_RULE_FN unsigned szs_pair_slot_words(unsigned a, unsigned b) {
    unsigned const words_a = szs_pair_words_alone(a), words_b = szs_pair_words_alone(b), shared = szs_pair_words_shared(a, b);
    return szs_pair_shares(shared, words_a, words_b) ? shared : words_a + words_b;
}

/** Slots of `count` queries, and how many of them hold a second query. */
SZS_PAIR_RULE_FN unsigned szs_pair_slots(unsigned count) { return (count + 1u) / 2u; }
SZS_PAIR_RULE_FN unsigned szs_pair_seconds(unsigned count) { return count - (count + 1u) / 2u; }

/** Candidate k of SZS_PAIR_RULE_CANDIDATES as a rule: 0, then 1 + the k-th of the evenly spaced shifts of n. */
SZS_PAIR_RULE_FN unsigned szs_pair_rule_candidate(unsigned k, unsigned seconds) {
    return k ? 1u + (k - 1u) * seconds / SZS_PAIR_RULE_SHIFTS : 0u;
}

/** The descending rank of slot `slot`'s second query; requires slot < seconds (so seconds > 0) and rule <= seconds. */
SZS_PAIR_RULE_FN unsigned szs_pair_second_rank(unsigned rule, unsigned slot, unsigned slots, unsigned seconds) {
    if (!rule) return slots + slot;
    unsigned const shifted = seconds - 1u - slot + (rule - 1u); /* both terms below `seconds`: one subtraction is the modulo */
    return slots + (shifted >= seconds ? shifted - seconds : shifted);
}

#endif /* SZS_PAIR_RULE_H_ */
