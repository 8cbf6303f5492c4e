"""What `clusters` must return (`szs_rocm_clusters*`, `szs_rocm_fingerprint_clusters`), in plain numpy and
Python: no GPU, no library.  `expected_labels` is a host union-find over a matrix of hits; `run_model` is the device's `find` / `unite`
(csrc/hip/clusters.hip), lane by lane under a seeded scheduler that also feeds the lanes STALE loads - the model of a vector L1 that no
other CU's store refreshes.  tests/test_clusters_model.py checks the termination argument there, the GPU tests check the calls."""
import random

import numpy as np

from within_cases import UNTOUCHED, hits_of  # noqa: F401  (the bounded searches' predicate is this call's edge)


def expected_labels(hits):
    """labels[i] = the smallest index of the connected component of i in the undirected graph `hits | hits.T`, diagonal cleared."""
    hits = np.asarray(hits, dtype=bool)
    n = hits.shape[0]
    assert hits.shape == (n, n)
    edges = (hits | hits.T) & ~np.eye(n, dtype=bool)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in zip(*np.nonzero(np.triu(edges))):
        a, b = find(int(i)), find(int(j))
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], dtype=np.uint64)


def labels_of_matrix(matrix, bound, descending):
    """`expected_labels` of the full self-matrix of scores under `within`'s predicate."""
    return expected_labels(hits_of(matrix, bound, descending, self_search=True))


# ---- the device's forest, one memory operation at a time ------------------------------------------------------------------------------


class Forest:
    """`parent`, with every value each word has ever held: what a stale load may still return."""

    def __init__(self, n):
        self.n = n
        self.history = [[x] for x in range(n)]

    def now(self, x):
        return self.history[x][-1]

    def store(self, x, value):
        """Every store, checked as it lands: the two halves of the invariant hold after every step."""
        assert value <= x, f"parent[{x}] = {value}: every value ever stored to parent[x] is <= x"
        assert self.now(x) == x or value != x, f"parent[{x}] = {x}: a non-root never becomes a root again"
        self.history[x].append(value)

    def swap(self, x, expected, value):
        """The compare-and-swap as L2 decides it: on the current value, which it returns."""
        old = self.now(x)
        if old == expected:
            self.store(x, value)
        return old

    def parents(self):
        return [self.now(x) for x in range(self.n)]


def find_steps(x):
    """The operations of `find(x)`: yields ("load", address) / ("store", address, value), is sent what a load returned, returns the
    root and the turns of its loop."""
    turns = 0
    while True:
        p = yield ("load", x)
        if p == x:
            return x, turns
        turns += 1
        g = yield ("load", p)
        if g != p:
            yield ("store", x, g)
        x = p


def unite_steps(a, b, bound):
    """The operations of `unite(a, b)`; asserts that neither loop exceeds `bound` turns."""
    turns = 0
    while True:
        turns += 1
        assert turns <= bound, f"unite took more than {bound} turns"
        a, walked = yield from find_steps(a)
        assert walked <= bound, f"find took more than {bound} turns"
        b, walked = yield from find_steps(b)
        assert walked <= bound, f"find took more than {bound} turns"
        if a == b:
            return
        if a < b:
            a, b = b, a
        old = yield ("swap", a, a, b)
        if old == a:
            return
        assert old < a, "a failed swap strictly lowers a"
        a = old


def run_model(n, edges, seed, stale=True):
    """Runs one lane per edge (i, j) - `unite(i, j)` - to completion, advancing a random lane by ONE memory operation at a time.  A load
    returns any value its word has held since the lane first touched it (`stale`), a swap acts on the current value.  `Forest.store`
    checks the invariant on every store as it lands.  Returns the parents."""
    rng = random.Random(seed)
    forest = Forest(n)
    lanes = []
    for i, j in edges:
        steps = unite_steps(i, j, n)
        lanes.append({"steps": steps, "request": next(steps), "first": {}})
    while lanes:
        lane = lanes[rng.randrange(len(lanes))]
        request, address = lane["request"], lane["request"][1]
        first = lane["first"].setdefault(address, len(forest.history[address]) - 1)
        if request[0] == "load":
            held = forest.history[address]
            answer = held[rng.randrange(first, len(held))] if stale else held[-1]
        elif request[0] == "store":
            assert forest.now(address) != address, "a halving store never writes a root: it saw a parent below it"
            forest.store(address, request[2])
            answer = None
        else:
            answer = forest.swap(address, request[2], request[3])
        try:
            lane["request"] = lane["steps"].send(answer)
        except StopIteration:
            lanes.remove(lane)
    return forest.parents()


def finish(parents):
    """The finish kernel: labels[i] = the root of i by a read-only walk, and the number of roots."""
    labels = []
    for x in range(len(parents)):
        steps = 0
        while parents[x] != x:
            x, steps = parents[x], steps + 1
            assert steps <= len(parents)
        labels.append(x)
    return np.array(labels, dtype=np.uint64), sum(1 for x, p in enumerate(parents) if p == x)


def adversarial_graphs():
    """(name, n, directed edges as the lanes receive them)"""
    chain = 24
    clique = 7
    two = [(i, j) for i in range(6) for j in range(6) if i != j] + [(6 + i, 6 + j) for i in range(6) for j in range(6) if i != j]
    return [
        ("chain in descending order", chain, [(i, i - 1) for i in range(chain - 1, 0, -1)]),
        ("chain, both directions", chain, [(i, i + 1) for i in range(chain - 1)] + [(i + 1, i) for i in range(chain - 1)]),
        ("star around the last node", 20, [(19, i) for i in range(19)] + [(i, 19) for i in range(19)]),
        ("star around node 0", 20, [(i, 0) for i in range(1, 20)]),
        ("clique", clique, [(i, j) for i in range(clique) for j in range(clique) if i != j]),
        ("two cliques joined by one edge", 12, two + [(11, 0)]),
    ]


def hits_of_edges(n, edges):
    hits = np.zeros((n, n), dtype=bool)
    for i, j in edges:
        hits[i, j] = True
    return hits
