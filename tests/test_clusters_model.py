"""The lock-free forest of csrc/hip/clusters.hip as a model (tests/clusters_cases.py): lanes advance one
memory operation at a time in a seeded random order, loads may be stale.  Whatever the schedule, every loop ends within n turns, every
value stored to parent[x] is <= x, no non-root becomes a root again, and the labels behind the finish walk are the host union-find's.
This is where the termination argument is checked - not on the GPU."""
import random

import numpy as np
import pytest

import clusters_cases as cases

SCHEDULES = 200


def _holds(n, edges, seeds, stale=True):
    want = cases.expected_labels(cases.hits_of_edges(n, edges))
    for seed in seeds:
        parents = cases.run_model(n, edges, seed, stale=stale)  # asserts the turn bounds and the invariant as it goes
        assert all(parents[x] <= x for x in range(n))
        labels, count = cases.finish(parents)
        assert np.array_equal(labels, want), (seed, labels, want)
        assert count == len(set(want.tolist())) and np.array_equal(labels[labels.astype(np.int64)], labels)


@pytest.mark.parametrize("graph", cases.adversarial_graphs(), ids=lambda graph: graph[0])
def test_adversarial_graphs_under_any_schedule(graph):
    _, n, edges = graph
    _holds(n, edges, range(SCHEDULES))


@pytest.mark.parametrize("density", [0.02, 0.08, 0.3])
def test_random_graphs_under_any_schedule(density):
    rng = random.Random(int(density * 100))
    seen = set()
    for graph in range(30):
        n = rng.randint(2, 40)
        edges = [(i, j) for i in range(n) for j in range(n) if i != j and rng.random() < density]
        _holds(n, edges, range(graph * 10, graph * 10 + 10))
        seen.add(len(set(cases.expected_labels(cases.hits_of_edges(n, edges)).tolist())) == 1)
    assert density != 0.08 or seen == {True, False}  # connected graphs and graphs of several components


def test_fresh_loads_give_the_same_labels():
    for _, n, edges in cases.adversarial_graphs():
        _holds(n, edges, range(20), stale=False)


def test_expected_labels():
    hits = np.zeros((7, 7), dtype=bool)
    hits[5, 2] = hits[2, 6] = hits[3, 1] = hits[4, 4] = True  # directed either way; a diagonal hit is no edge
    assert cases.expected_labels(hits).tolist() == [0, 1, 2, 1, 4, 2, 2]
    assert cases.expected_labels(np.zeros((0, 0), dtype=bool)).shape == (0,)
    assert cases.expected_labels(np.ones((4, 4), dtype=bool)).tolist() == [0, 0, 0, 0]
    scores = np.array([[0, 1, 9], [1, 0, 9], [9, 9, 0]], dtype=np.uint64)
    assert cases.labels_of_matrix(scores, 1, False).tolist() == [0, 0, 2]
    assert cases.labels_of_matrix(scores, -1, False).tolist() == [0, 1, 2]
    assert cases.labels_of_matrix(scores.astype(np.int64), 9, True).tolist() == [0, 0, 0]  # descending: scores >= 9 join 2 to both
