"""The cases of tests/chained_tier_cases.py are what they claim to be - from the CPU oracle alone, so that a later edit cannot
hollow them out: every listed length is in its grid, every planted optimum scores 5 a row and ends in the claimed cell, the
structured contents hold a band whose partial sum is negative before one where it is positive, and the large costs send
values far beyond 127 x 64 through the parked rows.  The same cases run on the hardware in tests/test_gpu_chained_tiers.py.
"""
import numpy as np
import pytest

import chained_tier_cases as cases


@pytest.mark.parametrize("tier", ["systolic", "chain"])
def test_every_listed_length_is_in_its_grid(tier):
    rows, columns = cases.grid_lengths(tier)
    listed = {"systolic": ((1, 7, 8, 9, 15, 16, 17, 504, 505, 511, 512, 513, 520, 1023, 1024, 1025, 1536, 1537),
                           (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 66, 67, 68, 127, 128, 129, 255, 256, 257, 319, 320, 321, 383, 384, 385)),
              "chain": ((1, 31, 32, 33, 63, 64, 65, 2016, 2017, 2047, 2048, 2049, 2080, 2081, 4095, 4096, 4097),
                        (1, 7, 8, 9, 15, 16, 17, 127, 128, 129, 135, 136, 137, 255, 256, 257, 639, 640, 641, 767, 768, 769))}[tier]
    queries, candidates = cases.grid(tier)
    assert tuple(map(len, queries)) == rows == listed[0] + (0,) and tuple(map(len, candidates)) == columns == listed[1] + (0,)
    runes = cases.grid("systolic", runes=True)
    if tier == "systolic":  # lengths count codepoints; all four widths occur
        assert tuple(len(text.decode()) for text in runes[0]) == rows and tuple(len(text.decode()) for text in runes[1]) == columns
        assert {len(rune.encode()) for rune in runes[0][-2].decode()} == {1, 2, 3, 4}
    band, word, step = (cases.SYSTOLIC_BAND, cases.SYSTOLIC_ROWS, cases.SYSTOLIC_COLUMNS) if tier == "systolic" else (
        cases.CHAIN_BAND, cases.CHAIN_WORD, cases.CHAIN_COLUMNS)
    chunk, steady = (cases.SYSTOLIC_CHUNK, cases.SYSTOLIC_FIRST_STEADY) if tier == "systolic" else (cases.CHAIN_CHUNK, cases.CHAIN_FIRST_STEADY)
    assert steady == 64 * step + chunk  # a chunk of 16 steps that starts at step 64 and ends inside the text
    for bands in (1, 2):  # a whole band, one row more (a last lane with 1 real row), one row less
        assert {bands * band - 1, bands * band, bands * band + 1} <= set(rows)
    assert max(rows) <= 4 * band and {m % word for m in rows} >= {0, 1, word - 1}
    # the ragged last step: one column, a whole step, one column short of it - and, at 4 columns a step, every remainder
    assert {n % step for n in columns} >= ({0, 1, step - 1} if tier == "chain" else set(range(step)))
    assert {chunk - 1, chunk, chunk + 1, steady - 1, steady, steady + 1, steady + chunk - 1, steady + chunk, steady + chunk + 1} <= set(columns)


@pytest.mark.parametrize("gaps", [(-4, -4), (-11, -2)], ids=["linear", "affine"])
@pytest.mark.parametrize("m", [1100, 1024])
def test_planted_optima_end_in_the_claimed_cells(m, gaps):
    batch = cases.planted(m)
    engine = cases.Engine("smith_waterman", "planted", gaps)
    whole = cases.expected(engine, batch.queries, batch.candidates)
    names = [placement.name for placement in batch.placements]
    assert len(set(names)) == len(names)
    for wanted in ["band 0", "band 1", "row 512", "row 513", "rows 507 ... 518", "the last row", "column 1", "columns 1 ... 12"] + [
            f"column n = {n}" for n in (201, 202, 203, 204)] + [f"row 513, column {c}" for c in (256, 257, 320, 321, 384, 385)]:
        assert wanted in names, wanted
    if m == 1100:
        assert {"the last band", "a lane with 1 real row", "a lane with 4 real rows", "a lane with 7 real rows"} <= set(names)
        real = {name: len(batch.queries[p.query]) - (p.last_row - 1) // 8 * 8 for name, p in zip(names, batch.placements) if name.startswith("a lane with")}
        assert all(rows == int(name.split()[3]) for name, rows in real.items()) and set(real.values()) == {1, 4, 7}, real
        assert len(batch.queries[0]) == 1100 and -(-1100 // cases.SYSTOLIC_BAND) == 3
    assert {len(batch.candidates[p.candidate]) % 4 for p in batch.placements if p.name.startswith("column n")} == {0, 1, 2, 3}
    oracle_of = lambda queries, candidates: cases.expected(engine, tuple(queries), tuple(candidates))
    # the same pairs without the optimum's last row, and without its last column
    above = oracle_of([batch.queries[p.query][: p.last_row - 1] for p in batch.placements], [batch.candidates[p.candidate] for p in batch.placements])
    left = oracle_of([batch.queries[p.query] for p in batch.placements], [batch.candidates[p.candidate][: p.last_column - 1] for p in batch.placements])
    upto = oracle_of([batch.queries[p.query][: p.last_row] for p in batch.placements], [batch.candidates[p.candidate][: p.last_column] for p in batch.placements])
    for index, p in enumerate(batch.placements):
        score = cases.MATCH * p.length
        assert whole[p.query, p.candidate] == score and upto[index, index] == score, (p, int(whole[p.query, p.candidate]))
        assert whole[p.query, p.candidate + 1] < score, p  # the control: the same background, no segment
        assert above[index, index] < score and left[index, index] < score, (p, int(above[index, index]), int(left[index, index]))
        assert p.last_row <= len(batch.queries[p.query]) and p.last_column <= len(batch.candidates[p.candidate])


def test_structured_contents_hold_runs_and_partial_sums_of_both_signs():
    unit = cases.Engine("levenshtein", None, (0, 1, 1, 1))
    partials, distances = {}, {}
    for m in cases.STRUCTURED_M:
        query, labels, candidates = cases.structured(m)
        assert labels[0] == "itself" and candidates[0] == query and not set(candidates[1]) & set(query)
        assert {f"shifted up by {s}" for s in (1, 31, 32, 33)} <= set(labels) and "every 64th byte replaced" in labels
        wanted = {length for length in (m - 1, m // 2, 2048, 2047) if length < m}
        assert {f"prefix of {length}" for length in wanted} | {f"suffix of {length}" for length in wanted} <= set(labels)
        cuts = list(range(cases.CHAIN_BAND, m, cases.CHAIN_BAND)) + [m]  # the rows where the chain's bands end
        down = cases.expected(unit, tuple(query[:cut] for cut in cuts), candidates)  # D[cut][n] per candidate
        for column, (label, text) in enumerate(zip(labels, candidates)):
            levels = [len(text)] + [int(down[row, column]) for row in range(len(cuts))]
            partials[m, label] = [after - before for before, after in zip(levels, levels[1:])]
            distances[m, label] = (levels[-1], max(m, len(text)))
    flat = [value for values in partials.values() for value in values]
    assert min(flat) < 0 < max(flat)
    assert any(before < 0 < after for values in partials.values() for before, after in zip(values, values[1:])), "no band hands a negative sum to a positive one"
    assert any(distance == 0 for distance, _ in distances.values()) and any(distance == longest for distance, longest in distances.values())
    for m in cases.STRUCTURED_M:  # the runs: a copy never moves, a foreign text costs a letter a column
        assert distances[m, "itself"][0] == 0 and distances[m, "foreign, as long"][0] == m and distances[m, "foreign, 9 longer"][0] == m + 9
        assert distances[m, "shifted up by 32"][0] <= 64 and distances[m, "every 64th byte replaced"][0] == m // 64


@pytest.mark.parametrize("engine", cases.LARGE_ENGINES, ids=lambda e: f"{e.kind}{e.costs}".replace(" ", ""))
def test_large_costs_travel_through_the_parked_rows(engine):
    queries, candidates = cases.large()
    assert tuple(map(len, queries)) == cases.LARGE_M == (9, 512, 513, 1025) and tuple(map(len, candidates)) == cases.LARGE_N == (5, 64, 65, 321)
    matrix = cases.expected(engine, queries, candidates)
    assert np.abs(matrix).max() > 127 * 64, int(np.abs(matrix).max())
    assert np.abs(matrix).max() < (1025 + 321 + 3) * 128  # the reach: far inside 32 bits
    if engine.table:
        _, table = cases.table_of(engine.table)
        assert {127, -127, -128, 0} == set(table.reshape(-1).tolist()) and not np.array_equal(table, table.T)
    # the value under a band's last row itself: the two-band queries against the piece that straddles row 512
    if engine.kind == "smith_waterman" and engine.costs[0] <= 0:
        assert matrix[1, 3] > 127 * 64 and matrix[2, 3] >= matrix[1, 3], (int(matrix[1, 3]), int(matrix[2, 3]))
        if engine.costs[0] == -128:  # no cheap gap to end the alignment elsewhere: it ends on row 512, and row 513 adds a match
            assert matrix[2, 3] == matrix[1, 3] + 127, (int(matrix[1, 3]), int(matrix[2, 3]))
