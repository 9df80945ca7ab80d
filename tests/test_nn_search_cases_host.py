"""The premises of tests/nn_search_cases.py, proven on the host (no GPU): fp32 evaluates every squared distance of every case exactly in
three summation orders, the ties are there, and the case list reaches every kernel instance of nn::launch."""
import numpy as np
import pytest

import nn_search_cases as NC

CASES = NC.cases()
BY_WIDTH = {n: [c for c in CASES if c.n == n] for n in NC.WIDTHS}


def _fp32_distances(table, query):
    """|q - t|^2 in np.float32 only, summed forwards, backwards and pairwise: three (Q, N) float32 arrays."""
    d = query[:, None, :] - table[None, :, :]
    sq = d * d
    assert d.dtype == np.float32 and sq.dtype == np.float32
    n = sq.shape[2]
    fwd = np.zeros(sq.shape[:2], np.float32)
    bwd = np.zeros(sq.shape[:2], np.float32)
    for c in range(n):
        fwd = fwd + sq[:, :, c]
        bwd = bwd + sq[:, :, n - 1 - c]
    level = [sq[:, :, c] for c in range(n)]
    while len(level) > 1:
        level = [level[i] + level[i + 1] if i + 1 < len(level) else level[i] for i in range(0, len(level), 2)]
    assert fwd.dtype == bwd.dtype == level[0].dtype == np.float32
    return fwd, bwd, level[0]


@pytest.mark.parametrize("n", NC.WIDTHS)
def test_fp32_is_exact_and_ties_are_present(n):
    for case in BY_WIDTH[n]:
        table, query = NC.make(case)
        assert table.shape == (case.N, n) and query.shape == (case.Q, n) and table.dtype == query.dtype == np.float32
        assert np.array_equal(table, np.round(table)) and np.abs(table).max() <= 8
        assert np.array_equal(query - 0.25, np.round(query - 0.25)) and np.abs(query - 0.25).max() <= 8
        d64 = ((query[:, None, :].astype(np.float64) - table[None, :, :].astype(np.float64)) ** 2).sum(-1)
        for name, d32 in zip(("forwards", "backwards", "pairwise"), _fp32_distances(table, query)):
            assert np.array_equal(d32.astype(np.float64), d64), (NC.case_id(case), name)
        D, I = NC.expected(case, table, query)
        kk = min(case.k, case.N)
        assert np.array_equal(D[:, :kk], np.take_along_axis(d64, I[:, :kk], 1))          # the oracle's distances are those values
        assert np.array_equal(D.astype(np.float32).astype(np.float64), D)                  # and fp32 holds them
        if case.N >= 2:                                                                    # (one row cannot tie)
            from oracle import np_oracle as O
            first = O.flat_l2_search(table, query, min(case.k + 1, case.N))[0]
            share = (np.diff(first, axis=1) == 0).any(1).mean()
            assert share >= 0.9, (NC.case_id(case), share)


def test_case_list_reaches_every_kernel_instance():
    """Every (layout, NQ form, K) instance of nn::launch, k = 3 on the four-deep list, and the shapes the case list promises."""
    assert len(CASES) == len(NC.WIDTHS) * 4 + len(NC.ONE_PER_LAYOUT) * 9
    inst = {(NC.layout(c.n), c.n > 10 if NC.layout(c.n) == 12 else None, 1 if c.k == 1 else (2 if c.k == 2 else 4)) for c in CASES if c.kind == "big"}
    want = {(d, f, K) for d in NC.LAYOUTS for f in ((False, True) if d == 12 else (None,)) for K in (1, 2, 4)}
    assert inst == want
    assert {c.n for c in CASES if c.k == 3 and c.kind == "big"} == set(NC.WIDTHS)
    assert {NC.layout(n) for n in NC.ONE_PER_LAYOUT} == set(NC.LAYOUTS) and {10, 11} <= set(NC.ONE_PER_LAYOUT)
    for n in NC.WIDTHS:
        ts, rpp = NC.tile_rows(n), NC.tile_rows(n) // NC.PARTS
        assert NC.big_rows(n) == {128: 306, 64: 154}[ts]
        tail = NC.big_rows(n) - 2 * ts
        per_part = [min(rpp, max(0, tail - p * rpp)) for p in range(NC.PARTS)]
        assert per_part == [rpp] * 3 + [2] + [0] * 4 and 2 % NC.JB != 0
    for n in NC.ONE_PER_LAYOUT:
        rpp = NC.tile_rows(n) // NC.PARTS
        assert {c.N for c in CASES if c.n == n and c.kind == "small"} == {1, 2, 3, 5, rpp - 1, rpp, rpp + 1}
        assert {c.Q for c in CASES if c.n == n} == {1, 32 * NC.owners(n) - 1, 32 * NC.owners(n) + 1}
    assert max(c.N for c in CASES) == 306
