"""Cases for clica_nn_search (csrc/nn_search.hip) on which fp32 is EXACT, with ties on purpose; shared by the host proof
(test_nn_search_cases_host.py) and the GPU comparison (test_gpu_nn_search.py).

Exact data.  Table coordinates are integers in [-8, 8], query coordinates integers in [-8, 8] plus 0.25.  Every difference is a multiple
of 1/4 of magnitude <= 16.25, every square a multiple of 1/16 and <= 264.0625, a sum of up to 64 of them is below 2^24 / 16: every
partial sum in any order, fused or not, is representable, so every fp32 evaluation gives the fp64 value.  The expectation is therefore
compared with NO column left out and NO tolerance: indices equal, distances bit-equal.

Ties.  A table is a block of distinct random integer rows, each present three times (two times for the at most two rows that make the
row count fit), in a seeded shuffled order: the best rows of every query are tied at scattered positions, and the stable argsort of
oracle.np_oracle.flat_l2_search (ties to the lower row) decides.  For n <= 2 there are too few distinct rows for "distinct": the small
range alone gives tens of duplicates per value there.

The launcher's geometry, restated from csrc/lp_kernels.h / nn_search.hip (a change there must be followed here by hand): eight padded
layouts, R = 2 query rows per lane up to the 24-wide one, tiles of 128 rows up to the 40-wide one and of 64 at 64, eight on-chip
partitions of RPP = TS / 8 rows per tile, JB = 4 rows per inner step, lists of K = 1, 2 or 4 candidates (k = 3 emits three of four)."""
from collections import namedtuple

import numpy as np

LAYOUTS = (4, 8, 12, 16, 24, 32, 40, 64)
WIDTHS = (1, 2, 4, 5, 8, 9, 10, 11, 12, 13, 16, 17, 24, 25, 32, 33, 40, 41, 63, 64)     # both ends of every layout, both NQ forms of 12
KS = (1, 2, 3, 4)
# one width per kernel instance: the eight layouts, the 12-wide one in both forms (NQ = 5: n = 10, NQ = 6: n = 11)
ONE_PER_LAYOUT = (2, 5, 10, 11, 13, 17, 25, 33, 63)
PARTS, JB = 8, 4

Case = namedtuple("Case", "n k N Q kind")


def layout(n):
    return next(d for d in LAYOUTS if n <= d)


def owners(n):
    return 2 if layout(n) <= 24 else 1


def tile_rows(n):
    return 128 if layout(n) <= 40 else 64


def big_rows(n):
    """2 TS + 3 RPP + 2: two full tiles, then a ragged one with three full partitions, one of 2 rows (not a multiple of JB), four empty."""
    ts = tile_rows(n)
    return 2 * ts + 3 * (ts // PARTS) + 2


def case_id(c):
    return f"n{c.n}-k{c.k}-N{c.N}-Q{c.Q}"


def cases():
    """Every case, in a fixed order.  kind "big": N = 2 TS + 3 RPP + 2 (these also run under one split); "small": a table below or around
    one partition."""
    out = []
    for n in WIDTHS:
        for k in KS:
            out.append(Case(n, k, big_rows(n), 32 * owners(n) + 1, "big"))          # a second query tile holding one query
    for a, n in enumerate(ONE_PER_LAYOUT):
        rpp = tile_rows(n) // PARTS
        for b, N in enumerate((1, 2, 3, 5, rpp - 1, rpp, rpp + 1)):
            out.append(Case(n, KS[(a + b) % 4], N, 32 * owners(n) + 1, "small"))
        for b, Q in enumerate((1, 32 * owners(n) - 1)):
            out.append(Case(n, KS[(a + b + 1) % 4], big_rows(n), Q, "big"))
    assert len(set(out)) == len(out)
    return out


def make(case):
    """(table [N, n], query [Q, n]) float32, a function of the case alone."""
    n, N, Q = case.n, case.N, case.Q
    rng = np.random.default_rng([n, case.k, N, Q])
    m = -(-N // 3)
    if n <= 2:
        block = rng.integers(-8, 9, size=(m, n))
    else:
        block = np.unique(rng.integers(-8, 9, size=(4 * m + 8, n)), axis=0)
        assert len(block) >= m, (case, len(block))
        block = block[rng.permutation(len(block))[:m]]
    copies = np.tile(np.arange(m), 3)[:N]              # the 3 m - N <= 2 rows that lose a copy are different rows
    assert len(copies) == N
    table = block[rng.permutation(copies)].astype(np.float32)
    query = (rng.integers(-8, 9, size=(Q, n)) + 0.25).astype(np.float32)
    return table, query


def expected(case, table, query):
    """(dist [Q, k] float64, idx [Q, k] int64) of oracle.np_oracle.flat_l2_search; columns beyond the table's rows hold (+inf, -1), what
    include/clica.h states for them."""
    from oracle import np_oracle as O
    kk = min(case.k, case.N)
    D, I = O.flat_l2_search(table, query, kk)
    if kk < case.k:
        D = np.concatenate([D, np.full((case.Q, case.k - kk), np.inf)], 1)
        I = np.concatenate([I, np.full((case.Q, case.k - kk), -1, np.int64)], 1)
    return D, I
