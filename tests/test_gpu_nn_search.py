"""clica_nn_search (csrc/nn_search.hip) against oracle.np_oracle.flat_l2_search in every padded layout, list depth, launch plan and tie.

The data of tests/nn_search_cases.py make fp32 exact (proven per case on the host by test_nn_search_cases_host.py), so EVERY query and
EVERY column is compared: indices equal, distances bit-equal, no tolerance and nothing left out.  Under the product plan these small
tables are cut into one LDS tile per workgroup and the merge kernel decides the ties between tiles; under
clica_set_tuning("lp_max_splits", 1) one workgroup streams all three tiles and the ties are decided on chip, across partitions,
half-waves and waves.  Both must give the oracle's answer, hence each other's, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import nn_search_cases as NC
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu

E_WORKSPACE = -2        # include/clica.h
CASES = NC.cases()
BY_WIDTH = {n: [c for c in CASES if c.n == n] for n in NC.WIDTHS}
_MEMO = {}


def _case(case):
    """(table, query, expected dist, expected idx) of a case, computed once for the whole file and never modified."""
    if case not in _MEMO:
        table, query = NC.make(case)
        D, I = NC.expected(case, table, query)
        for a in (table, query, D, I):
            a.setflags(write=False)
        _MEMO[case] = (table, query, D, I)
    return _MEMO[case]


def _search(table, query, k, want_dist=True):
    from cl_ica_amd import ops
    tab = table if torch.is_tensor(table) else torch.tensor(table, device="cuda")
    qry = query if torch.is_tensor(query) else torch.tensor(query, device="cuda")
    dist, idx = ops.nn_search(tab, qry, k, want_dist=want_dist)
    assert idx.shape == (qry.shape[0], k) and idx.dtype == torch.int64
    return (dist.cpu().numpy() if want_dist else None), idx.cpu().numpy()


def _exact(case, dist, idx, D, I, what):
    bad = np.argwhere(idx != I)
    assert bad.size == 0, (what, NC.case_id(case), "first wrong (query, column)", bad[0], "got", idx[bad[0][0]], "want", I[bad[0][0]])
    assert dist.dtype == np.float32 and np.array_equal(dist.astype(np.float64), D), (what, NC.case_id(case))


@pytest.fixture
def split_cap(request):
    """set(k): clica_set_tuning("lp_max_splits", k) for the rest of one test; 0 (the product plan) afterwards."""
    from cl_ica_amd import _lib
    lib = _lib.load()

    def set_cap(k):
        _lib.check(lib.clica_set_tuning(b"lp_max_splits", int(k)), "clica_set_tuning")
    request.addfinalizer(lambda: set_cap(0))
    return set_cap


# ====================================================================================================================== the case list
@pytest.mark.parametrize("n", NC.WIDTHS)
def test_product_plan_every_case(n):
    for case in BY_WIDTH[n]:
        table, query, D, I = _case(case)
        dist, idx = _search(table, query, case.k)
        _exact(case, dist, idx, D, I, "product plan")


@pytest.mark.parametrize("n", NC.WIDTHS)
def test_one_split_every_big_case(n, split_cap):
    """The three-tile tables again with one workgroup per query tile; equal to the oracle and, bit for bit, to the product plan's result."""
    big = [c for c in BY_WIDTH[n] if c.kind == "big"]
    assert len(big) >= 4
    product = [_search(*_case(c)[:2], c.k) for c in big]
    split_cap(1)
    for case, (pd, pi) in zip(big, product):
        table, query, D, I = _case(case)
        dist, idx = _search(table, query, case.k)
        _exact(case, dist, idx, D, I, "one split")
        assert np.array_equal(idx, pi) and np.array_equal(dist.view(np.uint32), pd.view(np.uint32)), NC.case_id(case)


@pytest.mark.parametrize("n", NC.ONE_PER_LAYOUT)
def test_fewer_rows_than_k(n):
    """N < k: the missing columns are -1 at distance +inf (include/clica.h), the present ones the whole table in order."""
    for N in (1, 2, 3):
        for k in range(N + 1, 5):
            case = NC.Case(n, k, N, 32 * NC.owners(n) + 1, "small")
            table, query, D, I = _case(case)
            assert (I[:, N:] == -1).all() and np.isposinf(D[:, N:]).all() and (I[:, :N] >= 0).all()
            dist, idx = _search(table, query, k)
            _exact(case, dist, idx, D, I, "N < k")


# ====================================================================================================================== the call's forms
def _padded(a, pad=3):
    """`a` as a view with leading dimension n + pad of a buffer whose padding columns hold NaN."""
    buf = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), device="cuda")
    buf[:, :a.shape[1]] = torch.tensor(a, device="cuda")
    view = buf[:, :a.shape[1]]
    assert view.stride(0) == a.shape[1] + pad and view.stride(1) == 1
    return view


@pytest.mark.parametrize("n", NC.ONE_PER_LAYOUT)
def test_leading_dimensions_keep_the_bits(n, split_cap):
    """Table and query with leading dimension n + 3 and NaN in the padding columns, under both plans: the bits of the contiguous call."""
    case = NC.Case(n, 3, NC.big_rows(n), 32 * NC.owners(n) + 1, "big")
    table, query, D, I = _case(case)
    for cap in (0, 1):
        split_cap(cap)
        dist0, idx0 = _search(table, query, case.k)
        _exact(case, dist0, idx0, D, I, f"contiguous, cap {cap}")
        dist, idx = _search(_padded(table), _padded(query), case.k)
        assert np.array_equal(idx, idx0) and np.array_equal(dist.view(np.uint32), dist0.view(np.uint32)), (n, cap)


@pytest.mark.parametrize("n", NC.ONE_PER_LAYOUT)
def test_without_distances_same_rows(n):
    for k in NC.KS:
        case = NC.Case(n, k, NC.big_rows(n), 32 * NC.owners(n) + 1, "big")
        table, query, D, I = _case(case)
        none, idx = _search(table, query, k, want_dist=False)
        assert none is None and np.array_equal(idx, I), (n, k)


@pytest.mark.parametrize("n", NC.ONE_PER_LAYOUT)
def test_c_abi_workspace_exact_and_one_byte_short(n):
    """clica_nn_search with a workspace of exactly the reported size carved out of a larger buffer (the sentinel behind it stays), and one
    byte short: CLICA_E_WORKSPACE with idx and dist unwritten."""
    from cl_ica_amd import _lib
    lib = _lib.load()
    case = NC.Case(n, 4, NC.big_rows(n), 32 * NC.owners(n) + 1, "big")
    table, query, D, I = _case(case)
    tab, qry = torch.tensor(table, device="cuda"), torch.tensor(query, device="cuda")
    need = C.c_size_t()
    assert lib.clica_nn_search_workspace_bytes(case.Q, case.N, n, case.k, C.byref(need)) == 0 and need.value > 0
    tail = 4096
    ws = torch.full((need.value + tail,), 0xA5, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0

    def call(nbytes):
        idx = torch.full((case.Q, case.k), -77, dtype=torch.int64, device="cuda")
        dist = torch.full((case.Q, case.k), -77.0, device="cuda")
        rc = lib.clica_nn_search(tab.data_ptr(), n, case.N, qry.data_ptr(), n, case.Q, n, case.k, idx.data_ptr(), dist.data_ptr(), ws.data_ptr(),
                                 nbytes, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, dist.cpu().numpy(), idx.cpu().numpy()

    rc, dist, idx = call(need.value - 1)
    assert rc == E_WORKSPACE and b"workspace" in lib.clica_last_error()
    assert (idx == -77).all() and (dist == -77.0).all() and bool((ws == 0xA5).all())            # nothing ran
    rc, dist, idx = call(need.value)
    assert rc == 0
    _exact(case, dist, idx, D, I, "exact workspace")
    assert bool((ws[need.value:] == 0xA5).all())                                                  # nothing written behind it


# ====================================================================================================================== non-finite rows
@pytest.mark.parametrize("n", NC.ONE_PER_LAYOUT)
def test_non_finite_rows(n, split_cap):
    """include/clica.h: a row with a NaN coordinate is never returned; a row with an infinite coordinate only when fewer than k rows at
    finite distance exist.  Under both plans: with such rows put into the table, every answer is that of the table without them."""
    case = NC.Case(n, 4, NC.big_rows(n), 32 * NC.owners(n) + 1, "big")
    table, query, D, I = _case(case)
    rpp = NC.tile_rows(n) // NC.PARTS
    # the best row of query 0, a row inside a full group of four, one in the ragged partition of the last tile, the last row
    nan_rows = np.array(sorted({int(I[0, 0]), 5, 2 * NC.tile_rows(n) + 3 * rpp, case.N - 1}))
    inf_rows = np.array(sorted(set((nan_rows + 1) % case.N) - set(nan_rows)))
    bad = table.copy()
    bad[nan_rows, (nan_rows * 7) % n] = np.nan
    bad[inf_rows, (inf_rows * 5) % n] = np.where(inf_rows % 2 == 0, np.inf, -np.inf)
    keep = np.setdiff1d(np.arange(case.N), np.concatenate([nan_rows, inf_rows]))
    Dk, Ik = O.flat_l2_search(table[keep], query, case.k)
    for cap in (0, 1):
        split_cap(cap)
        dist, idx = _search(bad, query, case.k)
        assert np.array_equal(idx, keep[Ik]) and np.array_equal(dist.astype(np.float64), Dk), (n, cap)
    split_cap(0)
    # fewer than k finite rows: the finite ones come first, in order; what follows is an infinite row at distance +inf or -1, never the NaN row
    few = table[:4].copy()
    few[1, 0] = np.nan
    few[2, n - 1] = np.inf
    dist, idx = _search(few, query, 4)
    Df, If = O.flat_l2_search(few[[0, 3]], query, 2)
    assert np.array_equal(idx[:, :2], np.array([0, 3])[If]) and np.array_equal(dist[:, :2].astype(np.float64), Df)
    assert np.isin(idx[:, 2:], (2, -1)).all() and np.isposinf(dist[:, 2:]).all() and (idx[:, 3] == -1).all()


# ====================================================================================================================== the snap rule
def test_snap_on_a_table_of_duplicates():
    """ThreeDIdentLatentPairs.snap against oracle.np_oracle.threedident_snap where every grid row exists twice: z sits exactly on a grid
    row (distance 0 to it and to its duplicate: the lower one is index_z), z~ is equidistant to that row and its duplicate, so the
    "closest row that differs from index_z" is decided by the tie order of both searches."""
    from cl_ica_amd import latent_spaces, spaces
    from cl_ica_amd.datasets import ThreeDIdentLatentPairs
    n = 10
    rng = np.random.default_rng(10)
    block = np.unique(rng.integers(-8, 9, size=(400, n)), axis=0)[:153]
    assert len(block) == 153
    table = block[rng.permutation(np.tile(np.arange(153), 2))].astype(np.float32)              # 306 rows, every row twice, scattered
    space = spaces.NBoxSpace(n, -8.0, 8.0)
    ls = latent_spaces.LatentSpace(space, lambda sp, size, device="cuda": sp.uniform(size, device=device),
                                   lambda sp, z, size, device="cuda": sp.normal(z, 0.05, size, device=device))
    ds = ThreeDIdentLatentPairs(table, ls)
    pick = rng.permutation(306)[:65]
    z = table[pick]
    zt = (z + 0.25).astype(np.float32)
    oz, ozt = O.threedident_snap(table, z, zt)
    first = np.array([np.flatnonzero((table == row).all(1)) for row in z])                     # the two copies of every z, ascending
    assert first.shape == (65, 2) and np.array_equal(oz, first[:, 0]) and np.array_equal(ozt, first[:, 1])
    iz, izt, gz, gzt = ds.snap(torch.tensor(z, device="cuda"), torch.tensor(zt, device="cuda"))
    assert iz.dtype == torch.int64 and np.array_equal(iz.cpu().numpy(), oz) and np.array_equal(izt.cpu().numpy(), ozt)
    assert np.array_equal(gz.cpu().numpy(), z) and np.array_equal(gzt.cpu().numpy(), z)
