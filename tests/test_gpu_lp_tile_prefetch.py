"""The tile loop of the Lp loss sweeps (csrc/lp_kernels.h: Stager, the staged stream statistics) with MORE THAN ONE LDS tile per workgroup.

Under the product plan a workgroup's chunk of the pool only exceeds one tile from B ~ 2500 on, so the small shapes of the other files never
run the prefetch (tile t + 1 loaded while tile t is swept, stored behind it) nor a ragged tile that is not the first.  Here every case runs
with clica_set_tuning("lp_max_splits", 1): one workgroup per owner tile streams the whole pool -- 129 rows are two tiles with a one-row
tail, 256 and 384 exact multiples, 385 four tiles with a ragged last (tiles of 128 rows up to 40 coordinates, of 64 rows at 64).

Reference, data, floors and the 1e-5 bound are those of tests/test_gpu_train_pairs.py; test_inputs_hold_the_bound_in_plain_fp32 (no GPU)
shows that a plain fp32 evaluation of every case here sits within 2.5e-6 of fp64 and that max |lse| < 20: no allowance."""
import numpy as np
import pytest
import torch

from conftest import PARITY
from oracle import np_oracle as O
from test_gpu_loss import dev, grad_scale, run_hip, summand_floors
from test_gpu_train_pairs import LpPair, _lp_check, _lp_data, _lp_expect, _lp_id, _lp_run, _padded, _padding_untouched, _rows

gpu = pytest.mark.gpu


@pytest.fixture
def one_split(request):
    """lp_max_splits = 1 for one test, 0 (the product plan) afterwards.  The loss modules cache the workspace size per shape: sizes
    queried under the cap are dropped again, so that no later test meets one."""
    from cl_ica_amd import _lib, losses
    lib = _lib.load()

    def restore():
        _lib.check(lib.clica_set_tuning(b"lp_max_splits", 0), "clica_set_tuning")
        losses._WS_BYTES.clear()
    request.addfinalizer(restore)
    losses._WS_BYTES.clear()
    _lib.check(lib.clica_set_tuning(b"lp_max_splits", 1), "clica_set_tuning")


# ===================================================================================================================== cases
def _train_meta():
    """The training pair.  Rows 0-3: the headline form (n = 10 in the 12-wide layout, p = 2, pow) at every pool size; then every padded
    layout of the register sweeps (4, 12, 16, 24, 40, 64 wide) with p, pow and compat spread over them; last the pooled case (n = 12: the
    matrix cores take p = 2, pow, n <= 10 against a pool of >= 4 B rows, and this file is about the difference sweeps)."""
    rows = [  # B, B3, n, p, pow, compat, tau, alpha, local chunk
        (129, 129, 10, 2.0, 1, 1, 1.0, 0.5, 0), (256, 256, 10, 2.0, 1, 0, 0.5, 0.3, 0),
        (384, 384, 10, 2.0, 1, 1, 2.0, 0.8, 0), (385, 385, 10, 2.0, 1, 0, 1.0, 0.5, 0),
        (385, 385, 1, 1.0, 1, 1, 1.0, 0.5, 0), (129, 129, 12, 3.0, 1, 0, 0.5, 0.3, 0),
        (256, 256, 13, 1.5, 1, 1, 1.0, 0.8, 0), (384, 384, 17, 1.0, 0, 0, 2.0, 0.5, 0),
        (385, 385, 40, 2.0, 0, 1, 1.0, 0.3, 0), (129, 129, 64, 3.0, 1, 1, 0.5, 0.5, 0),
        (385, 385, 12, 1.0, 1, 0, 1.0, 0.3, 0), (256, 256, 40, 1.5, 0, 0, 2.0, 0.5, 0),
        (385, 385, 13, 3.0, 0, 1, 1.0, 0.8, 0), (384, 384, 64, 2.0, 1, 0, 0.5, 0.3, 0),
        (129, 129, 17, 1.5, 0, 1, 1.0, 0.5, 0), (385, 385, 64, 1.0, 1, 1, 2.0, 0.8, 0),
        (64, 450, 12, 2.0, 1, 1, 1.0, 0.5, 3)]
    return [dict(part="tile", k=k, B=B, B3=B3, n=n, p=p, pow=pw, compat=c, tau=tau, alpha=alpha, rows=slice(ch * B, (ch + 1) * B))
            for k, (B, B3, n, p, pw, c, tau, alpha, ch) in enumerate(rows)]


TRAIN = _train_meta()

# the generic entry points (clica_lp_loss_fwd + clica_lp_loss_bwd_sym for z3 = roll(z1); clica_lp_loss_fwd + clica_lp_loss_bwd with its
# two one-sided sweeps -- owner-only statistics for dz1, stream-only for dz3 -- for negatives of their own): B, B3, n, p, pow, compat, tau, alpha
GENERIC = [(385, 385, 10, 2.0, 1, 1, 1.0, 0.5), (129, 129, 13, 1.0, 1, 0, 0.5, 0.3), (256, 256, 40, 3.0, 0, 1, 2.0, 0.8),
           (384, 384, 1, 1.5, 1, 0, 1.0, 0.5), (385, 385, 64, 2.0, 0, 0, 1.0, 0.3), (129, 129, 17, 3.0, 1, 1, 0.5, 0.5),
           (385, 385, 12, 1.5, 0, 1, 1.0, 0.8)]
# one-sided only: B anchors against B3 negatives of their own
ONE_SIDED = [(64, 450, 10, 2.0, 1, 0, 1.0, 0.5), (129, 385, 17, 1.0, 1, 1, 0.5, 0.3), (100, 256, 12, 3.0, 0, 0, 1.0, 0.8)]


def _gen_id(g):
    B, B3, n, p, pw, c, tau, alpha = g
    return f"B{B}of{B3}-n{n}-p{p:g}-pow{pw}-compat{c}-tau{tau:g}-alpha{alpha:g}"


def _gen_data(g, own_negatives):
    """z1, z2 as _lp_data draws them (0.7 / sqrt(n)); z3 = roll(z1), or B3 rows of its own from the same distribution."""
    B, B3, n = g[:3]
    rng = np.random.default_rng([11, int(own_negatives), B, B3, n])
    scale = 0.7 / np.sqrt(n)
    z1 = (rng.normal(size=(B, n)) * scale).astype(np.float32)
    z2 = (z1 + 0.1 * scale * rng.normal(size=z1.shape)).astype(np.float32)
    z3 = (rng.normal(size=(B3, n)) * scale).astype(np.float32) if own_negatives else np.roll(z1, 1, 0)
    return z1, z2, z3


_GEN_EXPECT = {}


def _gen_expect(g, own_negatives, dtype=np.float64):
    """[(what, reference, floor)]: the comparisons of test_gpu_loss.py::test_lp_loss_seeded_sweep_vs_oracle (summand_floors / grad_scale,
    the pow = 0 gradient floor; dz3 against its own maximum).  z3 = roll(z1): the module returns the complete d loss / d z1, the oracle's
    dz1 + roll^-1(dz3), judged against the alignment pull as dz1 is."""
    key = (g, own_negatives, np.dtype(dtype).name)
    if key in _GEN_EXPECT:
        return _GEN_EXPECT[key]
    B, B3, n, p, pw, compat, tau, alpha = g
    z1, z2, z3 = _gen_data(g, own_negatives)
    orc = O.lp_simclr_loss(z1, z2, z3, p=p, tau=tau, alpha=alpha, compat=bool(compat), pow=bool(pw), dtype=dtype)
    lf, gf = summand_floors(orc, alpha, tau, grad_scale(z1, z2, p, tau, alpha))
    if not pw:
        gf = max(gf, 2 * alpha / (B * tau))
    out = [("loss_i", orc["loss_i"], lf), ("loss_mean", float(orc["loss_mean"]), lf), ("dz2", orc["dz2"], gf)]
    if own_negatives:
        out += [("dz1", orc["dz1"], gf), ("dz3", orc["dz3"], float(np.abs(np.asarray(orc["dz3"], np.float64)).max()))]
    else:
        out += [("dz1", orc["dz1"] + np.roll(orc["dz3"], -1, 0), gf)]
    out.append(("max|lse|", float(np.abs(orc["lse"] + (0.0 if compat else np.log(B3))).max()), None))
    _GEN_EXPECT[key] = out
    return out


# ===================================================================================================================== host-side guard
def test_inputs_hold_the_bound_in_plain_fp32():
    """Every case of this file, regenerated: the oracle in plain fp32 sits within 2.5e-6 of its fp64 evaluation on the denominators the
    GPU checks use, and max |lse| < 20 -- the GPU checks are the plain 1e-5 bound."""
    todo = [(f"train {_lp_id(c)}", _lp_expect(c), _lp_expect(c, np.float32)) for c in TRAIN]
    todo += [(f"generic {_gen_id(g)}", _gen_expect(g, False), _gen_expect(g, False, np.float32)) for g in GENERIC]
    todo += [(f"one-sided {_gen_id(g)}", _gen_expect(g, True), _gen_expect(g, True, np.float32)) for g in GENERIC[:3] + ONE_SIDED]
    worst = (0.0, None)
    for name, e64, e32 in todo:
        for (what, r64, floor), (_, r32, _) in zip(e64, e32):
            if what == "max|lse|":
                assert r64 < 20.0, (name, r64)
                continue
            r64 = np.asarray(r64, np.float64); r32 = np.asarray(r32, np.float64)
            assert np.isfinite(r32).all() and np.isfinite(r64).all(), (name, what)
            err = float(np.abs(r32 - r64).max()) / max(float(np.abs(r64).max()), float(floor), 1e-30)
            if err > worst[0]:
                worst = (err, f"{name} {what}")
            assert err < 2.5e-6, f"{name} {what}: fp32 oracle is {err:.2e} from fp64"
    print("fp32 oracle vs fp64, worst:", worst)


# ===================================================================================================================== vs oracle
@gpu
@pytest.mark.parametrize("c", TRAIN, ids=_lp_id)
def test_train_pair_many_tiles_vs_oracle(c, one_split):
    """clica_lp_loss_fwd_train / clica_lp_loss_bwd_sym_train with the whole pool streamed by one workgroup per owner tile."""
    o, dz, path = _lp_run(c)
    assert path == 0
    _lp_check("lp_tile_prefetch/train", c, o, dz)


def _gen_check(fam, g, own_negatives):
    from cl_ica_amd.losses import LpSimCLRLoss
    B, B3, n, p, pw, compat, tau, alpha = g
    z1, z2, z3 = _gen_data(g, own_negatives)
    L = LpSimCLRLoss(p=int(p) if p == int(p) else p, tau=tau, alpha=alpha, simclr_compatibility_mode=bool(compat), pow=bool(pw))
    out = run_hip(L, z1, z2, z3, roll=not own_negatives)
    assert all(np.isfinite(np.asarray(v)).all() for v in out.values())
    for what, ref, floor in _gen_expect(g, own_negatives):
        if floor is not None:
            PARITY.check(fam, _gen_id(g), what, out[what], ref, floor=floor)


@gpu
@pytest.mark.parametrize("g", GENERIC, ids=_gen_id)
def test_generic_sym_many_tiles_vs_oracle(g, one_split):
    """clica_lp_loss_fwd + clica_lp_loss_bwd_sym (z3 = roll(z1): the pool is z1 itself, one symmetric sweep)."""
    from cl_ica_amd import losses
    before = losses.PATHS["sym_one_sweep"]
    _gen_check("lp_tile_prefetch/generic_sym", g, False)
    assert losses.PATHS["sym_one_sweep"] == before + 1


@gpu
@pytest.mark.parametrize("g", GENERIC[:3] + ONE_SIDED, ids=_gen_id)
def test_one_sided_backward_many_tiles_vs_oracle(g, one_split):
    """clica_lp_loss_fwd + clica_lp_loss_bwd with negatives of their own: dz1 from the owner-statistics sweep over the z3 stream, dz3 from
    the stream-statistics sweep over the z1 stream."""
    _gen_check("lp_tile_prefetch/one_sided", g, True)


# ===================================================================================================================== bit checks
BIT_CASES = [(385, 385, 10, 2, 1, 1), (129, 129, 13, 3, 0, 0), (385, 385, 40, 1, 1, 0), (256, 256, 64, 1.5, 1, 1), (64, 450, 12, 2, 1, 1)]
BIT_IDS = [f"B{B}of{B3}-n{n}-p{p}-pow{pw}-compat{c}" for B, B3, n, p, pw, c in BIT_CASES]


def _bit_problem(B, B3, n, p, pw, compat):
    z, zt = _rows(B3, n, 1000 + B3 + n)
    pair = LpPair(B, B3, n, p, tau=0.5, alpha=0.3, compat=compat, pw=pw)
    pool_lse = dev(np.random.default_rng(2).uniform(3.0, 9.0, B3)) if B3 != B else None      # any finite statistics serve a bit comparison
    return pair, z, zt, pool_lse


@gpu
@pytest.mark.parametrize("case", BIT_CASES, ids=BIT_IDS)
def test_leading_dimension_and_repeated_calls_keep_the_bits(case, one_split):
    """The same pool with ld = n and as a copy with ld = n + 3 (NaN in the padding columns), and two more calls on one workspace:
    identical outputs, the outputs' padding columns untouched, the arrival counters zero between launches."""
    B, B3, n, p, pw, compat = case
    pair, z, zt, pool_lse = _bit_problem(*case)
    pool, z2 = dev(z), dev(zt[:B])
    o, dzb = pair.run(pool[:B], z2, pool, pool_lse=pool_lse)
    assert torch.isfinite(o).all() and torch.isfinite(dzb).all()
    pv, _ = _padded(z, 3, float("nan"))
    z2v, _ = _padded(zt[:B], 3, float("nan"))
    o2, dzb2 = pair.run(pv[:B], z2v, pv, ldo=n + 3, pool_lse=pool_lse)
    assert torch.equal(o2, o) and torch.equal(dzb2[:, :n], dzb)
    assert _padding_untouched(dzb2, n)
    ws = pair.workspace()
    for rep in range(2):
        o3, dzb3 = pair.run(pool[:B], z2, pool, ws=ws, pool_lse=pool_lse)
        assert torch.equal(o3, o) and torch.equal(dzb3, dzb), rep
        for cnt in pair.counters(ws):
            assert int(cnt.abs().max()) == 0


@gpu
@pytest.mark.parametrize("n,p", [(10, 2), (40, 1)])
def test_leading_dimension_beyond_32_bit_offsets_keeps_the_bits(n, p, one_split):
    """A pool whose rows lie 2^22 + 3 floats apart: a 128-row tile no longer fits the Stager's 32-bit byte offsets, and it reads the tile
    with 64-bit indexing at store time instead of prefetching it.  Two tiles, the second of two rows (a 2.2 GB buffer of which 130 rows of
    n floats are touched; the rest is never written).  Same bits as the contiguous pool."""
    B, LD = 130, (1 << 22) + 3
    pair, z, zt, _ = _bit_problem(B, B, n, p, 1, 1)
    pool, z2 = dev(z), dev(zt)
    o, dzb = pair.run(pool, z2, pool)
    buf = torch.empty(B * LD, device="cuda")
    far = buf.as_strided((B, n), (LD, 1))
    far.copy_(pool)
    o2, dzb2 = pair.run(far, z2, far)
    assert torch.isfinite(o).all() and torch.isfinite(dzb).all()
    assert torch.equal(o2, o) and torch.equal(dzb2, dzb)


@gpu
@pytest.mark.parametrize("case", [c for c in BIT_CASES if c[2] <= 16], ids=[i for c, i in zip(BIT_CASES, BIT_IDS) if c[2] <= 16])
def test_fused_finalize_switch_keeps_the_bits(case, one_split, request):
    """lp_fused_finalize 0 (sweep + finalize launch) against 1 (one launch), under the cap: identical outputs."""
    from cl_ica_amd import _lib
    lib = _lib.load()
    request.addfinalizer(lambda: _lib.check(lib.clica_set_tuning(b"lp_fused_finalize", 1), "clica_set_tuning"))
    B, B3, n, p, pw, compat = case
    pair, z, zt, pool_lse = _bit_problem(*case)
    pool, z2 = dev(z), dev(zt[:B])
    ws = pair.workspace()
    outs = []
    for fused in (1, 0, 1):
        _lib.check(lib.clica_set_tuning(b"lp_fused_finalize", fused), "clica_set_tuning")
        outs.append(pair.run(pool[:B], z2, pool, ws=ws, pool_lse=pool_lse))
    for o, dzb in outs[1:]:
        assert torch.equal(o, outs[0][0]) and torch.equal(dzb, outs[0][1])


# ===================================================================================================================== nn_search
@gpu
def test_nn_search_three_tiles_ragged_last(one_split):
    """clica_nn_search shares the Stager: a 300-row table under the cap is one chunk of three tiles, the last of 44 rows.  Against a NumPy
    argsort of the fp64 squared distances (columns whose fp64 gap to a neighbour is not resolvable in fp32 are left out, as in
    test_nn_search_vs_oracle)."""
    from cl_ica_amd import ops
    N, Q, n, k = 300, 70, 10, 2
    rng = np.random.default_rng(300)
    tab = rng.uniform(-1, 1, size=(N, n)).astype(np.float32)
    qry = rng.uniform(-1, 1, size=(Q, n)).astype(np.float32)
    dist, idx = ops.nn_search(torch.tensor(tab, device="cuda"), torch.tensor(qry, device="cuda"), k)
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    D = ((qry[:, None, :].astype(np.float64) - tab[None].astype(np.float64)) ** 2).sum(-1)
    I = np.argsort(D, axis=1, kind="stable")[:, :k + 1]
    Ds = np.take_along_axis(D, I, 1)
    decided = np.ones((Q, k), bool)
    for c in range(k):
        decided[:, c] &= (Ds[:, c + 1] - Ds[:, c]) > 1e-6 * n
        if c > 0:
            decided[:, c] &= (Ds[:, c] - Ds[:, c - 1]) > 1e-6 * n
    assert decided.mean() > 0.95
    assert (idx[decided] == I[:, :k][decided]).all()
    assert (I[:, :k] >= 256).any(), "some neighbours must lie in the ragged third tile"
    PARITY.check("lp_tile_prefetch/nn_search", f"N={N} Q={Q} n={n} k={k}", "dist", dist, Ds[:, :k], floor=1e-3 * n)
