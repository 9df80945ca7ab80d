"""The two training pairs of C entry points -- clica_lp_loss_fwd_train / clica_lp_loss_bwd_sym_train (csrc/lp_loss.hip, lp_kernels.h,
lp_loss_pk.hip) and clica_dot_loss_fwd_train / clica_dot_loss_bwd_sym_train (csrc/dot_train.hip) -- against the fp64 oracle in every form
the C ABI accepts: all exponents (1, 2, 3 and non-integer), both `pow` forms, both compat modes, three temperatures and weights, every
padded width incl. wide rows, ragged row counts, pools larger than the batch, leading dimensions beyond n, NULL outputs, repeated calls on
one workspace, the one-launch forward's A/B switch, the counter tick and the error paths.

Every case is small (B <= 640, B3 <= 1537; one dot case of 2304 rows, see test_dot_running_maximum_both_orders) and the inputs are
unsaturated: test_inputs_hold_the_bound_in_plain_fp32 (no GPU) shows that a plain fp32 evaluation of every case sits within 2.5e-6 of
fp64 on the denominators used here and that max |lse| < 20, so every GPU check is the plain 1e-5 bound with no allowance."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import PARITY
from oracle import np_oracle as O
from test_gpu_loss import _train_pair, dev, grad_scale, matrix_cores_every_pool, summand_floors  # noqa: F401  (fixture)
from test_gpu_simclr_engine import check_vs_oracle, make_rows, train_pair

gpu = pytest.mark.gpu
LN2 = float(np.log(2.0))
E_INVALID, E_WORKSPACE = -1, -2          # include/clica.h


# ===================================================================================================================== cases
LP_B = [1, 2, 31, 63, 64, 65, 127, 129, 200, 511, 640]
LP_N = [1, 3, 4, 5, 10, 12, 13, 14, 15, 16, 17, 24, 25, 33, 40, 41, 64, 65, 129]
LP_P = [1.0, 2.0, 3.0, 1.5, 2.5]
LP_SWEEP_CASES = 40


def _lp_sweep_meta():
    """Forty seeded cases.  Every knob is drawn at random; B and n are drawn WITHOUT replacement until their list is used up (so every
    row count and every width occurs, each at least twice / three times), and the first twenty cases carry the twenty (p, pow, compat)
    combinations.  (The seed is the first from 20261 on whose list holds at least three p = 2, pow = 1, n <= 10 cases, in both compat
    modes, for the matrix-core extra: a property of the case list alone, asserted below.)"""
    rng = np.random.default_rng(20280)
    combos = [(p, pw, c) for p in LP_P for pw in (1, 0) for c in (1, 0)]
    bs = np.concatenate([rng.permutation(LP_B) for _ in range(4)])
    ns = np.concatenate([rng.permutation(LP_N) for _ in range(3)])
    out = []
    for k in range(LP_SWEEP_CASES):
        p, pw, compat = float(rng.choice(LP_P)), int(rng.integers(2)), int(rng.integers(2))
        tau, alpha = float(rng.choice([0.5, 1.0, 2.0])), float(rng.choice([0.5, 0.3, 0.8]))
        if k < len(combos):
            p, pw, compat = combos[k]
        B = int(bs[k])
        out.append(dict(part="sweep", k=k, B=B, B3=B, n=int(ns[k]), p=p, pow=pw, compat=compat, tau=tau, alpha=alpha, rows=slice(0, B)))
    return out


def _lp_pooled_meta():
    """Ragged pools, B < B3 (below and above 4 B), with p, pow, compat, n, tau and alpha spread over them.  Local rows = a whole chunk
    of the pool.  None of them is a matrix-core shape under the default policy (p = 2, pow, n <= 10 only against B3 < 4 B)."""
    rows = [  # B, B3, n, p, pow, compat, tau, alpha, local chunk
        (64, 65, 10, 2.0, 1, 1, 1.0, 0.5, 0), (64, 65, 17, 2.5, 0, 0, 0.5, 0.3, 0),
        (100, 257, 40, 1.0, 1, 0, 2.0, 0.8, 1), (100, 257, 10, 3.0, 0, 1, 1.0, 0.3, 0),
        (129, 400, 4, 3.0, 1, 1, 0.5, 0.5, 2), (129, 400, 65, 2.0, 1, 0, 1.0, 0.8, 1),
        (200, 1537, 17, 1.5, 1, 1, 1.0, 0.3, 3), (200, 1537, 4, 1.0, 0, 1, 2.0, 0.5, 6),
        (33, 1000, 65, 2.0, 0, 0, 0.5, 0.5, 7), (33, 1000, 40, 3.0, 1, 0, 2.0, 0.8, 29)]
    return [dict(part="pooled", k=k, B=B, B3=B3, n=n, p=p, pow=pw, compat=c, tau=tau, alpha=alpha, rows=slice(ch * B, (ch + 1) * B))
            for k, (B, B3, n, p, pw, c, tau, alpha, ch) in enumerate(rows)]


LP_SWEEP = _lp_sweep_meta()
LP_POOLED = _lp_pooled_meta()
LP_MATRIX_CORES = [c for c in LP_SWEEP if c["p"] == 2.0 and c["pow"] == 1 and c["n"] <= 10]
assert len(LP_MATRIX_CORES) >= 3 and {c["compat"] for c in LP_MATRIX_CORES} == {0, 1}, "the sweep must feed the matrix-core extra"


def _lp_id(c):
    return (f"{c['k']:02d}-p{c['p']:g}-pow{c['pow']}-compat{c['compat']}-B{c['B']}" + (f"of{c['B3']}" if c["B3"] != c["B"] else "") +
            f"-n{c['n']}-tau{c['tau']:g}-alpha{c['alpha']:g}")


def _lp_data(c):
    """The pool and its partner rows, drawn as tests/test_gpu_loss.py::test_lp_loss_seeded_sweep_vs_oracle draws z1 / z2 (scale
    0.7 / sqrt(n): summed distances stay O(1), unsaturated rows).  Every pool row is an anchor with a partner of its own."""
    rng = np.random.default_rng([7 if c["part"] == "sweep" else 8, c["k"]])
    scale = 0.7 / np.sqrt(c["n"])
    z = (rng.normal(size=(c["B3"], c["n"])) * scale).astype(np.float32)
    zt = (z + 0.1 * scale * rng.normal(size=z.shape)).astype(np.float32)
    return z, zt


_EXPECT = {}      # (kind, part, k, dtype) -> expectations: computed once per session, shared by the GPU tests and the host-side guard


def _lp_expect(c, dtype=np.float64):
    """[(what, reference, floor)] of the local rows of case c from oracle.lp_simclr_loss on the WHOLE pool with z1 = z3 = pool.
    The symmetric sweep gives the gradient of (1 / B) sum over pool rows of loss_j, so dz1 is (B3 / B) (dz1 + dz3)[rows] and dz2 is
    (B3 / B) dz2[rows] (single rank: B3 = B).  Floors: summand_floors / grad_scale as the generic sweep, with its pow = 0 gradient floor;
    the row statistics and their means as test_full_size_vs_oracle.  lse_i / neg_mean in logmeanexp mode are the difference
    lse_raw - ln B3: judged against the larger summand, as every cancelling sum here."""
    key = ("lp", c["part"], c["k"], np.dtype(dtype).name)
    if key in _EXPECT:
        return _EXPECT[key]
    z, zt = _lp_data(c)
    p, tau, alpha, rows, B, B3 = c["p"], c["tau"], c["alpha"], c["rows"], c["B"], c["B3"]
    orc = O.lp_simclr_loss(z, zt, z, p=p, tau=tau, alpha=alpha, compat=bool(c["compat"]), pow=bool(c["pow"]), dtype=dtype)
    loc = dict(pos=orc["pos"][rows], lse=orc["lse"][rows])
    lf, gf = summand_floors(loc, alpha, tau, grad_scale(z[rows], zt[rows], p, tau, alpha))
    if not c["pow"]:          # pow = 0: d|x|/dx of the root at a near-zero positive pair is O(1) whatever p is
        gf = max(gf, 2 * alpha / (B * tau))
    pf = float(np.abs(loc["pos"]).max()) / tau
    nf = float(np.abs(loc["lse"]).max())
    if not c["compat"]:
        nf = max(float(np.abs(loc["lse"] + np.log(B3)).max()), float(np.log(B3)))
    sc = B3 / B
    out = [("loss_i", orc["loss_i"][rows], lf), ("pos_i", loc["pos"] / tau, 0.0), ("lse_i", loc["lse"], nf),
           ("loss_mean", orc["loss_i"][rows].mean(), lf), ("pos_mean", (loc["pos"] / tau).mean(), pf), ("neg_mean", loc["lse"].mean(), nf),
           ("dz1", sc * (orc["dz1"] + orc["dz3"])[rows], gf), ("dz2", sc * orc["dz2"][rows], gf),
           ("max|lse|", float(np.abs(orc["lse"] + (0.0 if c["compat"] else np.log(B3))).max()), None)]
    _EXPECT[key] = out
    return out


# dot kind -------------------------------------------------------------------------------------------------------------
def _dot_meta():
    out = []
    kinds = ("unit", 0.1, 1.0)            # (scale 3 at tau = 0.5 saturates the rows: |lse| up to 50; test_dot_running_maximum covers norm 3)
    k = 0
    for B in (65, 300):
        for n in (1, 2, 33, 63, 64):
            out.append(dict(part="roll", k=k, B=B, B3=B, n=n, tau=(1.0, 0.5)[k % 2], alpha=(0.5, 0.3)[(k // 2) % 2], kind=kinds[k % 3],
                            rows=slice(0, B)))
            k += 1
    for k, (B, B3, n, tau, alpha, kind, ch) in enumerate([(100, 257, 10, 0.5, 0.5, 1.0, 1), (129, 400, 33, 1.0, 0.3, "unit", 2)]):
        out.append(dict(part="pooled", k=k, B=B, B3=B3, n=n, tau=tau, alpha=alpha, kind=kind, rows=slice(ch * B, (ch + 1) * B)))
    for k, B in enumerate((200, 2304)):
        out.append(dict(part="runmax", k=k, B=B, B3=B, n=10, tau=0.5, alpha=0.5, kind="norm 0.1..3", rows=slice(0, B)))
    return out


DOT_CASES = _dot_meta()


def _dot_id(c):
    return f"{c['part']}{c['k']}-B{c['B']}" + (f"of{c['B3']}" if c["B3"] != c["B"] else "") + f"-n{c['n']}-tau{c['tau']:g}-alpha{c['alpha']:g}-{c['kind']}"


def _dot_data(c):
    """(z1, z2, z3) of the ORACLE problem: z3 = roll(z1) in the 'roll' family (the reference's z3_rec), the pool itself otherwise.
    'runmax': rows of norm 0.1 ... 3 in ASCENDING order (every later pool tile / partition / split raises the row maximum)."""
    rng = np.random.default_rng([9, ("roll", "pooled", "runmax").index(c["part"]), c["k"]])
    if c["part"] == "runmax":
        z1, z2 = make_rows(rng, c["B"], c["n"], "unit")
        s = np.linspace(0.1, 3.0, c["B"], dtype=np.float32)[:, None]
        return z1 * s, z2 * s, z1 * s
    z1, z2 = make_rows(rng, c["B3"], c["n"], c["kind"])
    return z1, z2, (np.roll(z1, 1, 0) if c["part"] == "roll" else z1)


def _dot_refs(c, dtype=np.float64):
    """The oracle's dz1 / dz2 for the pair's local rows (see _lp_expect for the pooled identity; 'roll': dz3 comes back through roll^-1)."""
    z1, z2, z3 = _dot_data(c)
    orc = O.simclr_loss(z1, z2, z3, tau=c["tau"], alpha=c["alpha"], dtype=dtype)
    sc, rows = c["B3"] / c["B"], c["rows"]
    d3 = np.roll(orc["dz3"], -1, 0) if c["part"] == "roll" else orc["dz3"]
    return orc, sc * (orc["dz1"] + d3)[rows], sc * orc["dz2"][rows]


def _dot_expect(c, dtype=np.float64):
    """The comparisons check_vs_oracle(..., scale=1) makes, as [(what, reference, floor)] (its floors restated: loss_i against the larger of
    its two summands, the gradients against the alignment pull 2 alpha / (B tau) max |z2|)."""
    key = ("dot", c["part"], c["k"], np.dtype(dtype).name)
    if key in _EXPECT:
        return _EXPECT[key]
    z1, z2, z3 = _dot_data(c)
    orc, d1, d2 = _dot_refs(c, dtype)
    tau, alpha, rows = c["tau"], c["alpha"], c["rows"]
    pos = (np.asarray(z1, dtype) * np.asarray(z2, dtype)).sum(1)[rows]
    lse, li = orc["lse"][rows], orc["loss_i"][rows]
    lf = 2.0 * max(alpha * float(np.abs(pos).max()) / tau, (1.0 - alpha) * float(np.abs(lse).max()))
    gf = 2.0 * alpha / (len(li) * tau) * float(np.abs(z2).max())
    out = [("loss_i", li, lf), ("pos_i", -pos / tau, 0.0), ("lse_i", lse, 0.0), ("loss_mean", li.mean(), lf),
           ("pos_mean", (-pos / tau).mean(), float(np.abs(pos).max()) / tau), ("neg_mean", lse.mean(), float(np.abs(lse).max())),
           ("dz1", d1, gf), ("dz2", d2, gf), ("max|lse|", float(np.abs(orc["lse"]).max()), None)]
    _EXPECT[key] = out
    return out


# ===================================================================================================================== 5. host-side guard
def test_inputs_hold_the_bound_in_plain_fp32():
    """Every case of the Lp sweep, the Lp pooled family and the dot families, regenerated: the oracle evaluated in plain fp32 (numpy,
    dtype=np.float32) sits within 2.5e-6 of its fp64 evaluation on the denominators the GPU checks use, and max |lse| < 20.  The GPU
    checks then need no allowance: a correct fp32 evaluation of these inputs holds the 1e-5 bound with a 4 x margin."""
    worst = (0.0, None)
    for kind, cases, expect, ident in (("lp", LP_SWEEP + LP_POOLED, _lp_expect, _lp_id), ("dot", DOT_CASES, _dot_expect, _dot_id)):
        for c in cases:
            e64, e32 = expect(c), expect(c, np.float32)
            for (what, r64, floor), (_, r32, _) in zip(e64, e32):
                if what == "max|lse|":
                    assert r64 < 20.0, (kind, ident(c), r64)
                    continue
                r64 = np.asarray(r64, np.float64); r32 = np.asarray(r32, np.float64)
                assert np.isfinite(r32).all() and np.isfinite(r64).all(), (kind, ident(c), what)
                den = max(float(np.abs(r64).max()), float(floor), 1e-30)
                err = float(np.abs(r32 - r64).max()) / den
                if err > worst[0]:
                    worst = (err, f"{kind} {ident(c)} {what}")
                assert err < 2.5e-6, f"{kind} {ident(c)} {what}: fp32 oracle is {err:.2e} from fp64"
    print("fp32 oracle vs fp64, worst:", worst)


# ===================================================================================================================== 1 + 2. Lp pair vs oracle
def _lp_run(c):
    """The pair on the GPU for case c -> (out [3 B + 3], dz [2 B, n], path).  B < B3: the pool's lse comes from forward-only calls over
    consecutive chunks of B pool rows (the last one shorter), and the local rows' own forward must reproduce its chunk's bits."""
    z, zt = _lp_data(c)
    pool, pool2 = dev(z), dev(zt)
    B, B3, rows = c["B"], c["B3"], c["rows"]
    args = (c["n"], c["p"], c["tau"], c["alpha"], c["compat"], c["pow"])
    if B3 == B:
        return _train_pair(pool, pool2, pool, None, *args)
    lse_all = torch.empty(B3, device="cuda")
    empty = torch.empty(0, device="cuda")
    for c0 in range(0, B3, B):
        sl = slice(c0, min(c0 + B, B3))
        b = sl.stop - sl.start
        o_r, _, _ = _train_pair(pool[sl], pool2[sl], pool, empty, *args)
        lse_all[sl] = o_r[2 * b:3 * b]
    o, dz, path = _train_pair(pool[rows], pool2[rows], pool, lse_all, *args)
    assert torch.equal(o[2 * B:3 * B], lse_all[rows]), "the local rows' own forward must reproduce its chunk's bits"
    return o, dz, path


def _lp_check(fam, c, o, dz):
    B, B3 = c["B"], c["B3"]
    oc, dzc = o.cpu().numpy().astype(np.float64), dz.cpu().numpy()
    got = dict(loss_i=oc[:B], pos_i=oc[B:2 * B], lse_i=oc[2 * B:3 * B] * LN2 - (0.0 if c["compat"] else np.log(B3)),
               loss_mean=oc[3 * B], pos_mean=oc[3 * B + 1], neg_mean=oc[3 * B + 2], dz1=dzc[:B], dz2=dzc[B:])
    assert all(np.isfinite(v).all() for v in got.values()), {k: bool(np.isfinite(v).all()) for k, v in got.items()}
    for what, ref, floor in _lp_expect(c):
        if floor is not None:
            PARITY.check(fam, _lp_id(c), what, got[what], ref, floor=floor)


@gpu
@pytest.mark.parametrize("c", LP_SWEEP, ids=_lp_id)
def test_lp_train_pair_sweep_vs_oracle(c):
    """Single rank (pool = z1) on the coordinate-difference sweeps (default matrix-core policy: clica_lp_loss_train_path reports 0):
    loss_i, pos_i, lse_i, the three means, dz1 (= the oracle's dz1 + dz3) and dz2 at 1e-5."""
    o, dz, path = _lp_run(c)
    assert path == 0
    _lp_check("lp_train_pair_sweep", c, o, dz)


@gpu
@pytest.mark.parametrize("c", LP_MATRIX_CORES, ids=_lp_id)
def test_lp_train_pair_sweep_on_matrix_cores(c, matrix_cores_every_pool):
    """The sweep's p = 2, pow = 1, n <= 10 cases once more with the matrix cores switched on for every pool (policy 2)."""
    o, dz, path = _lp_run(c)
    assert path == 1
    _lp_check("lp_train_pair_sweep/matrix_cores", c, o, dz)


@gpu
@pytest.mark.parametrize("c", LP_POOLED, ids=_lp_id)
def test_lp_train_pair_pooled_vs_oracle(c):
    """B < B3, ragged: pool_stats_k and the streamed pool's ragged tail behind the training pair, for every kind of exponent."""
    o, dz, path = _lp_run(c)
    assert path == 0
    _lp_check("lp_train_pair_pooled", c, o, dz)


# ===================================================================================================================== 3. Lp pair: ABI edges
SENTINEL = -777.25
NEG_ZERO_BITS = -2 ** 31      # the padding columns of an output view hold -0.0: any store shows, `x += 0` included (-0 + 0 = +0)


def _padding_untouched(buf, n):
    return bool((buf[:, n:].contiguous().view(torch.int32) == NEG_ZERO_BITS).all())


class LpPair:
    """The two calls through the C ABI with every argument in the caller's hands (leading dimensions, workspace, tick counter)."""

    def __init__(self, B, B3, n, p, tau=1.0, alpha=0.5, compat=1, pw=1):
        from cl_ica_amd import _lib
        self.L, self.lib = _lib, _lib.load()
        self.B, self.B3, self.n = B, B3, n
        self.d = _lib.LpLossDesc(B=B, B3=B3, n=n, p=float(p), tau=tau, alpha=alpha, compat=compat, pow=pw)
        nb = C.c_size_t()
        _lib.check(self.lib.clica_lp_loss_train_workspace_bytes(C.byref(self.d), C.byref(nb)), "ws")
        self.nbytes = nb.value

    def workspace(self):
        return torch.zeros(self.nbytes, dtype=torch.uint8, device="cuda")

    def outputs(self, ldo=None):
        B, ldo = self.B, ldo or self.n
        dzb = torch.full((2 * B, ldo), SENTINEL, device="cuda")
        dzb[:, self.n:] = -0.0
        return torch.full((3 * B + 3,), SENTINEL, device="cuda"), dzb

    def fwd(self, z1, z2, pool, o, dzb, ws, ws_bytes=None, ld1=None, ldd=None, d=None):
        B, ldd = self.B, ldd or dzb.stride(0)
        return self.lib.clica_lp_loss_fwd_train(C.byref(d or self.d), z1.data_ptr(), ld1 or z1.stride(0), z2.data_ptr(), z2.stride(0), pool.data_ptr(),
                                                pool.stride(0), o[:B].data_ptr(), o[B:2 * B].data_ptr(), o[2 * B:3 * B].data_ptr(),
                                                dzb[:B].data_ptr(), ldd, dzb[B:].data_ptr(), ldd, ws.data_ptr(),
                                                ws.numel() if ws_bytes is None else ws_bytes, self.L.stream_ptr())

    def bwd(self, z1, pool, o, dzb, ws, pool_lse=None, tick=None, ws_bytes=None, ld1=None, ldd=None, d=None):
        B = self.B
        lse = o[2 * B:3 * B]
        return self.lib.clica_lp_loss_bwd_sym_train(C.byref(d or self.d), z1.data_ptr(), ld1 or z1.stride(0), pool.data_ptr(), pool.stride(0), lse.data_ptr(),
                                                    (lse if pool_lse is None else pool_lse).data_ptr(), dzb[:B].data_ptr(), ldd or dzb.stride(0),
                                                    o[3 * B:].data_ptr(), None if tick is None else tick.data_ptr(), ws.data_ptr(),
                                                    ws.numel() if ws_bytes is None else ws_bytes, self.L.stream_ptr())

    def run(self, z1, z2, pool, ws=None, ldo=None, pool_lse=None, tick=None):
        ws = self.workspace() if ws is None else ws
        o, dzb = self.outputs(ldo)
        self.L.check(self.fwd(z1, z2, pool, o, dzb, ws), "fwd_train")
        self.L.check(self.bwd(z1, pool, o, dzb, ws, pool_lse=pool_lse, tick=tick), "bwd_sym_train")
        torch.cuda.synchronize()
        return o, dzb

    def counters(self, ws):
        """The arrival counters of the 4 KB header and TrainWs::arrive (csrc/lp_loss.hip, carve_train: behind the header and the
        256-byte-aligned block sums, one int per 64-row tile)."""
        tiles = (self.B + 63) // 64
        off = 4096 + (tiles * 12 + 255) // 256 * 256
        return ws[64:4096].view(torch.int32), ws[off:off + 4 * tiles].view(torch.int32)


def _padded(a, pad, fill):
    """A [rows, n] view with leading dimension n + pad over a buffer whose padding columns hold `fill`."""
    a = torch.as_tensor(a)
    buf = torch.full((a.shape[0], a.shape[1] + pad), fill, device="cuda")
    buf[:, :a.shape[1]] = a.cuda()
    return buf[:, :a.shape[1]], buf


def _rows(B, n, seed):
    rng = np.random.default_rng(seed)
    scale = 0.7 / np.sqrt(n)
    z = (rng.normal(size=(B, n)) * scale).astype(np.float32)
    return z, (z + 0.1 * scale * rng.normal(size=z.shape)).astype(np.float32)


# B, B3, n, p, pow, compat: one-launch forward, two-launch forward (n > 16 / generic exponent / root form), wide rows, a ragged pool
ABI_CASES = [(129, 129, 10, 2, 1, 1), (65, 65, 17, 1, 1, 0), (64, 200, 4, 3, 0, 1), (33, 33, 65, 1.5, 1, 1), (100, 257, 14, 3, 1, 0)]
ABI_IDS = [f"B{B}of{B3}-n{n}-p{p}-pow{pw}-compat{c}" for B, B3, n, p, pw, c in ABI_CASES]


def _abi_problem(B, B3, n, p, pw, compat):
    z, zt = _rows(B3, n, B3 + n)
    pair = LpPair(B, B3, n, p, tau=0.5, alpha=0.3, compat=compat, pw=pw)
    pool_lse = None
    if B3 != B:       # any finite statistics serve a bit-for-bit comparison
        pool_lse = dev(np.random.default_rng(1).uniform(3.0, 9.0, B3))
    return pair, z, zt, pool_lse


@gpu
@pytest.mark.parametrize("case", ABI_CASES, ids=ABI_IDS)
def test_lp_train_pair_leading_dimensions(case):
    """z1, z2, pool, dz1, dz2 with leading dimension n + 3 (NaN in the inputs' padding columns): the bits of the plain call, and the
    outputs' padding columns (-0.0, compared as bits) untouched."""
    B, B3, n, p, pw, compat = case
    pair, z, zt, pool_lse = _abi_problem(*case)
    pool = dev(z)
    o, dzb = pair.run(pool[:B], dev(zt[:B]), pool, pool_lse=pool_lse)
    pv, _ = _padded(z, 3, float("nan"))
    z2v, _ = _padded(zt[:B], 3, float("nan"))
    o2, dzb2 = pair.run(pv[:B], z2v, pv, ldo=n + 3, pool_lse=pool_lse)
    assert torch.isfinite(o).all() and torch.isfinite(dzb).all()
    assert torch.equal(o2, o) and torch.equal(dzb2[:, :n], dzb)
    assert _padding_untouched(dzb2, n), "padding columns of dz1 / dz2 were written"
    if B3 == B:      # and with the anchors in a buffer of their own, another leading dimension again
        z1v, _ = _padded(z, 5, float("nan"))
        o3, dzb3 = pair.run(z1v, z2v, pv, ldo=n + 1)
        assert torch.equal(o3, o) and torch.equal(dzb3[:, :n], dzb) and _padding_untouched(dzb3, n)


@gpu
@pytest.mark.parametrize("case", ABI_CASES, ids=ABI_IDS)
def test_lp_train_pair_repeated_calls_on_one_workspace(case):
    """Three calls of the pair on ONE workspace with fresh output buffers: identical bits each time (and those of a fresh workspace), the
    arrival counters of the header and of the training carve zero afterwards."""
    B, B3, n, p, pw, compat = case
    pair, z, zt, pool_lse = _abi_problem(*case)
    pool, z2 = dev(z), dev(zt[:B])
    ref = pair.run(pool[:B], z2, pool, pool_lse=pool_lse)
    ws = pair.workspace()
    for rep in range(3):
        o, dzb = pair.run(pool[:B], z2, pool, ws=ws, pool_lse=pool_lse)
        assert torch.equal(o, ref[0]) and torch.equal(dzb, ref[1]), rep
        for cnt in pair.counters(ws):
            assert int(cnt.abs().max()) == 0, "arrival counters must be zero between launches"


@gpu
@pytest.mark.parametrize("n", [4, 14, 16])
@pytest.mark.parametrize("p", [1, 2, 3])
def test_lp_train_pair_fused_finalize_switch(p, n, request):
    """clica_set_tuning("lp_fused_finalize", 0) (sweep + finalize launch) against 1 (one launch) on the training entry point: equal
    outputs, both pow forms and compat modes, a ragged last tile, one workspace throughout."""
    from cl_ica_amd import _lib
    lib = _lib.load()
    request.addfinalizer(lambda: _lib.check(lib.clica_set_tuning(b"lp_fused_finalize", 1), "clica_set_tuning"))
    B = 200
    z, zt = _rows(B, n, 10 * p + n)
    pool, z2 = dev(z), dev(zt)
    for pw, compat in ((1, 1), (0, 0), (1, 0)):
        pair = LpPair(B, B, n, p, tau=2.0, alpha=0.8, compat=compat, pw=pw)
        ws = pair.workspace()
        outs = []
        for fused in (1, 0, 1):
            _lib.check(lib.clica_set_tuning(b"lp_fused_finalize", fused), "clica_set_tuning")
            outs.append(pair.run(pool, z2, pool, ws=ws))
            assert torch.isfinite(outs[-1][0]).all() and torch.isfinite(outs[-1][1]).all()
        for o, dzb in outs[1:]:
            assert torch.equal(o, outs[0][0]) and torch.equal(dzb, outs[0][1]), (pw, compat)
        for cnt in pair.counters(ws):
            assert int(cnt.abs().max()) == 0


@gpu
def test_lp_train_pair_tick_counter():
    """tick_counter non-NULL advances by exactly 1 per backward call; NULL gives the same outputs."""
    for case in ABI_CASES[:3]:
        B = case[0]
        pair, z, zt, pool_lse = _abi_problem(*case)
        pool, z2 = dev(z), dev(zt[:B])
        ref = pair.run(pool[:B], z2, pool, pool_lse=pool_lse)
        tick = torch.full((3,), 41, dtype=torch.int32, device="cuda")
        for k in (1, 2):
            got = pair.run(pool[:B], z2, pool, pool_lse=pool_lse, tick=tick[1:])
            assert tick.tolist() == [41, 41 + k, 41]
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


@gpu
def test_lp_train_pair_error_paths_write_nothing():
    """p = 0.5, a leading dimension below n, a workspace one byte short, B3 < B in the backward: an error code, and neither the outputs
    nor the workspace are written."""
    B, n = 70, 12      # (not a matrix-core shape: for those the reported workspace size includes the operand planes, which a call on the
                       #  difference sweeps does not need -- one byte less than reported is then not short for that call)
    z, zt = _rows(B, n, 3)
    pool, z2 = dev(z), dev(zt)
    good = LpPair(B, B, n, 2)
    o_ok, dz_ok = good.run(pool, z2, pool)            # the forward's outputs a failing backward must leave alone
    frac = LpPair(B, B, n, 0.5)
    small = LpPair(B, B - 1, n, 2)
    ws = good.workspace()
    o, dzb = good.outputs()
    calls = [("fwd p = 0.5", frac.fwd(pool, z2, pool, o, dzb, ws), E_INVALID),
             ("bwd p = 0.5", frac.bwd(pool, pool, o, dzb, ws), E_INVALID),
             ("fwd ld1 < n", good.fwd(pool, z2, pool, o, dzb, ws, ld1=n - 1), E_INVALID),
             ("fwd ldd < n", good.fwd(pool, z2, pool, o, dzb, ws, ldd=n - 1), E_INVALID),
             ("bwd ld1 < n", good.bwd(pool, pool, o, dzb, ws, ld1=n - 1), E_INVALID),
             ("bwd ldd < n", good.bwd(pool, pool, o, dzb, ws, ldd=n - 1), E_INVALID),
             ("fwd workspace one byte short", good.fwd(pool, z2, pool, o, dzb, ws, ws_bytes=good.nbytes - 1), E_WORKSPACE),
             ("bwd workspace one byte short", good.bwd(pool, pool, o, dzb, ws, ws_bytes=good.nbytes - 1), E_WORKSPACE),
             ("bwd B3 < B", good.bwd(pool, pool, o, dzb, ws, d=small.d), E_INVALID)]
    torch.cuda.synchronize()
    for what, rc, want in calls:
        assert rc == want, (what, rc, good.lib.clica_last_error())
    assert bool((o == SENTINEL).all()) and bool((dzb == SENTINEL).all()) and int(ws.abs().max()) == 0
    # ... and the library still works afterwards, on the workspace the failed calls were handed
    o2, dz2 = good.run(pool, z2, pool, ws=ws)
    assert torch.equal(o2, o_ok) and torch.equal(dz2, dz_ok)


# ===================================================================================================================== 4. dot pair
def _dot_run(c, order=None):
    z1, z2, z3 = _dot_data(c)
    tau, alpha, B, B3, rows = c["tau"], c["alpha"], c["B"], c["B3"], c["rows"]
    if order is not None:
        z1, z2 = z1[order], z2[order]
    g1, g2 = torch.tensor(z1, device="cuda"), torch.tensor(z2, device="cuda")
    if c["part"] == "roll":
        return train_pair(g1, g2, torch.roll(g1, 1, 0), tau, alpha, pool_lse=lambda l: torch.roll(l, 1, 0))
    if B3 == B:
        return train_pair(g1, g2, g1, tau, alpha)
    chunks = [slice(c0, min(c0 + B, B3)) for c0 in range(0, B3, B)]
    lse_all = torch.cat([torch.tensor(train_pair(g1[sl], g2[sl], g1, tau, alpha, backward=False)["lse_i"]) for sl in chunks]).cuda()
    out = train_pair(g1[rows], g2[rows], g1, tau, alpha, pool_lse=lambda l: lse_all)
    assert np.array_equal(out["lse_i"], lse_all[rows].cpu().numpy())
    return out


def _dot_check(fam, c, out):
    z1, z2, z3 = _dot_data(c)
    _, d1, d2 = _dot_refs(c)
    # scale = 1: the floor of the gradients is the alignment pull of the LOCAL rows, 2 alpha / (B tau) max |z2| (the pooled gradients
    # are (B3 / B) x the oracle's gradient of the global mean, whose pull is 2 alpha / (B3 tau))
    check_vs_oracle(fam, _dot_id(c), out, z1, z2, z3, c["tau"], c["alpha"], rows=None if c["B3"] == c["B"] else c["rows"], scale=1.0,
                    dz1_ref=d1, dz2_ref=d2)


@gpu
@pytest.mark.parametrize("c", [c for c in DOT_CASES if c["part"] == "roll"], ids=_dot_id)
def test_dot_train_pair_widths_vs_oracle(c):
    """n in {1, 2, 33, 63, 64} (one coordinate, one pair, odd and even widths up to the last one the pair takes) at B = 65 and 300,
    pool = roll(z1) as the existing family."""
    _dot_check("simclr_train_pair_vs_oracle", c, _dot_run(c))


@gpu
@pytest.mark.parametrize("c", [c for c in DOT_CASES if c["part"] == "pooled"], ids=_dot_id)
def test_dot_train_pair_ragged_pools_vs_oracle(c):
    """Pools of (100, 257) and (129, 400) rows: B < B3 < 4 B, a ragged last chunk and a ragged last pool tile."""
    _dot_check("simclr_train_pair_pooled", c, _dot_run(c))


@gpu
@pytest.mark.parametrize("c", [c for c in DOT_CASES if c["part"] == "runmax"], ids=_dot_id)
def test_dot_running_maximum_both_orders(c):
    """Rows of norm 0.1 ... 3 at tau = 0.5, pool = z1, sorted by ascending norm (each later pool row raises the row maximum) and, in a
    second run, by descending norm: both against the oracle row by row after un-permuting; max |lse| < 20 (host-side guard), so the plain
    bound applies.  B = 200: every workgroup sees ONE 64-row pool tile (the plan streams more only from B > 2048), so the maximum moves in
    the merges of the partitions, waves and splits; B = 2304 (the one case above this file's size limit; its oracle is a 2304 x 2304
    matrix product) is the smallest multiple of 64 rows at which a workgroup streams two tiles and rescales its running sums."""
    fam = "simclr_train_pair_running_max"
    up = _dot_run(c)
    _dot_check(fam, dict(c, kind="ascending"), up)
    order = np.arange(c["B"])[::-1].copy()
    down = _dot_run(c, order)
    back = {k: (v if k == "means" else v[order]) for k, v in down.items()}        # the reversal is its own inverse
    _dot_check(fam, dict(c, kind="descending"), back)


class DotPair:
    def __init__(self, B, B3, n, tau=0.5, alpha=0.3):
        from cl_ica_amd import _lib
        self.L, self.lib = _lib, _lib.load()
        self.B, self.B3, self.n = B, B3, n
        self.d = _lib.DotLossDesc(B=B, B3=B3, n=n, tau=tau, alpha=alpha, normalize=0)
        self.nb = C.c_size_t()
        self.rc = self.lib.clica_dot_loss_train_workspace_bytes(C.byref(self.d), C.byref(self.nb))

    def run(self, z1, z2, pool, ldo=None, want=(True, True), backward=True, tick=None):
        """-> (stats [3, B], dz1 buffer or None, dz2 buffer or None, means [3]); an output not wanted is passed as NULL."""
        B, ldo = self.B, ldo or self.n
        ws = torch.zeros(self.nb.value, dtype=torch.uint8, device="cuda")
        stats = torch.full((3, B), SENTINEL, device="cuda")
        dzs = [torch.full((B, ldo), SENTINEL, device="cuda") if w else None for w in want]
        means = torch.full((3,), SENTINEL, device="cuda")
        p = [None if t is None else t.data_ptr() for t in dzs]
        st = self.L.stream_ptr()
        self.L.check(self.lib.clica_dot_loss_fwd_train(C.byref(self.d), z1.data_ptr(), z1.stride(0), z2.data_ptr(), z2.stride(0), pool.data_ptr(),
                                                       pool.stride(0), stats[0].data_ptr(), stats[1].data_ptr(), stats[2].data_ptr(), p[0], ldo,
                                                       p[1], ldo, ws.data_ptr(), ws.numel(), st), "dot fwd_train")
        if backward:
            self.L.check(self.lib.clica_dot_loss_bwd_sym_train(C.byref(self.d), z1.data_ptr(), z1.stride(0), pool.data_ptr(), pool.stride(0),
                                                           stats[2].data_ptr(), stats[2].data_ptr(), p[0], ldo, means.data_ptr(),
                                                           None if tick is None else tick.data_ptr(), ws.data_ptr(), ws.numel(), st), "dot bwd_sym_train")
        torch.cuda.synchronize()
        assert int(ws[:4 * ((B + 63) // 64)].view(torch.int32).abs().max()) == 0      # the arrival counters
        return stats, dzs[0], dzs[1], means


@gpu
@pytest.mark.parametrize("B,n", [(65, 33), (130, 2), (64, 64)])
def test_dot_train_pair_leading_dimensions_and_null_outputs(B, n):
    """Leading dimension n + 3 on inputs (NaN padding) and outputs (sentinel padding, untouched); dz1 = NULL, dz2 = NULL and both NULL in
    the forward: every other output keeps the bits of the full call; tick_counter NULL / non-NULL."""
    rng = np.random.default_rng(B + n)
    z1, z2 = make_rows(rng, B, n, 1.0)
    g1, g2 = torch.tensor(z1, device="cuda"), torch.tensor(z2, device="cuda")
    pair = DotPair(B, B, n)
    assert pair.rc == 0
    tick = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    stats, dz1, dz2, means = pair.run(g1, g2, g1, tick=tick)
    assert int(tick.item()) == 8
    for t in (stats, dz1, dz2, means):
        assert torch.isfinite(t).all() and not bool((t == SENTINEL).any())
    fwd_only = pair.run(g1, g2, g1, backward=False)
    v1, _ = _padded(z1, 3, float("nan"))
    v2, _ = _padded(z2, 3, float("nan"))
    s, a, b, m = pair.run(v1, v2, v1, ldo=n + 3)                                      # tick_counter NULL here
    assert torch.equal(s, stats) and torch.equal(m, means) and torch.equal(a[:, :n], dz1) and torch.equal(b[:, :n], dz2)
    assert bool((a[:, n:] == SENTINEL).all()) and bool((b[:, n:] == SENTINEL).all())
    for want in ((False, True), (True, False), (False, False)):
        s, a, b, _ = pair.run(g1, g2, g1, want=want, backward=False)
        assert torch.equal(s, fwd_only[0])
        assert a is None or torch.equal(a, fwd_only[1])
        assert b is None or torch.equal(b, fwd_only[2])
    s, a, b, m = pair.run(g1, g2, g1, want=(True, False))                             # dz2 = NULL through the whole pair
    assert torch.equal(s, stats) and torch.equal(a, dz1) and torch.equal(m, means) and b is None


@gpu
def test_dot_train_pair_rejects_65_coordinates():
    from cl_ica_amd import _lib
    pair = DotPair(8, 8, 65)
    assert pair.rc == E_INVALID
    z = torch.zeros(8, 65, device="cuda")
    out = torch.full((5, 8 * 65), SENTINEL, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    st = _lib.stream_ptr()
    rc_f = pair.lib.clica_dot_loss_fwd_train(C.byref(pair.d), z.data_ptr(), 65, z.data_ptr(), 65, z.data_ptr(), 65, out[0].data_ptr(), out[1].data_ptr(),
                                             out[2].data_ptr(), out[3].data_ptr(), 65, out[4].data_ptr(), 65, ws.data_ptr(), ws.numel(), st)
    rc_b = pair.lib.clica_dot_loss_bwd_sym_train(C.byref(pair.d), z.data_ptr(), 65, z.data_ptr(), 65, out[2].data_ptr(), out[2].data_ptr(),
                                                 out[3].data_ptr(), 65, out[0].data_ptr(), None, ws.data_ptr(), ws.numel(), st)
    torch.cuda.synchronize()
    assert rc_f == E_INVALID and rc_b == E_INVALID
    assert bool((out == SENTINEL).all()) and int(ws.abs().max()) == 0
