"""The small stand-alone kernels every training step runs through -- csrc/adam.hip with adam_math.h, csrc/heads.hip, csrc/mixing.hip --
against the fp64 restatements of tests/elementwise_oracle.py, at the sizes and values where such kernels go wrong: vector tails and
grid-stride loops beyond the launch caps, all five Adam entry points, ragged 256-row reductions, leading dimensions beyond n, NULL
outputs, saturated sigmoids, gradients parallel to x, signed zeros and denormals, every mixing activation on both sides of its branches.

Wherever cl_ica_amd.ops hides an argument (leading dimensions, NULL outputs) the call goes through ctypes on the C ABI.  The Adam bounds
(2 / 3 / 4 eps32, elementwise_oracle.ADAM_*_LIMIT) are the ones tests/test_elementwise_host.py shows plain fp32 arithmetic to keep.  Lines
that start with MEASURED carry the figures DESIGN.md quotes (pytest -s)."""

import numpy as np
import pytest
import torch

import elementwise_oracle as E
from conftest import PARITY

pytestmark = pytest.mark.gpu
E_INVALID = -1          # include/clica.h
SENTINEL = -777.25
NEG_ZERO = 0x80000000


def dev(a):
    return torch.tensor(np.asarray(a, np.float32), device="cuda")


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return host(t).view(np.uint32)


@pytest.fixture(scope="module")
def lib():
    from cl_ica_amd import _lib
    return _lib.load()


def stream():
    from cl_ica_amd import _lib
    return _lib.stream_ptr()


def i32(value=0):
    return torch.full((1,), int(value), dtype=torch.int32, device="cuda")


# ====================================================================================================================== Adam
ADAM_COUNTS = [1, 2, 3, 4, 5, 7, 1023, 1025, 262_147, 2_097_152 + 1029]      # the last two pass the ticket cap (256 x 1024 elements) / the plain cap (2048 x 1024)
ADAM_FORMS = ["plain", "at1", "at0", "tick", "s16", "s16_tick"]
TAIL = 64


class Arena:
    """p, g, m, v on the device, each followed by 64 sentinel floats."""

    def __init__(self, p, g, m, v):
        self.count = int(np.asarray(p).size)
        self.t = {}
        for k, a in (("p", p), ("g", g), ("m", m), ("v", v)):
            buf = torch.full((self.count + TAIL,), SENTINEL, dtype=torch.float32, device="cuda")
            buf[:self.count] = dev(a)
            assert buf.data_ptr() % 16 == 0
            self.t[k] = buf

    def ptrs(self, offset=None):
        """The four base pointers (offset = {"p": 1}: that arena starts one float later, i.e. not 16-byte aligned)."""
        return [self.t[k].data_ptr() + 4 * (offset or {}).get(k, 0) for k in "pgmv"]

    def get(self, k):
        return host(self.t[k][:self.count])

    def tails_intact(self):
        want = np.float32(SENTINEL).view(np.uint32)
        return all((bits(self.t[k][self.count:]) == want).all() for k in "pgmv")


def adam_call(lib, form, ptrs, count, combo, step, ticket=None, s16=None, t_offset=None):
    """One launch of the entry point `form` names; returns the C return code."""
    b1, b2, eps, gs, lr = combo
    common = list(ptrs) + [count, lr, b1, b2, eps, gs]
    tk = None if ticket is None else ticket.data_ptr()
    if form == "plain":
        return lib.clica_adam_step(*common, step.data_ptr(), stream())
    if form in ("at1", "at0"):
        return lib.clica_adam_step_at(*common, step.data_ptr(), (1 if form == "at1" else 0) if t_offset is None else t_offset, stream())
    if form == "tick":
        return lib.clica_adam_step_tick(*common, step.data_ptr(), tk, stream())
    if form == "s16":
        return lib.clica_adam_step_s16(*common, step.data_ptr(), 1 if t_offset is None else t_offset, s16.buf.data_ptr(), s16.n_layers, stream())
    if form == "s16_tick":
        return lib.clica_adam_step_s16_tick(*common, step.data_ptr(), tk, s16.buf.data_ptr(), s16.n_layers, stream())
    raise ValueError(form)


def assert_update_within_limits(A, p, g, m, v, t, combo, what):
    e = E.adam_errors(A.get("m"), A.get("v"), A.get("p"), p, g, m, v, t, combo)
    print(f"MEASURED adam/update {what}: m {e['m']:.3f} v {e['v']:.3f} p {e['p']:.3f} eps32, v below {E.ADAM_V_TINY:g}: {e['v_tiny']:.2e}")
    assert e["m"] <= E.ADAM_M_LIMIT, (what, "exp_avg", e)
    assert e["v"] <= E.ADAM_V_LIMIT and e["v_tiny"] <= E.ADAM_V_TINY, (what, "exp_avg_sq", e)
    assert e["p"] <= E.ADAM_P_LIMIT, (what, "param", e)
    assert e["moved"] == 0, (what, "a parameter with g = m = v = 0 changed", e)
    assert np.array_equal(A.get("g").view(np.uint32), np.asarray(g, np.float32).view(np.uint32)), (what, "the gradient arena was written")
    assert A.tails_intact(), (what, "wrote behind count")
    return e


@pytest.mark.parametrize("combo", range(len(E.ADAM_COMBOS)), ids=lambda c: "b1_{}-b2_{}-eps_{}-gs_{:.3g}-lr_{}".format(*E.ADAM_COMBOS[c]))
def test_adam_single_update_from_arbitrary_state(lib, combo):
    """One update from a state written to the device, over 31 decades of gradient and nine step numbers: every element of m', v' and p'
    inside the limits plain fp32 keeps (eps inside the root, before the bias correction, a float bias correction, a gradient scale
    missing from g^2 are all far outside)."""
    worst = dict(m=0.0, v=0.0, p=0.0)
    for t in E.ADAM_TS:
        p, g, m, v = E.adam_state(combo, t, 100_000)
        A = Arena(p, g, m, v)
        step = i32(t - 1)
        assert adam_call(lib, "plain", A.ptrs(), A.count, E.ADAM_COMBOS[combo], step) == 0
        e = assert_update_within_limits(A, p, g, m, v, t, E.ADAM_COMBOS[combo], f"combo {combo} t {t}")
        assert e["n_zero"] >= 50 and int(step.item()) == t - 1
        for k in worst:
            worst[k] = max(worst[k], e[k])
    print(f"MEASURED adam/update combo {combo} worst: m {worst['m']:.3f} / {E.ADAM_M_LIMIT:g}, v {worst['v']:.3f} / {E.ADAM_V_LIMIT:g}, "
          f"p {worst['p']:.3f} / {E.ADAM_P_LIMIT:g} eps32")


def plain_state(count, seed):
    rng = np.random.default_rng([13, count, seed])
    g = (rng.normal(size=count) * 10.0 ** rng.uniform(-3, 1, size=count)).astype(np.float32)
    m = (rng.normal(size=count) * 10.0 ** rng.uniform(-3, 1, size=count)).astype(np.float32)
    v = ((rng.normal(size=count) * 10.0 ** rng.uniform(-3, 1, size=count)) ** 2).astype(np.float32)
    return rng.normal(size=count).astype(np.float32), g, m, v


@pytest.mark.parametrize("count", ADAM_COUNTS)
def test_adam_sizes_tails_and_grid_stride(lib, count):
    """Every element of every size is updated once and correctly (float4 body, scalar tail of 1..3, grid stride beyond the launch cap),
    nothing behind `count` is written."""
    p, g, m, v = plain_state(count, 0)
    for form in ("plain", "tick"):      # 2048 and 256 workgroups at most
        A = Arena(p, g, m, v)
        step, ticket = i32(6), i32(0)
        assert adam_call(lib, form, A.ptrs(), count, E.ADAM_COMBOS[0], step, ticket=ticket) == 0
        assert_update_within_limits(A, p, g, m, v, 7, E.ADAM_COMBOS[0], f"count {count} {form}")
        # (the limits also say that no element was skipped or updated twice: an untouched m is 0.1 |g - m| / eps32 summands off)


def test_adam_refuses_unaligned_and_bad_arguments(lib):
    from cl_ica_amd import ops
    count = 1023
    p, g, m, v = plain_state(count + 1, 1)
    A = Arena(p, g, m, v)
    before = {k: bits(A.t[k]).copy() for k in "pgmv"}
    step, ticket = i32(3), i32(0)
    s16 = ops.Split16(3, "cuda")
    for form in ("plain", "at1", "tick", "s16", "s16_tick"):
        for k in "pgmv":
            assert adam_call(lib, form, A.ptrs({k: 1}), count, E.ADAM_COMBOS[0], step, ticket=ticket, s16=s16) == E_INVALID, (form, k)
    assert b"16-byte" in lib.clica_last_error()
    for form in ("at1", "s16"):
        for off in (2, -1):
            assert adam_call(lib, form, A.ptrs(), count, E.ADAM_COMBOS[0], step, s16=s16, t_offset=off) == E_INVALID, (form, off)
    for form in ("tick", "s16_tick"):
        assert adam_call(lib, form, A.ptrs(), count, E.ADAM_COMBOS[0], step, ticket=None, s16=s16) == E_INVALID, form
    assert adam_call(lib, "plain", A.ptrs(), 0, E.ADAM_COMBOS[0], step) == E_INVALID
    torch.cuda.synchronize()
    for k in "pgmv":
        assert np.array_equal(bits(A.t[k]), before[k]), k
    assert int(step.item()) == 3 and int(ticket.item()) == 0 and s16.guard()["updates"] == 0


@pytest.mark.parametrize("count", ADAM_COUNTS)
def test_adam_entry_points_agree_bit_for_bit(lib, count):
    """clica_adam_step, _at (t_offset 1, and 0 on a counter clica_tick advanced first), _tick, _s16 and _s16_tick launch different grids
    (the ticket forms cap at 256 workgroups, the s16 forms start 27 workgroups later): identical p, m, v over three consecutive updates,
    the counter advanced by the tick forms alone, by exactly one."""
    from cl_ica_amd import ops
    p, g0, m, v = plain_state(count, 2)
    grads = [g0] + [plain_state(count, 3 + k)[1] for k in range(2)]
    t0, combo = 6, E.ADAM_COMBOS[1]
    results = {}
    for form in ADAM_FORMS:
        A = Arena(p, grads[0], m, v)
        step, ticket = i32(t0), i32(0)
        s16 = ops.Split16(3, "cuda") if form.startswith("s16") else None
        for k, g in enumerate(grads):
            A.t["g"][:count] = dev(g)
            if form == "at0":
                ops.tick(step)
            before = int(step.item())
            assert adam_call(lib, form, A.ptrs(), count, combo, step, ticket=ticket, s16=s16) == 0, (form, k)
            after = int(step.item())
            if form in ("tick", "s16_tick"):
                assert after == before + 1 and int(ticket.item()) == 0, (form, k, before, after)
            else:
                assert after == before, (form, k, "the counter moved")
                if form != "at0":
                    ops.tick(step)
            assert int(step.item()) == t0 + k + 1
            if s16 is not None:
                gd = s16.guard()
                assert gd["updates"] == k + 1 and gd["flags"] == 0 and gd["skipped"] == 0 and not gd["poisoned"], (form, k, gd)
        assert A.tails_intact(), form
        results[form] = {x: A.get(x).view(np.uint32) for x in "pmv"}
    for form in ADAM_FORMS[1:]:
        for x in "pmv":
            assert np.array_equal(results[form][x], results["plain"][x]), (form, x, count)
    assert (results["plain"]["p"] != np.asarray(p).view(np.uint32)).any()


_TRAJ = {}


def trajectory_references(b2):
    """torch.optim.Adam on the CPU in float64 (the truth) and float32 (the reference), computed once per beta2."""
    if b2 not in _TRAJ:
        p0, grads = E.adam_trajectory_grads()
        _TRAJ[b2] = (p0, grads, E.adam_trajectory_torch(p0, grads, torch.float64, betas=(0.9, b2)),
                     E.adam_trajectory_torch(p0, grads, torch.float32, betas=(0.9, b2)))
    return _TRAJ[b2]


@pytest.mark.parametrize("b2", [0.999, 0.875])
def test_adam_200_step_trajectory_against_torch(b2):
    """200 steps on 4099 elements whose gradient scales span eight decades.  Parameters and exp_avg: no further from torch's float64 run
    than 4 x torch's own float32 run, element-wise.  exp_avg_sq against torch's FLOAT32 state: the C ABI takes fp32 betas and forms
    1.f - beta2 from them, 0.00099998713 at beta2 = 0.999, where torch multiplies by float(1 - 0.999) = 0.0010000000475:
        |fl32(1 - beta2) - (1 - fl32(beta2))| / (1 - beta2) = 1.29e-5
    -- a property of the ABI, not of the arithmetic (the bias correction uses the same fp32 beta2, so the parameters agree).  Hence 2e-5
    there, and 4 eps32 at beta2 = 0.875, which is an fp32 number."""
    from cl_ica_amd import ops
    p0, grads, (p64, m64, v64), (p32, m32, v32) = trajectory_references(b2)
    p = dev(p0); m = torch.zeros_like(p); v = torch.zeros_like(p)
    step, ticket = i32(0), i32(0)
    for g in grads:
        ops.adam_step(p, dev(g), m, v, step, lr=1e-3, beta1=0.9, beta2=b2, eps=1e-8, ticket=ticket)
    assert int(step.item()) == len(grads) == 200
    PARITY.check_elementwise("adam/trajectory", f"beta2={b2}", "param", host(p), p32, p64)
    PARITY.check_elementwise("adam/trajectory", f"beta2={b2}", "exp_avg", host(m), m32, m64)
    PARITY.check("adam/trajectory", f"beta2={b2}", "param", host(p), p64)
    rel = float((np.abs(host(v).astype(np.float64) - v32) / v32).max())
    bound = 2e-5 if b2 == 0.999 else 4 * E.EPS32
    print(f"MEASURED adam/trajectory beta2 {b2}: exp_avg_sq against torch float32, max relative difference {rel:.3e} (bound {bound:.3e}, "
          f"complement gap {E.beta2_complement_gap(b2):.3e})")
    assert rel <= bound, (b2, rel)


# ====================================================================================================================== heads
HEAD_SHAPES = [(1, 1), (1, 10), (255, 3), (256, 10), (257, 10), (513, 64), (1000, 129), (12_289, 10)]
HEAD_CASES = [(M, n, pad) for (M, n) in HEAD_SHAPES for pad in (0, 3)]
EXTRA_ROWS = 2


def head_id(c):
    return f"M{c[0]}-n{c[1]}-ld{c[1] + c[2]}"


def filled(shape, value=-0.0):
    return torch.full(shape, value, dtype=torch.float32, device="cuda")


def out_buffer(M, ld):
    return filled((M + EXTRA_ROWS, ld))


def assert_padding(buf, M, n, what):
    assert (E.padding_bits(host(buf), M, n) == NEG_ZERO).all(), (what, "padding columns / rows behind M were written")


def vec_buffer(k):
    return filled((k + 4,))


def assert_vec_tail(buf, k, what):
    assert (bits(buf[k:]) == NEG_ZERO).all(), (what, "wrote behind its last element")


def rescale_inputs(M, n, pad, parallel):
    rng = np.random.default_rng([21, M, n, pad, int(parallel)])
    d = rng.normal(size=(M, n))
    x = (d / np.linalg.norm(d, axis=-1, keepdims=True) * 10.0 ** rng.uniform(-3, 3, size=(M, 1))).astype(np.float32)
    if parallel:      # dy_i = c_i x_i, |dy_i| = 10 sqrt(n): ten times the random gradients, dy - u <dy, u> cancels completely
        c = np.where(rng.random((M, 1)) < 0.5, -1.0, 1.0) * 10.0 * np.sqrt(n) / np.linalg.norm(x.astype(np.float64), axis=-1, keepdims=True)
        dy = (c * x.astype(np.float64)).astype(np.float32)
    else:
        dy = rng.normal(size=(M, n)).astype(np.float32)
    return x, dy


@pytest.mark.parametrize("parallel", [False, True], ids=["random_dy", "parallel_dy"])
@pytest.mark.parametrize("case", HEAD_CASES, ids=head_id)
def test_rescale_head(lib, case, parallel):
    M, n, pad = case
    ld = n + pad
    x, dy = rescale_inputs(M, n, pad, parallel)
    X, DY = dev(E.padded(x, ld, EXTRA_ROWS)), dev(E.padded(dy, ld, EXTRA_ROWS))
    nb = (M + 255) // 256
    for r in (0.3, 1.7):
        name = f"{head_id(case)}-r{r}" + ("-parallel" if parallel else "")
        R = dev([r])
        y_ref, inv_ref = E.rescale_fwd(x, E.f32(r))
        dx_ref, dr_ref, dx_floor, dr_floor = E.rescale_bwd(x, E.f32(r), dy)
        # forward, inv_norm present and NULL
        Y, INV = out_buffer(M, ld), vec_buffer(M)
        assert lib.clica_rescale_fwd(X.data_ptr(), ld, R.data_ptr(), Y.data_ptr(), ld, INV.data_ptr(), M, n, stream()) == 0
        Y2 = out_buffer(M, ld)
        assert lib.clica_rescale_fwd(X.data_ptr(), ld, R.data_ptr(), Y2.data_ptr(), ld, None, M, n, stream()) == 0
        assert torch.equal(Y.view(torch.int32), Y2.view(torch.int32))
        assert_padding(Y, M, n, name + " y"); assert_vec_tail(INV, M, name + " inv_norm")
        y, inv = host(Y)[:M, :n], host(INV)[:M]
        PARITY.check("heads/rescale", name, "y", y, y_ref)
        PARITY.check("heads/rescale", name, "inv_norm", inv, inv_ref)
        inv_rel = float(np.abs(inv / inv_ref - 1.0).max())      # row by row as well: (n + 3) roundings at most
        assert inv_rel <= 1e-5, (name, inv_rel)
        # backward on the kernel's own inv_norm: all outputs, dX alone, dr alone
        DX, PART = out_buffer(M, ld), vec_buffer(nb)
        args = (X.data_ptr(), ld, R.data_ptr(), INV.data_ptr(), DY.data_ptr(), ld)
        assert lib.clica_rescale_bwd(*args, DX.data_ptr(), ld, PART.data_ptr(), M, n, stream()) == 0
        DX2, PART2 = out_buffer(M, ld), vec_buffer(nb)
        assert lib.clica_rescale_bwd(*args, DX2.data_ptr(), ld, None, M, n, stream()) == 0
        assert lib.clica_rescale_bwd(*args, None, 0, PART2.data_ptr(), M, n, stream()) == 0
        assert torch.equal(DX.view(torch.int32), DX2.view(torch.int32)) and torch.equal(PART.view(torch.int32), PART2.view(torch.int32))
        assert_padding(DX, M, n, name + " dx"); assert_vec_tail(PART, nb, name + " dr_partial")
        e_dx = PARITY.check("heads/rescale", name, "dx", host(DX)[:M, :n], dx_ref, floor=dx_floor)
        e_dr = PARITY.check("heads/rescale", name, "dr", [float(PART[:nb].sum().item())], [dr_ref], floor=dr_floor)
        print(f"MEASURED heads/rescale {name}: inv_norm row-wise {inv_rel:.2e}, dx {e_dx:.2e}, dr {e_dr:.2e}")
    assert_padding(X, M, n, "x"); assert_padding(DY, M, n, "dy")


SOFTCLIP_SPECIALS = [80.0, -80.0, 30.0, -30.0, 60.0, -60.0, 0.0, -0.0]


def softclip_inputs(M, n, pad):
    """x from U(-8, 8); the saturated and zero values as whole columns 0..7 where n >= 8, spread over the array otherwise."""
    rng = np.random.default_rng([22, M, n, pad])
    x = rng.uniform(-8, 8, size=(M, n)).astype(np.float32)
    sp = np.asarray(SOFTCLIP_SPECIALS, np.float32)
    if n >= 8:
        x[:, :8] = sp[None, :]
    else:
        flat = x.reshape(-1)
        k = min(8, flat.size)
        flat[np.arange(k) * (flat.size // k)] = np.roll(sp, pad)[:k]
    bound = (10.0 ** rng.uniform(-2, 2, size=n)).astype(np.float32)
    dy = rng.normal(size=(M, n)).astype(np.float32)
    return x, bound, dy


@pytest.mark.parametrize("case", HEAD_CASES, ids=head_id)
def test_softclip_head(lib, case):
    M, n, pad = case
    ld = n + pad
    name = head_id(case)
    x, bound, dy = softclip_inputs(M, n, pad)
    X, DY, Bd = dev(E.padded(x, ld, EXTRA_ROWS)), dev(E.padded(dy, ld, EXTRA_ROWS)), dev(bound)
    nb = (M + 255) // 256
    y_ref = E.softclip_fwd(x, bound)
    dx_ref, db_ref, db_floor = E.softclip_bwd(x, bound, dy)
    s32 = torch.sigmoid(torch.tensor(x))
    y32 = (s32 * torch.tensor(bound)).numpy()
    dx32 = (torch.tensor(dy) * torch.tensor(bound) * s32 * (1 - s32)).numpy()
    Y = out_buffer(M, ld)
    assert lib.clica_softclip_fwd(X.data_ptr(), ld, Bd.data_ptr(), Y.data_ptr(), ld, M, n, stream()) == 0
    assert_padding(Y, M, n, name + " y")
    y = host(Y)[:M, :n]
    DX, PART = out_buffer(M, ld), vec_buffer(nb * n)
    args = (X.data_ptr(), ld, Bd.data_ptr(), DY.data_ptr(), ld)
    assert lib.clica_softclip_bwd(*args, DX.data_ptr(), ld, PART.data_ptr(), M, n, stream()) == 0
    DX2, PART2 = out_buffer(M, ld), vec_buffer(nb * n)
    assert lib.clica_softclip_bwd(*args, DX2.data_ptr(), ld, None, M, n, stream()) == 0
    assert lib.clica_softclip_bwd(*args, None, 0, PART2.data_ptr(), M, n, stream()) == 0
    assert torch.equal(DX.view(torch.int32), DX2.view(torch.int32)) and torch.equal(PART.view(torch.int32), PART2.view(torch.int32))
    assert_padding(DX, M, n, name + " dx"); assert_vec_tail(PART, nb * n, name + " dbound_partial")
    dx = host(DX)[:M, :n]
    db = host(PART[:nb * n].reshape(nb, n).sum(0))
    assert np.isfinite(y).all() and np.isfinite(dx).all() and np.isfinite(db).all(), (name, "NaN / inf at a saturated input")
    e_y = PARITY.check("heads/softclip", name, "y", y, y_ref)
    e_dx = PARITY.check("heads/softclip", name, "dx", dx, dx_ref)
    PARITY.check_elementwise("heads/softclip", name, "y", y, y32, y_ref)
    PARITY.check_elementwise("heads/softclip", name, "dx", dx, dx32, dx_ref)
    e_db = max(PARITY.check("heads/softclip", name, f"dbound[{k}]", db[k:k + 1], db_ref[k:k + 1], floor=float(db_floor[k])) for k in range(n))
    print(f"MEASURED heads/softclip {name}: y {e_y:.2e}, dx {e_dx:.2e}, dbound (worst column) {e_db:.2e}")
    assert_padding(X, M, n, "x"); assert_padding(DY, M, n, "dy")


def test_heads_refuse_bad_arguments(lib):
    X, R, Y = filled((4, 5), 1.0), dev([1.0]), filled((4, 5))
    s = stream()
    assert lib.clica_rescale_fwd(X.data_ptr(), 4, R.data_ptr(), Y.data_ptr(), 5, None, 4, 5, s) == E_INVALID       # ldx < n
    assert lib.clica_rescale_fwd(X.data_ptr(), 5, R.data_ptr(), Y.data_ptr(), 5, None, 0, 5, s) == E_INVALID       # M = 0
    assert lib.clica_rescale_bwd(X.data_ptr(), 5, R.data_ptr(), None, X.data_ptr(), 5, Y.data_ptr(), 5, None, 4, 5, s) == E_INVALID      # no inv_norm
    assert lib.clica_rescale_bwd(X.data_ptr(), 5, R.data_ptr(), X.data_ptr(), X.data_ptr(), 5, Y.data_ptr(), 4, None, 4, 5, s) == E_INVALID   # lddx < n
    assert lib.clica_softclip_fwd(X.data_ptr(), 5, None, Y.data_ptr(), 5, 4, 5, s) == E_INVALID                    # no bound
    assert lib.clica_softclip_bwd(X.data_ptr(), 5, X.data_ptr(), X.data_ptr(), 4, Y.data_ptr(), 5, None, 4, 5, s) == E_INVALID         # lddy < n
    torch.cuda.synchronize()
    assert (bits(Y) == NEG_ZERO).all()


# ---------------------------------------------------------------------------------------------------------------------- LeakyReLU
LEAKY_SPECIALS = [0.0, -0.0, 1e-40, -1e-40, 1.17549435e-38, -1.17549435e-38, 3e38, -3e38]


@pytest.mark.parametrize("case", [(1, 1, 0), (1, 10, 3), (257, 10, 0), (257, 10, 3), (1000, 129, 3), (12_289, 10, 0)], ids=head_id)
def test_leaky_relu_bit_exact(lib, case):
    """A single multiply: bit for bit the NumPy fp32 result, forward and backward, zeros, signed zeros, denormals and the largest
    magnitudes included; the backward reads the forward's own output (slope 0 = ReLU still carries the gate)."""
    M, n, pad = case
    ld = n + pad
    rng = np.random.default_rng([23, M, n, pad])
    x = rng.normal(size=(M, n)).astype(np.float32); dy = rng.normal(size=(M, n)).astype(np.float32)
    sp = np.asarray(LEAKY_SPECIALS, np.float32)
    k = min(sp.size, x.size)
    x.reshape(-1)[:k] = np.roll(sp, pad)[:k]
    if x.size > 24:
        x.reshape(-1)[16:24] = np.float32(-1.0) * sp      # ... and the specials under a random upstream gradient and as the gradient itself
        dy.reshape(-1)[8:24] = np.concatenate([sp, sp])
    X, DY = dev(E.padded(x, ld, EXTRA_ROWS)), dev(E.padded(dy, ld, EXTRA_ROWS))
    assert np.array_equal(bits(X)[:M, :n], x.view(np.uint32))      # the upload keeps denormals and signed zeros
    for slope in (0.01, 0.2, 1.0, 0.0):
        sl = np.float32(slope)
        with np.errstate(all="ignore"):
            y_ref = np.where(x > 0, x, sl * x).astype(np.float32)
            dx_ref = np.where(y_ref > 0, dy, sl * dy).astype(np.float32)
        # (the fp64 product of two fp32 numbers is exact, so the oracle rounded once IS the fp32 product)
        assert np.array_equal(y_ref, E.leaky_fwd(x, sl).astype(np.float32)) and np.array_equal(dx_ref, E.leaky_bwd(y_ref, dy, sl).astype(np.float32))
        Y = out_buffer(M, ld)
        assert lib.clica_leaky_relu_fwd(X.data_ptr(), ld, Y.data_ptr(), ld, M, n, float(slope), stream()) == 0
        got = bits(Y)[:M, :n]
        assert np.array_equal(got, y_ref.view(np.uint32)), (slope, "forward", x.reshape(-1)[got.reshape(-1) != y_ref.view(np.uint32).reshape(-1)][:8])
        assert_padding(Y, M, n, f"leaky y slope {slope}")
        DX = out_buffer(M, ld)
        assert lib.clica_leaky_relu_bwd(Y.data_ptr(), ld, DY.data_ptr(), ld, DX.data_ptr(), ld, M, n, float(slope), stream()) == 0
        assert np.array_equal(bits(DX)[:M, :n], dx_ref.view(np.uint32)), (slope, "backward")
        assert_padding(DX, M, n, f"leaky dx slope {slope}")
        assert np.array_equal(y_ref > 0, x > 0)      # the gate recovered from the output is the gate of the input
    DX = out_buffer(M, ld)
    assert lib.clica_leaky_relu_bwd(X.data_ptr(), ld, DY.data_ptr(), ld, DX.data_ptr(), ld, M, n, -0.01, stream()) == E_INVALID
    torch.cuda.synchronize()
    assert (bits(DX) == NEG_ZERO).all()


def test_leaky_relu_layer_3d_against_torch():
    from cl_ica_amd import layers
    rng = np.random.default_rng(24)
    x = rng.normal(size=(5, 7, 10)).astype(np.float32); gy = rng.normal(size=(5, 7, 10)).astype(np.float32)
    x[0, 0, :4] = [0.0, -0.0, 1e-40, -1e-40]
    for slope in (0.01, 0.2):
        xt = dev(x).requires_grad_(True)
        y = layers.LeakyReLU(slope)(xt)
        y.backward(dev(gy))
        xr = torch.tensor(x, requires_grad=True)
        yr = torch.nn.functional.leaky_relu(xr, slope)
        yr.backward(torch.tensor(gy))
        assert y.shape == (5, 7, 10) and xt.grad.shape == (5, 7, 10)
        assert np.array_equal(bits(y), yr.detach().numpy().view(np.uint32)) and np.array_equal(bits(xt.grad), xr.grad.numpy().view(np.uint32))
    with pytest.raises(ValueError):
        layers.LeakyReLU(0.0)


# ====================================================================================================================== mixing net
MIX_N, MIX_L = [1, 2, 3, 10, 33, 64, 72], [1, 2, 3, 5]
MIX_ACTS = [(0, 0.0), (0, 0.2), (1, 1.0), (1, 0.5), (2, 0.2), (3, 0.5), (3, 1.0), (3, 3.0)]
MIX_TARGETS = [1.0, 60.0]
MIX_KIND_NAME = {v: k for k, v in E.MIX_KINDS.items()}


def mix_call(lib, Z, ldz, W, L, kind, a, Xo, ldx, M, n):
    return lib.clica_mixing_fwd_act(Z.data_ptr(), ldz, W.data_ptr(), L, kind, float(a), Xo.data_ptr(), ldx, M, n, stream())


@pytest.mark.parametrize("L", MIX_L)
@pytest.mark.parametrize("n", MIX_N)
def test_mixing_net_every_activation(lib, n, L):
    """All four hidden activations at pre-activations of order 1 and of order 60 (both sides of Softplus's beta v > 20 switch, expm1 and
    log(1 + e^v) far out), block sizes from one row (n > 256 is out of LDS reach: three rows at n = 72) to the 64-row clamp, ragged last
    blocks, every second case strided."""
    lds, rows = E.mixing_lds_bytes(n, L)
    z_all = np.random.default_rng([31, n]).normal(size=(1000, n)).astype(np.float32)
    if lds > 64 * 1024:
        W = filled((L, n, n), 0.0); Xo = filled((4, n))
        assert mix_call(lib, dev(z_all[:4]), n, W, L, 0, 0.2, Xo, n, 4, n) == E_INVALID
        torch.cuda.synchronize()
        assert (bits(Xo) == NEG_ZERO).all()
        return
    k = 0
    worst = {}
    for kind, a in MIX_ACTS:
        for target in MIX_TARGETS:
            Ws = E.mixing_weights(z_all, L, kind, E.f32(a), target, seed=[32, n, L, kind])
            pre = []
            ref_all = E.mixing_forward(list(Ws), z_all, kind, E.f32(a), pre=pre)
            top = max([float(np.abs(v).max()) for v in pre], default=0.0)
            assert top < 80.0, (n, L, kind, a, target, top)      # beyond 88 the reference's own fp32 log(1 + exp(x)) overflows
            if L > 1:
                assert top > 0.99 * target
            Wd = dev(Ws)
            for M in (1, rows - 1, rows + 1, 1000):
                pad = 5 if k % 2 else 0
                k += 1
                ld = n + pad
                Z, Xo = dev(E.padded(z_all[:M], ld, 1)), filled((M + 1, ld))
                assert mix_call(lib, Z, ld, Wd, L, kind, a, Xo, ld, M, n) == 0
                name = f"n{n}-L{L}-{MIX_KIND_NAME[kind]}({a})-pre{target:g}-M{M}-ld{ld}"
                err = PARITY.check(f"mixing_act/{MIX_KIND_NAME[kind]}", name, "x", host(Xo)[:M, :n], ref_all[:M])
                assert_padding(Xo, M, n, name)
                key = (MIX_KIND_NAME[kind], target)
                worst[key] = max(worst.get(key, 0.0), err)
    assert k == len(MIX_ACTS) * len(MIX_TARGETS) * 4
    print(f"MEASURED mixing_act n {n} L {L}: " + ", ".join(f"{kn} pre{t:g} {e:.2e}" for (kn, t), e in sorted(worst.items())))


def test_mixing_lds_limit_and_bad_kind(lib):
    z = dev(np.abs(np.random.default_rng(33).normal(size=(5, 73))))
    for n, L, ok in ((72, 3, True), (73, 3, False), (64, 4, False), (64, 3, True)):
        W = dev(np.stack([np.eye(n)] * L)); Xo = filled((5, n))
        Zs = z[:, :n].contiguous()
        rc = mix_call(lib, Zs, n, W, L, 0, 0.2, Xo, n, 5, n)
        assert rc == (0 if ok else E_INVALID), (n, L, rc)
        if ok:
            assert torch.equal(Xo, Zs)      # identity layers on positive rows
        else:
            assert b"LDS" in lib.clica_last_error() and (bits(Xo) == NEG_ZERO).all()
    W = dev(np.eye(4)[None]); Z4 = filled((3, 4), 1.0); Xo = filled((3, 4))
    for kind in (-1, 4, 17):
        assert mix_call(lib, Z4, 4, W, 1, kind, 0.2, Xo, 4, 3, 4) == E_INVALID, kind
    assert mix_call(lib, Z4, 3, W, 1, 0, 0.2, Xo, 4, 3, 4) == E_INVALID          # ldz < n
    assert mix_call(lib, Z4, 4, W, 0, 0, 0.2, Xo, 4, 3, 4) == E_INVALID          # no layer
    torch.cuda.synchronize()
    assert (bits(Xo) == NEG_ZERO).all()


def test_mixing_strided_out_through_ops():
    from cl_ica_amd import ops
    n, M, L = 10, 257, 3
    rng = np.random.default_rng(34)
    zbig = rng.normal(size=(M, n + 4)).astype(np.float32)
    for kind, a in ((2, 0.2), (3, 1.0)):
        Ws = E.mixing_weights(zbig[:, 2:2 + n], L, kind, E.f32(a), 10.0, seed=35)
        ref = E.mixing_forward(list(Ws), zbig[:, 2:2 + n], kind, E.f32(a))
        Zb = dev(zbig); big = filled((M, n + 5))
        out = ops.mixing_fwd(Zb[:, 2:2 + n], dev(Ws), a, out=big[:, 3:3 + n], act_kind=kind)
        assert out.data_ptr() == big[:, 3:3 + n].data_ptr()
        PARITY.check(f"mixing_act/{MIX_KIND_NAME[kind]}", f"strided out n{n} M{M}", "x", host(big)[:, 3:3 + n], ref)
        rest = host(big).view(np.uint32).copy(); rest[:, 3:3 + n] = NEG_ZERO
        assert (rest == NEG_ZERO).all()
