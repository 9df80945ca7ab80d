"""tests/elementwise_oracle.py without a GPU: (a) every fp64 helper against an independent float64 construction (torch.nn.functional with
torch.autograd, torch.optim.Adam), (b) a NumPy fp32 emulation of adam_math.h::update, operation by operation, held to the bounds that
tests/test_gpu_elementwise.py asserts of the kernel -- so those bounds rest on plain fp32 arithmetic and never on the code under test."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elementwise_oracle as E

EMU_COUNT = 200_000


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


def close(got, want, tol=1e-12):
    got = np.asarray(got, np.float64); want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    den = max(float(np.abs(want).max()), 1e-300)
    assert float(np.abs(got - want).max()) / den <= tol, float(np.abs(got - want).max()) / den


# ============================================================================================== (a) the helpers against torch in float64
@pytest.mark.parametrize("M,n", [(1, 1), (7, 3), (300, 10), (33, 129)])
def test_rescale_helpers_against_autograd(M, n):
    rng = np.random.default_rng([1, M, n])
    x = rng.normal(size=(M, n)) * 10.0 ** rng.uniform(-3, 3, size=(M, 1)); dy = rng.normal(size=(M, n)); r = 1.7
    xt, rt = t64(x, True), t64([r], True)
    y = F.normalize(xt, p=2.0, dim=-1, eps=0.0) * rt
    y.backward(t64(dy))
    yo, inv = E.rescale_fwd(x, r)
    dx, dr, dx_floor, dr_floor = E.rescale_bwd(x, r, dy)
    close(yo, y.detach().numpy()); close(inv, 1.0 / np.linalg.norm(x, axis=-1))
    close(dr, float(rt.grad), 1e-11 * max(1.0, dr_floor / max(abs(dr), 1e-300)))
    assert float(np.abs(dx - xt.grad.numpy()).max()) <= 1e-12 * dx_floor      # a cancelling difference: judged against its terms
    assert dx_floor >= float(np.abs(dx).max()) * (0.5 if n > 1 else 0.0) and dr_floor >= abs(dr)


def test_rescale_parallel_gradient_cancels():
    rng = np.random.default_rng(2)
    x = rng.normal(size=(50, 10))
    dx, dr, dx_floor, _ = E.rescale_bwd(x, 0.3, 7.0 * x)
    assert float(np.abs(dx).max()) <= 1e-14 * dx_floor
    close(dr, 7.0 * np.linalg.norm(x, axis=-1).sum())


@pytest.mark.parametrize("M,n", [(1, 1), (40, 10), (257, 13)])
def test_softclip_helpers_against_autograd(M, n):
    rng = np.random.default_rng([3, M, n])
    x = rng.uniform(-8, 8, size=(M, n))
    k = min(8, x.size)
    x.reshape(-1)[:k] = np.asarray([80.0, -80.0, 30.0, -30.0, 60.0, -60.0, 0.0, -0.0])[:k]
    bound = 10.0 ** rng.uniform(-2, 2, size=n); dy = rng.normal(size=(M, n))
    xt, bt = t64(x, True), t64(bound, True)
    y = torch.sigmoid(xt) * bt
    y.backward(t64(dy))
    dx, db, db_floor = E.softclip_bwd(x, bound, dy)
    close(E.softclip_fwd(x, bound), y.detach().numpy())
    close(dx, xt.grad.numpy())
    assert (np.abs(db - bt.grad.numpy()) <= 1e-12 * db_floor).all() and (db_floor >= np.abs(db) * (1 - 1e-12)).all()
    # the saturated ends: finite, non-zero where fp64 still resolves them, and s(-x) = 1 - s(x)
    s = E.sigmoid(np.asarray([-80.0, 80.0, -745.0, 745.0, -1e4, 1e4]))
    assert np.isfinite(s).all() and abs(s[0] - np.exp(-80.0)) <= 1e-15 * np.exp(-80.0) and s[1] == 1.0 and s[4] == 0.0 and s[5] == 1.0


@pytest.mark.parametrize("slope", [0.0, 0.01, 0.2, 1.0])
def test_leaky_helpers_against_autograd(slope):
    rng = np.random.default_rng(4)
    x = np.concatenate([rng.normal(size=200), [0.0, -0.0, 1e-40, -1e-40, 3e38, -3e38]]).reshape(-1, 2); dy = rng.normal(size=x.shape)
    xt = t64(x, True)
    y = F.leaky_relu(xt, slope)
    y.backward(t64(dy))
    yo = E.leaky_fwd(x, slope)
    assert np.array_equal(yo, y.detach().numpy())
    got = E.leaky_bwd(yo, dy, slope)
    # the gate from the OUTPUT equals the gate from the input for every slope >= 0 (x = 0: both take the slope side)
    assert np.array_equal(got, xt.grad.numpy())


@pytest.mark.parametrize("kind,a", [(0, 0.0), (0, 0.2), (1, 1.0), (1, 0.5), (2, 0.2), (3, 0.5), (3, 1.0), (3, 3.0)])
def test_mixing_activation_against_torch(kind, a):
    v = np.concatenate([np.linspace(-80, 80, 3201), [0.0, -0.0, 1e-30, -1e-30, 1e-8, -1e-8, 20.0 / max(a, 1e-9), np.nextafter(20.0 / max(a, 1e-9), 100.0)]])
    vt = t64(v)
    want = {0: lambda: F.leaky_relu(vt, a), 1: lambda: F.elu(vt, a), 2: lambda: a * vt + (1 - a) * F.softplus(vt, beta=1.0, threshold=1e9),
            3: lambda: F.softplus(vt, beta=a, threshold=20.0)}[kind]().numpy()
    got = E.mix_act(v, kind, a)
    assert np.isfinite(got).all()
    assert float(np.abs(got - want).max()) <= 1e-14 * 80.0
    sel = np.abs(want) > 1e-300
    assert float((np.abs(got - want)[sel] / np.abs(want)[sel]).max()) <= 1e-12      # element-wise too: the tails keep their digits
    big = E.mix_act(np.asarray([-1e4, 1e4]), kind, a)      # far outside the tested range the oracle still does not overflow
    assert np.isfinite(big).all()


@pytest.mark.parametrize("kind,a", [(0, 0.2), (1, 1.0), (2, 0.2), (3, 1.0)])
def test_mixing_forward_against_torch(kind, a):
    rng = np.random.default_rng([5, kind])
    z = rng.normal(size=(37, 6))
    for target in (1.0, 60.0):
        Ws = E.mixing_weights(z, 3, kind, a, target, seed=9)
        pre = []
        x = E.mixing_forward(list(Ws), z, kind, a, pre=pre)
        act = {0: lambda t: F.leaky_relu(t, a), 1: lambda t: F.elu(t, a), 2: lambda t: a * t + (1 - a) * torch.log1p(torch.exp(t)),
               3: lambda t: F.softplus(t, beta=a, threshold=20.0)}[kind]
        cur = t64(z)
        for l in range(3):
            cur = cur @ t64(Ws[l]).T
            if l < 2:
                cur = act(cur)
        close(x, cur.numpy())
        # the gains do what they say (the weights are rounded to fp32 after the gain was chosen) and the weights are gain x orthogonal
        assert len(pre) == 2 and all(abs(float(np.abs(v).max()) - target) <= 1e-6 * target for v in pre)
        for W in Ws:
            G = W.astype(np.float64) @ W.astype(np.float64).T
            assert float(np.abs(G / G[0, 0] - np.eye(6)).max()) < 1e-6


def test_mixing_lds_budget():
    assert E.mixing_lds_bytes(72, 3) == (63936, 3) and E.mixing_lds_bytes(73, 3)[0] > 65536 and E.mixing_lds_bytes(64, 4)[0] > 65536
    assert [E.mixing_lds_bytes(n, 1)[1] for n in (1, 2, 3, 10, 33, 64, 72, 300)] == [64, 64, 64, 25, 7, 4, 3, 1]


def test_padded_buffers():
    a = np.arange(6, dtype=np.float32).reshape(2, 3)
    buf = E.padded(a, 5, extra_rows=1)
    assert buf.shape == (3, 5) and np.array_equal(buf[:2, :3], a)
    bits = E.padding_bits(buf, 2, 3)
    assert bits.size == 15 - 6 and (bits == 0x80000000).all()
    buf[2, 4] = 0.0
    assert not (E.padding_bits(buf, 2, 3) == 0x80000000).all()


def test_adam_oracle_against_torch_float64():
    """Twenty steps of torch.optim.Adam on float64 parameters with betas that are fp32 numbers (both sides see the same values)."""
    rng = np.random.default_rng(6)
    N, lr, b1, b2, eps = 500, 0.0078125, 0.5, 0.875, 2.0 ** -20
    p0 = rng.normal(size=N)
    grads = [rng.normal(size=N) * 10.0 ** rng.uniform(-3, 1, size=N) for _ in range(20)]
    p, m, v = p0.copy(), np.zeros(N), np.zeros(N)
    for t, g in enumerate(grads, 1):
        m, v, p, summ = E.adam_update(p, g, m, v, t, lr, b1, b2, eps, 1.0)
        assert (summ >= np.abs(m) * (1 - 1e-15)).all()
    pt, mt, vt = E.adam_trajectory_torch(p0, grads, torch.float64, lr=lr, betas=(b1, b2), eps=eps)
    close(p, pt); close(m, mt); close(v, vt)
    # grad_scale multiplies g in both moments; the step formed from the new moments is the parameter change
    m2, v2, p2, _ = E.adam_update(p0, grads[0], m, v, 21, lr, b1, b2, eps, 0.25)
    m3, v3, p3, _ = E.adam_update(p0, 0.25 * grads[0], m, v, 21, lr, b1, b2, eps, 1.0)
    close(m2, m3); close(v2, v3); close(p2, p3)
    close(p0 - p2, E.adam_delta(m2, v2, 21, lr, b1, b2, eps), 1e-9)


def test_adam_scalars_are_the_abi_values():
    """The complements come from the fp32 betas: 1 - fl32(0.999) is 1.29e-5 (relative) away from fl32(1 - 0.999), the factor
    torch.optim.Adam applies to a float32 state; exact betas have no such gap."""
    assert E.f32(0.999) == 0.99900001287460327 and abs((1.0 - E.f32(0.999)) - 0.00099998712539672852) < 1e-18
    assert abs(E.f32(1.0 - 0.999) - 0.0010000000474974513) < 1e-18
    assert 1.28e-5 < E.beta2_complement_gap(0.999) < 1.30e-5 and E.beta2_complement_gap(0.875) == 0.0
    one = np.ones(1)
    _, v, _, _ = E.adam_update(one, one, 0 * one, 0 * one, 1, 1e-3, 0.9, 0.999, 1e-8, 1.0)
    assert abs(float(v[0]) - 0.00099998712539672852) < 1e-18
    # every complement the grid uses is exact in fp32, so the kernel's `1.f - b` is the oracle's `1.0 - f32(b)`
    for b1, b2, *_ in E.ADAM_COMBOS:
        for b in (b1, b2):
            assert float(np.float32(1) - np.float32(b)) == 1.0 - E.f32(b)


# ============================================================================================== (b) plain fp32 keeps the GPU test's bounds
@pytest.mark.parametrize("combo", range(len(E.ADAM_COMBOS)))
def test_fp32_emulation_stays_inside_the_asserted_limits(combo):
    worst = dict(m=0.0, v=0.0, v_tiny=0.0, p=0.0)
    for t in E.ADAM_TS:
        p, g, m, v = E.adam_state(combo, t, EMU_COUNT)
        assert int((g == 0).sum()) >= 100 and int((m == 0).sum()) >= 50 and int((v == 0).sum()) >= 50
        b1, b2, eps, gs, lr = E.ADAM_COMBOS[combo]
        got = E.adam_fp32_emulation(p, g, m, v, t, lr, b1, b2, eps, gs)
        e = E.adam_errors(*got, p, g, m, v, t, E.ADAM_COMBOS[combo])
        assert all(np.isfinite(x).all() for x in got)
        assert e["n_zero"] >= 50 and e["moved"] == 0
        for k in worst:
            worst[k] = max(worst[k], e[k])
    print(f"adam fp32 emulation, combo {combo} {E.ADAM_COMBOS[combo]}: worst m {worst['m']:.3f}, v {worst['v']:.3f}, p {worst['p']:.3f} eps32; "
          f"v below {E.ADAM_V_TINY:g}: {worst['v_tiny']:.3e} absolute")
    assert worst["m"] <= E.ADAM_M_LIMIT and worst["v"] <= E.ADAM_V_LIMIT and worst["p"] <= E.ADAM_P_LIMIT and worst["v_tiny"] <= E.ADAM_V_TINY


def test_error_figures_see_a_wrong_update():
    """The figures are not blind: eps inside the root, a float bias correction's 1e-6, and a gradient scale left out of g^2 all leave the limits."""
    combo = 1
    b1, b2, eps, gs, lr = E.ADAM_COMBOS[combo]
    p, g, m, v = E.adam_state(combo, 10, 20_000)
    m1, v1, p1 = E.adam_fp32_emulation(p, g, m, v, 10, lr, b1, b2, eps, gs)
    ok = E.adam_errors(m1, v1, p1, p, g, m, v, 10, E.ADAM_COMBOS[combo])
    assert ok["p"] <= E.ADAM_P_LIMIT and ok["v"] <= E.ADAM_V_LIMIT
    step, inv = E.adam_consts(10, lr, b1, b2)
    with np.errstate(all="ignore"):
        wrong_eps = (p.astype(np.float64) - step * m1 / (np.sqrt(v1.astype(np.float64) + E.f32(eps)) * inv)).astype(np.float32)
        wrong_bc = (p.astype(np.float64) - (1 + 1e-6) * E.adam_delta(m1, v1, 10, lr, b1, b2, eps)).astype(np.float32)
        wrong_v = (E.f32(b2) * v.astype(np.float64) + (1 - E.f32(b2)) * (g.astype(np.float64) * E.f32(gs)) * g).astype(np.float32)
    assert E.adam_errors(m1, v1, wrong_eps, p, g, m, v, 10, E.ADAM_COMBOS[combo])["p"] > E.ADAM_P_LIMIT
    assert E.adam_errors(m1, v1, wrong_bc, p, g, m, v, 10, E.ADAM_COMBOS[combo])["p"] > E.ADAM_P_LIMIT
    assert E.adam_errors(m1, wrong_v, p1, p, g, m, v, 10, E.ADAM_COMBOS[combo])["v"] > E.ADAM_V_LIMIT


@pytest.mark.parametrize("b2", [0.999, 0.875])
def test_fp32_emulation_trajectory_against_torch(b2):
    """The 200-step trajectory of the GPU test through the emulation: parameters and exp_avg no further from torch's float64 run than
    4 x torch's own float32 run (conftest's element-wise rule), exp_avg_sq within 2e-5 of torch's float32 state -- 1.29e-5 of it is the
    fp32 beta2's complement -- and within 4 eps32 where beta2 is an fp32 number."""
    from conftest import ParityLog
    log = ParityLog()      # a private log: nothing of this host test goes into the GPU parity table
    p0, grads = E.adam_trajectory_grads()
    p, m, v = p0, np.zeros_like(p0), np.zeros_like(p0)
    for t, g in enumerate(grads, 1):
        m, v, p = E.adam_fp32_emulation(p, g, m, v, t, 1e-3, 0.9, b2, 1e-8, 1.0)
    p64, m64, v64 = E.adam_trajectory_torch(p0, grads, torch.float64, betas=(0.9, b2))
    p32, m32, v32 = E.adam_trajectory_torch(p0, grads, torch.float32, betas=(0.9, b2))
    assert log.check_elementwise("emu", b2, "p", p, p32, p64) <= 4.0
    assert log.check_elementwise("emu", b2, "exp_avg", m, m32, m64) <= 4.0
    rel = float((np.abs(v.astype(np.float64) - v32) / v32).max())
    print(f"emulated exp_avg_sq against torch float32 after 200 steps, beta2 = {b2}: max relative difference {rel:.3e} "
          f"(complement gap {E.beta2_complement_gap(b2):.3e})")
    assert rel <= (2e-5 if b2 == 0.999 else 4 * E.EPS32)
    if b2 == 0.999:
        assert rel >= 1.0e-5      # the gap is really there: above the 1e-5 contract, below 2e-5
