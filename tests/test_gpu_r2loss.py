"""R2Loss (reference losses.py:480-503) on the HIP kernels clica_r2_loss_fwd / clica_r2_loss_bwd, and the supervised 3DIdent step
(main_3dident.py:569-601) built on it.

Measured on an MI355X (norm-wise relative error against fp64; the bound is 1e-5 everywhere):
see the r2loss_* families of the parity record and DESIGN.md, "R2 objective"."""
import argparse
import ctypes as C

import numpy as np
import pytest
import torch

import r2_oracle
from conftest import PARITY, fill_formula

pytestmark = pytest.mark.gpu

REDUCTIONS = ("none", "mean", "sum")
MODES = ("r2", "negative_r2")
N_PLAIN = 8          # golden cases c000 .. c007 carry gradients (c007: strided); c008 is the degenerate one


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda()


def golden_inputs(c):
    """(y_pred, y) of a golden case on the device; the strided case as [:, :k] views of its 64 x 8 base arrays (no copy)."""
    if str(c["meta"]["kind"]) == "strided":
        k = int(c["meta"]["cols"])
        return dev(c["in"]["y_pred_base"])[:, :k], dev(c["in"]["y_base"])[:, :k]
    return dev(c["in"]["y_pred"]), dev(c["in"]["y"])


def check_pair(fam, case, what, got, ref32, ref64):
    PARITY.check(fam, case, what, got, ref64)
    PARITY.check_elementwise(fam, case, what, got, ref32, ref64)


# ------------------------------------------------------------------------------------------------ 1. golden parity
@pytest.mark.parametrize("idx", range(N_PLAIN))
def test_golden_parity_through_the_abi(idx, golden):
    from cl_ica_amd import ops
    g = golden("g26_r2loss.npz")
    c = g.case(f"c{idx:03d}")
    y_pred, y = golden_inputs(c)
    assert (str(c["meta"]["kind"]) == "strided") == (not y_pred.is_contiguous())
    stride = int(c["meta"]["grad_stride"])
    for red in REDUCTIONS:
        up = dev(c["in"]["g_none"]) if red == "none" else dev([float(g.z["g_scalar"])])
        for mode in MODES:
            o = c["out"]
            out, r2_cols, inv_var = ops.r2_loss_fwd(y_pred, y, red, mode)
            dy = ops.r2_loss_bwd(y_pred, y, inv_var, up, red, mode)
            case = f"c{idx:03d} {red}/{mode}"
            got = out.cpu().numpy().reshape(o[f"{red}/{mode}/out64"].shape)
            check_pair("r2loss_abi", case, "out", got, o[f"{red}/{mode}/out32"], o[f"{red}/{mode}/out64"])
            gd = dy.cpu().numpy().reshape(-1)[::stride].reshape(o[f"{red}/{mode}/grad64"].shape)
            check_pair("r2loss_abi", case, "grad", gd, o[f"{red}/{mode}/grad32"], o[f"{red}/{mode}/grad64"])
            # the per-column by-products: r2 itself (unsigned, unreduced) and 1 / var
            PARITY.check("r2loss_abi", case, "r2_cols", r2_cols.cpu().numpy(), r2_oracle.r2_value(y_pred.cpu().numpy(), y.cpu().numpy(), "none", "r2"))


@pytest.mark.parametrize("idx", range(N_PLAIN))
def test_golden_parity_through_autograd(idx, golden):
    from cl_ica_amd import losses
    g = golden("g26_r2loss.npz")
    c = g.case(f"c{idx:03d}")
    stride = int(c["meta"]["grad_stride"])
    for red in REDUCTIONS:
        up = dev(c["in"]["g_none"]) if red == "none" else torch.tensor(float(g.z["g_scalar"]), device="cuda")
        for mode in MODES:
            o = c["out"]
            y_pred, y = golden_inputs(c)
            leaf = y_pred.detach().clone().requires_grad_(True) if y_pred.is_contiguous() else None
            if leaf is None:           # strided: the gradient flows back into the leading columns of the base array
                base = dev(c["in"]["y_pred_base"]).requires_grad_(True)
                arg = base[:, :y.shape[1]]
            else:
                arg = leaf
            out = losses.R2Loss(reduction=red, mode=mode)(arg, y)
            assert out.shape == torch.Size(o[f"{red}/{mode}/out64"].shape)
            out.backward(up)
            if leaf is None:
                assert float(base.grad[:, y.shape[1]:].abs().max()) == 0.0
                grad = base.grad[:, :y.shape[1]]
            else:
                grad = leaf.grad
            case = f"c{idx:03d} {red}/{mode}"
            check_pair("r2loss_autograd", case, "out", out.detach().cpu().numpy(), o[f"{red}/{mode}/out32"], o[f"{red}/{mode}/out64"])
            gd = grad.cpu().numpy().reshape(-1)[::stride].reshape(o[f"{red}/{mode}/grad64"].shape)
            check_pair("r2loss_autograd", case, "grad", gd, o[f"{red}/{mode}/grad32"], o[f"{red}/{mode}/grad64"])


def test_target_that_requires_grad_is_refused():
    from cl_ica_amd import losses
    y_pred = torch.randn(8, 3, device="cuda", requires_grad=True)
    y = torch.randn(8, 3, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError):
        losses.R2Loss("mean")(y_pred, y)
    with pytest.raises(RuntimeError):
        losses.R2Loss("mean")(y_pred, y.detach().double())          # the module's fp32 check


# ------------------------------------------------------------------------------------------------ 2. shape edges
# M around the 64-row group of a one-column wave and past the forward's grid cap; n at the lane layouts (1: 64 rows per wave pass,
# 3 -> 4 padded columns, 40 -> one row per pass, 65 and 256: more than one 64-column pass)
@pytest.mark.parametrize("M,n", [(63, 1), (64, 3), (65, 40), (257, 65), (4099, 40), (65, 256), (257, 3), (4099, 1), (64, 256)])
def test_shape_edges_against_the_oracle(M, n):
    from cl_ica_amd import losses
    rng = np.random.default_rng(1000 * M + n)
    y = (3.0 + rng.normal(size=(M, n))).astype(np.float32)
    y_pred = (y + 0.5 * rng.normal(size=(M, n))).astype(np.float32)
    g_cols = (0.5 + 0.25 * (np.arange(n) % 7)).astype(np.float32)
    for red in REDUCTIONS:
        for mode in MODES:
            yp = dev(y_pred).requires_grad_(True)
            out = losses.R2Loss(reduction=red, mode=mode)(yp, dev(y))
            up = g_cols if red == "none" else np.float32(0.7)
            out.backward(dev(up) if red == "none" else torch.tensor(0.7, device="cuda"))
            case = f"{M}x{n} {red}/{mode}"
            PARITY.check("r2loss_shapes", case, "out", out.detach().cpu().numpy(), np.asarray(r2_oracle.r2_value(y_pred, y, red, mode)))
            PARITY.check("r2loss_shapes", case, "grad", yp.grad.cpu().numpy(), r2_oracle.r2_grad(y_pred, y, up, red, mode))


# ------------------------------------------------------------------------------------------------ 3. degenerate columns
def test_degenerate_single_row_matches_the_golden_pattern(golden):
    from cl_ica_amd import losses
    c = golden("g26_r2loss.npz").case("c008")
    assert str(c["meta"]["kind"]) == "degenerate"
    for red in REDUCTIONS:
        for mode in MODES:
            want = c["out"][f"{red}/{mode}/out32"]
            assert not np.isfinite(want).any()
            got = losses.R2Loss(reduction=red, mode=mode)(dev(c["in"]["y_pred"]), dev(c["in"]["y"])).cpu().numpy()
            np.testing.assert_array_equal(got.reshape(want.shape), want)           # the same +-inf, element by element


def test_constant_column_disturbs_no_other_column():
    from cl_ica_amd import losses
    rng = np.random.default_rng(7)
    y = rng.normal(size=(64, 4)).astype(np.float32)
    y[:, 2] = 1.25                                   # zero variance
    y_pred = (y + 0.5 * rng.normal(size=(64, 4))).astype(np.float32)
    keep = [0, 1, 3]
    g_cols = np.asarray([0.5, 0.75, 1.0, 1.25], np.float32)
    for mode in MODES:
        yp = dev(y_pred).requires_grad_(True)
        out = losses.R2Loss(reduction="none", mode=mode)(yp, dev(y))
        out.backward(dev(g_cols))
        got, grad = out.detach().cpu().numpy(), yp.grad.cpu().numpy()
        assert not np.isfinite(got[2]) and not np.isfinite(grad[:, 2]).any()
        PARITY.check("r2loss_degenerate", f"const col {mode}", "out", got[keep], r2_oracle.r2_value(y_pred, y, "none", mode)[keep])
        PARITY.check("r2loss_degenerate", f"const col {mode}", "grad", grad[:, keep], r2_oracle.r2_grad(y_pred, y, g_cols, "none", mode)[:, keep])


# ------------------------------------------------------------------------------------------------ 4. determinism and capture
@pytest.mark.parametrize("M,n", [(65, 7), (4099, 40)])
def test_two_eager_calls_are_bitwise_equal(M, n):
    from cl_ica_amd import ops
    gen = torch.Generator().manual_seed(M)
    y = (2.0 + torch.randn(M, n, generator=gen)).cuda()
    y_pred = y + 0.5 * torch.randn(M, n, generator=gen).cuda()
    up = torch.full((1,), 0.7, device="cuda")
    runs = []
    for _ in range(2):
        out, r2_cols, inv_var = ops.r2_loss_fwd(y_pred, y, "mean", "negative_r2")
        dy = ops.r2_loss_bwd(y_pred, y, inv_var, up, "mean", "negative_r2")
        runs.append([t.cpu().numpy().copy() for t in (out, r2_cols, inv_var, dy)])
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    ws = ops.r2_loss_workspace(M, n, y.device)
    assert ws is ops.r2_loss_workspace(M, n, y.device)               # the cache hands the same buffer out, never a new one
    assert int(ws[:4].view(torch.int32).item()) == 0                 # the launch left its arrival counter at zero


def test_captured_forward_and_backward_replay_bit_for_bit():
    from cl_ica_amd import losses
    M, n = 65, 7
    loss = losses.R2Loss(reduction="mean", mode="negative_r2")
    gen = torch.Generator().manual_seed(3)
    batches = []
    for _ in range(4):
        y = (1.0 + torch.randn(M, n, generator=gen)).cuda()
        batches.append((y, y + 0.5 * torch.randn(M, n, generator=gen).cuda()))

    def eager(y, y_pred):
        yp = y_pred.clone().requires_grad_(True)
        out = loss(yp, y)
        out.backward()
        return out.detach().clone(), yp.grad.clone()

    static_y, static_yp = batches[0][0].clone(), batches[0][1].clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                    # warm-up off the default stream, as torch.cuda.graph asks
        loss(static_yp, static_y).backward()
    torch.cuda.current_stream().wait_stream(side)
    static_yp.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = loss(static_yp, static_y)
        static_out.backward()
    static_grad = static_yp.grad
    for y, y_pred in batches[1:]:
        want_out, want_grad = eager(y, y_pred)
        with torch.no_grad():
            static_y.copy_(y); static_yp.copy_(y_pred)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(static_out.detach().cpu().numpy().view(np.uint32), want_out.cpu().numpy().view(np.uint32))
        assert np.array_equal(static_grad.cpu().numpy().view(np.uint32), want_grad.cpu().numpy().view(np.uint32))


# ------------------------------------------------------------------------------------------------ 5. argument errors
def test_bad_arguments_fail_by_return_code_before_any_launch():
    from cl_ica_amd import _lib, ops
    L = _lib.load()
    M, n = 16, 4
    y = torch.randn(M, n, device="cuda"); y_pred = torch.randn(M, n, device="cuda")
    out = torch.full((n,), 123.0, device="cuda"); r2c = torch.full((n,), 123.0, device="cuda"); iv = torch.full((n,), 123.0, device="cuda")
    dy = torch.full((M, n), 123.0, device="cuda")
    ws = ops.r2_loss_workspace(M, n, y.device)
    nb = C.c_size_t()
    _lib.check(L.clica_r2_loss_workspace_bytes(M, n, C.byref(nb)), "clica_r2_loss_workspace_bytes")
    s = _lib.stream_ptr()

    def fwd(M=M, n=n, ldp=n, ldy=n, red=1, mode=1, wsp=ws.data_ptr(), wsb=ws.numel()):
        _lib.check(L.clica_r2_loss_fwd(y_pred.data_ptr(), ldp, y.data_ptr(), ldy, M, n, red, mode, out.data_ptr(), r2c.data_ptr(),
                                       iv.data_ptr(), wsp, wsb, s), "clica_r2_loss_fwd")

    def bwd(M=M, n=n, ldp=n, ldy=n, lddy=n, red=1, mode=1):
        _lib.check(L.clica_r2_loss_bwd(y_pred.data_ptr(), ldp, y.data_ptr(), ldy, M, n, red, mode, iv.data_ptr(), out.data_ptr(),
                                       dy.data_ptr(), lddy, s), "clica_r2_loss_bwd")

    bad_fwd = [dict(n=0), dict(n=257), dict(M=0), dict(ldp=n - 1), dict(ldy=n - 1), dict(wsb=nb.value - 1), dict(wsp=ws.data_ptr() + 4),
               dict(red=3), dict(mode=2)]
    for kw in bad_fwd:
        with pytest.raises(RuntimeError):
            fwd(**kw)
    for kw in [dict(n=0), dict(n=257), dict(M=0), dict(ldp=n - 1), dict(lddy=n - 1), dict(red=-1), dict(mode=7)]:
        with pytest.raises(RuntimeError):
            bwd(**kw)
    with pytest.raises(RuntimeError):
        ops.r2_loss_workspace(M, 257, y.device)
    torch.cuda.synchronize()
    for t in (out, r2c, iv, dy):
        assert bool((t == 123.0).all())            # nothing was launched
    assert int(ws[:4].view(torch.int32).item()) == 0
    fwd()                                           # the same buffers with good arguments do run
    bwd()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dy).all()) and not bool((out[:1] == 123.0).any())


# ------------------------------------------------------------------------------------------------ 6. supervised step
LR, STEPS = 1e-3, 5


def reference_trajectory(kind, x1, z1, params, dtype):
    """The arithmetic of the step written out in torch on the CPU: Linear / LeakyReLU / Linear, the objective, torch.optim.Adam."""
    W0, b0, W1, b1 = [torch.tensor(p, dtype=dtype, requires_grad=True) for p in params]
    x, z = torch.tensor(x1, dtype=dtype), torch.tensor(z1, dtype=dtype)
    opt = torch.optim.Adam([W0, b0, W1, b1], lr=LR)
    losses_, first_grads = [], None
    for s in range(STEPS):
        opt.zero_grad()
        h = torch.nn.functional.leaky_relu(x @ W0.T + b0, 0.01) @ W1.T + b1
        if kind == "r2":
            var = ((z - z.mean(0)) ** 2).mean(0)
            loss = -(1.0 - ((h - z) ** 2).mean(0) / var).mean()
        else:
            loss = ((h - z) ** 2).mean()
        loss.backward()
        if s == 0:
            first_grads = [p.grad.detach().numpy().astype(np.float64).copy() for p in (W0, b0, W1, b1)]
        opt.step()
        losses_.append(float(loss))
    return np.asarray(losses_, np.float64), first_grads, [p.detach().numpy().astype(np.float64) for p in (W0, b0, W1, b1)]


@pytest.mark.parametrize("kind", ["r2", "mse"])
def test_supervised_step_follows_the_fp64_trajectory(kind):
    from cl_ica_amd import encoders, optim, threedident
    f = encoders.get_mlp(n_in=8, n_out=3, layers=[16])
    fill_formula(f)
    params0 = [p.detach().numpy().copy() for p in f.parameters()]
    f = f.cuda()
    rng = np.random.default_rng(11)
    x1 = rng.uniform(-1.0, 1.0, size=(64, 8)).astype(np.float32)
    z1 = rng.uniform(-1.0, 1.0, size=(64, 3)).astype(np.float32)
    opt = optim.Adam(f.parameters(), lr=LR)
    loss = threedident.make_supervised_loss(argparse.Namespace(supervised_loss=kind))
    data = ((torch.tensor(z1), None), (dev(x1), None))          # latents arrive on the host, as from the reference's loader
    got_losses, got_first = [], None
    for s in range(STEPS):
        v = threedident.train_step_supervised(data, loss, opt, f)
        assert isinstance(v, float)
        got_losses.append(v)
        if s == 0:
            got_first = [p.grad.detach().cpu().numpy().copy() for p in f.parameters()]
    got_params = [p.detach().cpu().numpy().astype(np.float64) for p in f.parameters()]

    l64, g64, p64 = reference_trajectory(kind, x1, z1, params0, torch.float64)
    l32, _, p32 = reference_trajectory(kind, x1, z1, params0, torch.float32)
    fam = f"r2loss_supervised_{kind}"
    PARITY.check(fam, kind, "losses", np.asarray(got_losses), l64)
    for k, (a, b) in enumerate(zip(got_first, g64)):
        PARITY.check(fam, kind, f"step0 grad{k}", a, b)
    # final parameters: at most 4 x the torch-CPU fp32 run's own distance from fp64 (floor 1e-5), every element within 2 lr steps
    flat = lambda ps: np.concatenate([np.asarray(p, np.float64).reshape(-1) for p in ps])
    got, r64, r32 = flat(got_params), flat(p64), flat(p32)
    ref_dev = float(np.max(np.abs(r32 - r64)) / np.max(np.abs(r64)))
    bound = max(4.0 * ref_dev, 1e-5)
    hip_dev = PARITY.check(fam, kind, "final params", got, r64, tol=bound, note=f"4 x the fp32 reference's own deviation ({ref_dev:.2e}), floor 1e-5")
    PARITY.check(fam, kind, "final params (torch fp32 vs fp64)", r32, r64, tol=bound, note="the reference's own deviation")
    print(f"supervised {kind}: final parameters HIP vs fp64 {hip_dev:.3e}, torch fp32 vs fp64 {ref_dev:.3e}, bound {bound:.3e}")
    assert float(np.max(np.abs(got - r64))) <= 2.0 * LR * STEPS
    assert got_losses[-1] < got_losses[0]


@pytest.mark.parametrize("kind", ["r2", "mse"])
def test_supervised_step_without_sync_returns_the_device_scalar(kind):
    from cl_ica_amd import encoders, optim, threedident
    f = encoders.get_mlp(n_in=8, n_out=3, layers=[16])
    fill_formula(f)
    f = f.cuda()
    gen = torch.Generator().manual_seed(5)
    data = ((torch.rand(64, 3, generator=gen), None), (torch.rand(64, 8, generator=gen).cuda(), None))
    loss = threedident.make_supervised_loss(argparse.Namespace(supervised_loss=kind))
    v = threedident.train_step_supervised(data, loss, optim.Adam(f.parameters(), lr=LR), f, sync=False)
    assert isinstance(v, torch.Tensor) and v.is_cuda and v.dim() == 0 and bool(torch.isfinite(v))
