"""BatchNorm1d / GroupNorm(1, C) fused with LeakyReLU on the HIP kernels of csrc/norm.hip: the C ABI against the fp64 oracle
(tests/norm_oracle.py), get_mlp(layer_normalization=...) against the goldens G27 and G20, the proof that the HIP path is taken, the
configurations that keep torch's modules, bit reproducibility eager / graph replay, and the trainers' guard.

Measured on an MI355X: see the norm_* families of the parity record and DESIGN.md 4.8."""
import copy

import numpy as np
import pytest
import torch

import norm_oracle as O
from bn_family_util import bits, dev, host, raw
from conftest import PARITY, fill_formula

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 1. ABI sweep against the oracle
def check_backward(fam, kind, case, M, C, got, fw, bw, slope):
    """dx, dgamma, dbeta with the near-kink columns / rows left out (at most 5 % of them)."""
    cols, rows = O.left_out(kind, fw["z"], slope)
    assert O.left_out_fraction(kind, fw["z"], slope) <= O.MAX_LEFT_OUT
    dx, dgamma, dbeta = (host(t) for t in got)
    if not (kind == "bn" and M == 2):          # dx at M = 2 is ill-conditioned
        keep = np.ix_(~rows, ~cols) if kind == "bn" else np.ix_(~rows, np.ones(C, bool))
        PARITY.check(fam, case, "dx", dx[keep], bw["dx"][keep])
    PARITY.check(fam, case, "dgamma", dgamma[~cols], bw["dgamma"][~cols])
    PARITY.check(fam, case, "dbeta", dbeta[~cols], bw["dbeta"][~cols])


@pytest.mark.parametrize("cls", range(len(O.CLASSES)))
@pytest.mark.parametrize("M,C", O.BN_SHAPES)
def test_batchnorm_abi_against_the_oracle(M, C, cls):
    from cl_ica_amd import ops
    c = O.make_case("bn", M, C, cls)
    x, gamma, beta, dy = dev(c["x"]), dev(c["gamma"]), dev(c["beta"]), dev(c["dy"])
    for slope in O.SLOPES:
        fw = O.bn_forward(c["x"], c["gamma"], c["beta"], slope, running_mean=c["running_mean"], running_var=c["running_var"])
        bw = O.bn_backward(fw, c["gamma"], c["dy"], slope)
        rm, rv = dev(c["running_mean"]), dev(c["running_var"])
        y, save_mean, save_invstd = ops.batchnorm_lrelu_fwd(x, gamma, beta, rm, rv, O.EPS, O.MOMENTUM, slope)
        got = ops.batchnorm_lrelu_bwd(x, y, dy, gamma, save_mean, save_invstd, slope)
        case = f"{M}x{C} cls{cls} slope{slope}"
        PARITY.check("norm_abi_bn", case, "y", host(y), fw["y"])
        PARITY.check("norm_abi_bn", case, "save_mean", host(save_mean), fw["mean"])
        PARITY.check("norm_abi_bn", case, "save_invstd", host(save_invstd), fw["invstd"])
        PARITY.check("norm_abi_bn", case, "running_mean", host(rm), fw["running_mean"])
        PARITY.check("norm_abi_bn", case, "running_var", host(rv), fw["running_var"])
        check_backward("norm_abi_bn", "bn", case, M, C, got, fw, bw, slope)
    # without running statistics the forward is the same and nothing else is written
    y2, m2, i2 = ops.batchnorm_lrelu_fwd(x, gamma, beta, None, None, O.EPS, O.MOMENTUM, O.SLOPES[-1])
    assert np.array_equal(bits(y2), bits(y)) and np.array_equal(bits(m2), bits(save_mean)) and np.array_equal(bits(i2), bits(save_invstd))


@pytest.mark.parametrize("cls", range(len(O.CLASSES)))
@pytest.mark.parametrize("M,C", O.GN_SHAPES)
def test_groupnorm_abi_against_the_oracle(M, C, cls):
    from cl_ica_amd import ops
    c = O.make_case("gn", M, C, cls)
    x, gamma, beta, dy = dev(c["x"]), dev(c["gamma"]), dev(c["beta"]), dev(c["dy"])
    for slope in O.SLOPES:
        fw = O.gn_forward(c["x"], c["gamma"], c["beta"], slope)
        bw = O.gn_backward(fw, c["gamma"], c["dy"], slope)
        y, mean, rstd = ops.groupnorm_lrelu_fwd(x, gamma, beta, O.EPS, slope)
        got = ops.groupnorm_lrelu_bwd(x, y, dy, gamma, mean, rstd, slope)
        case = f"{M}x{C} cls{cls} slope{slope}"
        PARITY.check("norm_abi_gn", case, "y", host(y), fw["y"])
        PARITY.check("norm_abi_gn", case, "mean", host(mean), fw["mean"])
        PARITY.check("norm_abi_gn", case, "rstd", host(rstd), fw["rstd"])
        check_backward("norm_abi_gn", "gn", case, M, C, got, fw, bw, slope)


@pytest.mark.parametrize("M,C", O.BN_EVAL_SHAPES)
def test_batchnorm_eval_abi_against_the_oracle(M, C):
    from cl_ica_amd import ops
    for cls in range(len(O.CLASSES)):
        c = O.make_case("bn", M, C, cls)
        rm = (c["x"].mean(0) + c["running_mean"]).astype(np.float32)          # statistics of the size of the data's own
        rv = (c["x"].var(0) * c["running_var"]).astype(np.float32)
        for slope in O.SLOPES:
            y = ops.batchnorm_lrelu_eval(dev(c["x"]), dev(c["gamma"]), dev(c["beta"]), dev(rm), dev(rv), O.EPS, slope)
            PARITY.check("norm_abi_bn", f"eval {M}x{C} cls{cls} slope{slope}", "y", host(y),
                         O.bn_eval(c["x"], c["gamma"], c["beta"], rm, rv, slope)["y"])


@pytest.mark.parametrize("cls", range(len(O.CLASSES)))
def test_batchnorm_two_rows_on_the_unselected_draw_against_torch_fp32(cls):
    """The sweep draws its 2 x 65 case with max|x| / std <= 80 per column (tests/norm_oracle.py), so rows that nearly coincide are not in
    it.  Here is the FIRST draw of the same case, unselected (kappa in the hundreds to thousands): no fp32 evaluation is a yardstick at
    1e-5 there, so the HIP result is held to the fp32 reference's own error against fp64 -- torch's batch_norm + leaky_relu on the CPU --
    times the project's allowance factor 4, with the sweep's bound 1e-5 as a floor (the form of the supervised-step checks of
    tests/test_gpu_r2loss.py).  dx is left out as in the sweep (ill-conditioned at M = 2)."""
    from cl_ica_amd import ops
    M, C = 2, 65
    c = O.make_case("bn", M, C, cls, attempt=0)
    F = torch.nn.functional
    for slope in O.SLOPES:
        fw = O.bn_forward(c["x"], c["gamma"], c["beta"], slope, running_mean=c["running_mean"], running_var=c["running_var"])
        bw = O.bn_backward(fw, c["gamma"], c["dy"], slope)
        t = {k: torch.tensor(v) for k, v in c.items()}
        w, b = t["gamma"].requires_grad_(True), t["beta"].requires_grad_(True)
        y32 = F.leaky_relu(F.batch_norm(t["x"], t["running_mean"], t["running_var"], w, b, True, O.MOMENTUM, O.EPS), slope)
        y32.backward(t["dy"])
        ref32 = dict(y=y32.detach().numpy(), dgamma=w.grad.numpy(), dbeta=b.grad.numpy(), running_mean=t["running_mean"].numpy(),
                     running_var=t["running_var"].numpy())
        rm, rv = dev(c["running_mean"]), dev(c["running_var"])
        x, gamma = dev(c["x"]), dev(c["gamma"])
        y, save_mean, save_invstd = ops.batchnorm_lrelu_fwd(x, gamma, dev(c["beta"]), rm, rv, O.EPS, O.MOMENTUM, slope)
        _, dgamma, dbeta = ops.batchnorm_lrelu_bwd(x, y, dev(c["dy"]), gamma, save_mean, save_invstd, slope)
        got = dict(y=host(y), dgamma=host(dgamma), dbeta=host(dbeta), running_mean=host(rm), running_var=host(rv))
        cols, _ = O.left_out("bn", fw["z"], slope)
        for k, v in got.items():
            truth = fw[k] if k in fw else bw[k]
            keep = ~cols if k in ("dgamma", "dbeta") else slice(None)
            own = O.norm_err(ref32[k][..., keep] if k != "y" else ref32[k], truth[..., keep] if k != "y" else truth)
            bound = max(4.0 * own, 1e-5)
            err = PARITY.check("norm_abi_bn_unselected", f"2x65 cls{cls} slope{slope} kappa {O.kappa('bn', c['x']):.0f}", k,
                               v[..., keep] if k != "y" else v, truth[..., keep] if k != "y" else truth, tol=bound,
                               note="4 x torch fp32's own error against fp64, floor 1e-5")
            print(f"unselected 2x65 cls{cls} slope{slope} {k}: HIP {err:.3e}, torch fp32 {own:.3e}, bound {bound:.3e}")


def test_bad_arguments_are_refused():
    from cl_ica_amd import ops
    x = torch.randn(8, 4, device="cuda"); w = torch.ones(4, device="cuda"); b = torch.zeros(4, device="cuda")
    with pytest.raises(RuntimeError):
        ops.batchnorm_lrelu_fwd(x[:1], w, b)                    # one row
    with pytest.raises(RuntimeError):
        ops.batchnorm_lrelu_fwd(x, w, b, slope=-0.1)
    with pytest.raises(RuntimeError):
        ops.groupnorm_lrelu_fwd(x, w, b, slope=-0.1)
    with pytest.raises(ValueError):
        ops.groupnorm_lrelu_fwd(x[:, :3], w[:3], b[:3])         # not contiguous
    with pytest.raises(ValueError):
        ops.batchnorm_lrelu_fwd(x, w[:3], b)
    assert ops.norm_workspace("bn", 8, 4, x.device) is ops.norm_workspace("bn", 8, 4, x.device)      # never a new buffer


# ------------------------------------------------------------------------------------------------ 2. G27 and G20 through the module
def g27_module(mode):
    from cl_ica_amd import encoders
    f = encoders.get_mlp(5, 3, [7, 65, 24], layer_normalization=mode)
    fill_formula(f)
    for m in f:
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.GroupNorm)):
            m.weight.data += 1.0
    return f.to("cuda").train()


def check_pair(fam, case, what, got, z, key, floor=0.0):
    PARITY.check(fam, case, what, got, z[key + "64"], floor=floor)
    PARITY.check_elementwise(fam, case, what, got, z[key + "32"], z[key + "64"], factor=4.0, scale_floor=floor)


@pytest.mark.parametrize("mode", ["bn", "gn"])
def test_module_against_g27(golden, mode):
    from cl_ica_amd import encoders
    assert encoders.NORM_MODE == "hip"
    z = golden("g27_mlp_norm.npz").z
    f = g27_module(mode)
    mods = dict(f.named_children())
    for k in range(2):
        f.zero_grad(set_to_none=True)
        x = dev(z[f"x{k}"]).requires_grad_(True)
        y = f(x)
        (y * dev(z[f"c{k}"])).sum().backward()
        case = f"{mode} pass{k}"
        check_pair("norm_g27", case, "y", host(y), z, f"{mode}/p{k}/y")
        check_pair("norm_g27", case, "dx", host(x.grad), z, f"{mode}/p{k}/dx")
        for name, prm in f.named_parameters():
            # a Linear bias in front of a normalisation that removes the mean has an exactly-zero gradient (both sides hold rounding
            # noise there): relative to the gradient scale of the same layer's weight, as the G20 test does
            idx, leaf = name.split(".")
            floor = float(np.abs(z[f"{mode}/p{k}/grad/{idx}.weight64"]).max()) if leaf == "bias" and isinstance(mods[idx], torch.nn.Linear) else 0.0
            check_pair("norm_g27/grad", case, name, host(prm.grad), z, f"{mode}/p{k}/grad/{name}", floor=floor)
        for name, buf in f.named_buffers():
            if name.endswith("num_batches_tracked"):
                assert int(buf) == k + 1 == int(z[f"{mode}/p{k}/buf/{name}64"])
            else:
                check_pair("norm_g27/buf", case, name, host(buf), z, f"{mode}/p{k}/buf/{name}")
    if mode == "bn":
        assert [int(b) for n, b in f.named_buffers() if n.endswith("num_batches_tracked")] == [2, 2, 2]
    f.eval()
    with torch.no_grad():
        check_pair("norm_g27", mode, "y_eval", host(f(dev(z["x0"]))), z, f"{mode}/y_eval")


# ------------------------------------------------------------------------------------------------ 3. the HIP path is really taken
def refuse(*a, **k):
    raise AssertionError("torch's own normalisation kernel was called")


@pytest.mark.parametrize("mode", ["bn", "gn"])
def test_the_hip_path_is_taken(monkeypatch, mode):
    from cl_ica_amd import encoders
    monkeypatch.setattr(torch.nn.functional, "batch_norm", refuse)
    monkeypatch.setattr(torch.nn.functional, "group_norm", refuse)
    f = g27_module(mode)
    x = torch.randn(65, 5, device="cuda", requires_grad=True)
    f(x).sum().backward()
    assert x.grad is not None and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in f.parameters())
    f.eval()
    with torch.no_grad():
        assert bool(torch.isfinite(f(x)).all())
    monkeypatch.setattr(encoders, "NORM_MODE", "torch")           # today's path does call them
    with pytest.raises(AssertionError, match="torch's own normalisation"):
        with torch.no_grad():
            f(x)
    f.train()
    with pytest.raises(AssertionError, match="torch's own normalisation"):
        f(x)


# ------------------------------------------------------------------------------------------------ 4. what keeps torch's modules
def run_both_modes(monkeypatch, build, x, train=True, grad=True):
    """The same module (deep copies) under NORM_MODE "hip" and "torch": outputs, input gradient, parameter gradients, buffers."""
    from cl_ica_amd import encoders
    base = build()
    out = {}
    for nm in ("hip", "torch"):
        monkeypatch.setattr(encoders, "NORM_MODE", nm)
        f = copy.deepcopy(base).train(train)
        xin = x.clone().requires_grad_(grad)
        with torch.set_grad_enabled(grad):
            y = f(xin)
        res = [y.detach()]
        if grad:
            y.square().sum().backward()
            res += [xin.grad] + [p.grad for p in f.parameters()]
        out[nm] = res + [b.float() for b in f.buffers()]
    assert len(out["hip"]) == len(out["torch"])
    for a, b in zip(out["hip"], out["torch"]):
        assert a.dtype == b.dtype and np.array_equal(raw(a), raw(b))


def stack(norm, width=8):
    from cl_ica_amd import encoders
    torch.manual_seed(3)
    return lambda: encoders.NormedMLP(torch.nn.Linear(6, width), norm(), torch.nn.LeakyReLU(), torch.nn.Linear(width, 3)).cuda()


@pytest.mark.parametrize("name,norm,width,train", [
    ("bn without affine", lambda: torch.nn.BatchNorm1d(8, affine=False), 8, True),
    ("bn without running statistics", lambda: torch.nn.BatchNorm1d(8, track_running_stats=False), 8, True),
    ("bn with a cumulative average", lambda: torch.nn.BatchNorm1d(8, momentum=None), 8, True),
    ("bn in eval mode inside autograd", lambda: torch.nn.BatchNorm1d(8), 8, False),
    ("gn with two groups", lambda: torch.nn.GroupNorm(2, 8), 8, True),
    ("gn of one channel", lambda: torch.nn.GroupNorm(1, 1), 1, True),
])
def test_configurations_outside_the_kernels_run_as_before(monkeypatch, name, norm, width, train):
    x = torch.randn(33, 6, generator=torch.Generator().manual_seed(1)).cuda()
    run_both_modes(monkeypatch, stack(norm, width), x, train=train)


def test_inputs_outside_the_kernels_run_as_before(monkeypatch):
    from cl_ica_amd import encoders
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(33, 8, generator=gen)
    run_both_modes(monkeypatch, lambda: encoders.NormedMLP(torch.nn.BatchNorm1d(8)).cuda().double(), x.cuda().double())     # not fp32
    run_both_modes(monkeypatch, lambda: encoders.NormedMLP(torch.nn.GroupNorm(1, 8)).cuda().double(), x.cuda().double())
    run_both_modes(monkeypatch, lambda: encoders.NormedMLP(torch.nn.BatchNorm1d(8)), x)                                      # not on the GPU
    run_both_modes(monkeypatch, lambda: encoders.NormedMLP(torch.nn.GroupNorm(1, 8)), x)


def test_batchnorm_training_on_one_row_raises():
    from cl_ica_amd import encoders
    f = encoders.get_mlp(5, 3, [7], layer_normalization="bn").cuda().train()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        f(torch.randn(1, 5, device="cuda"))
    assert int(f[1].num_batches_tracked) == 0
    f.eval()
    with torch.no_grad():
        assert f(torch.randn(1, 5, device="cuda")).shape == (1, 3)


# ------------------------------------------------------------------------------------------------ 5. reproducibility
def norm_step(kind, x, gamma, beta, dy, rm, rv, slope=0.01):
    from cl_ica_amd import ops
    if kind == "bn":
        y, a, b = ops.batchnorm_lrelu_fwd(x, gamma, beta, rm, rv, O.EPS, O.MOMENTUM, slope)
        return (y, a, b) + tuple(ops.batchnorm_lrelu_bwd(x, y, dy, gamma, a, b, slope))
    y, a, b = ops.groupnorm_lrelu_fwd(x, gamma, beta, O.EPS, slope)
    return (y, a, b) + tuple(ops.groupnorm_lrelu_bwd(x, y, dy, gamma, a, b, slope))


@pytest.mark.parametrize("kind", ["bn", "gn"])
@pytest.mark.parametrize("M,C", [(257, 500), (4099, 40)])
def test_eager_calls_and_graph_replays_give_the_same_bits(M, C, kind):
    c = O.make_case(kind, M, C, 1)
    x, gamma, beta, dy = dev(c["x"]), dev(c["gamma"]), dev(c["beta"]), dev(c["dy"])
    rm, rv = dev(c["running_mean"]), dev(c["running_var"])
    first = [bits(t).copy() for t in norm_step(kind, x, gamma, beta, dy, rm, rv)]
    second = [bits(t).copy() for t in norm_step(kind, x, gamma, beta, dy, rm, rv)]           # (also the warm-up of the capture)
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    want_rm, want_rv = bits(rm).copy(), bits(rv).copy()                                      # after two calls
    srm, srv = dev(c["running_mean"]), dev(c["running_var"])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = norm_step(kind, x, gamma, beta, dy, srm, srv)
    with torch.no_grad():
        srm.copy_(dev(c["running_mean"])); srv.copy_(dev(c["running_var"]))                # capturing launches nothing
    for _ in range(2):
        for t in outs:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, t in zip(first, outs):
            assert np.array_equal(a, bits(t))
    if kind == "bn":
        assert np.array_equal(bits(srm), want_rm) and np.array_equal(bits(srv), want_rv)


# ------------------------------------------------------------------------------------------------ 6. the trainers' guard
def test_trainers_refuse_an_encoder_with_normalisation():
    from cl_ica_amd import encoders
    from cl_ica_amd.engine import ContrastiveTrainer, SamplerSpec, SupervisedTrainer
    n, B = 4, 64
    gW = torch.eye(n, device="cuda").repeat(3, 1, 1)
    for mode in ("bn", "gn"):
        f = encoders.get_mlp(n, n, [16, 16], layer_normalization=mode)
        with pytest.raises(ValueError, match="normalisation module"):
            ContrastiveTrainer(f, gW, SamplerSpec(n=n), batch_size=B, device="cuda")
        with pytest.raises(ValueError, match="normalisation module"):
            SupervisedTrainer(f, gW, SamplerSpec(n=n), batch_size=B, device="cuda")
    f = torch.nn.Sequential(torch.nn.Linear(n, 8), torch.nn.LayerNorm(8), torch.nn.LeakyReLU(), torch.nn.Linear(8, n))
    with pytest.raises(ValueError, match="normalisation module"):
        ContrastiveTrainer(f, gW, SamplerSpec(n=n), batch_size=B, device="cuda")
    ContrastiveTrainer(encoders.get_mlp(n, n, [16, 16]), gW, SamplerSpec(n=n), batch_size=B, device="cuda")
    SupervisedTrainer(encoders.get_mlp(n, n, [16, 16]), gW, SamplerSpec(n=n), batch_size=B, device="cuda")
