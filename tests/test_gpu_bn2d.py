"""BatchNorm2d fused with the shortcut add and the ReLU on the HIP kernels of csrc/bn2d.hip: the C ABI against the fp64 oracle
(tests/bn2d_oracle.py), a BasicBlock and the whole ResNet-18 stand-in against fp64 CPU copies, the proof that the HIP path is taken,
the configurations that keep torch's modules, and bit reproducibility eager / graph replay."""
import copy
import types

import numpy as np
import pytest
import torch

import bn2d_oracle as B
from bn_family_util import bits, deterministic_convolutions, dev, host, off_by_4_bytes, raw, refuse  # noqa: F401 (the autouse fixture)
from conftest import PARITY

pytestmark = pytest.mark.gpu


def maps(c, shape):
    """The case's rows as NCHW device tensors (r: None without a residual)."""
    f = lambda a: None if a is None else dev(B.to_nchw(a, *shape))
    return f(c["x"]), f(c["r"]), f(c["dy"])


# ------------------------------------------------------------------------------------------------ 1. ABI sweep against the oracle
@pytest.mark.parametrize("cls", range(len(B.CLASSES)))
@pytest.mark.parametrize("shape", B.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_abi_against_the_oracle(shape, cls):
    from cl_ica_amd import ops
    N, C, H, W = shape
    for residual in (False, True):
        for slope in B.SLOPES:
            c, fw, bw = B.reference(N, C, H, W, cls, residual, slope)
            x, r, dy = maps(c, shape)
            gamma, beta = dev(c["gamma"]), dev(c["beta"])
            rm, rv = dev(c["running_mean"]), dev(c["running_var"])
            y, save_mean, save_invstd = ops.batchnorm2d_act_fwd(x, gamma, beta, rm, rv, B.EPS, B.MOMENTUM, slope, residual=r)
            dx, dr, dgamma, dbeta = ops.batchnorm2d_act_bwd(x, y, dy, gamma, save_mean, save_invstd, slope, need_dr=residual)
            assert (dr is not None) == residual
            case = f"{N}x{C}x{H}x{W} cls{cls} slope{slope} res{int(residual)}"
            fam = "bn2d_abi"
            PARITY.check(fam, case, "y", B.to_rows(host(y)), fw["y"])
            PARITY.check(fam, case, "save_mean", host(save_mean), fw["mean"])
            PARITY.check(fam, case, "save_invstd", host(save_invstd), fw["invstd"])
            PARITY.check(fam, case, "running_mean", host(rm), fw["running_mean"])
            PARITY.check(fam, case, "running_var", host(rv), fw["running_var"])
            cols = B.left_out(fw["z"], slope)
            assert cols.mean() <= B.MAX_LEFT_OUT
            if N * H * W > 2:                      # dx at M = 2 is ill-conditioned
                PARITY.check(fam, case, "dx", B.to_rows(host(dx))[:, ~cols], bw["dx"][:, ~cols])
            if residual:
                PARITY.check(fam, case, "dr", B.to_rows(host(dr))[:, ~cols], bw["dr"][:, ~cols])
            PARITY.check(fam, case, "dgamma", host(dgamma)[~cols], bw["dgamma"][~cols])
            PARITY.check(fam, case, "dbeta", host(dbeta)[~cols], bw["dbeta"][~cols])
            # without running statistics the forward is the same and nothing else is written
            rm_bits, rv_bits = bits(rm).copy(), bits(rv).copy()
            y2, m2, i2 = ops.batchnorm2d_act_fwd(x, gamma, beta, None, None, B.EPS, B.MOMENTUM, slope, residual=r)
            assert np.array_equal(bits(y2), bits(y)) and np.array_equal(bits(m2), bits(save_mean)) and np.array_equal(bits(i2), bits(save_invstd))
            assert np.array_equal(bits(rm), rm_bits) and np.array_equal(bits(rv), rv_bits)


@pytest.mark.parametrize("shape", B.EVAL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_eval_abi_against_the_oracle(shape):
    from cl_ica_amd import ops
    N, C, H, W = shape
    for cls in range(len(B.CLASSES)):
        for residual in (False, True):
            c = B.make_case(N, C, H, W, cls, residual)
            rm = (c["x"].mean(0) + c["running_mean"]).astype(np.float32)          # statistics of the size of the data's own
            rv = (c["x"].var(0) * c["running_var"]).astype(np.float32)
            x, r, _ = maps(c, shape)
            for slope in B.SLOPES:
                y = ops.batchnorm2d_act_eval(x, dev(c["gamma"]), dev(c["beta"]), dev(rm), dev(rv), B.EPS, slope, residual=r)
                PARITY.check("bn2d_abi", f"eval {N}x{C}x{H}x{W} cls{cls} slope{slope} res{int(residual)}", "y", B.to_rows(host(y)),
                             B.evaluate(c, rm, rv, slope))


@pytest.mark.parametrize("shape", B.UNALIGNED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_unaligned_input_gives_the_same_bits(shape):
    """HW % 4 == 0 on both shapes: an unaligned tensor makes the kernels read and write the same quads of values with scalar accesses,
    in the same reduction order, so every result has the aligned call's bits."""
    from cl_ica_amd import ops
    N, C, H, W = shape
    slope = 0.0
    c, fw, bw = B.reference(N, C, H, W, 1, True, slope)
    x, r, dy = maps(c, shape)
    gamma, beta = dev(c["gamma"]), dev(c["beta"])

    def run(x, r, dy):
        y, a, b = ops.batchnorm2d_act_fwd(x, gamma, beta, None, None, B.EPS, B.MOMENTUM, slope, residual=r)
        return (y, a, b) + tuple(ops.batchnorm2d_act_bwd(x, y, dy, gamma, a, b, slope, need_dr=True))
    want = run(x, r, dy)
    PARITY.check("bn2d_abi", f"unaligned {shape}", "y", B.to_rows(host(want[0])), fw["y"])
    for variant in ((off_by_4_bytes(x), r, dy), (off_by_4_bytes(x), off_by_4_bytes(r), off_by_4_bytes(dy))):
        for a, b in zip(want, run(*variant)):
            assert np.array_equal(bits(a), bits(b))
    rm = dev(c["running_mean"]); rv = dev(c["running_var"])
    e0 = ops.batchnorm2d_act_eval(x, gamma, beta, rm, rv, B.EPS, slope, residual=r)
    e1 = ops.batchnorm2d_act_eval(off_by_4_bytes(x), gamma, beta, rm, rv, B.EPS, slope, residual=r)
    assert np.array_equal(bits(e0), bits(e1))


def test_bad_arguments_are_refused():
    from cl_ica_amd import ops
    x = torch.randn(4, 8, 2, 2, device="cuda"); w = torch.ones(8, device="cuda"); b = torch.zeros(8, device="cuda")
    with pytest.raises(RuntimeError):
        ops.batchnorm2d_act_fwd(x[:1, :, :1, :1].contiguous(), w, b)          # one value per channel
    with pytest.raises(RuntimeError):
        ops.batchnorm2d_act_fwd(x, w, b, slope=-0.1)
    with pytest.raises(ValueError):
        ops.batchnorm2d_act_fwd(x.contiguous(memory_format=torch.channels_last), w, b)
    with pytest.raises(ValueError):
        ops.batchnorm2d_act_fwd(x, w[:3], b)
    with pytest.raises(ValueError):
        ops.batchnorm2d_act_fwd(x, w, b, residual=x[:2])
    assert ops.bn2d_workspace(4, 8, 4, x.device) is ops.bn2d_workspace(4, 8, 4, x.device)      # never a new buffer


# ------------------------------------------------------------------------------------------------ 2. one block against fp64
def block_run(blk, x, c):
    """(output, input gradient, parameter gradients by name, buffers by name) of one training pass with objective sum(y c)."""
    blk.zero_grad(set_to_none=True)
    xin = x.clone().requires_grad_(True)
    y = blk(xin)
    (y * c).sum().backward()
    return (y.detach(), xin.grad, {k: p.grad for k, p in blk.named_parameters()}, {k: b.detach().clone() for k, b in blk.named_buffers()})


@pytest.mark.parametrize("case", B.BLOCK_CASES, ids=lambda s: "-".join(map(str, s)))
def test_block_against_fp64(monkeypatch, case):
    """NORM_MODE "hip" against an fp64 CPU copy of the same block: each quantity within 4 x the distance of the "torch"-mode fp32 GPU run
    from that fp64 result (the project's allowance factor), floor 1e-5.  The case has no pre-activation near a kink
    (tests/test_bn2d_host.py)."""
    from cl_ica_amd import resnet
    blk, x, c = B.make_block(*case)
    y64, dx64, g64, b64 = block_run(copy.deepcopy(blk).double(), x.double(), c.double())
    res = {}
    for mode in ("torch", "hip"):
        monkeypatch.setattr(resnet, "NORM_MODE", mode)
        res[mode] = block_run(copy.deepcopy(blk).cuda(), x.cuda(), c.cuda())
    name = "block " + "-".join(map(str, case))
    items = [("y", 0, None), ("dx", 1, None)] + [(f"grad {k}", 2, k) for k in g64]
    for what, idx, key in items:
        pick = (lambda t: t[idx]) if key is None else (lambda t: t[idx][key])
        truth = pick((y64, dx64, g64)).numpy()
        own = B.O.norm_err(host(pick(res["torch"])), truth)
        bound = max(4.0 * own, 1e-5)
        err = PARITY.check("bn2d_block", name, what, host(pick(res["hip"])), truth, tol=bound,
                           note="4 x torch fp32's own error against fp64, floor 1e-5")
        print(f"{name} {what}: HIP {err:.3e}, torch fp32 {own:.3e}, bound {bound:.3e}")
    for k, v in res["hip"][3].items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(res["torch"][3][k]) == int(b64[k]) == 1
        else:
            assert B.O.norm_err(host(v), host(res["torch"][3][k])) < 1e-6, k
            PARITY.check("bn2d_block", name, k, host(v), b64[k].numpy())


# ------------------------------------------------------------------------------------------------ 3. the whole backbone
def backbone():
    from cl_ica_amd import resnet
    torch.manual_seed(11)
    f = resnet.resnet18(num_classes=30)
    x = torch.randn(3, 3, 64, 64, generator=torch.Generator().manual_seed(12))
    return f.train(), x


def test_backbone_forward_against_fp64_and_reproducible(monkeypatch):
    from cl_ica_amd import resnet
    f, x = backbone()
    with torch.no_grad():
        y64 = copy.deepcopy(f).double()(x.double()).numpy()
    out = {}
    for mode in ("torch", "hip", "hip again"):
        monkeypatch.setattr(resnet, "NORM_MODE", mode.split()[0])
        g = copy.deepcopy(f).cuda()
        y = g(x.cuda())
        y.square().sum().backward()
        out[mode] = [y.detach()] + [p.grad for p in g.parameters()] + [b.float() for b in g.buffers()]
    own = B.O.norm_err(host(out["torch"][0]), y64)
    bound = max(4.0 * own, 1e-5)
    err = PARITY.check("bn2d_backbone", "resnet18 3x3x64x64", "y", host(out["hip"][0]), y64, tol=bound,
                       note="4 x torch fp32's own error against fp64, floor 1e-5")
    print(f"backbone y: HIP {err:.3e}, torch fp32 {own:.3e}, bound {bound:.3e}")
    assert all(bool(torch.isfinite(t).all()) for t in out["hip"])
    assert float(out["hip"][1].abs().max()) > 0                       # conv1.weight
    for a, b in zip(out["hip"], out["hip again"]):                    # two runs from the same state: the same bits
        assert np.array_equal(raw(a), raw(b))


def test_backbone_train_step_moves_every_parameter_by_at_most_lr(monkeypatch):
    from cl_ica_amd import resnet, threedident as T
    from cl_ica_amd.optim import Adam
    monkeypatch.setattr(resnet, "NORM_MODE", "hip")
    a = types.SimpleNamespace(position_only=True, rotation_and_color_only=False, rotation_only=False, color_only=False,
                              non_periodic_rotation_and_color=False, box_constraint=None, sphere_constraint=None,
                              unsupervised_loss="l2", identity_solution=False, encoder="rn18")
    torch.manual_seed(0)
    f = T.setup_f(a, 3, 0).to("cuda").train()
    assert isinstance(f[0], resnet.ResNet18) and f[0].fc.out_features == 30
    loss = T.make_unsupervised_loss(a, 3)
    g = torch.Generator().manual_seed(1)
    x1 = torch.randn(3, 3, 64, 64, generator=g)
    x2 = (x1 + 0.1 * torch.randn(3, 3, 64, 64, generator=g)).cuda()
    x1 = x1.cuda()
    lr = 1e-4
    opt = Adam(f.parameters(), lr=lr)
    before = {k: v.detach().clone() for k, v in f.named_parameters()}
    tot, per, lst = T.train_step(((None, None), (x1, x2)), loss, opt, f, sync=True)
    assert np.isfinite(tot)
    moved = [float((prm.detach() - before[k]).abs().max()) for k, prm in f.named_parameters()]
    assert all(np.isfinite(m) for m in moved) and max(moved) <= 1.001 * lr and max(moved) > 0.5 * lr
    assert int(f[0].bn1.num_batches_tracked) == 2                     # two views, one forward each


# ------------------------------------------------------------------------------------------------ 4. the HIP path is really taken
def test_the_hip_path_is_taken(monkeypatch):
    from cl_ica_amd import resnet
    f, x = backbone()
    f, x = f.cuda(), x.cuda()
    monkeypatch.setattr(resnet, "NORM_MODE", "hip")
    monkeypatch.setattr(torch.nn.functional, "batch_norm", refuse)
    monkeypatch.setattr(torch.nn.functional, "relu", refuse)
    f(x).sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in f.parameters())
    assert int(f.bn1.num_batches_tracked) == 1 and int(f.layer2[0].downsample[1].num_batches_tracked) == 1
    f.eval()
    with torch.no_grad():
        assert bool(torch.isfinite(f(x)).all())
    assert int(f.bn1.num_batches_tracked) == 1
    with pytest.raises(AssertionError, match="torch's own normalisation"):       # inference inside autograd: the modules' own forward
        f(x)
    monkeypatch.setattr(resnet, "NORM_MODE", "torch")                             # the parent's path does call them
    with pytest.raises(AssertionError, match="torch's own normalisation"):
        with torch.no_grad():
            f(x)
    f.train()
    with pytest.raises(AssertionError, match="torch's own normalisation"):
        f(x)


def run_both_modes(monkeypatch, build, x, train=True, grad=True):
    """The same module (deep copies) under NORM_MODE "hip" and "torch": output, input gradient, parameter gradients, buffers."""
    from cl_ica_amd import resnet
    base = build()
    out = {}
    for nm in ("hip", "torch"):
        monkeypatch.setattr(resnet, "NORM_MODE", nm)
        f = copy.deepcopy(base).train(train)
        xin = x.clone().requires_grad_(grad)
        with torch.set_grad_enabled(grad):
            y = f(xin)
        res = [y.detach()]
        if grad:
            y.square().sum().backward()
            res += [xin.grad] + [p.grad for p in f.parameters() if p.grad is not None]
        out[nm] = res + [b.float() for b in f.buffers()]
    assert len(out["hip"]) == len(out["torch"])
    for a, b in zip(out["hip"], out["torch"]):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(raw(a), raw(b))


def block_with(norm):
    def build():
        from cl_ica_amd import resnet
        torch.manual_seed(3)
        blk = resnet.BasicBlock(16, 32, 2)
        if norm is not None:
            blk.bn1, blk.bn2, blk.downsample[1] = norm(32), norm(32), norm(32)
        return blk.cuda()
    return build


@pytest.mark.parametrize("name,norm,train", [
    ("without affine", lambda n: torch.nn.BatchNorm2d(n, affine=False), True),
    ("without running statistics", lambda n: torch.nn.BatchNorm2d(n, track_running_stats=False), True),
    ("with a cumulative average", lambda n: torch.nn.BatchNorm2d(n, momentum=None), True),
    ("in eval mode inside autograd", None, False),
])
def test_configurations_outside_the_kernels_run_as_before(monkeypatch, name, norm, train):
    x = torch.randn(4, 16, 8, 8, generator=torch.Generator().manual_seed(1)).cuda()
    run_both_modes(monkeypatch, block_with(norm), x, train=train)


def test_inputs_outside_the_kernels_run_as_before(monkeypatch):
    x = torch.randn(4, 16, 8, 8, generator=torch.Generator().manual_seed(2))
    build = block_with(None)
    run_both_modes(monkeypatch, lambda: build().to(memory_format=torch.channels_last),
                   x.cuda().contiguous(memory_format=torch.channels_last))                             # channels-last
    run_both_modes(monkeypatch, lambda: build().double(), x.cuda().double())                           # not fp32
    run_both_modes(monkeypatch, lambda: build().cpu(), x)                                              # not on the GPU


# ------------------------------------------------------------------------------------------------ 5. graph replay
def unit_step(x, r, gamma, beta, dy, rm, rv, slope=0.0):
    from cl_ica_amd import ops
    y, a, b = ops.batchnorm2d_act_fwd(x, gamma, beta, rm, rv, B.EPS, B.MOMENTUM, slope, residual=r)
    return (y, a, b) + tuple(ops.batchnorm2d_act_bwd(x, y, dy, gamma, a, b, slope, need_dr=True))


@pytest.mark.parametrize("shape", [(16, 64, 16, 16), (8, 512, 2, 2)], ids=lambda s: "x".join(map(str, s)))
def test_eager_calls_and_graph_replays_give_the_same_bits(shape):
    N, C, H, W = shape
    c = B.make_case(N, C, H, W, 1, True)
    x, r, dy = maps(c, shape)
    gamma, beta = dev(c["gamma"]), dev(c["beta"])
    rm, rv = dev(c["running_mean"]), dev(c["running_var"])
    first = [bits(t).copy() for t in unit_step(x, r, gamma, beta, dy, rm, rv)]
    second = [bits(t).copy() for t in unit_step(x, r, gamma, beta, dy, rm, rv)]           # (also the warm-up of the capture)
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    want_rm, want_rv = bits(rm).copy(), bits(rv).copy()                                   # after two calls
    srm, srv = dev(c["running_mean"]), dev(c["running_var"])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = unit_step(x, r, gamma, beta, dy, srm, srv)
    with torch.no_grad():
        srm.copy_(dev(c["running_mean"])); srv.copy_(dev(c["running_var"]))             # capturing launches nothing
    for _ in range(2):
        for t in outs:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, t in zip(first, outs):
            assert np.array_equal(a, bits(t))
    assert np.array_equal(bits(srm), want_rm) and np.array_equal(bits(srv), want_rv)


def test_capturing_without_a_warm_up_raises():
    from cl_ica_amd import ops
    from cl_ica_amd._lib import ClicaError
    shape = (3, 11, 5, 6)                    # a shape no other test uses: no workspace yet
    x = torch.randn(*shape, device="cuda"); w = torch.ones(11, device="cuda"); b = torch.zeros(11, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(ClicaError, match="before capturing"):
        with torch.cuda.graph(graph):
            ops.batchnorm2d_act_fwd(x, w, b)
    assert not torch.cuda.is_current_stream_capturing()
    y, _, _ = ops.batchnorm2d_act_fwd(x, w, b)                         # the process goes on eagerly
    assert bool(torch.isfinite(y).all())
