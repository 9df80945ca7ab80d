"""The stem unit BatchNorm2d + ReLU + max-pool 3/2/1 and the global average pool on the HIP kernels of csrc/pool2d.hip: the C ABI
against the fp64 oracle (tests/pool2d_oracle.py) and, bit for bit, against the unfused unit followed by torch's pool; the first-maximum
rule on exact ties; the ResNet-18 stand-in with POOL_MODE "hip" against "torch"; the proof that the HIP path is taken; the
configurations that keep torch's modules; bit reproducibility eager / graph replay."""
import copy

import numpy as np
import pytest
import torch

import pool2d_oracle as Q
from bn_family_util import bits, deterministic_convolutions, dev, host, off_by_4_bytes, raw  # noqa: F401 (the autouse fixture)
from conftest import PARITY

pytestmark = pytest.mark.gpu
F = torch.nn.functional
ids = lambda s: "x".join(map(str, s))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def inputs(c, shape):
    return dev(Q.to_nchw(c["x"], *shape)), dev(c["dp"]), dev(c["gamma"]), dev(c["beta"])


def unit_step(x, dp, gamma, beta, rm, rv, slope):
    from cl_ica_amd import ops
    p, a, b = ops.batchnorm2d_act_maxpool_fwd(x, gamma, beta, rm, rv, Q.EPS, Q.MOMENTUM, slope)
    return (p, a, b) + tuple(ops.batchnorm2d_act_maxpool_bwd(x, dp, gamma, beta, a, b, slope))


# ------------------------------------------------------------------------------------------------ 1. ABI sweep against the oracle
@pytest.mark.parametrize("cls", range(len(Q.CLASSES)))
@pytest.mark.parametrize("shape", Q.SHAPES, ids=ids)
def test_abi_against_the_oracle(shape, cls):
    N, C, H, W = shape
    for slope in Q.SLOPES:
        c, fw, bw = Q.reference(N, C, H, W, cls, slope)
        x, dp, gamma, beta = inputs(c, shape)
        rm, rv = dev(c["running_mean"]), dev(c["running_var"])
        p, save_mean, save_invstd, dx, dgamma, dbeta = unit_step(x, dp, gamma, beta, rm, rv, slope)
        assert tuple(p.shape) == (N, C) + Q.out_hw(H, W)
        case, fam = f"{N}x{C}x{H}x{W} cls{cls} slope{slope}", "pool2d_abi"
        PARITY.check(fam, case, "p", host(p), fw["p"])
        PARITY.check(fam, case, "save_mean", host(save_mean), fw["mean"])
        PARITY.check(fam, case, "save_invstd", host(save_invstd), fw["invstd"])
        PARITY.check(fam, case, "running_mean", host(rm), fw["running_mean"])
        PARITY.check(fam, case, "running_var", host(rv), fw["running_var"])
        cols = Q.left_out(fw, shape, slope)
        assert cols.mean() <= Q.MAX_LEFT_OUT
        if N * H * W > 2:                      # dx at M = 2 is ill-conditioned
            PARITY.check(fam, case, "dx", Q.to_rows(host(dx))[:, ~cols], bw["dx"][:, ~cols])
        PARITY.check(fam, case, "dgamma", host(dgamma)[~cols], bw["dgamma"][~cols])
        PARITY.check(fam, case, "dbeta", host(dbeta)[~cols], bw["dbeta"][~cols])


# ------------------------------------------------------------------------------------------------ 2. the bits of the composition
@pytest.mark.parametrize("shape", Q.SHAPES, ids=ids)
def test_same_bits_as_the_unfused_unit_followed_by_torchs_pool(shape):
    """P, the saved and the running statistics equal, bit for bit, max_pool2d of the unfused unit's output and its statistics; the
    gradients are within 1e-5 of the unfused backward fed with torch's pool backward (their summation orders differ)."""
    from cl_ica_amd import ops
    N, C, H, W = shape
    for cls in range(len(Q.CLASSES)):
        for slope in Q.SLOPES:
            c = Q.make_case(N, C, H, W, cls)
            x, dp, gamma, beta = inputs(c, shape)
            rm, rv = dev(c["running_mean"]), dev(c["running_var"])
            p, a, b, dx, dgamma, dbeta = unit_step(x, dp, gamma, beta, rm, rv, slope)
            rm2, rv2 = dev(c["running_mean"]), dev(c["running_var"])
            y, a2, b2 = ops.batchnorm2d_act_fwd(x, gamma, beta, rm2, rv2, Q.EPS, Q.MOMENTUM, slope)
            y.requires_grad_(True)
            p2 = F.max_pool2d(y, 3, 2, 1)
            what = (shape, cls, slope)
            assert same_bits(p, p2), what
            assert same_bits(a, a2) and same_bits(b, b2) and same_bits(rm, rm2) and same_bits(rv, rv2), what
            dy, = torch.autograd.grad(p2, y, dp)
            dx2, _, dgamma2, dbeta2 = ops.batchnorm2d_act_bwd(x, y.detach(), dy.contiguous(), gamma, a2, b2, slope)
            if N * H * W > 2:
                assert Q.O.norm_err(host(dx), host(dx2)) < 1e-5, what
            assert Q.O.norm_err(host(dgamma), host(dgamma2)) < 1e-5 and Q.O.norm_err(host(dbeta), host(dbeta2)) < 1e-5, what


# ------------------------------------------------------------------------------------------------ 3. exact ties
@pytest.mark.parametrize("shape", [(1, 2, 3, 3), (3, 5, 7, 9), (2, 65, 8, 8), (6, 40, 32, 32)], ids=ids)
def test_ties_send_the_gradient_to_the_first_maximum(shape):
    """Planes of duplicated 2 x 2 blocks (and, at slope 0, every window of non-positive z): dx against the fp64 oracle, whose routing
    tests/test_pool2d_host.py holds against torch's."""
    N, C, H, W = shape
    for slope in Q.SLOPES:
        c, fw, bw = Q.reference(N, C, H, W, Q.TIE_CLASS, slope)
        x, dp, gamma, beta = inputs(c, shape)
        _, _, _, dx, dgamma, dbeta = unit_step(x, dp, gamma, beta, None, None, slope)
        cols = Q.left_out(fw, shape, slope)
        assert cols.mean() <= Q.MAX_LEFT_OUT
        PARITY.check("pool2d_ties", f"{shape} slope{slope}", "dx", Q.to_rows(host(dx))[:, ~cols], bw["dx"][:, ~cols])
        PARITY.check("pool2d_ties", f"{shape} slope{slope}", "dgamma", host(dgamma)[~cols], bw["dgamma"][~cols])


# ------------------------------------------------------------------------------------------------ 4. inference; unaligned tensors
@pytest.mark.parametrize("shape", Q.EVAL_SHAPES, ids=ids)
def test_eval_abi_against_the_oracle(shape):
    from cl_ica_amd import ops
    N, C, H, W = shape
    for cls in range(len(Q.CLASSES)):
        c = Q.make_case(N, C, H, W, cls)
        rm = (c["x"].mean(0) + c["running_mean"]).astype(np.float32)          # statistics of the size of the data's own
        rv = (c["x"].var(0) * c["running_var"]).astype(np.float32)
        x, _, gamma, beta = inputs(c, shape)
        for slope in Q.SLOPES:
            p = ops.batchnorm2d_act_maxpool_eval(x, gamma, beta, dev(rm), dev(rv), Q.EPS, slope)
            PARITY.check("pool2d_abi", f"eval {N}x{C}x{H}x{W} cls{cls} slope{slope}", "p", host(p), Q.evaluate(c, shape, rm, rv, slope))
            y = ops.batchnorm2d_act_eval(x, gamma, beta, dev(rm), dev(rv), Q.EPS, slope)
            assert same_bits(p, F.max_pool2d(y, 3, 2, 1))


@pytest.mark.parametrize("shape", Q.UNALIGNED_SHAPES, ids=ids)
def test_unaligned_input_gives_the_same_bits(shape):
    """W % 4 == 0 on both shapes: an unaligned tensor makes the kernels move the same values with scalar accesses, in the same reduction
    order, so every result has the aligned call's bits -- inference, training forward and backward."""
    from cl_ica_amd import ops
    N, C, H, W = shape
    slope = 0.0
    c, fw, _ = Q.reference(N, C, H, W, 1, slope)
    x, dp, gamma, beta = inputs(c, shape)
    assert x.data_ptr() % 16 == 0
    rm, rv = dev(c["running_mean"]), dev(c["running_var"])
    e0 = ops.batchnorm2d_act_maxpool_eval(x, gamma, beta, rm, rv, Q.EPS, slope)
    e1 = ops.batchnorm2d_act_maxpool_eval(off_by_4_bytes(x), gamma, beta, rm, rv, Q.EPS, slope)
    assert same_bits(e0, e1)
    want = unit_step(x, dp, gamma, beta, None, None, slope)
    PARITY.check("pool2d_abi", f"unaligned {shape}", "p", host(want[0]), fw["p"])
    for variant in ((off_by_4_bytes(x), dp), (off_by_4_bytes(x), off_by_4_bytes(dp))):
        for a, b in zip(want, unit_step(*variant, gamma, beta, None, None, slope)):
            assert same_bits(a, b)


def test_bad_arguments_are_refused():
    from cl_ica_amd import ops
    x = torch.randn(4, 8, 6, 6, device="cuda"); w = torch.ones(8, device="cuda"); b = torch.zeros(8, device="cuda")
    with pytest.raises(RuntimeError, match="N H W >= 2"):
        ops.batchnorm2d_act_maxpool_fwd(x[:1, :, :1, :1].contiguous(), w, b)
    with pytest.raises(RuntimeError, match="slope"):
        ops.batchnorm2d_act_maxpool_fwd(x, w, b, slope=1.5)
    with pytest.raises(RuntimeError, match="over the limit"):
        ops.batchnorm2d_act_maxpool_eval(torch.zeros(1, 8, 130, 130, device="cuda"), w, b, b, w)
    with pytest.raises(ValueError, match="shape of x"):
        ops.batchnorm2d_act_maxpool_bwd(x, x, w, b, b, w)                  # dp must be [N, C, Ho, Wo]
    with pytest.raises(ValueError):
        ops.batchnorm2d_act_maxpool_fwd(x, w[:3], b)
    assert ops.bn2d_maxpool_workspace(4, 8, 6, 6, x.device) is ops.bn2d_maxpool_workspace(4, 8, 6, 6, x.device)      # never a new buffer


# ------------------------------------------------------------------------------------------------ 5. global average pool
@pytest.mark.parametrize("C", [3, 512])
@pytest.mark.parametrize("hw", [(1, 1), (2, 2), (3, 5), (7, 7)], ids=ids)
def test_global_average_pool(hw, C):
    from cl_ica_amd import ops
    H, W = hw
    N = 5
    rng = np.random.default_rng(1000 * C + H * W)
    x = (1.0 + rng.normal(size=(N, C, H, W))).astype(np.float32)
    dy = rng.normal(size=(N, C)).astype(np.float32)
    y = ops.avgpool2d_global_fwd(dev(x))
    dx = ops.avgpool2d_global_bwd(dev(dy), H, W)
    assert tuple(y.shape) == (N, C) and tuple(dx.shape) == (N, C, H, W)
    case = f"{N}x{C}x{H}x{W}"
    PARITY.check("avgpool2d", case, "y", host(y), x.astype(np.float64).mean(axis=(2, 3)))
    PARITY.check("avgpool2d", case, "dx", host(dx), np.broadcast_to((dy.astype(np.float64) / (H * W))[:, :, None, None], x.shape))
    # the pair is adjoint: <dy, Y(x)> = <dX(dy), x>
    lhs = float((dy.astype(np.float64) * host(y)).sum()); rhs = float((host(dx).astype(np.float64) * x).sum())
    assert abs(lhs - rhs) <= 1e-5 * float((np.abs(dy) * np.abs(host(y))).sum())      # (each term carries a few ulp of fp32)
    assert same_bits(y, ops.avgpool2d_global_fwd(off_by_4_bytes(dev(x))))


# ------------------------------------------------------------------------------------------------ 6. the whole backbone
def backbone():
    from cl_ica_amd import resnet
    torch.manual_seed(11)
    f = resnet.resnet18(num_classes=30)
    x = torch.randn(3, 3, 64, 64, generator=torch.Generator().manual_seed(12))
    return f.train(), x


def pool_modes(monkeypatch, build, x, train=True, grad=True):
    """The same module (deep copies) under POOL_MODE "hip" and "torch", NORM_MODE "hip": output, then input and parameter gradients, then
    buffers."""
    from cl_ica_amd import resnet
    monkeypatch.setattr(resnet, "NORM_MODE", "hip")
    base = build()
    out = {}
    for mode in ("hip", "torch"):
        monkeypatch.setattr(resnet, "POOL_MODE", mode)
        f = copy.deepcopy(base).train(train)
        xin = x.clone().requires_grad_(grad)
        with torch.set_grad_enabled(grad):
            y = f(xin)
        res = [y.detach()]
        if grad:
            y.square().sum().backward()
            res += [xin.grad] + [p.grad for p in f.parameters()]
        out[mode] = res + [b.float() for b in f.buffers()]
    assert len(out["hip"]) == len(out["torch"])
    return out


def test_backbone_pool_modes_agree(monkeypatch):
    f, x = backbone()
    out = pool_modes(monkeypatch, lambda: copy.deepcopy(f).cuda(), x.cuda())
    assert np.array_equal(raw(out["hip"][0]), raw(out["torch"][0]))                  # outputs: the same bits
    for i, (a, b) in enumerate(zip(out["hip"], out["torch"])):                       # gradients and buffers: 1e-5 norm-wise
        err = Q.O.norm_err(host(a), host(b))
        assert err < 1e-5, (i, err)
    assert float(out["hip"][2].abs().max()) > 0                                      # conv1.weight's gradient
    out = pool_modes(monkeypatch, lambda: copy.deepcopy(f).cuda(), x.cuda(), train=False, grad=False)
    assert np.array_equal(raw(out["hip"][0]), raw(out["torch"][0]))


# ------------------------------------------------------------------------------------------------ 7. the HIP path is really taken
def refuse(*a, **k):
    raise AssertionError("torch's own pooling, normalisation or activation kernel was called")


def test_the_hip_path_is_taken(monkeypatch):
    from cl_ica_amd import resnet
    f, x = backbone()
    f, x = f.cuda(), x.cuda()
    monkeypatch.setattr(resnet, "NORM_MODE", "hip")
    monkeypatch.setattr(resnet, "POOL_MODE", "hip")
    for name in ("max_pool2d", "adaptive_avg_pool2d", "batch_norm", "relu"):
        monkeypatch.setattr(F, name, refuse)
    f(x).sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in f.parameters())
    assert int(f.bn1.num_batches_tracked) == 1
    f.eval()
    with torch.no_grad():
        assert bool(torch.isfinite(f(x)).all())
    assert int(f.bn1.num_batches_tracked) == 1
    monkeypatch.setattr(resnet, "POOL_MODE", "torch")                                 # the parent's path does call them
    with pytest.raises(AssertionError, match="torch's own pooling"):
        with torch.no_grad():
            f(x)
    f.train()
    with pytest.raises(AssertionError, match="torch's own pooling"):
        f(x)


# ------------------------------------------------------------------------------------------------ 8. configurations that keep torch's modules
def spy_on_pool_entry_points(monkeypatch):
    from cl_ica_amd import ops
    calls = []
    for name in ("batchnorm2d_act_maxpool_fwd", "batchnorm2d_act_maxpool_eval", "batchnorm2d_act_maxpool_bwd"):
        monkeypatch.setattr(ops, name, (lambda nm, fn: lambda *a, **k: (calls.append(nm), fn(*a, **k))[1])(name, getattr(ops, name)))
    return calls


def small_net(change=None):
    def build():
        from cl_ica_amd import resnet
        torch.manual_seed(3)
        f = resnet.resnet18(num_classes=10)
        if change is not None:
            change(f)
        return f.cuda()
    return build


def set_pool(pool):
    def change(f):
        f.maxpool = pool
    return change


@pytest.mark.parametrize("name,build,train", [
    ("a 2 x 2 max-pool", small_net(set_pool(torch.nn.MaxPool2d(2, 2))), True),
    ("ceil mode", small_net(set_pool(torch.nn.MaxPool2d(3, 2, 1, ceil_mode=True))), True),
    ("eval mode inside autograd", small_net(), False),
])
def test_configurations_outside_the_stem_kernels_run_as_before(monkeypatch, name, build, train):
    """The stem keeps the unfused unit and torch's module: no fused entry point is called, and the outputs, gradients and buffers have the
    bits of POOL_MODE "torch"."""
    calls = spy_on_pool_entry_points(monkeypatch)
    x = torch.randn(2, 3, 63, 63, generator=torch.Generator().manual_seed(1)).cuda()
    out = pool_modes(monkeypatch, build, x, train=train)
    assert not calls
    for a, b in zip(out["hip"], out["torch"]):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(raw(a), raw(b))


def test_inputs_outside_the_kernels_run_as_before(monkeypatch):
    calls = spy_on_pool_entry_points(monkeypatch)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    build = small_net()
    for make, xin in ((lambda: build().to(memory_format=torch.channels_last), x.cuda().contiguous(memory_format=torch.channels_last)),
                      (lambda: build().double(), x.cuda().double()),                             # not fp32
                      (lambda: build().cpu(), x)):                                               # not on the GPU
        out = pool_modes(monkeypatch, make, xin)
        assert not calls
        for a, b in zip(out["hip"], out["torch"]):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(raw(a), raw(b))


def test_a_plane_over_the_limit_keeps_torchs_max_pool(monkeypatch):
    """(1, 3, 260, 260): the stem plane is 130 x 130, over the limit of the fused unit, so none of its entry points is called."""
    from cl_ica_amd import ops, resnet
    monkeypatch.setattr(resnet, "NORM_MODE", "hip")
    monkeypatch.setattr(resnet, "POOL_MODE", "hip")
    calls = spy_on_pool_entry_points(monkeypatch)
    assert not ops.bn2d_maxpool_fits(130, 130)
    f = small_net()().eval()
    with torch.no_grad():
        y = f(torch.randn(1, 3, 260, 260, generator=torch.Generator().manual_seed(4)).cuda())
    assert bool(torch.isfinite(y).all()) and not calls


# ------------------------------------------------------------------------------------------------ 9. graph replay
@pytest.mark.parametrize("shape", [(6, 40, 32, 32), (3, 5, 7, 9)], ids=ids)
def test_eager_calls_and_graph_replays_give_the_same_bits(shape):
    from cl_ica_amd import ops
    N, C, H, W = shape
    c = Q.make_case(N, C, H, W, 1)
    x, dp, gamma, beta = inputs(c, shape)
    rm, rv = dev(c["running_mean"]), dev(c["running_var"])

    def step(rm, rv):
        out = unit_step(x, dp, gamma, beta, rm, rv, 0.0)
        y = ops.avgpool2d_global_fwd(out[0])
        return out + (y, ops.avgpool2d_global_bwd(y, *out[0].shape[2:]))
    first = [bits(t).copy() for t in step(rm, rv)]
    second = [bits(t).copy() for t in step(rm, rv)]                                       # (also the warm-up of the capture)
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    want_rm, want_rv = bits(rm).copy(), bits(rv).copy()                                   # after two calls
    srm, srv = dev(c["running_mean"]), dev(c["running_var"])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(srm, srv)
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
            ops.batchnorm2d_act_maxpool_fwd(x, w, b)
    assert not torch.cuda.is_current_stream_capturing()
    p, _, _ = ops.batchnorm2d_act_maxpool_fwd(x, w, b)                 # the process goes on eagerly
    assert bool(torch.isfinite(p).all())
