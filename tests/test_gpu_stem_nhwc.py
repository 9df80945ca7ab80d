"""The stem unit BatchNorm2d + ReLU + max-pool 3/2/1 on dense channels-last activations (the HIP kernels of csrc/bn2d_nhwc.hip): the C
ABI against the fp64 oracle (tests/pool2d_oracle.py through tests/stem_nhwc_cases.py) and, bit for bit, against the unfused channels-last
unit followed by torch's pool; the first-maximum rule on exact ties; inference; unaligned tensors; refusals; the ResNet-18 stand-in with
NHWC_STEM_MODE "hip" against "torch" and the proof that the fused path is taken; the configurations that keep torch's module; bit
reproducibility eager / graph replay."""
import copy

import numpy as np
import pytest
import torch

import pool2d_oracle as Q
import stem_nhwc_cases as K
from bn_family_util import bits, deterministic_convolutions, dev, host, raw  # noqa: F401 (the autouse fixture)
from conftest import PARITY

pytestmark = pytest.mark.gpu
F = torch.nn.functional
CL = torch.channels_last
ids = lambda s: "x".join(map(str, s))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def dense_cl(t):
    return t.is_contiguous(memory_format=CL) and t.permute(0, 2, 3, 1).is_contiguous()


def nhwc(rows, dims):
    """Rows [N H W, C] as the device tensor [N, C, H, W] whose memory they are."""
    N, C, H, W = dims
    t = dev(rows).reshape(N, H, W, C).permute(0, 3, 1, 2)
    assert t.is_contiguous(memory_format=CL)
    return t


def rows_of(t):
    """The memory of a dense channels-last [N, C, H, W] as host rows [N H W, C]."""
    assert dense_cl(t)
    return host(t.permute(0, 2, 3, 1)).reshape(-1, t.shape[1])


def inputs(c, shape):
    dp = dev(c["dp"]).contiguous(memory_format=CL)
    assert dense_cl(dp)
    return nhwc(c["x"], shape), dp, dev(c["gamma"]), dev(c["beta"])


def unit_step(x, dp, gamma, beta, rm, rv, slope):
    from cl_ica_amd import ops
    p, a, b = ops.batchnorm2d_act_maxpool_fwd_nhwc(x, gamma, beta, rm, rv, Q.EPS, Q.MOMENTUM, slope)
    return (p, a, b) + tuple(ops.batchnorm2d_act_maxpool_bwd_nhwc(x, dp, gamma, beta, a, b, slope))


def off_by_4_bytes(t):
    """A dense channels-last copy of t whose storage starts 4 bytes off a 16-byte boundary."""
    N, C, H, W = t.shape
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    u = buf[1:].view(N, H, W, C).permute(0, 3, 1, 2)
    u.copy_(t)
    assert u.data_ptr() % 16 == 4
    return u


# ------------------------------------------------------------------------------------------------ 1. ABI sweep against the oracle
@pytest.mark.parametrize("cls", range(len(K.CLASSES)))
@pytest.mark.parametrize("shape", K.SHAPES, ids=ids)
def test_abi_against_the_oracle(shape, cls):
    N, C, H, W = shape
    for slope in K.SLOPES:
        c, fw, bw = K.reference(shape, cls, slope)
        x, dp, gamma, beta = inputs(c, shape)
        rm, rv = dev(c["running_mean"]), dev(c["running_var"])
        p, save_mean, save_invstd, dx, dgamma, dbeta = unit_step(x, dp, gamma, beta, rm, rv, slope)
        assert tuple(p.shape) == (N, C) + Q.out_hw(H, W) and tuple(dx.shape) == shape
        case, fam = f"{N}x{C}x{H}x{W} cls{cls} slope{slope}", "stem_nhwc_abi"
        PARITY.check(fam, case, "p", host(p), fw["p"])
        PARITY.check(fam, case, "save_mean", host(save_mean), fw["mean"])
        PARITY.check(fam, case, "save_invstd", host(save_invstd), fw["invstd"])
        PARITY.check(fam, case, "running_mean", host(rm), fw["running_mean"])
        PARITY.check(fam, case, "running_var", host(rv), fw["running_var"])
        cols = Q.left_out(fw, shape, slope)
        assert cols.mean() <= Q.MAX_LEFT_OUT
        if N * H * W > 2:                      # dx at M = 2 is ill-conditioned
            PARITY.check(fam, case, "dx", rows_of(dx)[:, ~cols], bw["dx"][:, ~cols])
        PARITY.check(fam, case, "dgamma", host(dgamma)[~cols], bw["dgamma"][~cols])
        PARITY.check(fam, case, "dbeta", host(dbeta)[~cols], bw["dbeta"][~cols])


# ------------------------------------------------------------------------------------------------ 2. the bits of the composition
@pytest.mark.parametrize("shape", K.SHAPES, ids=ids)
def test_same_bits_as_the_unfused_unit_followed_by_torchs_pool(shape):
    """P, the saved and the running statistics equal, bit for bit, max_pool2d of the unfused channels-last unit's output and its
    statistics; P is channels-last; the gradients are within 1e-5 of the unfused backward fed with torch's pool backward and of the
    NCHW fused stem on the permuted tensor (their summation orders differ)."""
    from cl_ica_amd import ops
    N, C, H, W = shape
    for cls in range(len(K.CLASSES)):
        for slope in K.SLOPES:
            c = K.make_case(shape, cls)
            x, dp, gamma, beta = inputs(c, shape)
            rm, rv = dev(c["running_mean"]), dev(c["running_var"])
            p, a, b, dx, dgamma, dbeta = unit_step(x, dp, gamma, beta, rm, rv, slope)
            assert dense_cl(p) and dense_cl(dx)
            rm2, rv2 = dev(c["running_mean"]), dev(c["running_var"])
            y, a2, b2 = ops.batchnorm2d_act_fwd_nhwc(x, gamma, beta, rm2, rv2, Q.EPS, Q.MOMENTUM, slope)
            y.requires_grad_(True)
            p2 = F.max_pool2d(y, 3, 2, 1)
            what = (shape, cls, slope)
            assert same_bits(p, p2), what
            assert same_bits(a, a2) and same_bits(b, b2) and same_bits(rm, rm2) and same_bits(rv, rv2), what
            dy, = torch.autograd.grad(p2, y, dp)
            dx2, _, dgamma2, dbeta2 = ops.batchnorm2d_act_bwd_nhwc(x, y.detach(), dy.contiguous(memory_format=CL), gamma, a2, b2, slope)
            xn = x.contiguous()
            p3, a3, b3 = ops.batchnorm2d_act_maxpool_fwd(xn, gamma, beta, None, None, Q.EPS, Q.MOMENTUM, slope)
            dx3, dgamma3, dbeta3 = ops.batchnorm2d_act_maxpool_bwd(xn, dp.contiguous(), gamma, beta, a3, b3, slope)
            for dxo, dgo, dbo in ((dx2, dgamma2, dbeta2), (dx3, dgamma3, dbeta3)):
                if N * H * W > 2:
                    assert Q.O.norm_err(host(dx), host(dxo)) < 1e-5, what
                assert Q.O.norm_err(host(dgamma), host(dgo)) < 1e-5 and Q.O.norm_err(host(dbeta), host(dbo)) < 1e-5, what


# ------------------------------------------------------------------------------------------------ 3. exact ties
@pytest.mark.parametrize("shape", K.TIE_SHAPES, ids=ids)
def test_ties_send_the_gradient_to_the_first_maximum(shape):
    """Planes of duplicated 2 x 2 blocks (and, at slope 0, every window of non-positive z): dx against the fp64 oracle, whose routing
    tests/test_pool2d_host.py holds against torch's."""
    for slope in K.SLOPES:
        c, fw, bw = K.reference(shape, K.TIE_CLASS, slope)
        x, dp, gamma, beta = inputs(c, shape)
        _, _, _, dx, dgamma, dbeta = unit_step(x, dp, gamma, beta, None, None, slope)
        cols = Q.left_out(fw, shape, slope)
        assert cols.mean() <= Q.MAX_LEFT_OUT
        PARITY.check("stem_nhwc_ties", f"{shape} slope{slope}", "dx", rows_of(dx)[:, ~cols], bw["dx"][:, ~cols])
        PARITY.check("stem_nhwc_ties", f"{shape} slope{slope}", "dgamma", host(dgamma)[~cols], bw["dgamma"][~cols])


# ------------------------------------------------------------------------------------------------ 4. inference; 5. unaligned tensors
@pytest.mark.parametrize("shape", K.EVAL_SHAPES, ids=ids)
def test_eval_abi_against_the_oracle(shape):
    from cl_ica_amd import ops
    N, C, H, W = shape
    for cls in range(len(K.CLASSES)):
        c = K.make_case(shape, cls)
        rm = (c["x"].mean(0) + c["running_mean"]).astype(np.float32)          # statistics of the size of the data's own
        rv = (c["x"].var(0) * c["running_var"]).astype(np.float32)
        x, _, gamma, beta = inputs(c, shape)
        for slope in K.SLOPES:
            p = ops.batchnorm2d_act_maxpool_eval_nhwc(x, gamma, beta, dev(rm), dev(rv), Q.EPS, slope)
            assert dense_cl(p)
            PARITY.check("stem_nhwc_abi", f"eval {N}x{C}x{H}x{W} cls{cls} slope{slope}", "p", host(p), Q.evaluate(c, shape, rm, rv, slope))
            y = ops.batchnorm2d_act_eval_nhwc(x, gamma, beta, dev(rm), dev(rv), Q.EPS, slope)
            assert same_bits(p, F.max_pool2d(y, 3, 2, 1))


@pytest.mark.parametrize("shape", K.UNALIGNED_SHAPES, ids=ids)
def test_unaligned_tensors_give_the_same_bits(shape):
    """C % 4 == 0: an unaligned x or dp makes the kernels move the same four channels per lane with scalar accesses, in the same reduction
    order, so every result has the aligned call's bits -- inference, training forward and backward."""
    from cl_ica_amd import ops
    slope = 0.0
    c, fw, _ = K.reference(shape, 1, slope)
    x, dp, gamma, beta = inputs(c, shape)
    assert x.data_ptr() % 16 == 0 and dp.data_ptr() % 16 == 0
    rm, rv = dev(c["running_mean"]), dev(c["running_var"])
    e0 = ops.batchnorm2d_act_maxpool_eval_nhwc(x, gamma, beta, rm, rv, Q.EPS, slope)
    e1 = ops.batchnorm2d_act_maxpool_eval_nhwc(off_by_4_bytes(x), gamma, beta, rm, rv, Q.EPS, slope)
    assert same_bits(e0, e1)
    want = unit_step(x, dp, gamma, beta, None, None, slope)
    PARITY.check("stem_nhwc_abi", f"unaligned {shape}", "p", host(want[0]), fw["p"])
    for variant in ((off_by_4_bytes(x), dp), (x, off_by_4_bytes(dp)), (off_by_4_bytes(x), off_by_4_bytes(dp))):
        for a, b in zip(want, unit_step(*variant, gamma, beta, None, None, slope)):
            assert same_bits(a, b)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_bad_arguments_are_refused():
    from cl_ica_amd import _lib, ops
    x = torch.randn(4, 8, 6, 6, device="cuda").contiguous(memory_format=CL); w = torch.ones(8, device="cuda"); b = torch.zeros(8, device="cuda")
    with pytest.raises(ValueError, match="dense channels-last"):
        ops.batchnorm2d_act_maxpool_fwd_nhwc(x.contiguous(), w, b)                         # an NCHW tensor
    with pytest.raises(ValueError, match="dense channels-last"):
        ops.batchnorm2d_act_maxpool_eval_nhwc(x.contiguous(), w, b, b, w)
    with pytest.raises(RuntimeError, match="slope"):
        ops.batchnorm2d_act_maxpool_fwd_nhwc(x, w, b, slope=-0.1)
    with pytest.raises(RuntimeError, match="slope"):
        ops.batchnorm2d_act_maxpool_fwd_nhwc(x, w, b, slope=1.5)
    with pytest.raises(RuntimeError, match="slope"):
        ops.batchnorm2d_act_maxpool_eval_nhwc(x, w, b, b, w, slope=1.5)
    with pytest.raises(RuntimeError, match="N H W >= 2"):
        ops.batchnorm2d_act_maxpool_fwd_nhwc(x[:1, :, :1, :1].contiguous(memory_format=CL), w, b)
    with pytest.raises(ValueError, match="shape of x"):
        ops.batchnorm2d_act_maxpool_bwd_nhwc(x, x, w, b, b, w)                             # dp must be [N, C, Ho, Wo]
    with pytest.raises(ValueError):
        ops.batchnorm2d_act_maxpool_fwd_nhwc(x, w[:3], b)
    ws = ops.bn2d_nhwc_maxpool_workspace(4, 8, 6, 6, x.device)
    assert ws is ops.bn2d_nhwc_maxpool_workspace(4, 8, 6, 6, x.device)                     # never a new buffer
    # a short workspace at the ABI: CLICA_E_WORKSPACE, before any launch
    L = _lib.load()
    p = torch.empty(4, 8, 3, 3, device="cuda").contiguous(memory_format=CL); sm = torch.empty(8, device="cuda"); si = torch.empty(8, device="cuda")
    q = lambda t: t.data_ptr()
    assert L.clica_bn2d_nhwc_act_maxpool_fwd_train(q(x), q(w), q(b), 4, 8, 6, 6, 1e-5, 0.1, 0.0, q(p), q(sm), q(si), None, None, q(ws), 16,
                                                   None) == -2
    assert b"workspace of 16 bytes" in L.clica_last_error()
    assert L.clica_bn2d_nhwc_act_maxpool_bwd(q(x), q(p), q(w), q(b), q(sm), q(si), 4, 8, 6, 6, 0.0, q(x), q(sm), q(si), q(ws), 16, None) == -2
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 7. the whole backbone
NHWC_OPS = ("batchnorm2d_act_fwd_nhwc", "batchnorm2d_act_eval_nhwc", "batchnorm2d_act_bwd_nhwc", "batchnorm2d_act_maxpool_fwd_nhwc",
            "batchnorm2d_act_maxpool_eval_nhwc", "batchnorm2d_act_maxpool_bwd_nhwc", "avgpool2d_global_fwd_nhwc", "avgpool2d_global_bwd_nhwc")
NCHW_OPS = ("batchnorm2d_act_fwd", "batchnorm2d_act_eval", "batchnorm2d_act_bwd", "batchnorm2d_act_maxpool_fwd", "batchnorm2d_act_maxpool_eval",
            "batchnorm2d_act_maxpool_bwd", "avgpool2d_global_fwd", "avgpool2d_global_bwd")


def spy_on(monkeypatch):
    """Counts the calls of every bn2d / pool entry of cl_ica_amd.ops (resnet.py calls them through the module)."""
    from cl_ica_amd import ops
    calls = {k: 0 for k in NHWC_OPS + NCHW_OPS}

    def wrap(name, fn):
        def counted(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return counted
    for name in calls:
        monkeypatch.setattr(ops, name, wrap(name, getattr(ops, name)))
    return calls


def refuse(*a, **k):
    raise AssertionError("torch's own max-pool was called")


def backbone():
    from cl_ica_amd import resnet
    torch.manual_seed(11)
    f = resnet.resnet18(num_classes=30)
    x = torch.randn(3, 3, 64, 64, generator=torch.Generator().manual_seed(12))
    return f.train(), x


def cl_cuda(f, x):
    return f.cuda().to(memory_format=CL), x.cuda().contiguous(memory_format=CL)


def all_hip(monkeypatch, stem="hip"):
    from cl_ica_amd import resnet
    for name in ("NORM_MODE", "POOL_MODE", "NHWC_MODE"):
        monkeypatch.setattr(resnet, name, "hip")
    monkeypatch.setattr(resnet, "NHWC_STEM_MODE", stem)


def train_pass(f, x):
    """(output, parameter gradients, buffers) of one training pass of a copy of f."""
    g = copy.deepcopy(f).train()
    y = g(x)
    y.square().sum().backward()
    return [y.detach()] + [p.grad for p in g.parameters()] + [b.float() for b in g.buffers()], g


def test_the_fused_stem_is_taken_and_agrees_with_the_unfused_one(monkeypatch):
    f, x = backbone()
    f, x = cl_cuda(f, x)
    all_hip(monkeypatch, "torch")
    calls = spy_on(monkeypatch)
    want, _ = train_pass(f, x)
    assert calls["batchnorm2d_act_fwd_nhwc"] == 20 and calls["batchnorm2d_act_bwd_nhwc"] == 20          # today's counts
    assert calls["batchnorm2d_act_maxpool_fwd_nhwc"] == 0 and calls["batchnorm2d_act_maxpool_bwd_nhwc"] == 0
    for k in calls:
        calls[k] = 0
    all_hip(monkeypatch, "hip")
    torchs_pool = F.max_pool2d
    monkeypatch.setattr(F, "max_pool2d", refuse)
    got, g = train_pass(f, x)
    assert calls["batchnorm2d_act_fwd_nhwc"] == 19 and calls["batchnorm2d_act_bwd_nhwc"] == 19
    assert calls["batchnorm2d_act_maxpool_fwd_nhwc"] == 1 and calls["batchnorm2d_act_maxpool_bwd_nhwc"] == 1
    assert calls["avgpool2d_global_fwd_nhwc"] == 1 and calls["avgpool2d_global_bwd_nhwc"] == 1
    assert calls["batchnorm2d_act_eval_nhwc"] == 0 and calls["batchnorm2d_act_maxpool_eval_nhwc"] == 0 and all(calls[k] == 0 for k in NCHW_OPS)
    assert int(g.bn1.num_batches_tracked) == 1
    assert len(got) == len(want) and np.array_equal(raw(got[0]), raw(want[0]))                        # outputs: the same bits
    for i, (a, b) in enumerate(zip(got, want)):                                                       # gradients and buffers: 1e-5 norm-wise
        err = Q.O.norm_err(host(a), host(b))
        assert err < 1e-5, (i, err)
    assert float(got[1].abs().max()) > 0                                                              # conv1.weight's gradient
    # inference outside autograd: the fused inference entry, once
    g.eval()
    with torch.no_grad():
        ye = g(x)
    assert calls["batchnorm2d_act_maxpool_eval_nhwc"] == 1 and calls["batchnorm2d_act_eval_nhwc"] == 19
    assert int(g.bn1.num_batches_tracked) == 1 and all(calls[k] == 0 for k in NCHW_OPS)
    all_hip(monkeypatch, "torch")                                                                   # the unfused stem: the same bits
    with pytest.raises(AssertionError, match="torch's own max-pool"):
        with torch.no_grad():
            g(x)
    monkeypatch.setattr(F, "max_pool2d", torchs_pool)
    with torch.no_grad():
        assert np.array_equal(raw(ye), raw(g(x)))
    assert calls["batchnorm2d_act_maxpool_eval_nhwc"] == 1


# ------------------------------------------------------------------------------------------------ 8. configurations that keep torch's module
def small_net(change=None):
    from cl_ica_amd import resnet
    torch.manual_seed(3)
    f = resnet.resnet18(num_classes=10)
    if change is not None:
        change(f)
    return f


def set_pool(pool):
    def change(f):
        f.maxpool = pool
    return change


@pytest.mark.parametrize("name,change", [("a 2 x 2 max-pool", set_pool(torch.nn.MaxPool2d(2, 2))),
                                         ("ceil mode", set_pool(torch.nn.MaxPool2d(3, 2, 1, ceil_mode=True)))])
def test_other_pools_run_the_unit_then_the_module(monkeypatch, name, change):
    """No fused stem entry is called: the unit, then the module, with the bits of NHWC_STEM_MODE "torch" in outputs, gradients, buffers."""
    x = torch.randn(2, 3, 63, 63, generator=torch.Generator().manual_seed(1))
    f, x = cl_cuda(small_net(change), x)
    calls = spy_on(monkeypatch)
    out = {}
    for stem in ("hip", "torch"):
        all_hip(monkeypatch, stem)
        out[stem], _ = train_pass(f, x)
    assert calls["batchnorm2d_act_maxpool_fwd_nhwc"] == 0 and calls["batchnorm2d_act_maxpool_bwd_nhwc"] == 0
    assert calls["batchnorm2d_act_fwd_nhwc"] == 40
    for a, b in zip(out["hip"], out["torch"]):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(raw(a), raw(b))


def test_a_plane_over_the_limit_runs_the_unit_then_the_module(monkeypatch):
    """The stem of resnet.py on a 2 x 32769 plane of 4 channels, one column over the limit on a side (without the convolution in front:
    MIOpen's search for such a shape takes most of a minute): no fused entry is called, and outputs, gradients and buffers have the bits
    of NHWC_STEM_MODE "torch".  One column less runs fused."""
    from cl_ica_amd import ops, resnet
    assert ops.bn2d_nhwc_maxpool_fits(2, 32768, 4) and not ops.bn2d_nhwc_maxpool_fits(2, 32769, 4)
    x = torch.randn(1, 4, 2, 32769, generator=torch.Generator().manual_seed(4)).cuda().contiguous(memory_format=CL)
    torch.manual_seed(5)
    bn, relu, pool = torch.nn.BatchNorm2d(4).cuda().train(), torch.nn.ReLU(), torch.nn.MaxPool2d(3, 2, 1)
    calls = spy_on(monkeypatch)
    out = {}
    for stem in ("hip", "torch"):
        all_hip(monkeypatch, stem)
        m = copy.deepcopy(bn)
        xin = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
        y = resnet._stem(m, relu, pool, xin)
        y.square().sum().backward()
        out[stem] = [y.detach(), xin.grad, m.weight.grad, m.bias.grad, m.running_mean, m.running_var]
    assert calls["batchnorm2d_act_maxpool_fwd_nhwc"] == 0 and calls["batchnorm2d_act_fwd_nhwc"] == 2
    for a, b in zip(out["hip"], out["torch"]):
        assert a.shape == b.shape and np.array_equal(raw(a), raw(b))
    all_hip(monkeypatch, "hip")
    m = copy.deepcopy(bn)
    xin = x[..., :32768].contiguous(memory_format=CL)
    y = resnet._stem(m, relu, pool, xin)
    assert calls["batchnorm2d_act_maxpool_fwd_nhwc"] == 1 and calls["batchnorm2d_act_fwd_nhwc"] == 2
    y2 = pool(ops.batchnorm2d_act_fwd_nhwc(xin, bn.weight, bn.bias, None, None, bn.eps, bn.momentum, 0.0)[0])
    assert same_bits(y, y2)


# ------------------------------------------------------------------------------------------------ 9. graph replay
def test_eager_calls_and_graph_replays_give_the_same_bits():
    shape = K.GRAPH_SHAPE
    c = K.make_case(shape, 1)
    x, dp, gamma, beta = inputs(c, shape)
    rm, rv = dev(c["running_mean"]), dev(c["running_var"])
    first = [bits(t).copy() for t in unit_step(x, dp, gamma, beta, rm, rv, 0.0)]
    second = [bits(t).copy() for t in unit_step(x, dp, gamma, beta, rm, rv, 0.0)]          # (also the warm-up of the capture)
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    want_rm, want_rv = bits(rm).copy(), bits(rv).copy()                                   # after two calls
    srm, srv = dev(c["running_mean"]), dev(c["running_var"])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = unit_step(x, dp, gamma, beta, srm, srv, 0.0)
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
    shape = (3, 11, 5, 6)                    # a shape no other test of this unit uses: no workspace yet
    x = torch.randn(*shape, device="cuda").contiguous(memory_format=CL); w = torch.ones(11, device="cuda"); b = torch.zeros(11, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(ClicaError, match="before capturing"):
        with torch.cuda.graph(graph):
            ops.batchnorm2d_act_maxpool_fwd_nhwc(x, w, b)
    assert not torch.cuda.is_current_stream_capturing()
    p, _, _ = ops.batchnorm2d_act_maxpool_fwd_nhwc(x, w, b)                 # the process goes on eagerly
    assert bool(torch.isfinite(p).all())
