"""BatchNorm2d fused with the shortcut add and the ReLU, and the global average pool, on dense channels-last activations (the HIP kernels
of csrc/bn2d_nhwc.hip): the C ABI against the fp64 oracle (tests/bn2d_oracle.py; a case's rows [N H W, C] are the NHWC tensor), a
BasicBlock and the whole ResNet-18 stand-in in channels-last against fp64 CPU copies, the proof that the NHWC path is taken under
NHWC_MODE "hip" and not by default, and bit reproducibility eager / graph replay."""
import copy
import types

import numpy as np
import pytest
import torch

import bn2d_nhwc_cases as K
import bn2d_oracle as B
from bn_family_util import bits, deterministic_convolutions, dev, host, raw, refuse  # noqa: F401 (the autouse fixture)
from conftest import PARITY

pytestmark = pytest.mark.gpu
CL = torch.channels_last


def nhwc(rows, shape):
    """Rows [N H W, C] as the device tensor [N, C, H, W] whose memory they are."""
    if rows is None:
        return None
    N, C, H, W = shape
    t = dev(rows).reshape(N, H, W, C).permute(0, 3, 1, 2)
    assert t.is_contiguous(memory_format=CL)
    return t


def maps(c, shape):
    return nhwc(c["x"], shape), nhwc(c["r"], shape), nhwc(c["dy"], shape)


def dense_cl(t):
    return t.is_contiguous(memory_format=CL) and t.permute(0, 2, 3, 1).is_contiguous()


# ------------------------------------------------------------------------------------------------ 1. ABI sweep against the oracle
@pytest.mark.parametrize("cls", range(len(B.CLASSES)))
@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_abi_against_the_oracle(shape, cls):
    from cl_ica_amd import ops
    N, C, H, W = shape
    for residual in (False, True):
        for slope in B.SLOPES:
            c, fw, bw = K.reference(N, C, H, W, cls, residual, slope)
            x, r, dy = maps(c, shape)
            gamma, beta = dev(c["gamma"]), dev(c["beta"])
            rm, rv = dev(c["running_mean"]), dev(c["running_var"])
            y, save_mean, save_invstd = ops.batchnorm2d_act_fwd_nhwc(x, gamma, beta, rm, rv, B.EPS, B.MOMENTUM, slope, residual=r)
            dx, dr, dgamma, dbeta = ops.batchnorm2d_act_bwd_nhwc(x, y, dy, gamma, save_mean, save_invstd, slope, need_dr=residual)
            assert (dr is not None) == residual
            assert dense_cl(y) and dense_cl(dx) and (dr is None or dense_cl(dr))
            case = f"{N}x{C}x{H}x{W} cls{cls} slope{slope} res{int(residual)}"
            fam = "bn2d_nhwc_abi"
            PARITY.check(fam, case, "y", K.rows_of(y), fw["y"])
            PARITY.check(fam, case, "save_mean", host(save_mean), fw["mean"])
            PARITY.check(fam, case, "save_invstd", host(save_invstd), fw["invstd"])
            PARITY.check(fam, case, "running_mean", host(rm), fw["running_mean"])
            PARITY.check(fam, case, "running_var", host(rv), fw["running_var"])
            cols = B.left_out(fw["z"], slope)
            assert cols.mean() <= B.MAX_LEFT_OUT
            if N * H * W > 2:                      # dx at M = 2 is ill-conditioned
                PARITY.check(fam, case, "dx", K.rows_of(dx)[:, ~cols], bw["dx"][:, ~cols])
            if residual:
                PARITY.check(fam, case, "dr", K.rows_of(dr)[:, ~cols], bw["dr"][:, ~cols])
            PARITY.check(fam, case, "dgamma", host(dgamma)[~cols], bw["dgamma"][~cols])
            PARITY.check(fam, case, "dbeta", host(dbeta)[~cols], bw["dbeta"][~cols])
            # without running statistics the forward is the same and nothing else is written
            rm_bits, rv_bits = bits(rm).copy(), bits(rv).copy()
            y2, m2, i2 = ops.batchnorm2d_act_fwd_nhwc(x, gamma, beta, None, None, B.EPS, B.MOMENTUM, slope, residual=r)
            assert np.array_equal(bits(y2), bits(y)) and np.array_equal(bits(m2), bits(save_mean)) and np.array_equal(bits(i2), bits(save_invstd))
            assert np.array_equal(bits(rm), rm_bits) and np.array_equal(bits(rv), rv_bits)


@pytest.mark.parametrize("cls", range(len(B.CLASSES)))
def test_the_cap_on_the_splits_against_the_oracle(cls):
    """M = 16500 rows of 256 channels: 64 splits (the cap with one merging thread per channel), the last one short, 516 tiles.  Slope 1
    (no kink: no channel left out, see tests/bn2d_nhwc_cases.py).
    The two means are measured against the largest standard deviation of a channel where that exceeds them: in class 0 the true mean is
    0, the sample mean of M rows is of the order std / sqrt(M), and an fp32 mean carries an error of a few ulp of the VALUES it averages
    whatever the order of the sum, so its error relative to itself grows as sqrt(M) eps -- 128 x 6e-8 here, at the 1e-5 bar by the
    construction of the case, not by the kernel.  (Class 1, offset 3 std, has means above that floor: it changes nothing there.)"""
    from cl_ica_amd import ops
    shape = K.CAPPED_SHAPE
    slope = 1.0
    c = B.make_case(*shape, cls, True, attempt=0)
    fw = B.forward(c, slope)
    bw = B.backward(fw, c, slope)
    x, r, dy = maps(c, shape)
    gamma, beta = dev(c["gamma"]), dev(c["beta"])
    rm, rv = dev(c["running_mean"]), dev(c["running_var"])
    y, a, b = ops.batchnorm2d_act_fwd_nhwc(x, gamma, beta, rm, rv, B.EPS, B.MOMENTUM, slope, residual=r)
    dx, dr, dgamma, dbeta = ops.batchnorm2d_act_bwd_nhwc(x, y, dy, gamma, a, b, slope, need_dr=True)
    case = "x".join(map(str, shape)) + f" cls{cls} slope1 res1"
    for what, got, ref in (("y", K.rows_of(y), fw["y"]), ("save_mean", host(a), fw["mean"]), ("save_invstd", host(b), fw["invstd"]),
                           ("running_mean", host(rm), fw["running_mean"]), ("running_var", host(rv), fw["running_var"]),
                           ("dx", K.rows_of(dx), bw["dx"]), ("dr", K.rows_of(dr), bw["dr"]), ("dgamma", host(dgamma), bw["dgamma"]),
                           ("dbeta", host(dbeta), bw["dbeta"])):
        floor = float(np.sqrt(c["x"].astype(np.float64).var(0).max())) if what in ("save_mean", "running_mean") else 0.0
        PARITY.check("bn2d_nhwc_abi", case, what, got, ref, floor=floor)


@pytest.mark.parametrize("shape", K.EVAL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_eval_abi_against_the_oracle(shape):
    from cl_ica_amd import ops
    N, C, H, W = shape
    for cls in range(len(B.CLASSES)):
        for residual in (False, True):
            c = K.reference(N, C, H, W, cls, residual, 0.0)[0]
            rm = (c["x"].mean(0) + c["running_mean"]).astype(np.float32)          # statistics of the size of the data's own
            rv = (c["x"].var(0) * c["running_var"]).astype(np.float32)
            x, r, _ = maps(c, shape)
            for slope in B.SLOPES:
                y = ops.batchnorm2d_act_eval_nhwc(x, dev(c["gamma"]), dev(c["beta"]), dev(rm), dev(rv), B.EPS, slope, residual=r)
                assert dense_cl(y)
                PARITY.check("bn2d_nhwc_abi", f"eval {N}x{C}x{H}x{W} cls{cls} slope{slope} res{int(residual)}", "y", K.rows_of(y),
                             B.evaluate(c, rm, rv, slope))


def off_by_4_bytes(t):
    """A dense channels-last copy of t whose storage starts 4 bytes off a 16-byte boundary."""
    N, C, H, W = t.shape
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    u = buf[1:].view(N, H, W, C).permute(0, 3, 1, 2)
    u.copy_(t)
    assert u.is_contiguous(memory_format=CL) and u.data_ptr() % 16 == 4
    return u


@pytest.mark.parametrize("shape", K.UNALIGNED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_unaligned_input_gives_the_same_bits(shape):
    """C % 4 == 0: an unaligned tensor makes the kernels read and write the same four channels per lane with scalar accesses, in the same
    reduction order, so every result has the aligned call's bits."""
    from cl_ica_amd import ops
    N, C, H, W = shape
    slope = 0.0
    c, fw, bw = K.reference(N, C, H, W, 1, True, slope)
    x, r, dy = maps(c, shape)
    assert x.data_ptr() % 16 == 0
    gamma, beta = dev(c["gamma"]), dev(c["beta"])

    def run(x, r, dy):
        y, a, b = ops.batchnorm2d_act_fwd_nhwc(x, gamma, beta, None, None, B.EPS, B.MOMENTUM, slope, residual=r)
        return (y, a, b) + tuple(ops.batchnorm2d_act_bwd_nhwc(x, y, dy, gamma, a, b, slope, need_dr=True))
    want = run(x, r, dy)
    PARITY.check("bn2d_nhwc_abi", f"unaligned {shape}", "y", K.rows_of(want[0]), fw["y"])
    for variant in ((off_by_4_bytes(x), r, dy), (off_by_4_bytes(x), off_by_4_bytes(r), off_by_4_bytes(dy))):
        for a, b in zip(want, run(*variant)):
            assert np.array_equal(bits(a), bits(b))
    rm = dev(c["running_mean"]); rv = dev(c["running_var"])
    e0 = ops.batchnorm2d_act_eval_nhwc(x, gamma, beta, rm, rv, B.EPS, slope, residual=r)
    e1 = ops.batchnorm2d_act_eval_nhwc(off_by_4_bytes(x), gamma, beta, rm, rv, B.EPS, slope, residual=r)
    assert np.array_equal(bits(e0), bits(e1))


def test_bad_arguments_are_refused():
    from cl_ica_amd import ops
    x = torch.randn(4, 8, 2, 2, device="cuda").contiguous(memory_format=CL); w = torch.ones(8, device="cuda"); b = torch.zeros(8, device="cuda")
    with pytest.raises(RuntimeError):
        ops.batchnorm2d_act_fwd_nhwc(x[:1, :, :1, :1].contiguous(memory_format=CL), w, b)          # one value per channel
    with pytest.raises(RuntimeError):
        ops.batchnorm2d_act_fwd_nhwc(x, w, b, slope=-0.1)
    with pytest.raises(ValueError):
        ops.batchnorm2d_act_fwd_nhwc(x.contiguous(), w, b)
    with pytest.raises(ValueError):
        ops.batchnorm2d_act_fwd_nhwc(x, w[:3], b)
    with pytest.raises(ValueError):
        ops.batchnorm2d_act_fwd_nhwc(x, w, b, residual=x.contiguous())
    with pytest.raises(ValueError):
        ops.batchnorm2d_act_fwd(x, w, b)                                        # the NCHW function keeps its contract
    assert ops.bn2d_nhwc_workspace(16, 8, x.device) is ops.bn2d_nhwc_workspace(16, 8, x.device)      # never a new buffer


# ------------------------------------------------------------------------------------------------ 2. one block against fp64
def block_run(blk, x, c):
    """(output, input gradient, parameter gradients by name, buffers by name) of one training pass with objective sum(y c)."""
    blk.zero_grad(set_to_none=True)
    xin = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
    y = blk(xin)
    (y * c).sum().backward()
    return (y.detach(), xin.grad, {k: p.grad for k, p in blk.named_parameters()}, {k: b.detach().clone() for k, b in blk.named_buffers()})


@pytest.mark.parametrize("case", B.BLOCK_CASES, ids=lambda s: "-".join(map(str, s)))
def test_block_against_fp64(monkeypatch, case):
    """A channels-last block under NHWC_MODE "hip" against an fp64 CPU copy: each quantity within 4 x the distance of the NHWC_MODE "torch"
    fp32 GPU run (torch's own channels-last modules) from that fp64 result, floor 1e-5.  Outputs and input gradients stay channels-last."""
    from cl_ica_amd import resnet
    monkeypatch.setattr(resnet, "NORM_MODE", "hip")
    blk, x, c = B.make_block(*case)
    y64, dx64, g64, b64 = block_run(copy.deepcopy(blk).double(), x.double(), c.double())
    res = {}
    for mode in ("torch", "hip"):
        monkeypatch.setattr(resnet, "NHWC_MODE", mode)
        res[mode] = block_run(copy.deepcopy(blk).cuda().to(memory_format=CL), x.cuda().contiguous(memory_format=CL),
                              c.cuda().contiguous(memory_format=CL))
    assert dense_cl(res["hip"][0]) and dense_cl(res["hip"][1])
    name = "block " + "-".join(map(str, case))
    items = [("y", 0, None), ("dx", 1, None)] + [(f"grad {k}", 2, k) for k in g64]
    for what, idx, key in items:
        pick = (lambda t: t[idx]) if key is None else (lambda t: t[idx][key])
        truth = pick((y64, dx64, g64)).numpy()
        own = B.O.norm_err(host(pick(res["torch"])), truth)
        bound = max(4.0 * own, 1e-5)
        err = PARITY.check("bn2d_nhwc_block", name, what, host(pick(res["hip"])), truth, tol=bound,
                           note="4 x torch fp32's own error against fp64, floor 1e-5")
        print(f"{name} {what}: HIP {err:.3e}, torch fp32 {own:.3e}, bound {bound:.3e}")
    for k, v in res["hip"][3].items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(res["torch"][3][k]) == int(b64[k]) == 1
        else:
            assert B.O.norm_err(host(v), host(res["torch"][3][k])) < 1e-6, k
            PARITY.check("bn2d_nhwc_block", name, k, host(v), b64[k].numpy())


# ------------------------------------------------------------------------------------------------ 3. the whole backbone
def backbone():
    from cl_ica_amd import resnet
    torch.manual_seed(11)
    f = resnet.resnet18(num_classes=30)
    x = torch.randn(3, 3, 64, 64, generator=torch.Generator().manual_seed(12))
    return f.train(), x


def cl_cuda(f, x):
    return f.cuda().to(memory_format=CL), x.cuda().contiguous(memory_format=CL)


def test_backbone_forward_against_fp64_and_reproducible(monkeypatch):
    from cl_ica_amd import resnet
    monkeypatch.setattr(resnet, "NORM_MODE", "hip")
    f, x = backbone()
    with torch.no_grad():
        y64 = copy.deepcopy(f).double()(x.double()).numpy()
    out = {}
    for mode in ("torch", "hip", "hip again"):
        monkeypatch.setattr(resnet, "NHWC_MODE", mode.split()[0])
        g, xc = cl_cuda(copy.deepcopy(f), x)
        y = g(xc)
        y.square().sum().backward()
        out[mode] = [y.detach()] + [p.grad for p in g.parameters()] + [b.float() for b in g.buffers()]
    own = B.O.norm_err(host(out["torch"][0]), y64)
    bound = max(4.0 * own, 1e-5)
    err = PARITY.check("bn2d_nhwc_backbone", "resnet18 3x3x64x64 channels-last", "y", host(out["hip"][0]), y64, tol=bound,
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
    monkeypatch.setattr(resnet, "NHWC_MODE", "hip")
    a = types.SimpleNamespace(position_only=True, rotation_and_color_only=False, rotation_only=False, color_only=False,
                              non_periodic_rotation_and_color=False, box_constraint=None, sphere_constraint=None,
                              unsupervised_loss="l2", identity_solution=False, encoder="rn18")
    torch.manual_seed(0)
    f = T.setup_f(a, 3, 0).to("cuda").to(memory_format=CL).train()
    assert isinstance(f[0], resnet.ResNet18) and f[0].fc.out_features == 30
    loss = T.make_unsupervised_loss(a, 3)
    g = torch.Generator().manual_seed(1)
    x1 = torch.randn(3, 3, 64, 64, generator=g)
    x2 = (x1 + 0.1 * torch.randn(3, 3, 64, 64, generator=g)).cuda().contiguous(memory_format=CL)
    x1 = x1.cuda().contiguous(memory_format=CL)
    lr = 1e-4
    opt = Adam(f.parameters(), lr=lr)
    before = {k: v.detach().clone() for k, v in f.named_parameters()}
    calls = spy_on(monkeypatch)
    tot, per, lst = T.train_step(((None, None), (x1, x2)), loss, opt, f, sync=True)
    assert np.isfinite(tot)
    moved = [float((prm.detach() - before[k]).abs().max()) for k, prm in f.named_parameters()]
    assert all(np.isfinite(m) for m in moved) and max(moved) <= 1.001 * lr and max(moved) > 0.5 * lr
    assert int(f[0].bn1.num_batches_tracked) == 2                     # two views, one forward each
    assert calls["batchnorm2d_act_fwd_nhwc"] == 40 and calls["batchnorm2d_act_bwd_nhwc"] == 40 and calls["batchnorm2d_act_fwd"] == 0


# ------------------------------------------------------------------------------------------------ 4. the NHWC path is really taken
NHWC_OPS = ("batchnorm2d_act_fwd_nhwc", "batchnorm2d_act_eval_nhwc", "batchnorm2d_act_bwd_nhwc", "avgpool2d_global_fwd_nhwc",
            "avgpool2d_global_bwd_nhwc")
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


def test_the_nhwc_path_is_taken(monkeypatch):
    from cl_ica_amd import resnet
    f, x = backbone()
    f, x = cl_cuda(f, x)
    monkeypatch.setattr(resnet, "NORM_MODE", "hip")
    monkeypatch.setattr(resnet, "POOL_MODE", "hip")
    monkeypatch.setattr(resnet, "NHWC_MODE", "hip")
    calls = spy_on(monkeypatch)
    monkeypatch.setattr(torch.nn.functional, "batch_norm", refuse)
    monkeypatch.setattr(torch.nn.functional, "relu", refuse)
    f(x).sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in f.parameters())
    assert int(f.bn1.num_batches_tracked) == 1 and int(f.layer2[0].downsample[1].num_batches_tracked) == 1
    assert calls["batchnorm2d_act_fwd_nhwc"] == 20 and calls["batchnorm2d_act_bwd_nhwc"] == 20
    assert calls["avgpool2d_global_fwd_nhwc"] == 1 and calls["avgpool2d_global_bwd_nhwc"] == 1
    assert calls["batchnorm2d_act_eval_nhwc"] == 0 and all(calls[k] == 0 for k in NCHW_OPS)
    f.eval()
    with torch.no_grad():
        assert bool(torch.isfinite(f(x)).all())
    assert int(f.bn1.num_batches_tracked) == 1
    assert calls["batchnorm2d_act_eval_nhwc"] == 20 and calls["avgpool2d_global_fwd_nhwc"] == 2
    assert calls["batchnorm2d_act_fwd_nhwc"] == 20 and all(calls[k] == 0 for k in NCHW_OPS)
    # POOL_MODE "torch": the units alone
    monkeypatch.setattr(resnet, "POOL_MODE", "torch")
    with torch.no_grad():
        f(x)
    assert calls["batchnorm2d_act_eval_nhwc"] == 40 and calls["avgpool2d_global_fwd_nhwc"] == 2
    # the default: channels-last inputs run torch's modules
    monkeypatch.setattr(resnet, "NHWC_MODE", "torch")
    with pytest.raises(AssertionError, match="torch's own normalisation"):
        with torch.no_grad():
            f(x)


def test_by_default_channels_last_runs_torch_modules(monkeypatch):
    """NHWC_MODE's default: no NHWC kernel runs on a channels-last backbone, and a channels-last block has the bits of NORM_MODE "torch" in
    outputs, gradients and buffers."""
    from cl_ica_amd import resnet
    assert resnet.NHWC_MODE == "torch"
    monkeypatch.setattr(resnet, "NORM_MODE", "hip")
    calls = spy_on(monkeypatch)
    f, x = backbone()
    f, x = cl_cuda(f, x)
    f(x).sum().backward()
    f.eval()
    with torch.no_grad():
        f(x)
    assert all(calls[k] == 0 for k in NHWC_OPS)

    torch.manual_seed(3)
    base = resnet.BasicBlock(16, 32, 2).cuda().to(memory_format=CL)
    xb = torch.randn(4, 16, 8, 8, generator=torch.Generator().manual_seed(2)).cuda().contiguous(memory_format=CL)
    out = {}
    for nm in ("hip", "torch"):
        monkeypatch.setattr(resnet, "NORM_MODE", nm)
        blk = copy.deepcopy(base).train()
        xin = xb.clone(memory_format=torch.preserve_format).requires_grad_(True)
        y = blk(xin)
        y.square().sum().backward()
        out[nm] = [y.detach(), xin.grad] + [p.grad for p in blk.parameters()] + [b.float() for b in blk.buffers()]
    assert all(calls[k] == 0 for k in NHWC_OPS)
    for a, b in zip(out["hip"], out["torch"]):
        assert a.shape == b.shape and np.array_equal(raw(a), raw(b))


def test_a_residual_in_the_other_layout_runs_torch_path(monkeypatch):
    """x channels-last, residual NCHW-contiguous: no hidden copy -- the unit is torch's modules, bit for bit, forward and backward."""
    from cl_ica_amd import resnet
    monkeypatch.setattr(resnet, "NORM_MODE", "hip")
    monkeypatch.setattr(resnet, "NHWC_MODE", "hip")
    calls = spy_on(monkeypatch)
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(4, 16, 6, 6, generator=gen).cuda().contiguous(memory_format=CL)
    r = torch.randn(4, 16, 6, 6, generator=gen).cuda()
    c = torch.randn(4, 16, 6, 6, generator=gen).cuda()
    torch.manual_seed(5)
    bn = torch.nn.BatchNorm2d(16).cuda().train()
    with torch.no_grad():
        bn.weight.normal_(1.0, 0.3); bn.bias.normal_(0.0, 0.3)
    relu = torch.nn.ReLU()
    out = []
    for which in ("unit", "torch"):
        m = copy.deepcopy(bn)
        xin, rin = x.clone(memory_format=torch.preserve_format).requires_grad_(True), r.clone().requires_grad_(True)
        y = resnet._unit(m, relu, xin, rin) if which == "unit" else relu(m(xin) + rin)
        (y * c).sum().backward()
        out.append([y.detach(), xin.grad, rin.grad, m.weight.grad, m.bias.grad, m.running_mean, m.running_var])
    assert all(v == 0 for v in calls.values())
    for a, b in zip(*out):
        assert a.stride() == b.stride() and np.array_equal(raw(a), raw(b))
    # and the same pair in one layout does take the kernels
    y = resnet._unit(copy.deepcopy(bn), relu, x, r.contiguous(memory_format=CL))
    assert calls["batchnorm2d_act_fwd_nhwc"] == 1 and dense_cl(y)


# ------------------------------------------------------------------------------------------------ 5. graph replay
def unit_step(x, r, gamma, beta, dy, rm, rv, slope=0.0):
    from cl_ica_amd import ops
    y, a, b = ops.batchnorm2d_act_fwd_nhwc(x, gamma, beta, rm, rv, B.EPS, B.MOMENTUM, slope, residual=r)
    return (y, a, b) + tuple(ops.batchnorm2d_act_bwd_nhwc(x, y, dy, gamma, a, b, slope, need_dr=True))


@pytest.mark.parametrize("shape", [(16, 64, 16, 16), (8, 512, 2, 2)], ids=lambda s: "x".join(map(str, s)))
def test_eager_calls_and_graph_replays_give_the_same_bits(shape):
    N, C, H, W = shape
    c = K.reference(N, C, H, W, 1, True, 0.0)[0]
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
    x = torch.randn(*shape, device="cuda").contiguous(memory_format=CL); w = torch.ones(11, device="cuda"); b = torch.zeros(11, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(ClicaError, match="before capturing"):
        with torch.cuda.graph(graph):
            ops.batchnorm2d_act_fwd_nhwc(x, w, b)
    assert not torch.cuda.is_current_stream_capturing()
    y, _, _ = ops.batchnorm2d_act_fwd_nhwc(x, w, b)                    # the process goes on eagerly
    assert bool(torch.isfinite(y).all())


# ------------------------------------------------------------------------------------------------ 6. global average pool
@pytest.mark.parametrize("shape", [(3, 7, 2, 2), (2, 65, 3, 5), (4, 512, 2, 2)], ids=lambda s: "x".join(map(str, s)))
def test_average_pool_against_fp64(shape):
    from cl_ica_amd import ops
    N, C, H, W = shape
    gen = torch.Generator().manual_seed(N * 1000 + C)
    x = (torch.randn(*shape, generator=gen) + 0.5).contiguous(memory_format=CL)
    dy = torch.randn(N, C, generator=gen)
    y = ops.avgpool2d_global_fwd_nhwc(x.cuda())
    assert y.shape == (N, C) and y.is_contiguous()
    case = "x".join(map(str, shape))
    PARITY.check("avgpool_nhwc", case, "y", host(y), x.double().mean((2, 3)).numpy())
    dx = ops.avgpool2d_global_bwd_nhwc(dy.cuda(), H, W)
    assert dx.shape == shape and dense_cl(dx)
    PARITY.check("avgpool_nhwc", case, "dx", host(dx), (dy.double() / (H * W))[:, :, None, None].expand(N, C, H, W).numpy())
    # through autograd, as resnet.py calls it
    from cl_ica_amd import resnet
    xin = x.cuda().requires_grad_(True)
    out = resnet._GlobalAvgPoolFn.apply(xin, "nhwc")
    (out * dy.cuda()).sum().backward()
    assert np.array_equal(bits(out), bits(y)) and np.array_equal(raw(xin.grad), raw(dx)) and dense_cl(xin.grad)
