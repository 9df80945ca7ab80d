"""The channels-last BatchNorm2d unit, the fused stem unit and the global average pool on bf16 ACTIVATIONS (the ``_bf16`` entry points of
csrc/bn2d_nhwc.hip) against the fp32 entry points on the upcast operands, which tests/test_gpu_bn2d_nhwc.py and tests/test_gpu_stem_nhwc.py
hold to fp64.  The bf16 instances keep the fp32 geometry and widen exactly, so the comparison needs no tolerance:

  * a bf16 output equals ``fp32_kernel(upcast inputs).to(torch.bfloat16)``, compared as int16;
  * an fp32 output (save_mean, save_invstd, running statistics, dgamma, dbeta, the average pool's Y) has the fp32 kernel's bits.

Then the same on the tensors a real ResNet-18 produces under ``torch.autocast(bfloat16)`` with resnet.BF16_MODE "hip", the proof that this
path is taken there and nowhere by default, unaligned pointers, graph replay and the refusals."""
import copy
import zlib

import pytest
import torch

import bn2d_nhwc_cases as K
import stem_nhwc_cases as P
from bn_family_util import deterministic_convolutions  # noqa: F401 (the autouse fixture)

pytestmark = pytest.mark.gpu
CL, BF, F32 = torch.channels_last, torch.bfloat16, torch.float32
EPS, MOMENTUM = 1e-5, 0.1
SLOPES = (0.0, 0.01, 1.0)
# input classes of x, each rounded to bf16: standard normal; mean 100 / std 1 (bf16 spacing 0.5: most of a channel's values collide);
# one constant channel (variance 0); the first draw with non-trivial running statistics; and, for the stem, values from {-1, 0, 1, 2}
# (most windows hold exact ties)
CLASSES = ("normal", "offset100", "constant-channel", "running-stats")
TIES = "ties"
AVGPOOL_SHAPES = [(3, 7, 2, 2), (2, 65, 3, 5), (4, 512, 2, 2)]          # those of test_gpu_bn2d_nhwc.test_average_pool_against_fp64
ids = lambda s: "x".join(map(str, s))  # noqa: E731


# ------------------------------------------------------------------------------------------------ inputs and comparisons
def gen_for(tag, shape, cls):
    return torch.Generator().manual_seed(zlib.crc32(f"{tag}:{ids(shape)}".encode()) + 7919 * (CLASSES + (TIES,)).index(cls))


def cl(t):
    """[N, C, H, W] on the device, dense channels-last."""
    return t.cuda().contiguous(memory_format=CL)


def draw_x(shape, cls, g):
    N, C, H, W = shape
    if cls == TIES:
        x = torch.randint(-1, 3, shape, generator=g).float()
    else:
        x = torch.randn(shape, generator=g)
        if cls == "offset100":
            x = x + 100.0
        if cls == "constant-channel":
            x[:, C // 2] = 0.75
    return cl(x).to(BF)


def params(C, cls, g):
    gamma = 1.0 + 0.3 * torch.randn(C, generator=g)
    beta = 0.3 * torch.randn(C, generator=g)
    if cls == "running-stats":
        rm, rv = torch.randn(C, generator=g), 0.5 + 1.5 * torch.rand(C, generator=g)
    else:
        rm, rv = torch.zeros(C), torch.ones(C)
    return gamma.cuda(), beta.cuda(), rm.cuda(), rv.cuda()


class Flags:
    """Bit comparisons collected on the device, read back once."""

    def __init__(self):
        self.names, self.bad = [], []

    def same(self, name, got, want):
        """got and want: tensors of one dtype, shape and strides; equal as integers (a NaN equals itself)."""
        assert got.dtype == want.dtype and got.shape == want.shape and got.stride() == want.stride(), (name, got.dtype, want.dtype)
        view = torch.int16 if got.dtype == BF else torch.int32
        self.names.append(name)
        self.bad.append((got.view(view) != want.view(view)).any())

    def rounded(self, name, got_bf16, want_f32):
        assert got_bf16.dtype == BF and want_f32.dtype == F32, name
        assert got_bf16.is_contiguous(memory_format=CL) and got_bf16.permute(0, 2, 3, 1).is_contiguous(), name
        self.same(name, got_bf16, want_f32.to(BF))

    def check(self):
        assert self.names
        bad = torch.stack(self.bad).cpu().tolist()
        wrong = [n for n, b in zip(self.names, bad) if b]
        assert not wrong, f"{len(wrong)} of {len(bad)} differ: {wrong[:12]}"


def unit_case(fl, shape, cls, residual, slope, need_dr_values=(False, True)):
    """Training forward and backward of the unit, bf16 against fp32 on the upcasts."""
    from cl_ica_amd import ops
    N, C, H, W = shape
    g = gen_for("unit", shape, cls)
    x = draw_x(shape, cls, g)
    r = cl(torch.randn(shape, generator=g)).to(BF) if residual else None
    dy = cl(torch.randn(shape, generator=g)).to(BF)
    gamma, beta, rm0, rv0 = params(C, cls, g)
    rm, rv, rm32, rv32 = rm0.clone(), rv0.clone(), rm0.clone(), rv0.clone()
    tag = f"{ids(shape)} {cls} res{int(residual)} slope{slope}"
    y, mean, invstd = ops.batchnorm2d_act_fwd_nhwc(x, gamma, beta, rm, rv, EPS, MOMENTUM, slope, residual=r)
    y32, mean32, invstd32 = ops.batchnorm2d_act_fwd_nhwc(x.float(), gamma, beta, rm32, rv32, EPS, MOMENTUM, slope,
                                                         residual=None if r is None else r.float())
    fl.rounded(tag + " y", y, y32)
    for name, a, b in (("save_mean", mean, mean32), ("save_invstd", invstd, invstd32), ("running_mean", rm, rm32), ("running_var", rv, rv32)):
        fl.same(f"{tag} {name}", a, b)
    for need_dr in need_dr_values:
        dx, dr, dg, db = ops.batchnorm2d_act_bwd_nhwc(x, y, dy, gamma, mean, invstd, slope, need_dr=need_dr)
        dx32, dr32, dg32, db32 = ops.batchnorm2d_act_bwd_nhwc(x.float(), y.float(), dy.float(), gamma, mean, invstd, slope, need_dr=need_dr)
        assert (dr is None) == (not need_dr)
        fl.rounded(f"{tag} dr{int(need_dr)} dx", dx, dx32)
        if need_dr:
            fl.rounded(f"{tag} dr", dr, dr32)
        fl.same(f"{tag} dr{int(need_dr)} dgamma", dg, dg32)
        fl.same(f"{tag} dr{int(need_dr)} dbeta", db, db32)


# ------------------------------------------------------------------------------------------------ 1. the unit
@pytest.mark.parametrize("shape", K.SHAPES, ids=ids)
def test_unit_training_forward_and_backward(shape):
    fl = Flags()
    for cls in CLASSES:
        for residual in (False, True):
            for slope in SLOPES:
                unit_case(fl, shape, cls, residual, slope)
    fl.check()


def test_unit_at_the_cap_on_the_splits():
    fl = Flags()
    for cls in CLASSES:
        for residual in (False, True):
            for slope in SLOPES:
                unit_case(fl, K.CAPPED_SHAPE, cls, residual, slope, need_dr_values=(residual,))
    fl.check()


@pytest.mark.parametrize("shape", K.EVAL_SHAPES, ids=ids)
def test_unit_inference(shape):
    from cl_ica_amd import ops
    fl = Flags()
    N, C, H, W = shape
    for cls in CLASSES:
        g = gen_for("unit-eval", shape, cls)
        x = draw_x(shape, cls, g)
        r = cl(torch.randn(shape, generator=g)).to(BF)
        gamma, beta, _, _ = params(C, cls, g)
        xf = x.float()
        rm, rv = xf.mean((0, 2, 3)) + 0.1, xf.var((0, 2, 3), unbiased=False) * 1.3 + 0.01          # of the size of the data's own
        for rr in (None, r):
            for slope in SLOPES:
                y = ops.batchnorm2d_act_eval_nhwc(x, gamma, beta, rm, rv, EPS, slope, residual=rr)
                y32 = ops.batchnorm2d_act_eval_nhwc(xf, gamma, beta, rm, rv, EPS, slope, residual=None if rr is None else rr.float())
                fl.rounded(f"eval {ids(shape)} {cls} res{int(rr is not None)} slope{slope}", y, y32)
    fl.check()


# ------------------------------------------------------------------------------------------------ 2. the stem
def stem_case(fl, shape, cls, slope):
    from cl_ica_amd import ops
    N, C, H, W = shape
    g = gen_for("stem", shape, cls)
    x = draw_x(shape, cls, g)
    gamma, beta, rm0, rv0 = params(C, cls if cls != TIES else "normal", g)
    Ho, Wo = ops.maxpool_out_hw(H, W)
    dp = cl(torch.randn((N, C, Ho, Wo), generator=g)).to(BF)
    rm, rv, rm32, rv32 = rm0.clone(), rv0.clone(), rm0.clone(), rv0.clone()
    tag = f"stem {ids(shape)} {cls} slope{slope}"
    p, mean, invstd = ops.batchnorm2d_act_maxpool_fwd_nhwc(x, gamma, beta, rm, rv, EPS, MOMENTUM, slope)
    p32, mean32, invstd32 = ops.batchnorm2d_act_maxpool_fwd_nhwc(x.float(), gamma, beta, rm32, rv32, EPS, MOMENTUM, slope)
    fl.rounded(tag + " p", p, p32)
    for name, a, b in (("save_mean", mean, mean32), ("save_invstd", invstd, invstd32), ("running_mean", rm, rm32), ("running_var", rv, rv32)):
        fl.same(f"{tag} {name}", a, b)
    dx, dg, db = ops.batchnorm2d_act_maxpool_bwd_nhwc(x, dp, gamma, beta, mean, invstd, slope)
    dx32, dg32, db32 = ops.batchnorm2d_act_maxpool_bwd_nhwc(x.float(), dp.float(), gamma, beta, mean, invstd, slope)
    fl.rounded(tag + " dx", dx, dx32)
    fl.same(tag + " dgamma", dg, dg32)
    fl.same(tag + " dbeta", db, db32)


STEM_SHAPES = P.SHAPES + [s for s in P.TIE_SHAPES + P.EVAL_SHAPES if s not in P.SHAPES]


@pytest.mark.parametrize("shape", STEM_SHAPES, ids=ids)
def test_stem_training_forward_and_backward(shape):
    """Every class and the tie class: the first maximum in scan order is the fp32 kernel's (taken among the fp32 activations, rounded
    afterwards), and the gradient lands where the fp32 kernel puts it."""
    fl = Flags()
    for cls in CLASSES + (TIES,):
        for slope in SLOPES:
            stem_case(fl, shape, cls, slope)
    fl.check()


@pytest.mark.parametrize("shape", STEM_SHAPES, ids=ids)
def test_stem_inference(shape):
    from cl_ica_amd import ops
    fl = Flags()
    N, C, H, W = shape
    for cls in CLASSES + (TIES,):
        g = gen_for("stem-eval", shape, cls)
        x = draw_x(shape, cls, g)
        gamma, beta, _, _ = params(C, "normal", g)
        xf = x.float()
        rm, rv = xf.mean((0, 2, 3)) + 0.1, xf.var((0, 2, 3), unbiased=False) * 1.3 + 0.01
        for slope in SLOPES:
            p = ops.batchnorm2d_act_maxpool_eval_nhwc(x, gamma, beta, rm, rv, EPS, slope)
            p32 = ops.batchnorm2d_act_maxpool_eval_nhwc(xf, gamma, beta, rm, rv, EPS, slope)
            fl.rounded(f"stem eval {ids(shape)} {cls} slope{slope}", p, p32)
    fl.check()


# ------------------------------------------------------------------------------------------------ 3. the average pool
@pytest.mark.parametrize("shape", AVGPOOL_SHAPES, ids=ids)
def test_average_pool(shape):
    from cl_ica_amd import ops, resnet
    fl = Flags()
    N, C, H, W = shape
    g = gen_for("avgpool", shape, "normal")
    x = cl(torch.randn(shape, generator=g) + 0.5).to(BF)
    dy = torch.randn(N, C, generator=g).cuda()
    y = ops.avgpool2d_global_fwd_nhwc(x)
    assert y.dtype == F32 and y.shape == (N, C) and y.is_contiguous()
    fl.same("y", y, ops.avgpool2d_global_fwd_nhwc(x.float()))
    dx = ops.avgpool2d_global_bwd_nhwc(dy, H, W, BF)
    fl.rounded("dx", dx, ops.avgpool2d_global_bwd_nhwc(dy, H, W))
    xin = x.clone(memory_format=torch.preserve_format).requires_grad_(True)          # through autograd, as resnet.py calls it
    out = resnet._GlobalAvgPoolFn.apply(xin, "nhwc")
    (out * dy).sum().backward()
    assert out.dtype == F32 and xin.grad.dtype == BF
    fl.same("autograd y", out.detach(), y)
    fl.same("autograd dx", xin.grad, dx)
    fl.check()


# ------------------------------------------------------------------------------------------------ 4. unaligned pointers
def offset_view(t, elems):
    """A dense channels-last copy of the bf16 tensor t that starts `elems` elements (2 bytes each) into a buffer."""
    N, C, H, W = t.shape
    buf = torch.empty(t.numel() + elems, dtype=t.dtype, device=t.device)
    u = buf[elems:].view(N, H, W, C).permute(0, 3, 1, 2)
    u.copy_(t)
    assert u.is_contiguous(memory_format=CL) and u.data_ptr() % 8 == (2 * elems) % 8 != 0
    return u


@pytest.mark.parametrize("elems", (1, 2))
@pytest.mark.parametrize("shape", K.UNALIGNED_SHAPES, ids=ids)
def test_unit_unaligned_pointers_give_the_same_bits(shape, elems):
    """C % 4 == 0: a pointer off the 8-byte boundary makes the kernels take the same four channels per lane with 2-byte accesses, in the
    same reduction order."""
    from cl_ica_amd import ops
    N, C, H, W = shape
    g = gen_for("unit-unaligned", shape, "normal")
    x, r, dy = (cl(torch.randn(shape, generator=g)).to(BF) for _ in range(3))
    gamma, beta, rm, rv = params(C, "running-stats", g)
    assert x.data_ptr() % 8 == 0

    def run(x, r, dy):
        y, a, b = ops.batchnorm2d_act_fwd_nhwc(x, gamma, beta, None, None, EPS, MOMENTUM, 0.0, residual=r)
        e = ops.batchnorm2d_act_eval_nhwc(x, gamma, beta, rm, rv, EPS, 0.0, residual=r)
        return (y, a, b, e) + tuple(ops.batchnorm2d_act_bwd_nhwc(x, y, dy, gamma, a, b, 0.0, need_dr=True))
    want = run(x, r, dy)
    fl = Flags()
    o = lambda t: offset_view(t, elems)  # noqa: E731
    for v, variant in enumerate(((o(x), r, dy), (o(x), o(r), o(dy)))):
        for k, (a, b) in enumerate(zip(want, run(*variant))):
            fl.same(f"variant {v} output {k}", b, a)
    fl.check()


@pytest.mark.parametrize("elems", (1, 2))
@pytest.mark.parametrize("shape", P.UNALIGNED_SHAPES, ids=ids)
def test_stem_unaligned_pointers_give_the_same_bits(shape, elems):
    from cl_ica_amd import ops
    N, C, H, W = shape
    g = gen_for("stem-unaligned", shape, TIES)
    x = draw_x(shape, TIES, g)
    gamma, beta, rm, rv = params(C, "running-stats", g)
    dp = cl(torch.randn((N, C) + ops.maxpool_out_hw(H, W), generator=g)).to(BF)

    def run(x, dp):
        p, a, b = ops.batchnorm2d_act_maxpool_fwd_nhwc(x, gamma, beta, None, None, EPS, MOMENTUM, 0.0)
        e = ops.batchnorm2d_act_maxpool_eval_nhwc(x, gamma, beta, rm, rv, EPS, 0.0)
        return (p, a, b, e) + tuple(ops.batchnorm2d_act_maxpool_bwd_nhwc(x, dp, gamma, beta, a, b, 0.0))
    want = run(x, dp)
    fl = Flags()
    o = lambda t: offset_view(t, elems)  # noqa: E731
    for v, variant in enumerate(((o(x), dp), (o(x), o(dp)))):
        for k, (a, b) in enumerate(zip(want, run(*variant))):
            fl.same(f"variant {v} output {k}", b, a)
    fl.check()


# ------------------------------------------------------------------------------------------------ 5. eager against a replayed graph
def replays_like_eager(step, outs_of):
    first = [t.clone() for t in outs_of(step())]
    second = outs_of(step())                               # (also the warm-up of the capture)
    fl = Flags()
    for k, (a, b) in enumerate(zip(first, second)):
        fl.same(f"eager twice {k}", b, a)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = outs_of(step())
    for rep in range(2):
        for t in outs:
            t.zero_()
        graph.replay()
        for k, (a, t) in enumerate(zip(first, outs)):
            fl.same(f"replay {rep} output {k}", t, a)
    torch.cuda.synchronize()
    fl.check()


def test_unit_eager_and_graph_replay_give_the_same_bits():
    from cl_ica_amd import ops
    shape = (16, 64, 16, 16)
    g = gen_for("unit-graph", shape, "normal")
    x, r, dy = (cl(torch.randn(shape, generator=g)).to(BF) for _ in range(3))
    gamma, beta, _, _ = params(64, "normal", g)

    def step():
        y, a, b = ops.batchnorm2d_act_fwd_nhwc(x, gamma, beta, None, None, EPS, MOMENTUM, 0.0, residual=r)
        return (y, a, b) + tuple(ops.batchnorm2d_act_bwd_nhwc(x, y, dy, gamma, a, b, 0.0, need_dr=True))
    replays_like_eager(step, lambda o: list(o))


def test_stem_eager_and_graph_replay_give_the_same_bits():
    from cl_ica_amd import ops
    shape = P.GRAPH_SHAPE
    N, C, H, W = shape
    g = gen_for("stem-graph", shape, TIES)
    x = draw_x(shape, TIES, g)
    gamma, beta, _, _ = params(C, "normal", g)
    dp = cl(torch.randn((N, C) + ops.maxpool_out_hw(H, W), generator=g)).to(BF)

    def step():
        p, a, b = ops.batchnorm2d_act_maxpool_fwd_nhwc(x, gamma, beta, None, None, EPS, MOMENTUM, 0.0)
        return (p, a, b) + tuple(ops.batchnorm2d_act_maxpool_bwd_nhwc(x, dp, gamma, beta, a, b, 0.0))
    replays_like_eager(step, lambda o: list(o))


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_before_any_launch():
    from cl_ica_amd import _lib, ops
    L = _lib.load()
    x = cl(torch.randn(4, 8, 4, 4)).to(BF)
    y = torch.empty_like(x)
    v = torch.ones(8, device="cuda")
    ws = ops.bn2d_nhwc_workspace(64, 8, x.device)
    p = lambda t: t.data_ptr()  # noqa: E731
    ok = (p(x), None, p(v), p(v), 64, 8, EPS, MOMENTUM, 0.0, p(y), p(v.clone()), p(v.clone()), None, None, p(ws), ws.numel(), None)
    fwd = L.clica_bn2d_nhwc_act_fwd_train_bf16

    def with_(i, value):
        a = list(ok)
        a[i] = value
        return a
    assert fwd(*with_(0, None)) == -1 and b"NULL" in L.clica_last_error()                    # X
    assert fwd(*with_(9, None)) == -1                                                        # Y
    assert fwd(*with_(14, None)) == -1                                                       # workspace
    assert fwd(*with_(5, (1 << 20) + 1)) == -1 and b"clica_bn2d_nhwc_act_fwd_train_bf16" in L.clica_last_error()      # C above the cap
    assert fwd(*with_(4, 1)) == -1                                                           # M < 2 in training
    assert fwd(*with_(15, 16)) == -1 and b"workspace" in L.clica_last_error()                # a workspace that is too small
    assert L.clica_bn2d_nhwc_act_bwd_bf16(p(x), p(x), None, p(v), p(v), p(v), 64, 8, 0.0, p(y), None, p(v), p(v), p(ws), ws.numel(), None) == -1
    assert L.clica_bn2d_nhwc_act_fwd_eval_bf16(p(x), None, p(v), p(v), None, p(v), 64, 8, EPS, 0.0, p(y), None) == -1
    pws = ops.bn2d_nhwc_maxpool_workspace(4, 8, 4, 4, x.device)
    stem = (p(x), p(v), p(v), 4, 8, 4, 4, EPS, MOMENTUM, 0.0, p(y), p(v.clone()), p(v.clone()), None, None, p(pws), pws.numel(), None)
    sf = L.clica_bn2d_nhwc_act_maxpool_fwd_train_bf16
    assert sf(*[None if i == 0 else a for i, a in enumerate(stem)]) == -1
    assert sf(*[16 if i == 16 else a for i, a in enumerate(stem)]) == -2                      # CLICA_E_WORKSPACE, as the fp32 stem
    assert sf(*[1.5 if i == 9 else a for i, a in enumerate(stem)]) == -1                      # slope outside [0, 1]
    assert L.clica_bn2d_nhwc_act_maxpool_bwd_bf16(p(x), None, p(v), p(v), p(v), p(v), 4, 8, 4, 4, 0.0, p(y), p(v), p(v), p(pws), pws.numel(),
                                                  None) == -1
    assert L.clica_avgpool2d_global_nhwc_fwd_bf16(None, 4, 16, 8, p(v), None) == -1
    assert L.clica_avgpool2d_global_nhwc_bwd_bf16(p(v), 4, (1 << 14) + 1, 8, p(y), None) == -1
    torch.cuda.synchronize()
    # through ops: one element type per call
    w, b = torch.ones(8, device="cuda"), torch.zeros(8, device="cuda")
    with pytest.raises(_lib.ClicaError, match="share one element type"):
        ops.batchnorm2d_act_fwd_nhwc(x, w, b, residual=x.float())
    with pytest.raises(_lib.ClicaError, match="float32"):
        ops.batchnorm2d_act_fwd_nhwc(x.float(), w, b, residual=x)
    yy, m, i = ops.batchnorm2d_act_fwd_nhwc(x, w, b)
    with pytest.raises(_lib.ClicaError, match="share one element type"):
        ops.batchnorm2d_act_bwd_nhwc(x, yy, x.float(), w, m, i)
    with pytest.raises(_lib.ClicaError, match="share one element type"):
        ops.batchnorm2d_act_eval_nhwc(x, w, b, m, i, residual=x.float())
    with pytest.raises(_lib.ClicaError, match="share one element type"):
        ops.batchnorm2d_act_maxpool_bwd_nhwc(x, torch.zeros(4, 8, 2, 2, device="cuda").contiguous(memory_format=CL), w, b, m, i)
    with pytest.raises(_lib.ClicaError):
        ops.batchnorm2d_act_fwd_nhwc(x, w.to(BF), b)                                         # parameters stay fp32
    with pytest.raises(_lib.ClicaError):
        ops.batchnorm2d_act_fwd_nhwc(x.half(), w, b)                                         # fp16 is not in scope
    with pytest.raises(_lib.ClicaError):
        ops.batchnorm2d_act_fwd(x.contiguous(), w, b)                                        # NCHW stays fp32
    with pytest.raises(_lib.ClicaError):
        ops.avgpool2d_global_bwd_nhwc(torch.zeros(4, 8, device="cuda"), 2, 2, torch.float16)


# ------------------------------------------------------------------------------------------------ 7. in the network
UNIT_OPS = ("batchnorm2d_act_fwd_nhwc", "batchnorm2d_act_eval_nhwc", "batchnorm2d_act_bwd_nhwc")
STEM_OPS = ("batchnorm2d_act_maxpool_fwd_nhwc", "batchnorm2d_act_maxpool_eval_nhwc", "batchnorm2d_act_maxpool_bwd_nhwc")
POOL_OPS = ("avgpool2d_global_fwd_nhwc", "avgpool2d_global_bwd_nhwc")
TORCH_FNS = ("batch_norm", "max_pool2d", "adaptive_avg_pool2d")


def backbone():
    from cl_ica_amd import resnet
    torch.manual_seed(11)
    f = resnet.ResNet18(num_classes=30)
    x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(12))
    return f.cuda().to(memory_format=CL).train(), x.cuda().contiguous(memory_format=CL)


def set_modes(monkeypatch, bf16):
    from cl_ica_amd import resnet
    for name in ("NORM_MODE", "POOL_MODE", "NHWC_MODE", "NHWC_STEM_MODE"):
        monkeypatch.setattr(resnet, name, "hip")
    if bf16 is not None:
        monkeypatch.setattr(resnet, "BF16_MODE", bf16)


def count_torch(monkeypatch):
    import torch.nn.functional as F
    counts = {k: 0 for k in TORCH_FNS}

    def wrap(name, fn):
        def counted(*a, **k):
            counts[name] += 1
            return fn(*a, **k)
        return counted
    for name in TORCH_FNS:
        monkeypatch.setattr(F, name, wrap(name, getattr(F, name)))
    return counts


def record_ops(monkeypatch):
    """Every call of the ops.*_nhwc functions with what it read (running statistics: before and after) and what it returned; the library's
    entry points by name."""
    from cl_ica_amd import ops
    calls, entries = [], []
    real = {name: getattr(ops, name) for name in UNIT_OPS + STEM_OPS + POOL_OPS}

    def wrap(name, fn):
        def recorded(*a, **k):
            training = name in ("batchnorm2d_act_fwd_nhwc", "batchnorm2d_act_maxpool_fwd_nhwc")
            before = [t.clone() for t in a[3:5]] if training else []
            out = fn(*a, **k)
            after = [t.clone() for t in a[3:5]] if training else []
            calls.append((name, a, k, before, after, out))
            return out
        return recorded
    for name, fn in real.items():
        monkeypatch.setattr(ops, name, wrap(name, fn))
    real_entry = ops._entry

    def entry(name, dtype):
        fn, full = real_entry(name, dtype)
        entries.append(full)
        return fn, full
    monkeypatch.setattr(ops, "_entry", entry)
    return calls, entries, real


def up(t):
    return t.float() if torch.is_tensor(t) and t.dtype == BF else t


def test_in_the_network_bf16_kernels_run_and_match_the_fp32_kernels(monkeypatch):
    set_modes(monkeypatch, "hip")
    f, x = backbone()
    torch_calls = count_torch(monkeypatch)
    calls, entries, real = record_ops(monkeypatch)
    seen = {}
    f.fc.register_forward_hook(lambda m, i, o: seen.update(fc_in=i[0].dtype, fc_out=o.dtype))
    with torch.autocast("cuda", dtype=BF):
        out = f(x)
        assert out.dtype == F32 and seen == dict(fc_in=F32, fc_out=F32)
        out.float().square().sum().backward()
    names = [c[0] for c in calls]
    assert names.count("batchnorm2d_act_maxpool_fwd_nhwc") == 1 and names.count("batchnorm2d_act_fwd_nhwc") == 19
    assert names.count("avgpool2d_global_fwd_nhwc") == 1 and names.count("avgpool2d_global_bwd_nhwc") == 1
    assert names.count("batchnorm2d_act_maxpool_bwd_nhwc") == 1 and names.count("batchnorm2d_act_bwd_nhwc") == 19
    assert len(names) == 42
    assert all(p.grad is not None and p.grad.dtype == F32 and bool(torch.isfinite(p.grad).all()) for p in f.parameters())
    f.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        out = f(x)
    assert out.dtype == F32 and bool(torch.isfinite(out).all()) and seen == dict(fc_in=F32, fc_out=F32)
    names = [c[0] for c in calls]
    assert names.count("batchnorm2d_act_maxpool_eval_nhwc") == 1 and names.count("batchnorm2d_act_eval_nhwc") == 19
    assert names.count("avgpool2d_global_fwd_nhwc") == 2 and len(names) == 63
    assert torch_calls == {k: 0 for k in TORCH_FNS}
    assert len(entries) == 63 and all(e.endswith("_bf16") for e in entries)

    def act(t, name):
        assert t.dtype == BF and t.dim() == 4 and t.is_contiguous(memory_format=CL), (name, t.dtype, t.shape, t.stride())
        return t
    fl = Flags()
    for n, (name, a, k, before, after, out) in enumerate(calls):
        fn, tag = real[name], f"call {n} {name}"
        if name in ("batchnorm2d_act_fwd_nhwc", "batchnorm2d_act_maxpool_fwd_nhwc"):
            act(a[0], tag)
            res = k.get("residual")
            kw = dict(residual=up(act(res, tag))) if res is not None else ({} if "maxpool" in name else dict(residual=None))
            rm, rv = before[0].clone(), before[1].clone()
            y32, m32, i32 = fn(up(a[0]), a[1], a[2], rm, rv, *a[5:], **kw)
            fl.rounded(tag + " y", act(out[0], tag), y32)
            fl.same(tag + " save_mean", out[1], m32); fl.same(tag + " save_invstd", out[2], i32)
            fl.same(tag + " running_mean", after[0], rm); fl.same(tag + " running_var", after[1], rv)
        elif name in ("batchnorm2d_act_eval_nhwc", "batchnorm2d_act_maxpool_eval_nhwc"):
            res = k.get("residual")
            kw = dict(residual=up(act(res, tag))) if res is not None else ({} if "maxpool" in name else dict(residual=None))
            fl.rounded(tag + " y", act(out, tag), fn(up(act(a[0], tag)), *a[1:], **kw))
        elif name == "batchnorm2d_act_bwd_nhwc":
            for t in a[:3]:
                act(t, tag)
            dx32, dr32, dg32, db32 = fn(up(a[0]), up(a[1]), up(a[2]), *a[3:], **k)
            fl.rounded(tag + " dx", act(out[0], tag), dx32)
            assert (out[1] is None) == (dr32 is None)
            if dr32 is not None:
                fl.rounded(tag + " dr", act(out[1], tag), dr32)
            fl.same(tag + " dgamma", out[2], dg32); fl.same(tag + " dbeta", out[3], db32)
        elif name == "batchnorm2d_act_maxpool_bwd_nhwc":
            dx32, dg32, db32 = fn(up(act(a[0], tag)), up(act(a[1], tag)), *a[2:], **k)
            fl.rounded(tag + " dx", act(out[0], tag), dx32)
            fl.same(tag + " dgamma", out[1], dg32); fl.same(tag + " dbeta", out[2], db32)
        elif name == "avgpool2d_global_fwd_nhwc":
            assert out.dtype == F32
            fl.same(tag + " y", out, fn(up(act(a[0], tag))))
        else:
            assert name == "avgpool2d_global_bwd_nhwc" and a[0].dtype == F32 and a[3] == BF
            fl.rounded(tag + " dx", act(out, tag), fn(a[0], a[1], a[2]))
    fl.check()


# ------------------------------------------------------------------------------------------------ 8. defaults do not move
def test_by_default_bf16_inputs_run_torch_modules(monkeypatch):
    from cl_ica_amd import resnet
    assert resnet.BF16_MODE == "torch"
    set_modes(monkeypatch, None)
    f, x = backbone()
    torch_calls = count_torch(monkeypatch)
    calls, entries, _ = record_ops(monkeypatch)
    with torch.autocast("cuda", dtype=BF):
        f(x).float().square().sum().backward()
    assert torch_calls == dict(batch_norm=20, max_pool2d=1, adaptive_avg_pool2d=1)
    f.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=BF):
        f(x)
    assert torch_calls == dict(batch_norm=40, max_pool2d=2, adaptive_avg_pool2d=2)
    assert not calls and not entries


def test_fp32_inputs_do_not_see_the_switch(monkeypatch):
    from cl_ica_amd import resnet
    f0, x = backbone()
    res = {}
    for mode in ("torch", "hip"):
        set_modes(monkeypatch, mode)
        f = copy.deepcopy(f0)
        y = f(x)
        y.square().sum().backward()
        f.eval()
        with torch.no_grad():
            e = f(x)
        res[mode] = [y.detach(), e] + [p.grad for p in f.parameters()] + [b.float() for b in f.buffers()]
    assert resnet.BF16_MODE == "hip"
    fl = Flags()
    for k, (a, b) in enumerate(zip(res["hip"], res["torch"])):
        fl.same(f"tensor {k}", a.contiguous(), b.contiguous())
    fl.check()
