"""Host-side checks of the channels-last BatchNorm2d unit and average pool (csrc/bn2d_nhwc.hip), no GPU: the sweep's cases satisfy
their caps from the fp64 oracle alone, the ops wrappers refuse other inputs before any launch, the workspace planner on fixed and random
shapes, the entry points' argument checks, the NHWC_MODE switch and the fall-through to torch's modules on CPU tensors."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import bn2d_nhwc_cases as K
import bn2d_oracle as B

RESNET_SHAPES = [(1048576, 64), (262144, 64), (65536, 128), (16384, 256), (4096, 512)]      # ResNet-18's units at N = 1024, 64 x 64 images


def lib():
    from cl_ica_amd import _lib
    return _lib.load()


def test_every_case_of_the_sweep_satisfies_both_caps():
    n = 0
    for shape, cls, residual in K.sweep():
        attempt = K.attempt_of(*shape, cls, residual)
        assert attempt < B.MAX_ATTEMPTS
        frac, kap = B.case_ok(*shape, cls, residual, attempt)
        assert frac <= B.MAX_LEFT_OUT, (shape, cls, residual, frac)
        assert kap <= B.MAX_KAPPA, (shape, cls, residual, kap)
        n += 1
    assert n == len(K.SHAPES) * 2 * 2 and len(set(K.SHAPES)) == len(K.SHAPES)
    assert set(K.EVAL_SHAPES) <= set(K.SHAPES) and set(K.UNALIGNED_SHAPES) <= set(K.SHAPES)
    assert all(C % 4 == 0 for (_, C, _, _) in K.UNALIGNED_SHAPES)           # what the bit-equality of the unaligned variant rests on
    assert all(key[:4] in K.EXTRA_SHAPES for key in K.EXTRA_ATTEMPT)
    for cls in range(len(B.CLASSES)):                                       # the slope-1 case at the cap on S: conditioning only
        assert B.O.kappa("bn", B.make_case(*K.CAPPED_SHAPE, cls, True, attempt=0)["x"]) <= B.MAX_KAPPA


def test_the_shared_reference_is_the_oracle_at_the_named_attempt():
    shape = (130, 12, 8, 8)
    c, fw, bw = K.reference(*shape, 0, False, 0.0)
    want = B.make_case(*shape, 0, False, attempt=3)
    assert np.array_equal(c["x"], want["x"]) and c["r"] is None
    assert K.reference(2, 3, 1, 1, 1, True, 0.0) is B.reference(2, 3, 1, 1, 1, True, 0.0)
    t = torch.tensor(B.to_nchw(c["x"], *shape)).contiguous(memory_format=torch.channels_last)
    assert np.array_equal(K.rows_of(t), c["x"])                             # the rows are the NHWC tensor


def test_ops_wrappers_refuse_other_inputs():
    from cl_ica_amd import ops
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    x = cl(torch.randn(4, 8, 2, 3))
    w, b = torch.ones(8), torch.zeros(8)
    nchw = x.contiguous()
    assert not nchw.is_contiguous(memory_format=torch.channels_last)
    for bad in (nchw, x[:, :, :, :2], x[:, :4], x[::2], x.reshape(4, 48), x[0]):
        with pytest.raises(ValueError, match="dense channels-last"):
            ops.batchnorm2d_act_fwd_nhwc(bad, w, b)
        with pytest.raises(ValueError, match="dense channels-last"):
            ops.batchnorm2d_act_eval_nhwc(bad, w, b, b, w)
        with pytest.raises(ValueError, match="dense channels-last"):
            ops.avgpool2d_global_fwd_nhwc(bad)
    with pytest.raises(ValueError, match="dense channels-last"):
        ops.batchnorm2d_act_fwd_nhwc(x, w, b, residual=nchw)                 # layout mismatch of the residual
    with pytest.raises(ValueError, match="shape of x"):
        ops.batchnorm2d_act_fwd_nhwc(x, w, b, residual=cl(torch.randn(4, 8, 3, 2)))
    with pytest.raises(ValueError, match="shape of x"):
        ops.batchnorm2d_act_eval_nhwc(x, w, b, b, w, residual=x[:2])
    with pytest.raises(ValueError, match="dense channels-last"):
        ops.batchnorm2d_act_bwd_nhwc(x, nchw, x, w, b, w)                    # y
    with pytest.raises(ValueError, match="dense channels-last"):
        ops.batchnorm2d_act_bwd_nhwc(x, x, nchw, w, b, w)                    # dy
    with pytest.raises(ValueError, match="shape of x"):
        ops.batchnorm2d_act_bwd_nhwc(x, x, x[:2], w, b, w)
    with pytest.raises(ValueError, match="contiguous values"):
        ops.batchnorm2d_act_fwd_nhwc(x, w[:3], b)
    with pytest.raises(ValueError, match="contiguous values"):
        ops.batchnorm2d_act_fwd_nhwc(x, w, torch.zeros(16)[::2])
    with pytest.raises(ValueError, match="come together"):
        ops.batchnorm2d_act_fwd_nhwc(x, w, b, running_mean=b)
    with pytest.raises(ValueError, match="contiguous values"):
        ops.batchnorm2d_act_eval_nhwc(x, w, b, b[:7], w)
    with pytest.raises(ValueError, match="contiguous values"):
        ops.batchnorm2d_act_bwd_nhwc(x, x, x, w, b[:2], w)
    with pytest.raises(ValueError, match="contiguous matrix"):
        ops.avgpool2d_global_bwd_nhwc(torch.randn(4, 8).t(), 2, 3)
    # the NCHW functions keep their contract
    with pytest.raises(ValueError, match="contiguous NCHW"):
        ops.batchnorm2d_act_fwd(x, w, b)


def test_workspace_planner_on_the_resnet_shapes_and_on_random_shapes():
    L = lib()
    nb = ctypes.c_size_t()
    shapes = list(RESNET_SHAPES) + [(N * H * W, C) for (N, C, H, W) in K.SHAPES + [K.CAPPED_SHAPE]]
    rng = np.random.default_rng(0)
    for _ in range(1000):
        M = int(rng.choice([1, 2, 3, 16, 17, 100, 1024, 4096, 16384, 100000, 1 << 20, 1 << 33]) + rng.integers(0, 3))
        C = int(rng.choice([1, 3, 4, 12, 63, 64, 65, 128, 256, 260, 512, 2048, (1 << 20) - 1]) + rng.integers(0, 2))
        shapes.append((M, C))
    S_MAX = 256
    seen = set()
    for (M, C) in shapes:
        assert L.clica_bn2d_nhwc_workspace_bytes(M, C, ctypes.byref(nb)) == 0, (M, C)
        S = K.rows_splits(M, C)
        assert 1 <= S <= S_MAX and S <= M
        assert nb.value == (12 * S * C + 15) // 16 * 16, (M, C, nb.value, S)          # three planes [S][C] of floats
        assert 16 <= nb.value <= S_MAX * C * 12 + 16
        seen.add(S)
    assert {1, 2, 64, 128, 256} <= seen                                               # the caps of the three merge widths are reached
    assert [K.rows_splits(M, C) for (M, C) in RESNET_SHAPES] == [256, 256, 128, 64, 32]


def test_workspace_planner_refuses_bad_shapes():
    L = lib()
    nb = ctypes.c_size_t()
    assert L.clica_bn2d_nhwc_workspace_bytes(0, 8, ctypes.byref(nb)) == -1 and b"M=0 C=8" in L.clica_last_error()
    assert L.clica_bn2d_nhwc_workspace_bytes(-3, 8, ctypes.byref(nb)) == -1 and b"M=-3" in L.clica_last_error()
    assert L.clica_bn2d_nhwc_workspace_bytes(4, 0, ctypes.byref(nb)) == -1 and b"C=0" in L.clica_last_error()
    assert L.clica_bn2d_nhwc_workspace_bytes(4, (1 << 20) + 1, ctypes.byref(nb)) == -1
    assert L.clica_bn2d_nhwc_workspace_bytes(4, 8, None) == -1 and b"bytes is NULL" in L.clica_last_error()
    assert L.clica_bn2d_nhwc_workspace_bytes(1, 8, ctypes.byref(nb)) == 0 and nb.value == 96


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    L = lib()
    assert L.clica_bn2d_nhwc_act_fwd_train(None, None, None, None, 1, 8, 1e-5, 0.1, 0.0, None, None, None, None, None, None, 0, None) == -1
    assert b"M = N H W >= 2" in L.clica_last_error()
    assert L.clica_bn2d_nhwc_act_fwd_train(None, None, None, None, 16, 8, 1e-5, 0.1, -0.5, None, None, None, None, None, None, 0, None) == -1
    assert b"slope" in L.clica_last_error()
    assert L.clica_bn2d_nhwc_act_fwd_train(None, None, None, None, 16, 8, 1e-5, 0.1, 0.0, None, None, None, None, None, None, 0, None) == -1
    assert b"NULL pointer" in L.clica_last_error()
    assert L.clica_bn2d_nhwc_act_fwd_eval(None, None, None, None, None, None, 16, 8, 1e-5, -1.0, None, None) == -1
    assert b"slope" in L.clica_last_error()
    assert L.clica_bn2d_nhwc_act_fwd_eval(None, None, None, None, None, None, 1, 8, 1e-5, 0.0, None, None) == -1      # one row: inference is fine
    assert b"NULL pointer" in L.clica_last_error()
    assert L.clica_bn2d_nhwc_act_fwd_eval(None, None, None, None, None, None, 0, 8, 1e-5, 0.0, None, None) == -1
    assert b"M=0" in L.clica_last_error()
    assert L.clica_bn2d_nhwc_act_bwd(None, None, None, None, None, None, 16, 8, -1.0, None, None, None, None, None, 0, None) == -1
    assert b"slope" in L.clica_last_error()
    assert L.clica_bn2d_nhwc_act_bwd(None, None, None, None, None, None, 1, 8, 0.0, None, None, None, None, None, 0, None) == -1
    assert b"M = N H W >= 2" in L.clica_last_error()
    assert L.clica_bn2d_nhwc_act_bwd(None, None, None, None, None, None, 16, 8, 0.0, None, None, None, None, None, 0, None) == -1
    assert b"NULL pointer" in L.clica_last_error()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    p16 = (p + 15) // 16 * 16
    assert L.clica_bn2d_nhwc_act_bwd(p, p, p, p, p, p, 16, 8, 0.0, p, None, p, p, p16 + 4, 1 << 20, None) == -1
    assert b"16-byte aligned" in L.clica_last_error()
    assert L.clica_bn2d_nhwc_act_bwd(p, p, p, p, p, p, 16, 8, 0.0, p, None, p, p, p16, 16, None) == -1
    assert b"bytes" in L.clica_last_error()
    assert L.clica_bn2d_nhwc_act_fwd_train(p, None, p, p, 16, 8, 1e-5, 0.1, 0.0, p, p, p, None, None, p16, 16, None) == -1
    assert b"clica_bn2d_nhwc_workspace_bytes" in L.clica_last_error()
    # the average pool
    assert L.clica_avgpool2d_global_nhwc_fwd(None, 4, 4, 8, None, None) == -1 and b"NULL pointer" in L.clica_last_error()
    assert L.clica_avgpool2d_global_nhwc_fwd(p, 0, 4, 8, p, None) == -1 and b"N=0" in L.clica_last_error()
    assert L.clica_avgpool2d_global_nhwc_fwd(p, 4, 0, 8, p, None) == -1 and b"HW=0" in L.clica_last_error()
    assert L.clica_avgpool2d_global_nhwc_fwd(p, 4, (1 << 14) + 1, 8, p, None) == -1
    assert L.clica_avgpool2d_global_nhwc_bwd(p, 4, 4, 0, p, None) == -1 and b"C=0" in L.clica_last_error()
    assert L.clica_avgpool2d_global_nhwc_bwd(None, 4, 4, 8, None, None) == -1 and b"NULL pointer" in L.clica_last_error()


def raw(t):
    return np.ascontiguousarray(t.detach().numpy()).reshape(-1).view(np.uint8)


def test_the_switch_defaults_to_torch_and_cpu_tensors_fall_through(monkeypatch):
    """NHWC_MODE exists, its default is "torch", and with "hip" a channels-last CPU model still runs torch's modules: the same bits."""
    from cl_ica_amd import resnet
    import os
    assert resnet.NHWC_MODE == os.environ.get("CLICA_RESNET_NHWC", "torch")
    torch.manual_seed(5)
    base = resnet.resnet18(num_classes=30).to(memory_format=torch.channels_last)
    x = torch.randn(3, 3, 64, 64).contiguous(memory_format=torch.channels_last)
    out = {}
    for mode in ("hip", "torch"):
        monkeypatch.setattr(resnet, "NHWC_MODE", mode)
        f = copy.deepcopy(base).train()
        y = f(x)
        y.square().sum().backward()
        out[mode] = [y] + [p.grad for p in f.parameters()] + [b.float() for b in f.buffers()]
    for a, b in zip(out["hip"], out["torch"]):
        assert np.array_equal(raw(a), raw(b))


def test_layout_dispatch_of_the_units(monkeypatch):
    from cl_ica_amd import resnet
    x = torch.randn(2, 8, 3, 3)
    cl = x.contiguous(memory_format=torch.channels_last)
    for mode, want in (("torch", None), ("hip", "nhwc")):
        monkeypatch.setattr(resnet, "NHWC_MODE", mode)
        assert resnet._layout(x) == "nchw" and resnet._layout(cl) == want
        # the same memory in both layouts: the NCHW kernels, exactly as before
        assert resnet._layout(torch.randn(2, 1, 3, 3).contiguous(memory_format=torch.channels_last)) == "nchw"
        assert resnet._layout(torch.randn(2, 8, 1, 1).contiguous(memory_format=torch.channels_last)) == "nchw"
        assert resnet._layout(cl[:, :, :, :2]) is None and resnet._layout(x[:, :4]) is None
