"""Host-side checks of the fused BatchNorm2d unit (csrc/bn2d.hip), no GPU: the sweep's cases satisfy their caps from the fp64 oracle
alone, the workspace planner on fixed and random shapes, the unchanged state dict of the ResNet-18 stand-in, and the fall-through to
torch's modules on CPU tensors."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import bn2d_oracle as B


def lib():
    from cl_ica_amd import _lib
    return _lib.load()


def test_every_case_of_the_sweep_satisfies_both_caps():
    n = 0
    for shape, cls, residual in B.sweep():
        frac, kap = B.case_ok(*shape, cls, residual)
        assert frac <= B.MAX_LEFT_OUT, (shape, cls, residual, frac)
        assert kap <= B.MAX_KAPPA, (shape, cls, residual, kap)
        assert B.SEED_ATTEMPT.get(shape + (cls, residual), 0) < B.MAX_ATTEMPTS
        n += 1
    assert n == len(B.SHAPES) * 2 * 2
    assert set(B.EVAL_SHAPES) <= set(B.SHAPES) and set(B.UNALIGNED_SHAPES) <= set(B.SHAPES)
    assert all(H * W % 4 == 0 for (_, _, H, W) in B.UNALIGNED_SHAPES)      # what the bit-equality of the unaligned variant rests on


def test_the_oracle_agrees_with_torch_in_fp64():
    """z = bn + r, dr = dz, and norm_oracle's BatchNorm backward on that dz, against torch's own batch_norm in double precision."""
    F = torch.nn.functional
    N, C, H, W = 5, 65, 3, 5
    for slope in (0.0, 0.01):
        c, fw, bw = B.reference(N, C, H, W, 1, True, slope)
        t = {k: torch.tensor(B.to_nchw(c[k], N, C, H, W), dtype=torch.float64) for k in ("x", "r", "dy")}
        x, r = t["x"].requires_grad_(True), t["r"].requires_grad_(True)
        w, b = (torch.tensor(c[k], dtype=torch.float64).requires_grad_(True) for k in ("gamma", "beta"))
        rm, rv = (torch.tensor(c[k], dtype=torch.float64) for k in ("running_mean", "running_var"))
        y = F.leaky_relu(F.batch_norm(x, rm, rv, w, b, True, B.MOMENTUM, B.EPS) + r, slope)
        y.backward(t["dy"])
        for got, ref in ((fw["y"], y), (bw["dx"], x.grad), (bw["dr"], r.grad)):
            assert np.allclose(got, B.to_rows(ref.detach().numpy()), rtol=1e-9, atol=1e-9)
        for got, ref in ((bw["dgamma"], w.grad), (bw["dbeta"], b.grad), (fw["running_mean"], rm), (fw["running_var"], rv)):
            assert np.allclose(got, ref.numpy(), rtol=1e-9, atol=1e-9)


def test_block_cases_have_no_pre_activation_near_the_kink():
    for case in B.BLOCK_CASES:
        assert B.block_near_kink(*case) == 0, case


def test_workspace_planner_on_the_sweep_and_on_random_shapes():
    L = lib()
    nb = ctypes.c_size_t()
    shapes = [(N, C, H * W) for (N, C, H, W) in B.SHAPES]
    shapes += [(1024, 64, 1024), (1024, 64, 256), (1024, 128, 64), (1024, 256, 16), (1024, 512, 4)]
    rng = np.random.default_rng(0)
    for _ in range(1000):
        N = int(rng.choice([1, 2, 3, 16, 17, 100, 1024, 4096, 100000]) + rng.integers(0, 3))
        C = int(rng.choice([1, 3, 63, 64, 65, 512, 2048, (1 << 20) - 1]) + rng.integers(0, 2))
        HW = int(rng.choice([1, 2, 4, 8, 9, 15, 16, 64, 221, 256, 1024, 4096, 50176]) + rng.integers(0, 2))
        if N * HW >= 2 and C >= 1:
            shapes.append((N, C, HW))
    assert len(shapes) > 900
    for (N, C, HW) in shapes:
        assert L.clica_bn2d_workspace_bytes(N, C, HW, ctypes.byref(nb)) == 0, (N, C, HW)
        # three planes of at most 32 partials per channel
        assert 16 <= nb.value <= 3 * 32 * 4 * C + 16 and nb.value % 16 == 0, (N, C, HW, nb.value)


def test_workspace_planner_refuses_bad_shapes():
    L = lib()
    nb = ctypes.c_size_t()
    assert L.clica_bn2d_workspace_bytes(1, 8, 1, ctypes.byref(nb)) == -1 and b"N=1 C=8 HW=1" in L.clica_last_error()
    assert L.clica_bn2d_workspace_bytes(0, 8, 4, ctypes.byref(nb)) == -1 and b"N=0" in L.clica_last_error()
    assert L.clica_bn2d_workspace_bytes(4, 0, 4, ctypes.byref(nb)) == -1 and b"C=0" in L.clica_last_error()
    assert L.clica_bn2d_workspace_bytes(4, 8, 0, ctypes.byref(nb)) == -1 and b"HW=0" in L.clica_last_error()
    assert L.clica_bn2d_workspace_bytes(4, 8, 4, None) == -1 and b"bytes is NULL" in L.clica_last_error()


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    L = lib()
    assert L.clica_version() >= 101
    assert L.clica_bn2d_act_fwd_train(None, None, None, None, 1, 8, 1, 1e-5, 0.1, 0.0, None, None, None, None, None, None, 0, None) == -1
    assert b"N HW >= 2" in L.clica_last_error()
    assert L.clica_bn2d_act_fwd_train(None, None, None, None, 4, 8, 4, 1e-5, 0.1, -0.5, None, None, None, None, None, None, 0, None) == -1
    assert b"slope" in L.clica_last_error()
    assert L.clica_bn2d_act_fwd_train(None, None, None, None, 4, 8, 4, 1e-5, 0.1, 0.0, None, None, None, None, None, None, 0, None) == -1
    assert b"NULL pointer" in L.clica_last_error()
    assert L.clica_bn2d_act_fwd_eval(None, None, None, None, None, None, 4, 8, 4, 1e-5, -1.0, None, None) == -1
    assert b"slope" in L.clica_last_error()
    assert L.clica_bn2d_act_fwd_eval(None, None, None, None, None, None, 1, 8, 1, 1e-5, 0.0, None, None) == -1      # one value: inference is fine
    assert b"NULL pointer" in L.clica_last_error()
    assert L.clica_bn2d_act_bwd(None, None, None, None, None, None, 4, 8, 4, -1.0, None, None, None, None, None, 0, None) == -1
    assert b"slope" in L.clica_last_error()
    assert L.clica_bn2d_act_bwd(None, None, None, None, None, None, 4, 8, 4, 0.0, None, None, None, None, None, 0, None) == -1
    assert b"NULL pointer" in L.clica_last_error()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    p16 = (p + 15) // 16 * 16
    assert L.clica_bn2d_act_bwd(p, p, p, p, p, p, 4, 8, 4, 0.0, p, None, p, p, p16 + 4, 1 << 20, None) == -1
    assert b"16-byte aligned" in L.clica_last_error()
    assert L.clica_bn2d_act_bwd(p, p, p, p, p, p, 4, 8, 4, 0.0, p, None, p, p, p16, 16, None) == -1
    assert b"bytes" in L.clica_last_error()


def test_ops_wrappers_refuse_other_inputs():
    from cl_ica_amd import ops
    x = torch.randn(4, 8, 2, 2)
    w, b = torch.ones(8), torch.zeros(8)
    with pytest.raises(ValueError, match="contiguous NCHW"):
        ops.batchnorm2d_act_fwd(x.reshape(4, 32), w, b)
    with pytest.raises(ValueError, match="contiguous NCHW"):
        ops.batchnorm2d_act_fwd(x.contiguous(memory_format=torch.channels_last), w, b)
    with pytest.raises(ValueError, match="contiguous NCHW"):
        ops.batchnorm2d_act_eval(x[:, :, :, :1], w, b, b, w)
    with pytest.raises(ValueError, match="contiguous NCHW"):
        ops.batchnorm2d_act_bwd(x.permute(0, 1, 3, 2), x, x, w, b, w)
    # maps, then vectors, then devices, in both layouts: what the channels-last functions refuse on CPU tensors, these refuse alike
    cl = x.contiguous(memory_format=torch.channels_last)
    assert not cl.is_contiguous()
    with pytest.raises(ValueError, match="shape of x"):
        ops.batchnorm2d_act_fwd(x, w, b, residual=torch.randn(4, 8, 4, 1))
    with pytest.raises(ValueError, match="contiguous NCHW"):
        ops.batchnorm2d_act_fwd(x, w, b, residual=cl)                       # layout mismatch of the residual
    with pytest.raises(ValueError, match="contiguous NCHW"):
        ops.batchnorm2d_act_bwd(x, cl, x, w, b, w)                          # y
    with pytest.raises(ValueError, match="shape of x"):
        ops.batchnorm2d_act_bwd(x, x, x[:2], w, b, w)                       # dy
    with pytest.raises(ValueError, match="contiguous values"):
        ops.batchnorm2d_act_fwd(x, w[:3], b)
    with pytest.raises(ValueError, match="contiguous values"):
        ops.batchnorm2d_act_fwd(x, w, torch.zeros(16)[::2])
    with pytest.raises(ValueError, match="come together"):
        ops.batchnorm2d_act_fwd(x, w, b, running_mean=b)
    with pytest.raises(ValueError, match="contiguous values"):
        ops.batchnorm2d_act_eval(x, w, b, b[:7], w)
    with pytest.raises(ValueError, match="contiguous matrix"):
        ops.avgpool2d_global_bwd(torch.randn(4, 8).t(), 2, 2)


def test_state_dict_keys_are_unchanged():
    from cl_ica_amd import resnet
    keys = list(resnet.resnet18(num_classes=30).state_dict())
    want = ["conv1.weight"] + [f"bn1.{k}" for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    for layer, down in ((1, False), (2, True), (3, True), (4, True)):
        for i in range(2):
            p = f"layer{layer}.{i}."
            for bn, conv in (("bn1", "conv1"), ("bn2", "conv2")):
                want += [p + conv + ".weight"] + [p + f"{bn}.{k}" for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
            if down and i == 0:
                want += [p + "downsample.0.weight"] + [p + f"downsample.1.{k}" for k in
                                                       ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    want += ["fc.weight", "fc.bias"]
    assert keys == want
    assert all(type(m) is torch.nn.BatchNorm2d for m in resnet.resnet18(num_classes=30).modules() if "Norm" in type(m).__name__)


def raw(t):
    return np.ascontiguousarray(t.detach().numpy()).reshape(-1).view(np.uint8)


@pytest.mark.parametrize("train", [True, False])
def test_cpu_tensors_fall_through_to_torch_modules(monkeypatch, train):
    from cl_ica_amd import resnet
    assert resnet.NORM_MODE in ("hip", "torch")
    torch.manual_seed(5)
    base = resnet.resnet18(num_classes=30)
    x = torch.randn(3, 3, 64, 64)
    out = {}
    for mode in ("hip", "torch"):
        monkeypatch.setattr(resnet, "NORM_MODE", mode)
        f = copy.deepcopy(base).train(train)
        y = f(x)
        y.square().sum().backward()
        out[mode] = [y] + [p.grad for p in f.parameters()] + [b.float() for b in f.buffers()]
    assert len(out["hip"]) == len(out["torch"])
    for a, b in zip(out["hip"], out["torch"]):
        assert np.array_equal(raw(a), raw(b))
