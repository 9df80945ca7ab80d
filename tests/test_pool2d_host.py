"""Host-side checks of the fused stem unit and the global average pool (csrc/pool2d.hip), no GPU: the fp64 oracle
(tests/pool2d_oracle.py) against torch's own autograd in double precision on every shape and class of the sweep, the tie class
included; the caps every case of the sweep satisfies; the accept / refuse codes of the entry points; the output size of the wrapper."""
import ctypes

import numpy as np
import pytest
import torch

import pool2d_oracle as Q

F = torch.nn.functional
ids = lambda s: "x".join(map(str, s))


def lib():
    from cl_ica_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("shape", Q.SHAPES, ids=ids)
def test_the_oracle_agrees_with_torch_in_fp64(shape):
    """max_pool2d(leaky_relu(batch_norm(x)), 3, 2, 1) and its autograd on the CPU in double precision: the first-maximum rule among it."""
    N, C, H, W = shape
    for cls in range(len(Q.CLASSES)):
        for slope in Q.SLOPES:
            c, fw, bw = Q.reference(N, C, H, W, cls, slope)
            x = torch.tensor(Q.to_nchw(c["x"], *shape), dtype=torch.float64).requires_grad_(True)
            w, b = (torch.tensor(c[k], dtype=torch.float64).requires_grad_(True) for k in ("gamma", "beta"))
            rm, rv = (torch.tensor(c[k], dtype=torch.float64) for k in ("running_mean", "running_var"))
            p = F.max_pool2d(F.leaky_relu(F.batch_norm(x, rm, rv, w, b, True, Q.MOMENTUM, Q.EPS), slope), 3, 2, 1)
            assert tuple(p.shape[2:]) == Q.out_hw(H, W)
            p.backward(torch.tensor(c["dp"], dtype=torch.float64))
            close = lambda got, ref: np.allclose(got, ref.detach().numpy(), rtol=1e-9, atol=1e-9)
            assert close(fw["p"], p), (shape, cls, slope)
            assert close(fw["running_mean"], rm) and close(fw["running_var"], rv)
            assert close(bw["dx"], torch.tensor(Q.to_rows(x.grad.numpy()))), (shape, cls, slope)
            assert close(bw["dgamma"], w.grad) and close(bw["dbeta"], b.grad), (shape, cls, slope)


def test_first_maximum_rule_on_a_constant_plane():
    """A constant 5 x 5 plane: every window's gradient lands on its first pixel in scan order, as torch's indices say."""
    arg = Q.maxpool(np.zeros((1, 1, 5, 5)))[1]
    dy = Q.maxpool_backward(arg, np.ones((1, 1, 3, 3)), 5, 5)
    assert np.flatnonzero(dy).tolist() == [0, 1, 3, 5, 6, 8, 15, 16, 18]
    idx = F.max_pool2d(torch.zeros(1, 1, 5, 5, dtype=torch.float64), 3, 2, 1, return_indices=True)[1]
    assert idx.flatten().tolist() == [0, 1, 3, 5, 6, 8, 15, 16, 18]


def test_every_case_of_the_sweep_satisfies_its_caps():
    n = 0
    for shape, cls in Q.sweep():
        frac, kap, gap = Q.case_ok(*shape, cls)
        assert frac <= Q.MAX_LEFT_OUT, (shape, cls, frac)
        assert kap <= Q.MAX_KAPPA, (shape, cls, kap)
        assert gap >= Q.MIN_GAP_REL, (shape, cls, gap)
        assert Q.SEED_ATTEMPT.get(shape + (cls,), 0) < Q.MAX_ATTEMPTS
        c = Q.make_case(*shape, cls)
        assert 0.25 <= np.abs(c["gamma"]).min() and np.abs(c["gamma"]).max() <= 1.5
        n += 1
    assert n == len(Q.SHAPES) * len(Q.CLASSES)
    assert set(Q.EVAL_SHAPES) <= set(Q.SHAPES) and set(Q.UNALIGNED_SHAPES) <= set(Q.SHAPES)
    assert all(W % 4 == 0 for (_, _, _, W) in Q.UNALIGNED_SHAPES)
    # the tie class does hold exact ties inside windows: some window's first maximum is not its only one
    c, fw, _ = Q.reference(2, 4, 5, 5, Q.TIE_CLASS, 1.0)
    win = Q.windows(Q.to_nchw(fw["y"], 2, 4, 5, 5))
    assert ((win == win.max(0)).sum(0) > 1).any()


def test_workspace_entry_point_accepts_and_refuses():
    L = lib()
    nb = ctypes.c_size_t()
    for (N, C, H, W) in Q.SHAPES + [(1024, 64, 32, 32), (256, 64, 112, 112), (4, 8, 1, 12544 // 2)]:
        assert L.clica_bn2d_maxpool_workspace_bytes(N, C, H, W, ctypes.byref(nb)) == 0, (N, C, H, W)
        assert 16 <= nb.value <= 3 * 32 * 4 * C + 16 and nb.value % 16 == 0
    assert L.clica_bn2d_maxpool_workspace_bytes(1, 3, 130, 130, ctypes.byref(nb)) == -1      # plane over the limit
    assert b"H=130 W=130 over the limit" in L.clica_last_error()
    assert L.clica_bn2d_maxpool_workspace_bytes(1, 3, 113, 112, ctypes.byref(nb)) == -1
    assert L.clica_bn2d_maxpool_workspace_bytes(1, 8, 1, 1, ctypes.byref(nb)) == -1 and b"N H W >= 2" in L.clica_last_error()
    assert L.clica_bn2d_maxpool_workspace_bytes(0, 8, 4, 4, ctypes.byref(nb)) == -1 and b"N=0" in L.clica_last_error()
    assert L.clica_bn2d_maxpool_workspace_bytes(4, 8, 0, 4, ctypes.byref(nb)) == -1 and b"H=0" in L.clica_last_error()
    assert L.clica_bn2d_maxpool_workspace_bytes(4, 8, 4, 4, None) == -1 and b"bytes is NULL" in L.clica_last_error()


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    L = lib()
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    fwd = lambda N, H, W, slope, q, ws, nbytes: L.clica_bn2d_act_maxpool_fwd_train(q, q, q, N, 8, H, W, 1e-5, 0.1, slope, q, q, q, None, None,
                                                                                   ws, nbytes, None)
    bwd = lambda N, H, W, slope, q, ws, nbytes: L.clica_bn2d_act_maxpool_bwd(q, q, q, q, q, q, N, 8, H, W, slope, q, q, q, ws, nbytes, None)
    ev = lambda N, H, W, slope, q: L.clica_bn2d_act_maxpool_fwd_eval(q, q, q, q, q, N, 8, H, W, 1e-5, slope, q, None)
    for name, call in ((b"fwd_train", fwd), (b"bwd", bwd)):
        assert call(1, 130, 130, 0.0, p, p, 1 << 20) == -1 and b"over the limit" in L.clica_last_error() and name in L.clica_last_error()
        assert call(1, 1, 1, 0.0, p, p, 1 << 20) == -1 and b"N H W >= 2" in L.clica_last_error()
        assert call(4, 4, 4, 1.5, p, p, 1 << 20) == -1 and b"slope=1.5" in L.clica_last_error()
        assert call(4, 4, 4, -0.1, p, p, 1 << 20) == -1 and b"slope" in L.clica_last_error()
        assert call(4, 4, 4, 0.0, None, p, 1 << 20) == -1 and b"NULL pointer" in L.clica_last_error()
        assert call(4, 4, 4, 0.0, p, None, 1 << 20) == -1 and b"NULL pointer" in L.clica_last_error()
        assert call(4, 4, 4, 0.0, p, p + 4, 1 << 20) == -1 and b"16-byte aligned" in L.clica_last_error()
        assert call(4, 4, 4, 0.0, p, p, 0) == -2 and b"workspace of 0 bytes" in L.clica_last_error()          # CLICA_E_WORKSPACE
    assert ev(1, 130, 130, 0.0, p) == -1 and b"over the limit" in L.clica_last_error()
    assert ev(4, 4, 4, 1.5, p) == -1 and b"slope=1.5" in L.clica_last_error()
    assert ev(1, 1, 1, 0.0, None) == -1 and b"NULL pointer" in L.clica_last_error()          # one value: inference is fine
    for call in (L.clica_avgpool2d_global_fwd, L.clica_avgpool2d_global_bwd):
        assert call(p, 0, 4, p, None) == -1 and b"rows=0" in L.clica_last_error()
        assert call(p, 8, 0, p, None) == -1 and b"HW=0" in L.clica_last_error()
        assert call(p, 8, (1 << 14) + 1, p, None) == -1
        assert call(None, 8, 4, p, None) == -1 and b"NULL pointer" in L.clica_last_error()


def test_output_size_of_the_wrapper_is_torchs():
    from cl_ica_amd import ops
    for H in range(1, 10):
        for W in range(1, 10):
            assert ops.maxpool_out_hw(H, W) == tuple(F.max_pool2d(torch.zeros(1, 1, H, W), 3, 2, 1).shape[2:]) == Q.out_hw(H, W)
    assert ops.bn2d_maxpool_fits(112, 112) and ops.bn2d_maxpool_fits(32, 32) and ops.bn2d_maxpool_fits(1, 1)
    assert not ops.bn2d_maxpool_fits(130, 130) and not ops.bn2d_maxpool_fits(113, 112)
    nb = ctypes.c_size_t()
    for (H, W) in [(112, 112), (113, 112), (1, 12544), (1, 10453), (1, 10454), (130, 130), (125, 100), (126, 100)]:      # the same limit on both sides
        assert ops.bn2d_maxpool_fits(H, W) == (lib().clica_bn2d_maxpool_workspace_bytes(2, 3, H, W, ctypes.byref(nb)) == 0), (H, W)


def test_ops_wrappers_refuse_other_inputs():
    from cl_ica_amd import ops
    x = torch.randn(4, 8, 6, 6)
    w, b = torch.ones(8), torch.zeros(8)
    with pytest.raises(ValueError, match="contiguous NCHW"):
        ops.batchnorm2d_act_maxpool_fwd(x.contiguous(memory_format=torch.channels_last), w, b)
    with pytest.raises(ValueError, match="contiguous NCHW"):
        ops.batchnorm2d_act_maxpool_eval(x[:, :, :, :3], w, b, b, w)
    with pytest.raises(ValueError, match="contiguous NCHW"):
        ops.avgpool2d_global_fwd(x.permute(0, 1, 3, 2))
    with pytest.raises(ValueError, match="contiguous matrix"):
        ops.avgpool2d_global_bwd(torch.ones(4, 8, 1, 1), 6, 6)


@pytest.mark.parametrize("train", [True, False])
def test_cpu_tensors_fall_through_to_torch_modules(monkeypatch, train):
    from cl_ica_amd import resnet
    assert resnet.POOL_MODE in ("hip", "torch")
    torch.manual_seed(5)
    base = resnet.resnet18(num_classes=30)
    x = torch.randn(2, 3, 64, 64)
    raw = lambda t: np.ascontiguousarray(t.detach().numpy()).reshape(-1).view(np.uint8)
    out = {}
    for mode in ("hip", "torch"):
        monkeypatch.setattr(resnet, "NORM_MODE", "hip")
        monkeypatch.setattr(resnet, "POOL_MODE", mode)
        import copy
        f = copy.deepcopy(base).train(train)
        y = f(x)
        y.square().sum().backward()
        out[mode] = [y] + [p.grad for p in f.parameters()] + [b.float() for b in f.buffers()]
    for a, b in zip(out["hip"], out["torch"]):
        assert np.array_equal(raw(a), raw(b))
