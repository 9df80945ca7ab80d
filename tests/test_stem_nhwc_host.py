"""Host-side checks of the channels-last stem unit (csrc/bn2d_nhwc.hip), no GPU: the caps every case of tests/stem_nhwc_cases.py
satisfies, from the fp64 oracle alone; the four entry points in the header, in _lib.SIGNATURES and in the built library; the accept /
refuse codes of the host-only workspace entry and of the launching ones; ops.bn2d_nhwc_maxpool_fits against the library; the wrappers'
refusals; the default and the validation of resnet.NHWC_STEM_MODE."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import pool2d_oracle as Q
import stem_nhwc_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("clica_bn2d_nhwc_maxpool_workspace_bytes", "clica_bn2d_nhwc_act_maxpool_fwd_train", "clica_bn2d_nhwc_act_maxpool_fwd_eval",
           "clica_bn2d_nhwc_act_maxpool_bwd")


def lib():
    from cl_ica_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_case_satisfies_its_caps(shape):
    for cls in range(len(K.CLASSES)):
        frac, kap, gap = Q.case_ok(*shape, cls, K.attempt(shape, cls))
        assert frac <= Q.MAX_LEFT_OUT, (shape, cls, frac)
        assert kap <= Q.MAX_KAPPA, (shape, cls, kap)
        assert gap >= Q.MIN_GAP_REL, (shape, cls, gap)
        c = K.make_case(shape, cls)
        assert c["x"].shape == (shape[0] * shape[2] * shape[3], shape[1])          # rows [N H W, C]: the NHWC memory
        assert 0.25 <= np.abs(c["gamma"]).min() and np.abs(c["gamma"]).max() <= 1.5


def test_the_case_tables_are_consistent():
    assert Q.SEED_ATTEMPT == {}                                                    # the helper carries its own table and leaves the oracle's alone
    assert all(k[:4] in K.SHAPES and 0 <= k[4] < len(K.CLASSES) for k in K.ATTEMPT)
    for sub in (K.TIE_SHAPES, K.EVAL_SHAPES, K.UNALIGNED_SHAPES, [K.GRAPH_SHAPE]):
        assert set(sub) <= set(K.SHAPES)
    assert all(C % 4 == 0 for (_, C, _, _) in K.UNALIGNED_SHAPES)
    # the tie class does hold exact ties inside windows
    shape = (2, 8, 5, 5)
    _, fw, _ = K.reference(shape, K.TIE_CLASS, 1.0)
    win = Q.windows(Q.to_nchw(fw["y"], *shape))
    assert ((win == win.max(0)).sum(0) > 1).any()


def test_header_signatures_and_library_agree():
    from cl_ica_amd import _lib
    header = open(os.path.join(ROOT, "include", "clica.h")).read()
    L = lib()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
    nchw = {n: _lib.SIGNATURES[n.replace("_nhwc", "")] for n in ENTRIES}           # the arguments of the NCHW namesakes
    for name in ENTRIES:
        assert len(_lib.SIGNATURES[name]) == len(nchw[name]) and all(a is b for a, b in zip(_lib.SIGNATURES[name], nchw[name])), name


def test_workspace_entry_point_accepts_and_refuses():
    L = lib()
    nb = ctypes.c_size_t()
    fn = L.clica_bn2d_nhwc_maxpool_workspace_bytes
    for (N, C, H, W) in K.SHAPES + [(1024, 64, 32, 32), (256, 64, 112, 112), (2, 64, 300, 200)]:
        nb.value = 0
        assert fn(N, C, H, W, ctypes.byref(nb)) == 0, (N, C, H, W)
        assert nb.value >= 16 and nb.value % 16 == 0 and nb.value <= 3 * 256 * 4 * C + 16
    assert fn(1, 8, 1, 1, ctypes.byref(nb)) == -1 and b"N H W >= 2" in L.clica_last_error()
    assert fn(4, 0, 4, 4, ctypes.byref(nb)) == -1 and b"C=0" in L.clica_last_error()
    assert fn(4, 8, 0, 4, ctypes.byref(nb)) == -1 and b"H=0" in L.clica_last_error()
    assert fn(4, 8, 4, 0, ctypes.byref(nb)) == -1 and b"W=0" in L.clica_last_error()
    assert fn(0, 8, 4, 4, ctypes.byref(nb)) == -1 and b"N=0" in L.clica_last_error()
    assert fn(4, 8, 4, 4, None) == -1 and b"bytes is NULL" in L.clica_last_error()
    assert fn(1, 8, 4, (1 << 15) + 1, ctypes.byref(nb)) == -1 and fn(1, 8, 4, 1 << 15, ctypes.byref(nb)) == 0


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    L = lib()
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    fwd = lambda N, H, W, slope, q, ws, nbytes: L.clica_bn2d_nhwc_act_maxpool_fwd_train(q, q, q, N, 8, H, W, 1e-5, 0.1, slope, q, q, q, None,
                                                                                        None, ws, nbytes, None)
    bwd = lambda N, H, W, slope, q, ws, nbytes: L.clica_bn2d_nhwc_act_maxpool_bwd(q, q, q, q, q, q, N, 8, H, W, slope, q, q, q, ws, nbytes, None)
    ev = lambda N, H, W, slope, q: L.clica_bn2d_nhwc_act_maxpool_fwd_eval(q, q, q, q, q, N, 8, H, W, 1e-5, slope, q, None)
    for name, call in ((b"fwd_train", fwd), (b"bwd", bwd)):
        assert call(1, 1, 1, 0.0, p, p, 1 << 20) == -1 and b"N H W >= 2" in L.clica_last_error() and name in L.clica_last_error()
        assert call(4, 4, 4, 1.5, p, p, 1 << 20) == -1 and b"slope=1.5" in L.clica_last_error()
        assert call(4, 4, 4, -0.1, p, p, 1 << 20) == -1 and b"slope" in L.clica_last_error()
        assert call(4, 4, 4, 0.0, None, p, 1 << 20) == -1 and b"NULL pointer" in L.clica_last_error()
        assert call(4, 4, 4, 0.0, p, None, 1 << 20) == -1 and b"NULL pointer" in L.clica_last_error()
        assert call(4, 4, 4, 0.0, p, p + 4, 1 << 20) == -1 and b"16-byte aligned" in L.clica_last_error()
        assert call(4, 4, 4, 0.0, p, p, 0) == -2 and b"workspace of 0 bytes" in L.clica_last_error()          # CLICA_E_WORKSPACE
    assert ev(4, 4, 4, 1.5, p) == -1 and b"slope=1.5" in L.clica_last_error()
    assert ev(4, 4, 4, -0.1, p) == -1 and b"slope" in L.clica_last_error()
    assert ev(1, 1, 1, 0.0, None) == -1 and b"NULL pointer" in L.clica_last_error()          # one value: inference is fine
    assert ev(1, 0, 1, 0.0, p) == -1 and b"H=0" in L.clica_last_error()


def test_fits_agrees_with_the_library():
    from cl_ica_amd import ops
    L = lib()
    nb = ctypes.c_size_t()
    rng = np.random.default_rng(5)
    side = lambda: int(rng.choice([0, 1, 2, 7, 112, 113, 1 << 15, (1 << 15) + 1, int(rng.integers(1, 1 << 16))]))
    chan = lambda: int(rng.choice([0, 1, 3, 64, 1 << 20, (1 << 20) + 1, int(rng.integers(1, 1 << 21))]))
    seen = set()
    for _ in range(300):
        H, W, C = side(), side(), chan()
        fits = ops.bn2d_nhwc_maxpool_fits(H, W, C)
        assert fits == (L.clica_bn2d_nhwc_maxpool_workspace_bytes(2, C, H, W, ctypes.byref(nb)) == 0), (H, W, C)
        seen.add(fits)
    assert seen == {True, False}
    assert all(ops.bn2d_nhwc_maxpool_fits(H, W, 64) for H in range(1, 113) for W in (1, 31, 112))      # every plane up to 112 x 112 at C = 64
    assert ops.bn2d_nhwc_maxpool_fits(130, 130, 64)                                                    # no limit from LDS in this layout


def test_ops_wrappers_refuse_other_inputs():
    from cl_ica_amd import ops
    x = torch.randn(4, 8, 6, 6)
    w, b = torch.ones(8), torch.zeros(8)
    cl = x.contiguous(memory_format=torch.channels_last)
    with pytest.raises(ValueError, match="dense channels-last"):
        ops.batchnorm2d_act_maxpool_fwd_nhwc(x, w, b)
    with pytest.raises(ValueError, match="dense channels-last"):
        ops.batchnorm2d_act_maxpool_eval_nhwc(cl[:, :, :, :3], w, b, b, w)
    with pytest.raises(ValueError, match="dense channels-last"):
        ops.batchnorm2d_act_maxpool_bwd_nhwc(cl, torch.zeros(4, 8, 3, 3), w, b, b, w)      # dp in the other layout
    with pytest.raises(ValueError, match="shape of x"):
        ops.batchnorm2d_act_maxpool_bwd_nhwc(cl, cl, w, b, b, w)                           # dp must be [N, C, Ho, Wo]
    with pytest.raises(ValueError, match="8 contiguous values"):
        ops.batchnorm2d_act_maxpool_fwd_nhwc(cl, w[:3], b)
    with pytest.raises(ValueError, match="come together"):
        ops.batchnorm2d_act_maxpool_fwd_nhwc(cl, w, b, running_mean=b)


def test_the_switch_defaults_to_torch_and_is_validated():
    from cl_ica_amd import resnet
    assert resnet.NHWC_STEM_MODE == os.environ.get("CLICA_RESNET_NHWC_STEM", "torch")
    assert "CLICA_RESNET_NHWC_STEM" in os.environ or resnet.NHWC_STEM_MODE == "torch"
    # a bad value raises at import: a fresh child process (one: importing the package takes seconds)
    env = dict(os.environ, CLICA_RESNET_NHWC_STEM="cuda", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    bad = subprocess.run([sys.executable, "-c", "from cl_ica_amd import resnet"], env=env, capture_output=True, text=True)
    assert bad.returncode != 0 and "CLICA_RESNET_NHWC_STEM='cuda'" in bad.stderr, bad.stderr


def test_cpu_and_default_paths_are_unchanged(monkeypatch):
    """The switch alone changes nothing on the CPU, where no kernel applies: the backbone has the bits of NHWC_STEM_MODE "torch"."""
    import copy
    from cl_ica_amd import resnet
    torch.manual_seed(5)
    base = resnet.resnet18(num_classes=30).to(memory_format=torch.channels_last)
    x = torch.randn(2, 3, 64, 64).contiguous(memory_format=torch.channels_last)
    raw = lambda t: np.ascontiguousarray(t.detach().numpy()).reshape(-1).view(np.uint8)
    out = {}
    for mode in ("hip", "torch"):
        for name in ("NORM_MODE", "POOL_MODE", "NHWC_MODE"):
            monkeypatch.setattr(resnet, name, "hip")
        monkeypatch.setattr(resnet, "NHWC_STEM_MODE", mode)
        f = copy.deepcopy(base).train()
        y = f(x)
        y.square().sum().backward()
        out[mode] = [y] + [p.grad for p in f.parameters()] + [b.float() for b in f.buffers()]
    for a, b in zip(out["hip"], out["torch"]):
        assert np.array_equal(raw(a), raw(b))
