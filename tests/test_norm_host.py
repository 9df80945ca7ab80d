"""Host side of the fused BatchNorm1d / GroupNorm + LeakyReLU kernels (csrc/norm.hip): the fp64 oracle against torch's own fp64
autograd, the attainability of the GPU test's bound by torch's fp32 on the CPU, the G27 golden against the oracle, and the host-only
part of the C ABI.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import norm_oracle as O
from conftest import GOLDEN, ROOT, formula_weights

TOL = 1e-5
CASES = [(kind,) + c for kind in ("bn", "gn") for c in O.sweep(kind)]


def torch_reference(kind, c, slope, dtype):
    """The same case through torch's functional norms and autograd on the CPU."""
    F = torch.nn.functional
    t = {k: torch.tensor(v, dtype=dtype) for k, v in c.items()}
    x, w, b = t["x"].requires_grad_(True), t["gamma"].requires_grad_(True), t["beta"].requires_grad_(True)
    if kind == "bn":
        z = F.batch_norm(x, t["running_mean"], t["running_var"], w, b, True, O.MOMENTUM, O.EPS)
    else:
        z = F.group_norm(x, 1, w, b, O.EPS)
    y = F.leaky_relu(z, slope)
    y.backward(t["dy"])
    out = dict(y=y.detach().numpy(), dx=x.grad.numpy(), dgamma=w.grad.numpy(), dbeta=b.grad.numpy())
    if kind == "bn":
        out.update(running_mean=t["running_mean"].numpy(), running_var=t["running_var"].numpy())
    return out


def compare(kind, M, C_, got, fw, bw, slope):
    """Norm-wise errors of `got` against the oracle with the near-kink columns / rows left out of dx, dgamma, dbeta."""
    cols, rows = O.left_out(kind, fw["z"], slope)
    errs = dict(y=O.norm_err(got["y"], fw["y"]))
    if not (kind == "bn" and M == 2):          # dx at M = 2 is ill-conditioned: xhat = +-1 and dx is a difference that cancels
        keep = np.ix_(~rows, ~cols) if kind == "bn" else np.ix_(~rows, np.ones(C_, bool))
        errs["dx"] = O.norm_err(got["dx"][keep], bw["dx"][keep])
    errs["dgamma"] = O.norm_err(got["dgamma"][~cols], bw["dgamma"][~cols])
    errs["dbeta"] = O.norm_err(got["dbeta"][~cols], bw["dbeta"][~cols])
    for k in ("running_mean", "running_var"):
        if k in got:
            errs[k] = O.norm_err(got[k], fw[k])
    return errs


@pytest.fixture(scope="module")
def references():
    cache = {}

    def get(kind, M, C_, cls, slope):
        key = (kind, M, C_, cls, slope)
        if key not in cache:
            cache[key] = O.reference(kind, M, C_, cls, slope)
        return cache[key]

    return get


# ------------------------------------------------------------------------------------------------ 1. the oracle itself
@pytest.mark.parametrize("kind,M,C_,cls,slope", CASES)
def test_oracle_matches_torch_fp64_autograd(kind, M, C_, cls, slope, references):
    c, fw, bw = references(kind, M, C_, cls, slope)
    ref = torch_reference(kind, c, slope, torch.float64)
    for k, v in ref.items():
        want = fw[k] if k in fw else bw[k]
        assert O.norm_err(v, want) <= 1e-12, (k, O.norm_err(v, want))


# ------------------------------------------------------------------------------------------------ 2. the bound is attainable
@pytest.mark.parametrize("kind,M,C_,cls,slope", CASES)
def test_torch_fp32_meets_the_gpu_criterion(kind, M, C_, cls, slope, references):
    c, fw, bw = references(kind, M, C_, cls, slope)
    assert O.left_out_fraction(kind, fw["z"], slope) <= O.MAX_LEFT_OUT
    assert O.kappa(kind, c["x"]) <= O.MAX_KAPPA
    errs = compare(kind, M, C_, torch_reference(kind, c, slope, torch.float32), fw, bw, slope)
    assert all(e < TOL for e in errs.values()), errs


def test_near_kink_helper_marks_columns_and_rows():
    z = np.ones((4, 5)); z[2, 3] = 1e-7; z[0, 0] = -1e3
    cols, rows = O.left_out("bn", z, 0.01)
    assert cols.tolist() == [False, False, False, True, False] and not rows.any()
    cols, rows = O.left_out("gn", z, 0.0)
    assert rows.tolist() == [False, False, True, False] and cols.tolist() == [False, False, False, True, False]
    assert not any(m.any() for m in O.left_out("gn", z, 1.0))          # no kink without an activation


# ------------------------------------------------------------------------------------------------ 3. G27
def g27_params(dims):
    """The formula parameters of the golden's network in named_parameters() order: Linear weight, bias, norm weight (+ 1), bias."""
    Ws, bs, gammas, betas = [], [], [], []
    k = 0
    for l in range(len(dims) - 1):
        Ws.append(formula_weights((dims[l + 1], dims[l]), k + 1)); k += 1
        bs.append(formula_weights((dims[l + 1],), k + 1)); k += 1
        if l < len(dims) - 2:
            gammas.append(formula_weights((dims[l + 1],), k + 1) + np.float32(1.0)); k += 1
            betas.append(formula_weights((dims[l + 1],), k + 1)); k += 1
    return Ws, bs, gammas, betas


@pytest.mark.parametrize("mode", ["bn", "gn"])
def test_g27_loads_and_its_fp64_entries_agree_with_the_oracle(mode):
    z = np.load(os.path.join(GOLDEN, "g27_mlp_norm.npz"), allow_pickle=False)
    dims = [5, 7, 65, 24, 3]
    Ws, bs, gammas, betas = g27_params(dims)
    names = []
    for l in range(len(dims) - 1):
        names += [f"{3 * l}.weight", f"{3 * l}.bias"] + ([f"{3 * l + 1}.weight", f"{3 * l + 1}.bias"] if l < len(dims) - 2 else [])
    running = [(np.zeros(d), np.ones(d)) for d in dims[1:-1]] if mode == "bn" else None
    for k in range(2):
        assert z[f"x{k}"].shape == (65, 5) and z[f"x{k}"].dtype == np.float32
        y, dx, grads, running_new = O.mlp_train_pass(mode, Ws, bs, gammas, betas, z[f"x{k}"], z[f"c{k}"], running=running)
        assert O.norm_err(y, z[f"{mode}/p{k}/y64"]) < 1e-11 and O.norm_err(dx, z[f"{mode}/p{k}/dx64"]) < 1e-11
        assert z[f"{mode}/p{k}/y32"].dtype == np.float32 and O.norm_err(z[f"{mode}/p{k}/y32"], y) < TOL
        wfloor = {}
        for name, g in zip(names, grads):
            ref = z[f"{mode}/p{k}/grad/{name}64"]
            idx, leaf = name.split(".")
            if leaf == "weight":
                wfloor[idx] = float(np.abs(ref).max())
            # (a Linear bias in front of a norm has a zero gradient: rounding noise on both sides, measured against its weight's scale)
            assert O.norm_err(g.reshape(ref.shape), ref, floor=wfloor[idx] if leaf == "bias" and int(idx) % 3 == 0 else 0.0) < 1e-11, (name, k)
            assert f"{mode}/p{k}/grad/{name}32" in z.files
        if mode == "bn":
            running = running_new
            for l, (rm, rv) in enumerate(running):
                assert O.norm_err(rm, z[f"bn/p{k}/buf/{3 * l + 1}.running_mean64"]) < 1e-11
                assert O.norm_err(rv, z[f"bn/p{k}/buf/{3 * l + 1}.running_var64"]) < 1e-11
                assert int(z[f"bn/p{k}/buf/{3 * l + 1}.num_batches_tracked64"]) == k + 1
    y_eval = O.mlp_eval(mode, Ws, bs, gammas, betas, z["x0"], running=running)
    assert O.norm_err(y_eval, z[f"{mode}/y_eval64"]) < 1e-11


# ------------------------------------------------------------------------------------------------ 4. C ABI, host-only part
NEW = ("clica_bn_lrelu_fwd_train", "clica_bn_lrelu_fwd_eval", "clica_bn_lrelu_bwd", "clica_gn_lrelu_fwd", "clica_gn_lrelu_bwd",
       "clica_norm_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    from cl_ica_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_new_entry_points_are_declared_and_bound():
    from cl_ica_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clica.h")).read(), flags=re.S)
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert re.search(rf"\b{name}\s*\(", header), name


def test_workspace_planner_on_the_sweep_shapes(lib):
    nb = C.c_size_t()
    for kind, code, shapes in (("bn", 0, O.BN_SHAPES), ("gn", 1, O.GN_SHAPES)):
        for (M, C_) in shapes:
            assert lib.clica_norm_workspace_bytes(code, M, C_, 0.01, C.byref(nb)) == 0, (kind, M, C_)
            # partial rows of C floats: at most 64 splits x 3 planes (batch norm), 512 wave slots x 2 planes (group norm)
            assert 4 * C_ <= nb.value <= 4 * C_ * 1024 and nb.value % 4 == 0, (kind, M, C_, nb.value)


def test_workspace_planner_refuses_what_the_kernels_do_not_cover(lib):
    nb = C.c_size_t(12345)
    assert lib.clica_norm_workspace_bytes(0, 1, 8, 0.01, C.byref(nb)) == -1 and b"M=1" in lib.clica_last_error()
    assert lib.clica_norm_workspace_bytes(1, 1, 8, 0.01, C.byref(nb)) == 0                 # one row is a group norm's business
    nb = C.c_size_t(12345)
    for code in (0, 1):
        assert lib.clica_norm_workspace_bytes(code, 8, 0, 0.01, C.byref(nb)) == -1 and b"C=0" in lib.clica_last_error()
        assert lib.clica_norm_workspace_bytes(code, 8, 8, -0.5, C.byref(nb)) == -1 and b"slope" in lib.clica_last_error()
    assert lib.clica_norm_workspace_bytes(2, 8, 8, 0.01, C.byref(nb)) == -1 and b"kind" in lib.clica_last_error()
    assert lib.clica_norm_workspace_bytes(0, 8, 8, 0.01, None) == -1
    assert nb.value == 12345                                                               # a refusal writes nothing


def test_compute_entry_points_validate_before_any_launch(lib):
    """Shape and slope are checked first, pointers next: with bad arguments the calls return -1 on a host without a GPU."""
    assert lib.clica_bn_lrelu_fwd_train(None, None, None, 1, 8, 1e-5, 0.1, 0.01, None, None, None, None, None, None, 0, None) == -1
    assert b"M=1" in lib.clica_last_error()
    assert lib.clica_bn_lrelu_bwd(None, None, None, None, None, None, 8, 8, -1.0, None, None, None, None, 0, None) == -1
    assert b"slope" in lib.clica_last_error()
    assert lib.clica_gn_lrelu_fwd(None, None, None, 8, 0, 1e-5, 0.01, None, None, None, None) == -1
    assert b"C=0" in lib.clica_last_error()
    assert lib.clica_gn_lrelu_bwd(None, None, None, None, None, None, 8, 8, 0.01, None, None, None, None, 0, None) == -1
    assert b"NULL" in lib.clica_last_error()
    assert lib.clica_bn_lrelu_fwd_eval(None, None, None, None, None, 8, 8, 1e-5, -0.01, None, None) == -1
    assert b"slope" in lib.clica_last_error()
