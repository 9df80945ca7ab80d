"""The p = 0 (dot-product InfoNCE) engine step without a GPU: the dot kind's training pair is declared, bound and exported, its host-side
argument checks fail loudly before any launch, and ContrastiveTrainer no longer refuses p = 0."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "clica.h")
NEW = ("clica_dot_loss_train_workspace_bytes", "clica_dot_loss_fwd_train", "clica_dot_loss_bwd_sym_train")


@pytest.fixture(scope="module")
def lib():
    from cl_ica_amd import _lib
    return _lib.load()


def _desc(B=256, B3=256, n=10, tau=1.0, alpha=0.5, normalize=0):
    from cl_ica_amd import _lib
    return _lib.DotLossDesc(B=B, B3=B3, n=n, tau=tau, alpha=alpha, normalize=normalize)


def test_dot_train_entry_points_declared_bound_exported(lib):
    from cl_ica_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    # the pair takes the existing dot descriptor
    for name in NEW:
        assert _lib.SIGNATURES[name][0] is ctypes.POINTER(_lib.DotLossDesc), name


def test_dot_train_workspace_query(lib):
    nb = ctypes.c_size_t()
    d = _desc(B=6144, B3=6144, n=10)
    assert lib.clica_dot_loss_train_workspace_bytes(ctypes.byref(d), ctypes.byref(nb)) == 0
    # at least the backward's per-split partials of a B x n gradient, and the forward's (max, sum) partials
    assert 6144 * 10 * 4 + 6144 * 8 <= nb.value < 64 << 20
    big = ctypes.c_size_t()
    d4 = _desc(B=6144, B3=4 * 6144, n=10)
    assert lib.clica_dot_loss_train_workspace_bytes(ctypes.byref(d4), ctypes.byref(big)) == 0
    assert big.value >= nb.value
    for bad, msg in ((_desc(n=65), b"n=65"), (_desc(n=0), b"n=0"), (_desc(B3=128), b"B3=128"), (_desc(tau=0.0), b"tau"),
                     (_desc(normalize=1), b"normalize")):
        assert lib.clica_dot_loss_train_workspace_bytes(ctypes.byref(bad), ctypes.byref(nb)) == -1
        assert msg in lib.clica_last_error(), msg
    assert lib.clica_dot_loss_train_workspace_bytes(ctypes.byref(d), None) == -1


def test_dot_train_launch_argument_checks_fail_loudly(lib):
    """Every check runs on the host before anything is launched: dummy device addresses never reach a kernel."""
    d = _desc()
    nb = ctypes.c_size_t()
    assert lib.clica_dot_loss_train_workspace_bytes(ctypes.byref(d), ctypes.byref(nb)) == 0
    P = 1 << 20          # (never dereferenced: the calls return before any launch)

    def fwd(ld1=10, ldp=10, ldd=10, z1=P, ws_bytes=nb.value):
        return lib.clica_dot_loss_fwd_train(ctypes.byref(d), z1, ld1, P, 10, P, ldp, P, P, P, P, ldd, P, ldd, P, ws_bytes, None)

    def bwd(ld1=10, ldd=10, pool_lse=P, ws_bytes=nb.value):
        return lib.clica_dot_loss_bwd_sym_train(ctypes.byref(d), P, ld1, P, 10, P, pool_lse, P, ldd, P, None, P, ws_bytes, None)

    assert fwd(ld1=9) == -1 and b"leading dimension" in lib.clica_last_error()
    assert fwd(ldp=3) == -1 and b"leading dimension" in lib.clica_last_error()
    assert fwd(ldd=4) == -1 and b"leading dimension" in lib.clica_last_error()
    assert fwd(z1=None) == -1 and b"NULL" in lib.clica_last_error()
    assert fwd(ws_bytes=nb.value - 4) == -2 and b"workspace" in lib.clica_last_error()
    assert bwd(ld1=2) == -1 and b"leading dimension" in lib.clica_last_error()
    assert bwd(ldd=2) == -1 and b"leading dimension" in lib.clica_last_error()
    assert bwd(pool_lse=None) == -1 and b"NULL" in lib.clica_last_error()
    assert bwd(ws_bytes=16) == -2 and b"workspace" in lib.clica_last_error()


def test_contrastive_trainer_plans_the_dot_train_pair_for_p0():
    """The constructor used to raise NotImplementedError for p = 0.  Now it plans the step -- host work only, so a CPU device will do: the
    dot kind's descriptor with the caller's tau / alpha and no normalisation, a zero-filled workspace of the size the library asks for,
    the early tick, and the neutral guard reports (the dot logits need no spread guard)."""
    import torch
    from cl_ica_amd import _lib
    from cl_ica_amd.engine import ContrastiveTrainer, SamplerSpec
    f = torch.nn.Sequential(torch.nn.Linear(4, 4))
    tr = ContrastiveTrainer(f, torch.eye(4).repeat(3, 1, 1), SamplerSpec(space="sphere", n=4), batch_size=8, p=0, tau=0.5, alpha=0.3,
                            device="cpu")
    assert tr.dot and tr.loss_train and tr.early_tick
    assert isinstance(tr.desc, _lib.DotLossDesc)
    assert (tr.desc.B, tr.desc.B3, tr.desc.n, tr.desc.normalize) == (8, 8, 4, 0)
    assert tr.desc.tau == pytest.approx(0.5) and tr.desc.alpha == pytest.approx(0.3)
    nb = ctypes.c_size_t()
    assert _lib.load().clica_dot_loss_train_workspace_bytes(ctypes.byref(tr.desc), ctypes.byref(nb)) == 0
    assert tr.loss_ws.numel() == nb.value and int(tr.loss_ws.abs().sum()) == 0
    ps = tr.plan_summary()
    assert ps["loss_entry_points"] == "dot train pair" and ps["pool_rows"] == 8
    assert tr.loss_guard() == dict(max_spread=0.0, last_spread=0.0, limit=0.0, fallback_steps=0) and tr.loss_spread() == 0.0
    # p >= 1 keeps the Lp descriptor
    lp = ContrastiveTrainer(torch.nn.Sequential(torch.nn.Linear(4, 4)), torch.eye(4).repeat(3, 1, 1), SamplerSpec(n=4), batch_size=8, p=2,
                            device="cpu")
    assert not lp.dot and isinstance(lp.desc, _lib.LpLossDesc) and lp.plan_summary()["loss_entry_points"] == "train pair"
