"""R2Loss and the supervised 3DIdent step, the parts that need no GPU: the fp64 oracle against the reference's fp64 goldens, the
Python surface (constructor defaults, the bad-mode assertion, loss selection) and the C ABI's declarations."""
import argparse
import os
import re

import numpy as np
import pytest

import r2_oracle
from conftest import ROOT

REDUCTIONS = ("none", "mean", "sum")
MODES = ("r2", "negative_r2")


def case_inputs(c):
    """(y_pred, y) of a golden case as numpy views (the strided case: the leading columns of its base arrays)."""
    if str(c["meta"]["kind"]) == "strided":
        k = int(c["meta"]["cols"])
        return c["in"]["y_pred_base"][:, :k], c["in"]["y_base"][:, :k]
    return c["in"]["y_pred"], c["in"]["y"]


def test_oracle_matches_reference_fp64(golden):
    g = golden("g26_r2loss.npz")
    assert g.n_cases == 9
    g_scalar = float(g.z["g_scalar"])
    seen = set()
    for key, c in g.cases():
        kind = str(c["meta"]["kind"])
        seen.add(kind)
        y_pred, y = case_inputs(c)
        stride = int(c["meta"]["grad_stride"])
        for red in REDUCTIONS:
            for mode in MODES:
                want = c["out"][f"{red}/{mode}/out64"]
                got = np.asarray(r2_oracle.r2_value(y_pred, y, red, mode))
                assert got.shape == want.shape
                if kind == "degenerate":
                    assert not np.isfinite(want).any()
                    np.testing.assert_array_equal(got, want)        # the same +-inf pattern
                    assert f"{red}/{mode}/grad64" not in c["out"]
                    continue
                np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
                up = c["in"]["g_none"] if red == "none" else g_scalar
                grad = r2_oracle.r2_grad(y_pred, y, up, red, mode).reshape(-1)[::stride]
                want_g = c["out"][f"{red}/{mode}/grad64"].reshape(-1)
                np.testing.assert_allclose(grad, want_g, rtol=1e-12, atol=1e-12 * np.abs(want_g).max())
    assert seen == {"plain", "strided", "degenerate"}


def test_golden_fp32_reference_is_close_to_fp64(golden):
    """The reference's own fp32 deviation (what the 1e-5 contract has to leave room for) stays below 1e-6, offset cases included."""
    for key, c in golden("g26_r2loss.npz").cases():
        if str(c["meta"]["kind"]) == "degenerate":
            continue
        for red in REDUCTIONS:
            for mode in MODES:
                for what in ("out", "grad"):
                    a, b = c["out"][f"{red}/{mode}/{what}32"].astype(np.float64), c["out"][f"{red}/{mode}/{what}64"]
                    assert np.max(np.abs(a - b)) <= 1e-6 * np.max(np.abs(b)), (key, red, mode, what)


def test_r2loss_surface():
    from cl_ica_amd import losses
    l = losses.R2Loss()
    assert (l.reduction, l.mode) == ("none", "negative_r2")
    l = losses.R2Loss("mean", "r2")
    assert (l.reduction, l.mode) == ("mean", "r2")
    l = losses.R2Loss(reduction="sum", mode="negative_r2")
    assert (l.reduction, l.mode) == ("sum", "negative_r2")
    with pytest.raises(AssertionError):
        losses.R2Loss(mode="neg_r2")
    assert callable(l) and callable(l.forward)
    assert "R2Loss" in losses.__all__


def test_make_supervised_loss():
    from cl_ica_amd import losses, threedident
    assert "make_supervised_loss" in threedident.__all__ and "train_step_supervised" in threedident.__all__
    l = threedident.make_supervised_loss(argparse.Namespace(supervised_loss="r2"))
    assert isinstance(l, losses.R2Loss) and (l.reduction, l.mode) == ("mean", "negative_r2")
    m = threedident.make_supervised_loss(argparse.Namespace(supervised_loss="mse"))
    assert callable(m) and not isinstance(m, losses.R2Loss) and m.reduction == "mean"
    with pytest.raises(ValueError):
        threedident.make_supervised_loss(argparse.Namespace(supervised_loss="huber"))


def test_abi_names_declared_and_bound():
    from cl_ica_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clica.h")).read(), flags=re.S)
    for name in ("clica_r2_loss_workspace_bytes", "clica_r2_loss_fwd", "clica_r2_loss_bwd"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["clica_r2_loss_fwd"]) == 14 and len(_lib.SIGNATURES["clica_r2_loss_bwd"]) == 13


def test_workspace_query_validates_on_the_host():
    """The planning entry point is host code: it answers (and refuses) without a GPU."""
    import ctypes
    from cl_ica_amd import _lib
    L = _lib.load()
    nb = ctypes.c_size_t()
    for M, n in ((1, 1), (64, 10), (4099, 40), (65, 256), (1 << 20, 256)):
        assert L.clica_r2_loss_workspace_bytes(M, n, ctypes.byref(nb)) == 0
        assert 256 < nb.value <= 256 + 128 * n * 16, (M, n, nb.value)          # at most 128 wave slots of four floats per column
    for M, n in ((0, 3), (5, 0), (5, 257)):
        assert L.clica_r2_loss_workspace_bytes(M, n, ctypes.byref(nb)) == -1, (M, n)
    assert L.clica_r2_loss_workspace_bytes(5, 3, None) == -1
    assert L.clica_r2_loss_fwd(None, 3, None, 3, 5, 3, 1, 1, None, None, None, None, 0, None) == -1          # NULL pointers: nothing launched
