"""NumPy fp64 restatement of losses.R2Loss (reference losses.py:480-503) and of its gradient with respect to y_pred.

    var_j = mean_i (y_ij - mean_i y_ij)^2            torch.var(y, unbiased=False, dim=0), losses.py:490
    r2_j  = 1 - mean_i (y_pred_ij - y_ij)^2 / var_j  losses.py:491
    out   = s reduce(r2)                             reduce: mean / sum / none (losses.py:492-495); s = +1 for "r2", -1 otherwise (:497-500)
    d out / d y_pred_ij (times the upstream gradient g) = g_j s w (-2 / M) (y_pred_ij - y_ij) / var_j,  w = 1 / n for the mean, else 1
"""
import numpy as np


def r2_value(y_pred, y, reduction="none", mode="negative_r2"):
    y_pred = np.asarray(y_pred, np.float64); y = np.asarray(y, np.float64)
    with np.errstate(all="ignore"):
        var = np.mean((y - y.mean(0)) ** 2, 0)
        r2 = 1.0 - np.mean((y_pred - y) ** 2, 0) / var
        if reduction == "mean":
            r2 = np.mean(r2)
        elif reduction == "sum":
            r2 = np.sum(r2)
    return r2 if mode == "r2" else -r2


def r2_grad(y_pred, y, g, reduction="none", mode="negative_r2"):
    """g: the upstream gradient -- n values for reduction "none", one value otherwise."""
    y_pred = np.asarray(y_pred, np.float64); y = np.asarray(y, np.float64)
    M, n = y.shape
    g = np.broadcast_to(np.asarray(g, np.float64).reshape(-1), (n,))
    s = 1.0 if mode == "r2" else -1.0
    w = 1.0 / n if reduction == "mean" else 1.0
    with np.errstate(all="ignore"):
        var = np.mean((y - y.mean(0)) ** 2, 0)
        return g[None, :] * (s * w * (-2.0 / M)) * (y_pred - y) / var[None, :]
