"""Mean correlation coefficient (Hyvarinen & Morioka) of the KITTI-masks evaluation: the call surface of
/root/reference/kitti_masks/mcc_metric/metric.py (``correlation`` :11-55, ``compute_mcc`` :67-96, ``_compute_mcc`` :99-120) without
gin / absl / disentanglement_lib.  The metric is a correlation matrix, an assignment and a mean:

  * the correlation matrix of the factor rows against the code rows comes from ONE pass of ``clica_moments`` over the fp32 data
    (``ops.moments``; sums in fp64), Spearman from the same pass over the average ranks (``disentanglement_utils._average_ranks``);
  * the assignment on ``-|corr|`` is scipy's ``linear_sum_assignment`` (the same optimum as the reference's munkres.py; with ties
    between optima the chosen permutation may differ);
  * the correlation of the re-ordered code rows is the same matrix with its columns re-ordered (no second pass).

``compute_mcc`` consumes ``random_state`` exactly as disentanglement_lib's ``generate_batch_factor_code`` does through
``KittiMasks.sample`` -- one ``random_state.choice(len(data), n, replace=False)`` per chunk of ``min(num_train - i, batch_size)`` --
so the sample set equals the reference's for the same seed.  When the representation function is this package's encoder
(``EncoderRepresentation``) over a ``KittiMasks`` the work is done in bulk: all first-frame ids at once, one
``clica_kitti_gather_frames``, the encoder in ``eval()`` under ``no_grad`` over large chunks, codes on the device until the moment pass.
Any other callable (numpy in, numpy out) is served chunk by chunk through ``ground_truth_data.sample``.

Limits: ``num_train`` and ``correlation_fn`` have NO defaults here -- the reference takes them from ``metric_configs/*.gin``, which
its tree does not contain.  ``cl_ica_amd.train_kitti`` supplies them from ``--mcc-num-train`` / ``--mcc-correlation`` (this project's
choice of values).  Data are taken in fp32 (the encoder's dtype; the fp64 padding rows are rounded to it).
"""
from __future__ import annotations

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from .. import ops
from ..disentanglement_utils import _average_ranks, _dev32

__all__ = ["correlation", "compute_mcc", "_compute_mcc", "EncoderRepresentation", "generate_batch_factor_code"]

_METHODS = ("Pearson", "Spearman")


def _assign(corr: np.ndarray) -> np.ndarray:
    """sort_idx[i] = the code row assigned to factor row i by the optimal assignment on -|corr| (metric.py:38-45)."""
    rows, cols = linear_sum_assignment(-np.absolute(corr))
    return cols[np.argsort(rows)]


def _corr_matrix(x, y, method: str) -> np.ndarray:
    """corr[i, j] of row i of `y` against row j of `x` ([dim, N] each), from one moment pass on the device."""
    xd = _dev32(x).t().contiguous()
    yd = _dev32(y, xd.device).t().contiguous()
    if method == "Spearman":
        xd, yd = _average_ranks(xd), _average_ranks(yd)
    N, dx, dy = xd.shape[0], xd.shape[1], yd.shape[1]
    G = ops.moments(yd, xd).cpu().numpy()                                # [y | x | 1]^T [y | x | 1], fp64
    sy, sx = G[:dy, -1], G[dy:dy + dx, -1]
    cov = G[:dy, dy:dy + dx] - np.outer(sy, sx) / N
    vy = np.diag(G[:dy, :dy]) - sy ** 2 / N
    vx = np.diag(G[dy:dy + dx, dy:dy + dx]) - sx ** 2 / N
    return cov / np.sqrt(np.outer(vy, vx))


def correlation(x, y, method="Pearson"):
    """metric.py:11-55.  x: data to be sorted, y: target data, both ``[dim, N]`` (numpy arrays or device tensors).
    Returns ``(corr_sort, sort_idx, x_sort)``: the correlation of `y`'s rows against the re-ordered rows of `x`, the order, and `x`
    re-ordered (host arrays, ``sort_idx`` float as the reference's ``np.zeros(dim)``)."""
    if method not in _METHODS:
        raise ValueError(f"correlation method {method!r} (Pearson or Spearman)")
    corr = _corr_matrix(x, y, method)
    order = _assign(corr)
    xh = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return corr[:, order], order.astype(np.float64), xh[order].astype(np.float64)


def _pad_factors(mus_train, ys_train, random_state) -> np.ndarray:
    """metric.py:102-106: the factors padded up to the code dimension with ``random_state.normal(size=N)`` rows, in that order."""
    result = np.zeros(tuple(mus_train.shape))
    result[: ys_train.shape[0], : ys_train.shape[1]] = ys_train
    for i in range(len(mus_train) - len(ys_train)):
        result[ys_train.shape[0] + i, :] = random_state.normal(size=ys_train.shape[1])
    return result


def _compute_mcc(mus_train, ys_train, correlation_fn, random_state):
    """metric.py:99-120.  mus_train ``[dim, N]`` (numpy or device tensor), ys_train ``[n_factors, N]`` numpy."""
    ys_train = np.asarray(ys_train)
    result = _pad_factors(mus_train, ys_train, random_state)
    corr_sorted, sort_idx, _mu_sorted = correlation(mus_train, result, method=correlation_fn)
    score_dict = {"meanabscorr": np.mean(np.abs(np.diag(corr_sorted)[: len(ys_train)]))}
    for i in range(len(corr_sorted)):
        for j in range(len(corr_sorted[0])):
            score_dict["corr_sorted_{}{}".format(i, j)] = corr_sorted[i][j]
    for i in range(len(sort_idx)):
        score_dict["sort_idx_{}".format(i)] = sort_idx[i]
    return score_dict


class EncoderRepresentation:
    """The evaluation's ``mean_rep`` (evaluate_disentanglement.py:28-33) as an object ``compute_mcc`` recognises: called with a numpy
    batch it returns the encoder output as a numpy array, like any representation function; ``encode`` maps a device batch to device
    codes over chunks of `chunk` images."""

    def __init__(self, net, device=None, chunk: int = 4096):
        self.net = net
        self.device = torch.device(device) if device is not None else next(net.parameters()).device
        self.chunk = int(chunk)

    @torch.no_grad()
    def encode(self, images: torch.Tensor) -> torch.Tensor:
        was_training = self.net.training
        self.net.eval()
        try:
            return torch.cat([self.net._encode(images[i:i + self.chunk]) for i in range(0, images.shape[0], self.chunk)], 0)
        finally:
            self.net.train(was_training)

    def __call__(self, x):
        return self.encode(torch.from_numpy(np.asarray(x)).float().to(self.device)).cpu().numpy()


def _chunks(num_points: int, batch_size: int):
    i = 0
    while i < num_points:
        n = min(num_points - i, batch_size)
        yield n
        i += n


def generate_batch_factor_code(ground_truth_data, representation_function, num_points, random_state, batch_size):
    """disentanglement_lib's sampling loop: ``ground_truth_data.sample(min(num_points - i, batch_size), random_state)`` per chunk ->
    ``(codes [dim, num_points], factors [n_factors, num_points])``.  The bulk path (module docstring) returns the codes as a device
    tensor."""
    from .dataset import KittiMasks
    if isinstance(representation_function, EncoderRepresentation) and isinstance(ground_truth_data, KittiMasks):
        items = []
        for n in _chunks(num_points, batch_size):
            assert not (n % 2)                                            # KittiMasks.sample_observations' own rule
            items.append(random_state.choice(len(ground_truth_data), n, replace=False))
        ids = ground_truth_data.first_frame_ids(np.concatenate(items))
        images, factors = ops.kitti_gather_frames(ground_truth_data.frames, torch.as_tensor(ids), ground_truth_data.frame_latents)
        codes = representation_function.encode(images)
        return codes.t().contiguous(), np.transpose(factors.cpu().numpy())
    representations, factors = None, None
    for n in _chunks(num_points, batch_size):
        current_factors, current_observations = ground_truth_data.sample(n, random_state)
        current = representation_function(current_observations)
        if representations is None:
            factors, representations = current_factors, current
        else:
            factors = np.vstack((factors, current_factors))
            representations = np.vstack((representations, current))
    return np.transpose(representations), np.transpose(factors)


REQUIRED = object()      # the reference's gin.REQUIRED: no default


def compute_mcc(ground_truth_data, representation_function, random_state, artifact_dir=None, num_train=REQUIRED, correlation_fn=REQUIRED,
                batch_size=16):
    """metric.py:67-96: the mean correlation coefficient of `num_train` sampled points.  ``num_train`` and ``correlation_fn`` ("Pearson"
    or "Spearman") are required: the reference binds them from a gin file that is not part of its tree.  Returns the dictionary
    ``meanabscorr``, ``corr_sorted_{i}{j}``, ``sort_idx_{i}``."""
    del artifact_dir
    if num_train is REQUIRED or correlation_fn is REQUIRED:
        raise TypeError("compute_mcc: num_train and correlation_fn have no defaults (the reference binds them from metric_configs/mcc.gin)")
    mus_train, ys_train = generate_batch_factor_code(ground_truth_data, representation_function, num_train, random_state, batch_size)
    assert mus_train.shape[1] == num_train
    return _compute_mcc(mus_train, ys_train, correlation_fn, random_state)
