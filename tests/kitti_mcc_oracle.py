"""NumPy / SciPy restatement of the KITTI-masks MCC evaluation (kitti_masks/mcc_metric/metric.py of the reference and the sampling loop
of disentanglement_lib's ``generate_batch_factor_code``), for the tests of ``cl_ica_amd.kitti_masks.mcc_metric``.  fp64 throughout,
straight from the data (``np.corrcoef`` / ``scipy.stats.spearmanr``): nothing here shares code with the package."""
import itertools

import numpy as np
import scipy.stats
from scipy.optimize import linear_sum_assignment


def corr_matrix(x, y, method):
    """Rows of y against rows of x ([dim, N] each), metric.py:30-35."""
    dim = x.shape[0]
    if method == "Pearson":
        return np.corrcoef(y, x)[0:dim, dim:]
    corr, _ = scipy.stats.spearmanr(y.T, x.T)
    if dim == 1:                                    # (two variables: scipy returns the one coefficient, not a matrix)
        return np.array([[float(corr)]])
    return corr[0:dim, dim:]


def correlation(x, y, method="Pearson"):
    x = np.asarray(x, np.float64).copy(); y = np.asarray(y, np.float64).copy()
    dim = x.shape[0]
    corr = corr_matrix(x, y, method)
    rows, cols = linear_sum_assignment(-np.absolute(corr))
    sort_idx = np.zeros(dim)
    x_sort = np.zeros(x.shape)
    for r, c in zip(rows, cols):
        sort_idx[r] = c
        x_sort[r, :] = x[c, :]
    return corr_matrix(x_sort, y, method), sort_idx, x_sort


def brute_force_assignment(corr):
    """The permutation maximising sum_i |corr[i, perm[i]]| by trying all of them (dim <= 5)."""
    dim = corr.shape[0]
    best, best_perm = -np.inf, None
    for perm in itertools.permutations(range(dim)):
        s = sum(abs(corr[i, perm[i]]) for i in range(dim))
        if s > best:
            best, best_perm = s, perm
    return np.array(best_perm), best


def pad_factors(mus, ys, random_state):
    """metric.py:102-106."""
    result = np.zeros(mus.shape)
    result[: ys.shape[0], : ys.shape[1]] = ys
    for i in range(len(mus) - len(ys)):
        result[ys.shape[0] + i, :] = random_state.normal(size=ys.shape[1])
    return result


def compute_mcc_from_codes(mus, ys, method, random_state):
    """metric.py:99-120."""
    mus = np.asarray(mus, np.float64); ys = np.asarray(ys, np.float64)
    result = pad_factors(mus, ys, random_state)
    corr_sorted, sort_idx, _ = correlation(mus, result, method)
    out = {"meanabscorr": np.mean(np.abs(np.diag(corr_sorted)[: len(ys)]))}
    for i in range(len(corr_sorted)):
        for j in range(len(corr_sorted[0])):
            out["corr_sorted_{}{}".format(i, j)] = corr_sorted[i][j]
    for i in range(len(sort_idx)):
        out["sort_idx_{}".format(i)] = sort_idx[i]
    return out


def chunk_sizes(num_train, batch_size):
    sizes, i = [], 0
    while i < num_train:
        sizes.append(min(num_train - i, batch_size))
        i += sizes[-1]
    return sizes


def sampled_items(n_items, num_train, batch_size, random_state):
    """The data-set indices KittiMasks.sample draws chunk by chunk (dataset.py:68-82: one choice without replacement per call)."""
    return np.concatenate([random_state.choice(n_items, n, replace=False) for n in chunk_sizes(num_train, batch_size)])


def first_frames(data, latents, cumlens, items):
    """First frame (float32 [1, H, W]) and its latents for every item, by the reference's __getitem__ arithmetic (dataset.py:91-95)."""
    frames, labs = [], []
    for index in items:
        seq = int(np.searchsorted(cumlens, index, side="right"))
        start = int(index if seq == 0 else index - cumlens[seq - 1])
        frames.append((np.asarray(data[seq][start]).astype(np.uint8) * 255)[None].astype(np.float32) / 255.0)
        labs.append(latents[seq][start])
    return np.stack(frames), np.stack(labs)
