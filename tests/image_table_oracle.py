"""Oracles and seeded tables shared by tests/test_image_table_host.py and tests/test_gpu_image_table.py.

The image values are pinned to the DEFINITION of torchvision's two transforms (main_3dident.py:787-796): ``ToTensor`` is HWC uint8 -> CHW
float32 ``/ 255``, ``Normalize`` is ``(x - mean[c]) / std[c]`` with float32 constants -- three correctly rounded float32 operations per
element, so the expected batch is defined bit for bit."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture_normalize():
    """(mean, std) of tests/golden/threedident_normalize.json (the numbers of main_3dident.py:791-793)."""
    with open(os.path.join(GOLDEN, "threedident_normalize.json")) as fh:
        d = json.load(fh)
    return list(d["mean"]), list(d["std"])


def gather_oracle(table, index, mean=None, std=None):
    """float32 [len(index), C, H, W]: ((v / 255) - m) / s as three float32 operations, then HWC -> CHW."""
    v = np.asarray(table)[np.asarray(index, np.int64)].astype(np.float32)
    x = v / np.float32(255.0)
    if mean is not None:
        x = x - np.asarray(mean, np.float32)
        x = x / np.asarray(std, np.float32)
    assert x.dtype == np.float32
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def gather_torch_cpu(table, index, mean=None, std=None):
    """The same expression in torch CPU ops, written as the two transforms are: ``pic.permute(2, 0, 1).float().div(255)``, then
    ``.sub(mean[:, None, None]).div(std[:, None, None])``."""
    import torch
    x = torch.from_numpy(np.asarray(table)[np.asarray(index, np.int64)]).permute(0, 3, 1, 2).contiguous().float().div(255)
    if mean is not None:
        m = torch.as_tensor(mean, dtype=torch.float32).view(1, -1, 1, 1)
        s = torch.as_tensor(std, dtype=torch.float32).view(1, -1, 1, 1)
        x = x.sub(m).div(s)
    return x.numpy()


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def make_table(H, W, C, n_random=4, seed=0):
    """uint8 [N, H, W, C]: first a ramp that holds all 256 byte values in every channel (one image where H W >= 256, otherwise spread over
    the first ceil(256 / (H W)) images), then `n_random` seeded random images."""
    hw = H * W
    n_ramp = -(-256 // hw)
    p = np.arange(n_ramp * hw, dtype=np.int64).reshape(n_ramp, H, W, 1)
    ramp = ((p + 85 * np.arange(C, dtype=np.int64)) % 256).astype(np.uint8)
    rnd = np.random.default_rng([seed, H, W, C]).integers(0, 256, size=(n_random, H, W, C), dtype=np.uint8)
    return np.ascontiguousarray(np.concatenate([ramp, rnd], 0))


def sums_oracle(table):
    """int64 [N, C, 2]: the sum of the bytes and of their squares per image and channel."""
    t = np.asarray(table).astype(np.int64)
    return np.stack([t.sum((1, 2)), (t * t).sum((1, 2))], -1)


def mean_std_oracle(table):
    """get_mean_std.py in fp64: mean over images of the per-image channel mean / unbiased std of the ``/ 255`` values."""
    x = np.asarray(table).astype(np.float64) / 255.0
    N, H, W, C = x.shape
    x = x.reshape(N, H * W, C)
    return x.mean(1).mean(0), x.std(1, ddof=1).mean(0)


def mean_std_torch_fp32(table, batch=256):
    """The loop of tools/3dident/get_mean_std.py restated: float32 ToTensor batches, ``mean[i] += inputs[:, i].mean(dim=(-1, -2)).sum(0)``,
    ``std[i] += inputs[:, i].std(dim=(-1, -2)).sum(0)``, divided by the number of images."""
    import torch
    t = np.asarray(table)
    C = t.shape[3]
    mean, std = torch.zeros(C), torch.zeros(C)
    for r0 in range(0, t.shape[0], batch):
        inputs = torch.from_numpy(t[r0:r0 + batch]).permute(0, 3, 1, 2).contiguous().float().div(255)
        for i in range(C):
            mean[i] += inputs[:, i, :, :].mean(dim=(-1, -2)).sum(0)
            std[i] += inputs[:, i, :, :].std(dim=(-1, -2)).sum(0)
    mean.div_(t.shape[0]); std.div_(t.shape[0])
    return mean.numpy().astype(np.float64), std.numpy().astype(np.float64)
