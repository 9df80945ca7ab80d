"""The latent lookup of ``ThreeDIdentDataset`` (/root/reference/datasets/threedident_dataset.py:64-127) on the device.

The reference samples ONE latent pair per ``__getitem__`` on the host (``latent_space.sample_marginal(size=1, device="cpu")``),
asks a ``faiss.IndexFlatL2`` built over ``raw_latents.npy`` for the closest rendered grid point (``search(z, 1)``) and the
two closest to the positive (``search(z_tilde, 2)``, taking the second when the first coincides with z's), and loads the
two PNGs.  Here a whole batch is drawn by the on-device samplers and snapped to the table by ONE exact brute-force
squared-L2 kernel (``clica_nn_search``, csrc/nn_search.hip) over the table resident in HBM -- 250 000 x 10 floats = 10 MB.

faiss is a third-party dependency of the reference that is not in this image (the reference pins no version;
``IndexFlatL2`` is exact search by definition: D[i, c] = squared L2 distance to the c-th closest stored vector, ascending,
I = its position in ``add`` order); ``IndexFlatL2`` below has the three members the reference uses -- ``add``, ``search``
and ``ntotal`` -- with device tensors instead of NumPy arrays.  ``ThreeDIdentLatentPairs`` returns the row indices a loader would
read.

The image side (:27-127, 141-190; transform at main_3dident.py:787-796): ``ThreeDIdentDataset`` and
``SequentialThreeDIdentDataset`` keep the reference's constructor arguments and item structure, but the images are rows of an
``ImageTable`` (datasets/image_table.py: the folder decoded once, uint8 in HBM) and a batch is the latent lookup plus ONE gather
launch for both views (``batch``), fed to a training loop by ``BatchLoader`` -- no DataLoader workers, no per-step copies.  What has no
device counterpart raises ``NotImplementedError`` when asked for: a ``transform`` callable (the device-side transform is
``normalize=(mean, std)``: ToTensor + Normalize), a custom ``loader``, faiss's approximate index.
Parity note: the reference module cannot be imported here (torchvision, faiss): the image values are pinned to the definition of the
two transforms restated in torch CPU ops (tests/test_image_table_host.py), not to the reference's own execution.
"""
from __future__ import annotations

import os
import sys
from typing import Optional, Sequence

import numpy as np
import torch

from .. import ops
from .image_table import ImageTable, image_path_names

__all__ = ["IndexFlatL2", "ThreeDIdentLatentPairs", "ThreeDIdentDataset", "SequentialThreeDIdentDataset", "BatchLoader"]


class IndexFlatL2:
    """``faiss.IndexFlatL2(d)`` as used at threedident_dataset.py:71, 83, 104-105: exact squared-L2 search."""

    def __init__(self, d: int, device="cuda"):
        if not 1 <= int(d) <= 64:
            raise ValueError(f"IndexFlatL2: d={d} must be in 1..64")
        self.d = int(d)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("IndexFlatL2 searches on the GPU only; there is no host fallback")
        self._table = torch.empty((0, self.d), dtype=torch.float32, device=self.device)

    @property
    def ntotal(self) -> int:
        return self._table.shape[0]

    def add(self, x) -> None:
        x = torch.as_tensor(np.asarray(x, dtype=np.float32) if not torch.is_tensor(x) else x, dtype=torch.float32)
        if x.dim() != 2 or x.shape[1] != self.d:
            raise ValueError(f"IndexFlatL2.add: expected (N, {self.d}), got {tuple(x.shape)}")
        self._table = torch.cat([self._table, x.to(self.device)], 0).contiguous()

    def search(self, x, k: int):
        """-> (D, I): (Q, k) float32 squared distances ascending, (Q, k) int64 positions (device tensors)."""
        if self.ntotal == 0:
            raise RuntimeError("IndexFlatL2.search: the index is empty")
        x = torch.as_tensor(np.asarray(x, dtype=np.float32) if not torch.is_tensor(x) else x, dtype=torch.float32).to(self.device)
        if x.dim() == 1:
            x = x.unsqueeze(0)
        return ops.nn_search(self._table, x, int(k))


class ThreeDIdentLatentPairs:
    """Batched ``ThreeDIdentDataset.__getitem__`` without the images (threedident_dataset.py:96-127).

    Args:
        latents: ``raw_latents.npy`` contents (N, d) or the dataset root holding that file (threedident_dataset.py:40).
        latent_space: space with ``sample_marginal`` / ``sample_conditional`` (cl_ica_amd.latent_spaces.LatentSpace).
        latent_dimensions_to_use: optional column subset (threedident_dataset.py:43-46).
    """

    def __init__(self, latents, latent_space, latent_dimensions_to_use: Optional[Sequence[int]] = None, device="cuda"):
        if isinstance(latents, (str, os.PathLike)):
            latents = np.load(os.path.join(latents, "raw_latents.npy"))
        latents = np.asarray(latents)
        self.unfiltered_latents = latents
        if latent_dimensions_to_use is not None:
            latents = np.ascontiguousarray(latents[:, list(latent_dimensions_to_use)])
        if latents.ndim != 2 or latents.shape[0] < 2:
            raise ValueError("ThreeDIdentLatentPairs needs a table of at least two latents (z and z~ are snapped to DIFFERENT rows)")
        if latents.shape[1] != latent_space.dim:
            raise AssertionError(f"Shapes do not match, i.e. {latent_space.dim} vs. {latents.shape}")   # as :50-52
        self.latent_space = latent_space
        self.device = torch.device(device)
        self._index = IndexFlatL2(latents.shape[1], device=self.device)
        self._index.add(latents)
        self.latents = self._index._table            # (N, d) float32 on the device

    def __len__(self) -> int:
        return self._index.ntotal

    def sample(self, batch_size: int):
        """-> (index_z, index_z_tilde, z, z_tilde): grid rows (int64) and their latents for `batch_size` pairs."""
        z = self.latent_space.sample_marginal(size=batch_size, device=self.device)
        z_tilde = self.latent_space.sample_conditional(z, size=batch_size, device=self.device)
        return self.snap(z, z_tilde)

    def snap(self, z: torch.Tensor, z_tilde: torch.Tensor):
        """Closest grid point of z; closest of z~ that is not the same grid point (threedident_dataset.py:104-116)."""
        _, iz = ops.nn_search(self.latents, z, 1, want_dist=False)
        _, izt = ops.nn_search(self.latents, z_tilde, 2, want_dist=False)
        index_z = iz[:, 0]
        index_zt = torch.where(izt[:, 0] != index_z, izt[:, 0], izt[:, 1])
        return index_z, index_zt, self.latents[index_z], self.latents[index_zt]


def _no_host_hooks(cls_name: str, transform, loader) -> None:
    if transform is not None:
        raise NotImplementedError(f"{cls_name}(transform=...): host transform callables are not run; the device-side transform is "
                                  "normalize=(mean, std) (ToTensor + Normalize, main_3dident.py:787-796)")
    if loader is not None:
        raise NotImplementedError(f"{cls_name}(loader=...): images are decoded once into an ImageTable (PIL, RGB); for the reference's "
                                  "loader=lambda _: torch.ones(1) branch pass dummy_images=True")


def _load_latents(root, latent_dimensions_to_use):
    latents = np.load(os.path.join(root, "raw_latents.npy"))
    unfiltered = latents
    if latent_dimensions_to_use is not None:
        latents = np.ascontiguousarray(latents[:, list(latent_dimensions_to_use)])
    return latents, unfiltered


def _image_table(root, n: int, images, device, cache) -> tuple:
    """-> (image_paths, ImageTable) for the `n` latents under `root`: `images` (an ImageTable or a uint8 array [n, H, W, C]) or the decoded
    folder ``root/images`` (threedident_dataset.py:57-61)."""
    paths = [os.path.join(root, "images", name) for name in image_path_names(n)]
    if images is None:
        table = ImageTable.from_folder(paths, device=device, cache=cache)
    else:
        table = images if isinstance(images, ImageTable) else ImageTable(images, device=device)
    if len(table) != n:
        raise ValueError(f"{len(table)} images for {n} latents")
    return paths, table


class ThreeDIdentDataset:
    """``ThreeDIdentDataset`` (threedident_dataset.py:11-127) with the images in HBM.

    Args:
        root: folder holding ``raw_latents.npy`` and ``images/``.
        latent_space: space to sample the marginal and the conditional latents from.
        transform, loader: must stay ``None`` (no device counterpart); approximate_mode: must stay false (exact search only);
            use_gpu: accepted and ignored (the search always runs on the GPU).
        latent_dimensions_to_use: which latent columns are returned; ``None`` for all.
        images: a ready ``ImageTable`` or uint8 array ``[N, H, W, C]`` instead of decoding ``root/images``.
        normalize: ``(mean, std)`` per channel, applied on the device after ``/ 255``; ``None``: ToTensor alone.
        dummy_images: images are ``torch.ones(B, 1)`` and no file is read (the reference's ``loader=lambda _: torch.ones(1)``).
        cache: ``.npy`` file the decoded folder is written to once and memory-mapped from afterwards.
        image_format, image_dtype: layout (``torch.contiguous_format`` | ``torch.channels_last``) and element type (``torch.float32`` |
            ``torch.bfloat16``) of the image batches (``ImageTable.gather``); the defaults are float32 NCHW.
    """

    def __init__(self, root, latent_space, transform=None, approximate_mode=False, use_gpu=False, loader=None,
                 latent_dimensions_to_use=None, *, images=None, normalize=None, dummy_images=False, device="cuda", cache=None,
                 image_format=torch.contiguous_format, image_dtype=torch.float32):
        _no_host_hooks("ThreeDIdentDataset", transform, loader)
        ops.image_format_args(image_format, image_dtype)
        self.image_format, self.image_dtype = image_format, image_dtype
        if approximate_mode:
            raise NotImplementedError("ThreeDIdentDataset(approximate_mode=True): faiss's IVF / HNSW index is not built; the exact search "
                                      "over the table in HBM is one kernel (clica_nn_search)")
        del use_gpu
        self.root = root
        self.device = torch.device(device)
        latents, self.unfiltered_latents = _load_latents(root, latent_dimensions_to_use)
        self.latent_space = latent_space
        self.pairs = ThreeDIdentLatentPairs(latents, latent_space, device=self.device)
        self.latents = self.pairs.latents
        self.normalize = normalize
        self.dummy_images = bool(dummy_images)
        n = latents.shape[0]
        if self.dummy_images:
            self.image_paths = [os.path.join(root, "images", name) for name in image_path_names(n)]
            self.images = None
        else:
            self.image_paths, self.images = _image_table(root, n, images, self.device, cache)

    def __len__(self) -> int:
        return sys.maxsize

    def __repr__(self) -> str:
        return f"Dataset {self.__class__.__name__}\n    Number of datapoints: {len(self.pairs)}\n    Root location: {self.root}"

    def batch(self, batch_size: int, *, image_format=None, image_dtype=None):
        """``((z, z~), (x, x~))`` for `batch_size` freshly sampled pairs, everything on the device: latents float32 (B, d), images
        (B, C, H, W) in the dataset's (or the given) layout and element type -- the two halves of ONE gather's output."""
        image_format = self.image_format if image_format is None else image_format
        image_dtype = self.image_dtype if image_dtype is None else image_dtype
        index_z, index_zt, z, zt = self.pairs.sample(int(batch_size))
        if self.dummy_images:
            ones = torch.ones((2 * int(batch_size), 1), dtype=torch.float32, device=self.device)
            return (z, zt), (ones[:batch_size], ones[batch_size:])
        x = self.images.gather(torch.cat([index_z, index_zt]), self.normalize, memory_format=image_format, dtype=image_dtype)
        return (z, zt), (x[:batch_size], x[batch_size:])

    def __getitem__(self, item):
        del item
        (z, zt), (x, xt) = self.batch(1)
        return (z[0], zt[0]), (x[0], xt[0])


class SequentialThreeDIdentDataset:
    """``SequentialThreeDIdentDataset`` (threedident_dataset.py:130-190): every sample of the data set in order; arguments as
    ``ThreeDIdentDataset``'s."""

    def __init__(self, root, transform=None, loader=None, latent_dimensions_to_use=None, *, images=None, normalize=None, device="cuda",
                 cache=None, image_format=torch.contiguous_format, image_dtype=torch.float32):
        _no_host_hooks("SequentialThreeDIdentDataset", transform, loader)
        ops.image_format_args(image_format, image_dtype)
        self.image_format, self.image_dtype = image_format, image_dtype
        self.root = root
        self.device = torch.device(device)
        latents, self.unfiltered_latents = _load_latents(root, latent_dimensions_to_use)
        self.latents = torch.as_tensor(np.ascontiguousarray(latents, dtype=np.float32), device=self.device)
        self.normalize = normalize
        self.image_paths, self.images = _image_table(root, latents.shape[0], images, self.device, cache)

    def __len__(self) -> int:
        return self.latents.shape[0]

    def __repr__(self) -> str:
        return f"Dataset {self.__class__.__name__}\n    Number of datapoints: {len(self)}\n    Root location: {self.root}"

    def batch(self, index):
        """``(z, x)`` of the samples `index`: float32 (B, d) and float32 (B, C, H, W) on the device."""
        index = torch.as_tensor(index).to(device=self.device, dtype=torch.int64).reshape(-1)
        n = len(self)
        if index.numel() and (int(index.min()) < -n or int(index.max()) >= n):
            raise IndexError(f"index out of range for {n} samples")
        index = torch.where(index < 0, index + n, index)
        return self.latents[index], self.images.gather(index, self.normalize, memory_format=self.image_format, dtype=self.image_dtype)

    def __getitem__(self, item):
        z, x = self.batch([int(item)])
        return z[0], x[0]


class BatchLoader:
    """What a training loop iterates in place of the reference's ``DataLoader``.

    Over ``ThreeDIdentDataset`` (length ``sys.maxsize``, every item a fresh draw): an endless iterator of ``dataset.batch(batch_size)``.
    Over ``SequentialThreeDIdentDataset``: one epoch per ``iter()``, every index exactly once -- in order, or with ``shuffle`` in a fresh
    device permutation each epoch from a device generator seeded with `seed` -- and the ragged last batch is kept (``drop_last=False``).
    The epoch's index batches never visit the host.  `image_format` / `image_dtype`: layout and element type of the image batches
    (``ImageTable.gather``); ``None``, the default: the dataset's own.
    """

    def __init__(self, dataset, batch_size: int, shuffle: bool = False, seed: Optional[int] = None, *, image_format=None,
                 image_dtype=None):
        if int(batch_size) < 1:
            raise ValueError(f"batch_size={batch_size}")
        self.image_format = image_format if image_format is not None else getattr(dataset, "image_format", torch.contiguous_format)
        self.image_dtype = image_dtype if image_dtype is not None else getattr(dataset, "image_dtype", torch.float32)
        ops.image_format_args(self.image_format, self.image_dtype)
        self.dataset, self.batch_size, self.shuffle = dataset, int(batch_size), bool(shuffle)
        self.endless = isinstance(dataset, ThreeDIdentDataset)
        self.generator = None
        if not self.endless:
            self.generator = torch.Generator(device=dataset.device)
            if seed is not None:
                self.generator.manual_seed(int(seed))

    def __len__(self) -> int:
        n = len(self.dataset)
        return (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        if self.endless:
            while True:
                yield self.dataset.batch(self.batch_size, image_format=self.image_format, image_dtype=self.image_dtype)
        ds, n = self.dataset, len(self.dataset)
        order = torch.randperm(n, device=ds.device, generator=self.generator) if self.shuffle else torch.arange(n, device=ds.device)
        for b in range(len(self)):
            index = order[b * self.batch_size:(b + 1) * self.batch_size]
            yield ds.latents[index], ds.images.gather(index, ds.normalize, memory_format=self.image_format, dtype=self.image_dtype)
