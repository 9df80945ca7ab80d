"""Every image of a data set in HBM as uint8, batches by one gather launch: the image half of the reference's 3DIdent pipeline.

The reference's ``ThreeDIdentDataset`` (datasets/threedident_dataset.py:120-127) decodes two PNGs per item with torchvision's
``pil_loader`` on DataLoader workers, applies ``ToTensor`` + ``Normalize`` (main_3dident.py:787-796) on the host and copies the collated
batch to the GPU every step.  Here the folder is decoded ONCE (``Image.open(p).convert("RGB")``, what ``pil_loader`` does), the table
``[N, H, W, C]`` uint8 is uploaded once (250 000 x 224 x 224 x 3 bytes = 37.6 GB) and every batch is one launch of
``clica_image_gather_norm`` (csrc/image_table.hip) over a device index list -- no workers, no per-step copies.  A table that does not
fit the device raises ``MemoryError``; there is no host-resident fallback.

``channel_mean_std`` is tools/3dident/get_mean_std.py: the mean over images of the per-image channel mean and of the per-image unbiased
channel standard deviation of the ``/ 255`` values.  The data pass is exact integer sums on the device (``clica_image_channel_stats``);
the finish is fp64 on the host.

Parity note: the reference's dataset module cannot be imported here (torchvision, faiss), so the image values are pinned to the
DEFINITION of the two transforms, restated in torch CPU ops (``.float().div(255).sub(m).div(s)``) and asserted on the host
(tests/test_image_table_host.py) -- not to the reference's own execution.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .. import ops

__all__ = ["ImageTable", "image_path_names", "mean_std_from_sums"]

MAX_DECODE_THREADS = 16
UPLOAD_CHUNK_BYTES = 256 << 20


def image_path_names(n: int) -> list:
    """File names of the reference's naming rule (threedident_dataset.py:57-61): ``i`` zero-filled to ``ceil(log10(n))`` digits."""
    max_length = int(np.ceil(np.log10(n)))
    return [f"{str(i).zfill(max_length)}.png" for i in range(n)]


def decode_rgb(path) -> np.ndarray:
    """torchvision.datasets.folder.pil_loader: ``Image.open(f).convert("RGB")`` as a uint8 array [H, W, 3]."""
    from PIL import Image
    with open(path, "rb") as fh:
        return np.asarray(Image.open(fh).convert("RGB"), dtype=np.uint8)


def mean_std_from_sums(sums: np.ndarray, hw: int) -> Tuple[np.ndarray, np.ndarray]:
    """(mean, std), two fp64 arrays of length C, from the exact integer sums [N, C, 2] of the bytes and their squares over the ``hw``
    pixels of each image: per image mean = S1 / hw / 255 and unbiased var = (hw S2 - S1^2) / (hw (hw - 1)) / 255^2 (the numerator is an exact
    integer, below 2^53 at 224 x 224, and exactly 0 for a constant image), averaged over the images."""
    sums = np.asarray(sums)
    s1, s2 = sums[..., 0].astype(np.int64), sums[..., 1].astype(np.int64)
    hw = int(hw)
    mean = (s1.astype(np.float64) / hw / 255.0).mean(0)
    if hw < 2:
        return mean, np.full(mean.shape, np.nan)          # torch.std of one value
    if hw * hw * 65025 >= 2 ** 63:                        # images beyond 3400 x 3400: Python integers instead of int64
        s1, s2 = s1.astype(object), s2.astype(object)
    num = (hw * s2 - s1 * s1).astype(np.float64)          # integer arithmetic up to here
    var = num / (float(hw) * float(hw - 1)) / (255.0 * 255.0)
    return mean, np.sqrt(var).mean(0)


class ImageTable:
    """uint8 images ``[N, H, W, C]`` resident on the device.

    Args:
        images: uint8 array or tensor ``[N, H, W, C]`` (C in 1..4); uploaded in chunks into one preallocated device tensor.
        device: a CUDA device.
    """

    def __init__(self, images, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ImageTable lives on the GPU only; there is no host-resident fallback")
        if torch.is_tensor(images):
            shape, dtype_ok = tuple(images.shape), images.dtype == torch.uint8
        else:
            images = images if isinstance(images, np.ndarray) else np.asarray(images)
            shape, dtype_ok = images.shape, images.dtype == np.uint8
        if not dtype_ok:
            raise ValueError(f"ImageTable: images must be uint8 (got {images.dtype})")
        if len(shape) != 4 or min(shape) == 0:
            raise ValueError(f"ImageTable: images must be a non-empty [N, H, W, C] array (got shape {tuple(shape)})")
        if not 1 <= shape[3] <= 4:
            raise ValueError(f"ImageTable: C={shape[3]} channels (1..4 supported)")
        if torch.is_tensor(images) and images.is_cuda:
            self.table = images.to(self.device).contiguous()
        else:
            self.table = self._upload(images, shape)

    def _upload(self, images, shape) -> torch.Tensor:
        need = int(np.prod(shape, dtype=np.int64))
        free, _total = torch.cuda.mem_get_info(self.device)
        if need > free:
            raise MemoryError(f"ImageTable: the table needs {need} bytes, the device has {free} bytes free "
                              "(a host-resident table is not supported)")
        table = torch.empty(shape, dtype=torch.uint8, device=self.device)
        rows = max(1, UPLOAD_CHUNK_BYTES // max(1, need // shape[0]))
        for r0 in range(0, shape[0], rows):
            chunk = images[r0:r0 + rows]
            chunk = chunk if torch.is_tensor(chunk) else torch.from_numpy(np.ascontiguousarray(chunk))
            table[r0:r0 + rows].copy_(chunk)
        return table

    # ------------------------------------------------------------------ decoding a folder (host, once)
    @staticmethod
    def decode_folder(paths: Sequence, cache: Optional[str] = None) -> np.ndarray:
        """The decoded table of `paths` as a host uint8 array [N, H, W, 3].  With `cache`, the array is written once as a ``.npy`` file
        and memory-mapped on later calls (the files are then not opened at all)."""
        paths = list(paths)
        if not paths:
            raise ValueError("ImageTable.from_folder: no image paths")
        if cache is not None and os.path.exists(cache):
            arr = np.load(cache, mmap_mode="r")
            if arr.dtype != np.uint8 or arr.ndim != 4 or arr.shape[0] != len(paths):
                raise ValueError(f"ImageTable.from_folder: cache {cache} holds {arr.dtype} {arr.shape}, expected uint8 [{len(paths)}, H, W, C]")
            return arr
        first = decode_rgb(paths[0])
        shape = (len(paths),) + first.shape
        tmp = None
        if cache is not None:
            tmp = f"{cache}.tmp{os.getpid()}"       # renamed when complete: an interrupted decode leaves no half-written cache behind
            arr = np.lib.format.open_memmap(tmp, mode="w+", dtype=np.uint8, shape=shape)
        else:
            arr = np.empty(shape, np.uint8)
        arr[0] = first

        def work(i):
            img = decode_rgb(paths[i])
            if img.shape != first.shape:
                return i, img.shape
            arr[i] = img
            return None

        try:
            with ThreadPoolExecutor(max_workers=min(MAX_DECODE_THREADS, os.cpu_count() or 1)) as pool:
                bad = [r for r in pool.map(work, range(1, len(paths))) if r is not None]
            if bad:
                i, got = min(bad)
                raise ValueError(f"ImageTable.from_folder: {paths[i]} is {got[0]} x {got[1]}, the first image {paths[0]} is "
                                 f"{first.shape[0]} x {first.shape[1]}: all images must share one size")
            if tmp is not None:
                arr.flush()
                del arr
                os.replace(tmp, cache)
                tmp = None
                arr = np.load(cache, mmap_mode="r")
        finally:
            if tmp is not None and os.path.exists(tmp):
                os.remove(tmp)
        return arr

    @classmethod
    def from_folder(cls, paths: Sequence, device="cuda", cache: Optional[str] = None) -> "ImageTable":
        """Decode `paths` (PIL, RGB, at most 16 threads; all images one size) and upload the table."""
        return cls(cls.decode_folder(paths, cache), device=device)

    # ------------------------------------------------------------------ the device side
    def gather(self, index, normalize=None, out: Optional[torch.Tensor] = None, *, memory_format=torch.contiguous_format,
               dtype=torch.float32) -> torch.Tensor:
        """``(len(index), C, H, W)``: ToTensor of the rows `index`, then Normalize with ``normalize = (mean, std)`` if given.  float32 NCHW
        by default; `memory_format` ``torch.channels_last`` / `dtype` ``torch.bfloat16`` write the batch as a channels-last / mixed-precision
        backbone takes it (``ops.image_gather_norm``).  `out` must match shape, layout, dtype and device (``ValueError``)."""
        mean, std = (None, None) if normalize is None else normalize
        return ops.image_gather_norm(self.table, index, mean, std, out=out, memory_format=memory_format, dtype=dtype)

    def channel_sums(self) -> torch.Tensor:
        return ops.image_channel_sums(self.table)

    def channel_mean_std(self) -> Tuple[np.ndarray, np.ndarray]:
        """get_mean_std.py's (mean, std) of the ``/ 255`` values, two fp64 arrays of length C."""
        return mean_std_from_sums(self.channel_sums().cpu().numpy(), self.shape[1] * self.shape[2])

    def __len__(self) -> int:
        return self.table.shape[0]

    @property
    def shape(self) -> Tuple[int, int, int, int]:
        return tuple(self.table.shape)

    @property
    def nbytes(self) -> int:
        return self.table.numel()
