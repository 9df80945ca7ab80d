"""The image gather's bf16 output and its new keywords, without a GPU: the narrowing the kernel applies at the store (csrc/bn2d.h
bf16_rne, restated in NumPy) against ``Tensor.to(torch.bfloat16)`` on every value the transform can produce, and the argument checks
that run before any launch.

The narrowing test runs no device code: it pins the RULE (round to nearest even, NaN -> 0x7fc0) to torch's on the 768 values the
transform can produce, and would not notice a kernel that rounds otherwise.  The kernel's own stores are held to
``Tensor.to(torch.bfloat16)`` bit for bit by tests/test_gpu_image_gather_formats.py."""
import ctypes

import numpy as np
import pytest
import torch


def bf16_bits_rne(a):
    """csrc/bn2d.h bf16_rne on an fp32 array: the upper 16 bits after adding 0x7fff + (bit 16); a NaN becomes 0x7fc0."""
    u = np.asarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where((u & 0x7FFFFFFF) > 0x7F800000, np.uint16(0x7FC0), r)


def transform_values(normalize):
    """fp32 [256, 3]: ((v / 255) - mean[c]) / std[c] for every byte v and channel c, three correctly rounded fp32 operations."""
    x = torch.arange(256, dtype=torch.float32).div(255).reshape(256, 1).repeat(1, 3)
    if normalize is not None:
        mean, std = normalize
        x = x.sub(torch.tensor(mean, dtype=torch.float32)).div(torch.tensor(std, dtype=torch.float32))
    return x


def test_the_narrowing_is_torchs_on_every_value_of_the_transform():
    from cl_ica_amd import train_3dident
    for normalize in (train_3dident.NORMALIZE, None):
        x = transform_values(normalize)
        assert x.shape == (256, 3) and bool(torch.isfinite(x).all())
        want = x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        got = bf16_bits_rne(x.numpy())
        assert np.array_equal(got, want), normalize
        # the narrowing does round here: most of the 768 values are no bf16 numbers
        assert int((x.to(torch.bfloat16).float() != x).sum()) > 256


def test_format_keywords_are_validated():
    from cl_ica_amd import ops
    assert ops.image_format_args() == (0, 0)
    assert ops.image_format_args(torch.channels_last, torch.bfloat16) == (1, 1)
    assert ops.image_format_args(torch.contiguous_format, torch.bfloat16) == (0, 1)
    for bad in (dict(memory_format=torch.preserve_format), dict(memory_format=torch.channels_last_3d), dict(memory_format="nhwc"),
                dict(dtype=torch.float16), dict(dtype=torch.float64), dict(dtype=torch.uint8), dict(dtype=None)):
        with pytest.raises(ValueError):
            ops.image_format_args(**bad)


def test_the_entry_point_checks_its_arguments_before_any_launch():
    from cl_ica_amd import _lib
    L, p = _lib.load(), 4096
    good = dict(table=p, n=2, H=4, W=4, C=3, index=p, n_index=2, mean=None, std=None, out=p, layout=1, dtype=1, stream=None)

    def call(**kw):
        return L.clica_image_gather_norm_ex(*dict(good, **kw).values())
    m = (ctypes.c_float * 3)(0.1, 0.2, 0.3)
    for bad in (dict(table=None), dict(index=None), dict(out=None), dict(C=0), dict(C=5), dict(H=0), dict(W=-1), dict(n=0), dict(n_index=0),
                dict(mean=m), dict(std=m), dict(layout=2), dict(layout=-1), dict(dtype=2), dict(dtype=-1), dict(out=p + 1),
                dict(dtype=0, out=p + 2)):
        assert call(**bad) == -1, bad
        assert b"clica_image_gather_norm_ex" in L.clica_last_error(), bad
