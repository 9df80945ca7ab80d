"""What the GPU tests of the batch-normalisation family (test_gpu_norm.py, test_gpu_bn2d.py, test_gpu_bn2d_nhwc.py, test_gpu_pool2d.py) and
tools/norm_digest.py defined identically: moving arrays to the device and back, views of a tensor's bits, a misaligned copy, the
stand-in for a torch kernel that must not run, and the fixture that makes the convolutions between the units reproducible.  A module
that wants the fixture imports it by name: it is autouse in that module and in no other."""
import numpy as np
import pytest
import torch


@pytest.fixture(autouse=True)
def deterministic_convolutions(monkeypatch):
    """MIOpen's default choice of convolution kernels is not reproducible run to run (split-K weight gradients with atomics: two "torch"-mode
    passes of the backbone differ in every tensor); the tests that compare bits across passes are about the units and the pools, so the
    convolutions between them run in torch's deterministic mode."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)


def dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return host(t).view(np.uint32)


def raw(t):
    return np.ascontiguousarray(host(t)).reshape(-1).view(np.uint8)


def off_by_4_bytes(t):
    """A contiguous copy of t whose storage starts 4 bytes off a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    u = buf[1:].view(t.shape)
    u.copy_(t)
    assert u.is_contiguous() and u.data_ptr() % 16 == 4
    return u


def refuse(*a, **k):
    raise AssertionError("torch's own normalisation or activation kernel was called")
