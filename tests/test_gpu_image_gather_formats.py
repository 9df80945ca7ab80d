"""The image gather in the backbone's layout and element type (clica_image_gather_norm_ex, csrc/image_table.hip) on the GPU.  Every
comparison is integer equality of bits: the channels-last fp32 batch against the NCHW fp32 gather ``.contiguous(channels_last)``, either
bf16 batch against the corresponding fp32 batch ``.to(torch.bfloat16)``.  Shapes: C in {1, 3, 4} x (H, W) in {(1, 1), (5, 7), (8, 8),
(16, 16)} (H W C % 4 zero and non-zero; 1 x 1 and C = 1, where both layouts are one memory) and a (300, 2, 2, 3) table (more images than
a workgroup's items)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CL, CF = torch.channels_last, torch.contiguous_format
FORMATS = [(CF, torch.float32), (CF, torch.bfloat16), (CL, torch.float32), (CL, torch.bfloat16)]
SHAPES = [(6, H, W, C) for C in (1, 3, 4) for (H, W) in ((1, 1), (5, 7), (8, 8), (16, 16))] + [(300, 2, 2, 3)]
_TABLES = {}


def table(shape):
    """A seeded uint8 table on the device, built once per shape and never written; bytes 0 and 255 are in it."""
    if shape not in _TABLES:
        t = torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(sum(shape)))
        t.view(-1)[0], t.view(-1)[-1] = 0, 255
        _TABLES[shape] = t.cuda()
    return _TABLES[shape]


def norms(C):
    return [None, ([0.3292, 0.3278, 0.3215, 0.41][:C], [0.0778, 0.0776, 0.0771, 0.23][:C])]      # distinct per channel


def index_lists(N):
    rng = np.random.default_rng(N)
    rep = rng.integers(-2, N + 2, size=257)               # repeated and out of range on both sides (clamped)
    return [np.array([-2]), np.array([N + 3, 0]), rep, np.sort(rep)[::-1].copy()]


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.is_contiguous() == b.is_contiguous() and torch.equal(bits_dense(a), bits_dense(b))


def bits_dense(t):
    """The bits of t's memory in its own (dense) order."""
    if t.is_contiguous():
        return bits(t)
    return bits(t.permute(0, 2, 3, 1))


def oracle(base, memory_format, dtype):
    """`base`: the NCHW fp32 gather."""
    x = base.contiguous(memory_format=memory_format)
    return x if dtype == torch.float32 else x.to(torch.bfloat16)


def view_at(n, C, H, W, memory_format, dtype, offset):
    """A dense (n, C, H, W) view in `memory_format` that starts `offset` elements into a larger buffer."""
    buf = torch.zeros(n * C * H * W + 8, dtype=dtype, device="cuda")
    flat = buf[offset:offset + n * C * H * W]
    out = flat.view(n, C, H, W) if memory_format == CF else flat.view(n, H, W, C).permute(0, 3, 1, 2)
    return buf, out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_formats_bit_for_bit(shape):
    from cl_ica_amd import ops
    dev = table(shape)
    N, H, W, C = shape
    for index in index_lists(N):
        idx = torch.as_tensor(index, device="cuda")
        for nz in norms(C):
            mean, std = nz if nz is not None else (None, None)
            base = ops.image_gather_norm(dev, idx, mean, std)
            clamped = dev[idx.clamp(0, N - 1)].cpu().permute(0, 3, 1, 2).float().div(255)
            if nz is not None:
                clamped = clamped.sub(torch.tensor(mean).view(1, C, 1, 1)).div(torch.tensor(std).view(1, C, 1, 1))
            assert torch.equal(bits(base.cpu()), bits(clamped.contiguous())), (shape, len(index), nz)      # the base itself, clamping included
            for memory_format, dtype in FORMATS:
                got = ops.image_gather_norm(dev, idx, mean, std, memory_format=memory_format, dtype=dtype)
                want = oracle(base, memory_format, dtype)
                assert got.shape == (len(index), C, H, W) and got.dtype == dtype and got.is_contiguous(memory_format=memory_format)
                assert same(got, want), (shape, len(index), nz, memory_format, dtype)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_out_views_off_the_wide_alignment(shape):
    """`out` starting 1 and 3 elements into a buffer is not 8 / 16-byte aligned: the scalar path runs and writes the same bits, and
    nothing outside the view."""
    from cl_ica_amd import ops
    dev = table(shape)
    N, H, W, C = shape
    idx = torch.as_tensor(index_lists(N)[2], device="cuda")
    n = idx.numel()
    mean, std = norms(C)[1]
    base = ops.image_gather_norm(dev, idx, mean, std)
    for memory_format, dtype in FORMATS:
        want = oracle(base, memory_format, dtype)
        for offset in (0, 1, 3):
            buf, out = view_at(n, C, H, W, memory_format, dtype, offset)
            r = ops.image_gather_norm(dev, idx, mean, std, out=out, memory_format=memory_format, dtype=dtype)
            assert r is out and torch.equal(bits_dense(out), bits_dense(want)), (shape, memory_format, dtype, offset)
            assert not buf[:offset].any() and not buf[offset + out.numel():].any()


@pytest.mark.parametrize("memory_format,dtype", FORMATS[1:])
def test_replays_in_a_graph(memory_format, dtype):
    from cl_ica_amd import ops
    shape = (6, 8, 8, 3)
    dev = table(shape)
    mean, std = norms(3)[1]
    index = torch.tensor([0, 1, 2, 5, 3, 0], device="cuda")
    out = torch.empty((6, 3, 8, 8), dtype=dtype, device="cuda", memory_format=memory_format)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.image_gather_norm(dev, index, mean, std, out=out, memory_format=memory_format, dtype=dtype)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            ops.image_gather_norm(dev, index, mean, std, out=out, memory_format=memory_format, dtype=dtype)
    torch.cuda.current_stream().wait_stream(s)
    for new in ([0, 1, 2, 5, 3, 0], [5, 4, 1, 1, 0, 9], [2, 2, 2, 2, 2, -1]):
        index.copy_(torch.tensor(new, device="cuda"))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        eager = ops.image_gather_norm(dev, torch.tensor(new, device="cuda"), mean, std, memory_format=memory_format, dtype=dtype)
        assert same(out, eager)


def test_out_of_the_wrong_layout_or_dtype_raises():
    from cl_ica_amd import ops
    from cl_ica_amd.datasets import ImageTable
    dev = table((6, 8, 8, 3))
    idx = torch.tensor([0, 1], device="cuda")
    nchw32 = torch.empty((2, 3, 8, 8), device="cuda")
    nhwc32 = torch.empty((2, 3, 8, 8), device="cuda", memory_format=CL)
    nhwc16 = torch.empty((2, 3, 8, 8), device="cuda", memory_format=CL, dtype=torch.bfloat16)
    for out, kw in ((nchw32, dict(memory_format=CL)), (nhwc32, dict()), (nhwc32, dict(memory_format=CL, dtype=torch.bfloat16)),
                    (nhwc16, dict(memory_format=CL)), (nhwc16, dict(dtype=torch.bfloat16)), (nchw32, dict(dtype=torch.bfloat16)),
                    (torch.empty((3, 3, 8, 8), device="cuda", memory_format=CL), dict(memory_format=CL)),
                    (torch.empty((2, 3, 8, 8), device="cuda", dtype=torch.float16), dict(dtype=torch.float16)),
                    (torch.empty((2, 3, 8, 8)), dict())):                                           # another device
        with pytest.raises(ValueError):
            ops.image_gather_norm(dev, idx, out=out, **kw)
        with pytest.raises(ValueError):
            ImageTable(dev).gather(idx, None, out, **kw)
    with pytest.raises(ValueError):
        ops.image_gather_norm(dev, idx, memory_format=torch.channels_last_3d)
    assert ops.image_gather_norm(dev, idx, out=nhwc16, memory_format=CL, dtype=torch.bfloat16) is nhwc16


def test_the_abi_refuses_by_return_code():
    import ctypes as C
    from cl_ica_amd import _lib
    L = _lib.load()
    dev = table((6, 8, 8, 3))
    idx = torch.tensor([0, 1], device="cuda")
    out = torch.empty(2 * 3 * 8 * 8 + 4, dtype=torch.float32, device="cuda")

    def call(layout=1, dtype=0, o=out.data_ptr(), Cn=3, table_ptr=dev.data_ptr()):
        return L.clica_image_gather_norm_ex(table_ptr, 6, 8, 8, Cn, idx.data_ptr(), 2, None, None, o, layout, dtype, _lib.stream_ptr())

    assert call() == 0 and call(dtype=1) == 0 and call(layout=0) == 0 and call(o=out.data_ptr() + 4) == 0 and call(dtype=1, o=out.data_ptr() + 2) == 0
    for bad in (dict(layout=2), dict(dtype=2), dict(layout=-1), dict(o=None), dict(Cn=5), dict(Cn=0), dict(table_ptr=None),
                dict(o=out.data_ptr() + 2), dict(dtype=1, o=out.data_ptr() + 1)):
        assert call(**bad) == -1, bad
        assert b"clica_image_gather_norm_ex" in L.clica_last_error()
    m = (C.c_float * 3)(0.1, 0.2, 0.3)
    assert L.clica_image_gather_norm_ex(dev.data_ptr(), 6, 8, 8, 3, idx.data_ptr(), 2, m, None, out.data_ptr(), 1, 0, _lib.stream_ptr()) == -1
    torch.cuda.synchronize()


def test_dataset_keywords_give_the_tables_tensors(tmp_path):
    from cl_ica_amd import latent_spaces, spaces
    from cl_ica_amd.datasets import BatchLoader, ImageTable, SequentialThreeDIdentDataset, ThreeDIdentDataset
    n = 32
    np.save(tmp_path / "raw_latents.npy", np.random.default_rng(3).uniform(size=(n, 3)).astype(np.float32))
    images = table((32, 8, 8, 3))
    tab = ImageTable(images)
    nz = norms(3)[1]
    ls = latent_spaces.LatentSpace(spaces.NBoxSpace(3, 0, 1), lambda s, size, device="cuda": s.uniform(size, device=device),
                                   lambda s, z, size, device="cuda": s.normal(z, 0.3, size, device=device))
    for memory_format, dtype in FORMATS:
        kw = dict(image_format=memory_format, image_dtype=dtype)
        seq = SequentialThreeDIdentDataset(str(tmp_path), images=tab, normalize=nz, **kw)
        index = torch.tensor([3, 0, 31, 3], device="cuda")
        want = tab.gather(index, nz, memory_format=memory_format, dtype=dtype)
        assert same(seq.batch(index)[1], want)
        assert same(next(iter(BatchLoader(seq, 4)))[1], tab.gather(torch.arange(4), nz, memory_format=memory_format, dtype=dtype))
        plain = SequentialThreeDIdentDataset(str(tmp_path), images=tab, normalize=nz)
        assert same(next(iter(BatchLoader(plain, 4, **kw)))[1], tab.gather(torch.arange(4), nz, memory_format=memory_format, dtype=dtype))
        ds = ThreeDIdentDataset(str(tmp_path), ls, images=tab, normalize=nz, **kw)
        for batch in (ds.batch(5), next(iter(BatchLoader(ds, 5))), next(iter(BatchLoader(ThreeDIdentDataset(str(tmp_path), ls, images=tab, normalize=nz), 5, **kw)))):
            (z, zt), (x, xt) = batch
            rows = lambda v: (ds.latents.unsqueeze(0) == v.unsqueeze(1)).all(-1).float().argmax(1)  # noqa: E731
            both = tab.gather(torch.cat([rows(z), rows(zt)]), nz, memory_format=memory_format, dtype=dtype)
            assert x.dtype == dtype and torch.equal(bits_dense(torch.cat([x, xt])), bits_dense(both))
    # the defaults are today's tensors: float32 NCHW from the first entry point
    seq = SequentialThreeDIdentDataset(str(tmp_path), images=tab, normalize=nz)
    x = seq.batch([1, 2])[1]
    assert x.dtype == torch.float32 and x.is_contiguous() and same(x, tab.gather([1, 2], nz))
    with pytest.raises(ValueError):
        SequentialThreeDIdentDataset(str(tmp_path), images=tab, image_dtype=torch.float16)
    with pytest.raises(ValueError):
        ThreeDIdentDataset(str(tmp_path), ls, images=tab, image_format=torch.preserve_format)
    with pytest.raises(ValueError):
        BatchLoader(seq, 4, image_dtype=torch.float64)
