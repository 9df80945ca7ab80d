"""3DIdent image batches from a uint8 table in HBM (csrc/image_table.hip, datasets/image_table.py, the two dataset classes of
datasets/threedident_dataset.py) on the GPU: the gather against the float32 oracle BIT FOR BIT, the pair convention, graph replay,
the exact channel sums, the datasets feeding threedident.train_step.  Tables are built from arrays: nothing here needs PIL."""
import sys

import numpy as np
import pytest
import torch

import image_table_oracle as IO

pytestmark = pytest.mark.gpu

# (H, W, C): smallest fast-path image; 105 bytes per image (odd image bases, scalar path with a tail); one quad; 4 chunks per image;
# the data set's size; one / four / two channels; and two shapes whose last chunk of an image is ragged (324 quads, 323 pixels)
SHAPES = [(4, 4, 3), (5, 7, 3), (2, 2, 3), (64, 64, 3), (224, 224, 3), (8, 8, 1), (3, 5, 4), (6, 6, 2), (36, 36, 3), (17, 19, 2)]
_TABLES = {}


def tables(shape):
    """(host uint8 table, the same on the device), built once per shape and never written."""
    if shape not in _TABLES:
        host = IO.make_table(*shape, n_random=2 if shape == (224, 224, 3) else 4)
        _TABLES[shape] = (host, torch.as_tensor(host, device="cuda"))
    return _TABLES[shape]


def norms_for(C):
    out = [None, ([0.11, 0.47, 0.29, 0.73][:C], [0.31, 0.07, 0.19, 0.53][:C])]       # distinct per channel: a channel mix-up cannot pass
    if C == 3:
        out.insert(1, IO.fixture_normalize())
    return out


def index_lists(N, rng):
    rep = rng.integers(0, N, size=2 * N + 1)
    rep[0], rep[-1] = 0, N - 1
    return [np.array([N // 2]), np.arange(N)[::-1].copy(), rep]


@pytest.mark.parametrize("shape", SHAPES)
def test_gather_norm_bit_for_bit(shape):
    from cl_ica_amd import ops
    host, dev = tables(shape)
    N, (H, W, C) = host.shape[0], shape
    assert N == 3 if shape == (224, 224, 3) else N >= 5
    rng = np.random.default_rng(11)
    for index in index_lists(N, rng):
        for nz in norms_for(C):
            mean, std = nz if nz is not None else (None, None)
            got = ops.image_gather_norm(dev, torch.as_tensor(index, device="cuda"), mean, std)
            assert got.shape == (len(index), C, H, W) and got.dtype == torch.float32 and got.is_contiguous()
            ref = IO.gather_oracle(host, index, mean, std)
            g = got.cpu().numpy()
            assert IO.same_bits(g, ref), (shape, len(index), nz, float(np.abs(g - ref).max()), int((g != ref).sum()))


def test_gather_norm_grid_stride():
    """More work than one grid's worth of workgroups at 4 x 4 (8 x 256 workgroups of 256 quads = 131 072 images): every workgroup loops."""
    from cl_ica_amd import ops
    host, dev = tables((4, 4, 3))
    n = 3 * 8 * 256 * 256 // 4 + 5
    index = np.random.default_rng(3).integers(0, host.shape[0], size=n)
    mean, std = IO.fixture_normalize()
    got = ops.image_gather_norm(dev, torch.as_tensor(index, device="cuda"), mean, std).cpu().numpy()
    assert IO.same_bits(got, IO.gather_oracle(host, index, mean, std))


def test_plain_store_variant_has_the_same_bits():
    """clica_set_tuning("image_nt_stores", 0): the RGB path with plain instead of non-temporal stores (the A/B hook of
    tools/image_gather_bench.py) is a product-quality path too."""
    from cl_ica_amd import _lib, ops
    host, dev = tables((36, 36, 3))
    index = np.random.default_rng(8).integers(0, host.shape[0], size=19)
    mean, std = IO.fixture_normalize()
    L = _lib.load()
    try:
        assert L.clica_set_tuning(b"image_nt_stores", 0) == 0
        plain = ops.image_gather_norm(dev, torch.as_tensor(index, device="cuda"), mean, std).cpu().numpy()
    finally:
        assert L.clica_set_tuning(b"image_nt_stores", 1) == 0
    assert IO.same_bits(plain, IO.gather_oracle(host, index, mean, std))


def test_pair_convention_one_launch_for_both_views():
    """One launch for the 2 B concatenated indices equals two launches of B; the halves are views of one buffer."""
    from cl_ica_amd import ops
    from cl_ica_amd.datasets import ImageTable
    host, dev = tables((64, 64, 3))
    tab = ImageTable(dev)
    assert len(tab) == host.shape[0] and tab.shape == host.shape and tab.nbytes == host.size
    rng = np.random.default_rng(5)
    B = 37
    a, b = (torch.as_tensor(rng.integers(0, len(tab), size=B), device="cuda") for _ in range(2))
    nz = IO.fixture_normalize()
    both = tab.gather(torch.cat([a, b]), nz)
    x, xt = both[:B], both[B:]
    assert x.untyped_storage().data_ptr() == xt.untyped_storage().data_ptr() and x.is_contiguous() and xt.is_contiguous()
    assert torch.equal(x, tab.gather(a, nz)) and torch.equal(xt, tab.gather(b, nz))
    assert torch.equal(x, ops.image_gather_norm(dev, a, *nz))
    assert IO.same_bits(both.cpu().numpy(), IO.gather_oracle(host, torch.cat([a, b]).cpu().numpy(), *nz))


def test_gather_replays_in_a_graph():
    """Gathered into a fixed `out` inside a captured graph, the launch reads the index tensor on replay: new contents, new batch, the
    eager bits.  One launch: the graph is a single node."""
    from cl_ica_amd import ops
    host, dev = tables((64, 64, 3))
    N = host.shape[0]
    mean, std = IO.fixture_normalize()
    index = torch.tensor([0, 1, 2, N - 1, 3, 0], device="cuda")
    out = torch.empty((index.numel(), 3, 64, 64), dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.image_gather_norm(dev, index, mean, std, out=out)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            r = ops.image_gather_norm(dev, index, mean, std, out=out)
        assert r is out
    torch.cuda.current_stream().wait_stream(s)
    first = [0, 1, 2, N - 1, 3, 0]
    for new in (first, [N - 1, N - 2, 1, 1, 0, 4], [2, 2, 2, 2, 2, 2]):
        index.copy_(torch.tensor(new, device="cuda"))
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        eager = ops.image_gather_norm(dev, torch.tensor(new, device="cuda"), mean, std)
        assert torch.equal(out, eager)
        assert IO.same_bits(out.cpu().numpy(), IO.gather_oracle(host, new, mean, std))


@pytest.mark.parametrize("shape", SHAPES)
def test_channel_sums_exact(shape):
    from cl_ica_amd import ops
    from cl_ica_amd.datasets import ImageTable
    host, dev = tables(shape)
    H, W, C = shape
    extra = np.stack([np.full(shape, 255, np.uint8), np.zeros(shape, np.uint8)])          # all-255: 3 262 694 400 at 224 x 224, just under 2^32
    both = np.concatenate([host, extra])
    sums = ops.image_channel_sums(torch.as_tensor(both, device="cuda"))
    assert sums.shape == (both.shape[0], C, 2) and sums.dtype == torch.int64
    ref = IO.sums_oracle(both)
    assert np.array_equal(sums.cpu().numpy(), ref)
    if shape == (224, 224, 3):
        assert int(sums[-2, 0, 1]) == 3262694400
    mean, std = ImageTable(both).channel_mean_std()
    rm, rs = IO.mean_std_oracle(both)
    assert mean.dtype == np.float64 and std.dtype == np.float64 and mean.shape == (C,)
    # exact integer sums, then a handful of fp64 operations per image and one fp64 mean: a few ulps, 1e-12 with three decades to spare
    assert np.abs(mean - rm).max() <= 1e-12 * np.abs(rm).max() and np.abs(std - rs).max() <= 1e-12 * np.abs(rs).max()


def test_constant_table_has_zero_std():
    from cl_ica_amd.datasets import ImageTable
    const = np.stack([np.full((8, 12, 3), v, np.uint8) for v in (0, 7, 130, 255)])
    mean, std = ImageTable(const).channel_mean_std()
    assert (std == 0.0).all()
    assert np.abs(mean - np.mean([0, 7, 130, 255]) / 255.0).max() < 1e-15


# --------------------------------------------------------------------------------------------------- the dataset classes
def _latent_space():
    from cl_ica_amd import latent_spaces, spaces
    return latent_spaces.LatentSpace(spaces.NBoxSpace(3, 0.0, 1.0), lambda sp, size, device="cuda": sp.uniform(size, device=device),
                                     lambda sp, z, size, device="cuda": sp.normal(z, 0.05, size, device=device))


def _synthetic_root(tmp_path, n):
    """raw_latents.npy with `n` seeded points in [0, 1]^3 and an 8 x 8 x 3 image per point whose bytes encode its row."""
    latents = np.random.default_rng(21).uniform(size=(n, 3)).astype(np.float32)
    np.save(tmp_path / "raw_latents.npy", latents)
    p = np.arange(8 * 8 * 3, dtype=np.int64).reshape(1, 8, 8, 3)
    images = ((np.arange(n, dtype=np.int64).reshape(n, 1, 1, 1) * 3 + p * 5) % 256).astype(np.uint8)
    images[:, 0, 0, 0] = np.arange(n)
    return str(tmp_path), latents, images


def _row_of(x, normalize):
    """The row an image batch (B, 3, 8, 8) was gathered from, from the byte at [0, 0, 0]."""
    v = x[:, 0, 0, 0].double()
    if normalize is not None:
        v = v * float(np.float32(normalize[1][0])) + float(np.float32(normalize[0][0]))
    return torch.round(v * 255.0).long()


def test_threedident_dataset_batches_and_trains(tmp_path):
    from cl_ica_amd import layers, losses, optim, spaces, threedident
    from cl_ica_amd.datasets import BatchLoader, ImageTable, ThreeDIdentDataset
    root, latents, images = _synthetic_root(tmp_path, 64)
    nz = IO.fixture_normalize()
    spaces.manual_seed(4)
    ds = ThreeDIdentDataset(root, _latent_space(), images=images, normalize=nz)
    assert len(ds) == sys.maxsize and len(ds.image_paths) == 64 and ds.image_paths[5].endswith("images/05.png")
    B = 37
    (z, zt), (x, xt) = ds.batch(B)
    for t, shp in ((z, (B, 3)), (zt, (B, 3)), (x, (B, 3, 8, 8)), (xt, (B, 3, 8, 8))):
        assert t.shape == shp and t.dtype == torch.float32 and t.is_cuda
    assert x.untyped_storage().data_ptr() == xt.untyped_storage().data_ptr()           # two halves of one gather's output
    row, row_t = _row_of(x, nz), _row_of(xt, nz)
    lat = torch.as_tensor(latents, device="cuda")
    assert torch.equal(z, lat[row]) and torch.equal(zt, lat[row_t])                    # each image is its latent's rendering
    assert (row != row_t).all()
    table = ImageTable(images)
    assert torch.equal(x, table.gather(row, nz)) and torch.equal(xt, table.gather(row_t, nz))
    assert IO.same_bits(x.cpu().numpy(), IO.gather_oracle(images, row.cpu().numpy(), *nz))
    # one item, the reference's structure
    (z1, zt1), (x1, xt1) = ds[0]
    assert z1.shape == (3,) and zt1.shape == (3,) and x1.shape == (3, 8, 8) and xt1.shape == (3, 8, 8)
    # an ImageTable instead of an array; no normalisation: ToTensor alone
    ds2 = ThreeDIdentDataset(root, _latent_space(), images=table)
    (za, _), (xa, _) = ds2.batch(5)
    assert torch.equal(xa, table.gather(_row_of(xa, None))) and torch.equal(za, lat[_row_of(xa, None)])
    # the batches drive three steps of threedident.train_step
    f = torch.nn.Sequential(layers.Flatten(), threedident.HipLinear(192, 3)).cuda()
    loss = losses.LpSimCLRLoss(p=2, tau=1.0, simclr_compatibility_mode=True, pow=True)
    opt = optim.Adam(f.parameters(), lr=1e-3)
    before = [p.detach().clone() for p in f.parameters()]
    it = iter(BatchLoader(ds, B))
    for _ in range(3):
        total, _per_item, _parts = threedident.train_step(next(it), loss, opt, f, sync=True)
        assert np.isfinite(total)
    assert all(bool(torch.isfinite(p).all()) for p in f.parameters())
    assert all(float((p.detach() - b).abs().max()) > 0 for p, b in zip(f.parameters(), before))
    # the supervised step unpacks the same structure
    v = threedident.train_step_supervised(next(it), threedident.HipMSELoss(), opt, f, sync=True)
    assert np.isfinite(v)


def test_threedident_dataset_dummy_images(tmp_path):
    from cl_ica_amd.datasets import ThreeDIdentDataset
    root, _latents, _images = _synthetic_root(tmp_path, 16)
    ds = ThreeDIdentDataset(root, _latent_space(), dummy_images=True)                  # reads no image file: there is none
    (z, zt), (x, xt) = ds.batch(9)
    assert z.shape == (9, 3) and zt.shape == (9, 3)
    for t in (x, xt):
        assert t.shape == (9, 1) and t.dtype == torch.float32 and t.is_cuda and bool((t == 1).all())


def test_sequential_dataset_and_batch_loader(tmp_path):
    from cl_ica_amd.datasets import BatchLoader, ImageTable, SequentialThreeDIdentDataset
    root, latents, images = _synthetic_root(tmp_path, 10)
    nz = IO.fixture_normalize()
    ds = SequentialThreeDIdentDataset(root, images=images, normalize=nz)
    assert len(ds) == 10 and ds.image_paths[3].endswith("images/3.png")
    z3, x3 = ds[3]
    assert z3.shape == (3,) and np.array_equal(z3.cpu().numpy(), latents[3])
    assert IO.same_bits(x3.cpu().numpy(), IO.gather_oracle(images, [3], *nz)[0])
    zb, xb = ds.batch([9, 0, 4])
    assert np.array_equal(zb.cpu().numpy(), latents[[9, 0, 4]]) and IO.same_bits(xb.cpu().numpy(), IO.gather_oracle(images, [9, 0, 4], *nz))
    with pytest.raises(IndexError):
        ds.batch([10])

    def epoch(loader):
        sizes, rows = [], []
        for z, x in loader:
            r = _row_of(x, nz)
            assert torch.equal(z, ds.latents[r])                     # latent and image of one batch row belong together
            sizes.append(x.shape[0]); rows.append(r.cpu())
        return sizes, torch.cat(rows).tolist()

    plain = BatchLoader(ds, 4)
    assert len(plain) == 3
    sizes, rows = epoch(plain)
    assert sizes == [4, 4, 2] and rows == list(range(10))            # the ragged last batch is kept
    sh = BatchLoader(ds, 4, shuffle=True, seed=123)
    s1, e1 = epoch(sh)
    s2, e2 = epoch(sh)
    assert s1 == s2 == [4, 4, 2] and sorted(e1) == sorted(e2) == list(range(10))      # every index once per epoch
    assert e1 != e2 and e1 != list(range(10))                        # a fresh permutation each epoch
    again = BatchLoader(ds, 4, shuffle=True, seed=123)
    assert epoch(again)[1] == e1 and epoch(again)[1] == e2           # the same seed repeats


def test_errors():
    from cl_ica_amd import _lib, ops
    from cl_ica_amd._lib import ClicaError
    dev = torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device="cuda")
    idx = torch.tensor([0, 1], device="cuda")
    with pytest.raises(ClicaError):
        ops.image_gather_norm(dev.cpu(), idx)                                        # CPU table
    with pytest.raises(ValueError):
        ops.image_gather_norm(dev.float(), idx)                                      # wrong dtype
    with pytest.raises(ValueError):
        ops.image_gather_norm(dev.permute(0, 3, 1, 2), idx)                          # not contiguous
    with pytest.raises(ValueError):
        ops.image_gather_norm(torch.zeros((2, 4, 4, 5), dtype=torch.uint8, device="cuda"), idx)      # C = 5
    with pytest.raises(ValueError):
        ops.image_gather_norm(dev, idx, mean=[0.1, 0.2, 0.3])                        # mean without std
    with pytest.raises(ValueError):
        ops.image_gather_norm(dev, idx, [0.1, 0.2], [0.1, 0.2])                      # two constants for three channels
    with pytest.raises(ValueError):
        ops.image_gather_norm(dev, idx[:0])                                          # empty batch
    with pytest.raises(ValueError):
        ops.image_gather_norm(dev, idx, out=torch.empty((3, 3, 4, 4), device="cuda"))
    with pytest.raises(ClicaError):
        ops.image_channel_sums(dev.cpu())
    # the C ABI's own checks (clica_image_gather_norm / clica_image_channel_stats follow clica_kitti_gather_pairs)
    L = _lib.load()
    out = torch.empty((2, 3, 4, 4), dtype=torch.float32, device="cuda")
    import ctypes as C
    m = (C.c_float * 3)(0.1, 0.2, 0.3)
    args = dict(table=dev.data_ptr(), n=2, H=4, W=4, C=3, index=idx.data_ptr(), n_index=2, mean=None, std=None, out=out.data_ptr())

    def call(**kw):
        a = dict(args, **kw)
        return L.clica_image_gather_norm(a["table"], a["n"], a["H"], a["W"], a["C"], a["index"], a["n_index"], a["mean"], a["std"], a["out"],
                                         _lib.stream_ptr())

    assert call() == 0
    for bad in (dict(table=None), dict(index=None), dict(out=None), dict(C=5), dict(C=0), dict(n_index=0), dict(n=0), dict(mean=m),
                dict(std=m), dict(out=out.data_ptr() + 4), dict(H=0)):
        assert call(**bad) == -1, bad
        assert b"clica_image_gather_norm" in L.clica_last_error()
    sums = torch.empty((2, 3, 2), dtype=torch.int64, device="cuda")
    assert L.clica_image_channel_stats(dev.data_ptr(), 2, 4, 4, 3, sums.data_ptr(), _lib.stream_ptr()) == 0
    for bad in ((None, 2, 4, 4, 3, sums.data_ptr()), (dev.data_ptr(), 2, 4, 4, 3, None), (dev.data_ptr(), 0, 4, 4, 3, sums.data_ptr()),
                (dev.data_ptr(), 2, 4, 4, 5, sums.data_ptr())):
        assert L.clica_image_channel_stats(*bad, _lib.stream_ptr()) == -1, bad
    torch.cuda.synchronize()
