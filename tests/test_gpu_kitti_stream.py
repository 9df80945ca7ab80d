"""The three kernels of csrc/kitti_pairs.hip in every launch round, grid stride, width and counter word, bit for bit.

test_gpu_kitti_sampler.py checks batches for the (index, t) a launch REPORTS; here the reports themselves are compared with the host
restatement of the stream (tests/kitti_stream_oracle.py: Philox4x32-10 keyed by both seed words, counter (pair, c >> 32, c, "KITT"),
multiply-high time step, the permutation walk), so a launch that draws one time step per workgroup, ignores a high word, leaves a batch
position of a later round unwritten or strides wrongly past the grid cap cannot pass.  Frames are tiny so that large counts cost nothing."""
import numpy as np
import pytest
import torch

import kitti_stream_oracle as KS
from oracle import np_oracle as O
from test_gpu_kitti_sampler import _synthetic_kitti, _tiny

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
SPARE = 3               # rows behind the batch in every output buffer: they keep the sentinel


def _raw(lens, hw, n_lat=3, seed=0, p=0.4):
    rng = np.random.default_rng(seed)
    return {"pedestrians": [rng.random((int(T), hw, hw)) < p for T in lens],
            "pedestrians_latents": [rng.normal(size=(int(T), n_lat)).astype(np.float32) for T in lens]}


def _tables(raw):
    seq_len = np.array([len(s) for s in raw["pedestrians"]], np.int64)
    return np.cumsum(seq_len - 1), np.concatenate([[0], np.cumsum(seq_len)[:-1]]), seq_len


def _expect_batch(raw, cum, index, t):
    items = [O.kitti_getitem(raw["pedestrians"], raw["pedestrians_latents"], cum, int(i), int(tt)) for i, tt in zip(index, t)]
    return O.kitti_collate(items)


def _stream(raw, B, max_delta_t, seed, draws, graphed=False):
    """`draws` launches of a StreamPairSampler, eager or as replays of ONE captured launch, each against KS.draw and the oracle's
    collate; outputs go into buffers with SPARE sentinel rows behind the batch.  Returns the per-draw (index, t)."""
    from cl_ica_amd.kitti_masks import dataset as D
    ds = D.KittiMasks(data=raw, max_delta_t=max_delta_t)
    cum, seq_start, seq_len = _tables(raw)
    s = D.StreamPairSampler(ds, B, seed=seed)
    big_i = torch.full((2 * B + SPARE,) + s.image_shape[1:], SENTINEL, device="cuda")
    big_l = torch.full((2 * B + SPARE, s.label_shape[1]), SENTINEL, device="cuda")
    images, labels = big_i[:2 * B], big_l[:2 * B]
    graph = None
    if graphed:
        s.prepare()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            s.draw_into(images, labels)
        assert s.issued == 0 and s.state.tolist() == [0, 0]                          # the capture executed and counted nothing
    out = []
    for c in range(draws):
        if graphed:
            order = s.order.cpu().numpy()                                            # (replayed() refills it BEHIND the last draw of an epoch)
            graph.replay()
        else:
            s.draw_into(images, labels)
            order = s.order.cpu().numpy()
        got = [v.cpu().numpy() for v in s.last_draw()]
        if graphed:
            s.replayed()
        want = KS.draw(order, cum, seq_start, seq_len, B, c, seed, max_delta_t)
        for name, g, w in zip(("index", "t", "first", "second"), got, want):
            assert np.array_equal(g, w), (name, "draw", c, "first wrong pair", int(np.flatnonzero(g != w)[0]))
        ref_img, ref_lab = _expect_batch(raw, cum, want[0], want[1])
        assert np.array_equal(images.cpu().numpy(), ref_img) and np.array_equal(labels.cpu().numpy(), ref_lab), c
        assert s.state.tolist() == [c + 1, 0] and s.issued == c + 1                  # counter = draws, ticket back at zero
        assert bool((big_i[2 * B:] == SENTINEL).all()) and bool((big_l[2 * B:] == SENTINEL).all())
        out.append((want[0], want[1]))
    return out


# ====================================================================================================================== launch rounds
@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "replayed"])
@pytest.mark.parametrize("B", [1027, 2049])
def test_later_rounds_of_the_sampling_launch(B, graphed):
    """More than 4 x 256 pairs: the 256 workgroups loop.  B = 1027: a second round in which one workgroup works, with three of its four
    groups; B = 2049: three rounds.  2 x 2 frames, 2060 items, two epochs (B = 1027: two batches each, 2049: one)."""
    raw = _raw([104] * 20, hw=2, seed=B)
    assert int(_tables(raw)[0][-1]) == 2060
    drawn = _stream(raw, B, max_delta_t=5, seed=2 ** 32 + 5, draws=2 * (2060 // B), graphed=graphed)
    t = drawn[0][1]
    # (what the exact comparison above already implies, said directly: the four pairs of a workgroup do not share one draw -- a share
    # of 1 / 125 of the 256 first-round workgroups is expected to hold four equal steps by chance)
    assert sum(len(set(t[g:g + 4].tolist())) == 1 for g in range(0, 1024, 4)) < 32 and set(t.tolist()) == {1, 2, 3, 4, 5}


# ====================================================================================================================== exact time steps
@pytest.mark.parametrize("max_delta_t", [1, 5, 2 ** 31 - 1])
@pytest.mark.parametrize("shape", ["tiny", "synthetic"])
def test_time_steps_equal_the_restatement(shape, max_delta_t):
    """Seeds 5, 2^32 + 5 (same low word) and 2^63 + 1 (top bit) at the shapes of test_gpu_kitti_sampler's walks; past one epoch each.  The
    three streams of time steps differ wherever there is more than one value to draw."""
    if shape == "tiny":
        raw, B, draws = _tiny(), 3, 3
    else:
        raw, B = _synthetic_kitti(np.random.default_rng(5)), 32
        draws = int(_tables(raw)[0][-1]) // B + 1
    ts = [np.concatenate([t for _, t in _stream(raw, B, max_delta_t, seed, draws)]) for seed in (5, 2 ** 32 + 5, 2 ** 63 + 1)]
    if max_delta_t == 1:
        assert all((t == 1).all() for t in ts)
    else:
        assert not np.array_equal(ts[0], ts[1]) and not np.array_equal(ts[0], ts[2]) and not np.array_equal(ts[1], ts[2])


def test_counter_beyond_32_bits():
    """state[0] preset to 2^32 - 2 through ops.kitti_sample_pairs: four draws at c = 2^32 - 2 .. 2^32 + 1.  7 items, 2 pairs per batch: three
    steps per epoch, and 2^32 mod 3 = 1, so both the walk (c mod steps_per_epoch) and the Philox block word see the high word."""
    from cl_ica_amd import ops
    from cl_ica_amd.kitti_masks import dataset as D
    raw = _raw([2, 2, 3, 4], hw=4, seed=3)
    ds = D.KittiMasks(data=raw, max_delta_t=2 ** 31 - 1)
    cum, seq_start, seq_len = _tables(raw)
    B, seed, mdt = 2, 2 ** 32 + 5, 2 ** 31 - 1
    assert len(ds) == 7
    order_h = np.random.default_rng(0).permutation(7)
    order = torch.tensor(order_h, device="cuda")
    c0 = 2 ** 32 - 2
    state = torch.tensor([c0, 0], dtype=torch.int64, device="cuda")
    images = torch.empty((2 * B, 1, 4, 4), device="cuda")
    labels = torch.empty((2 * B, 3), device="cuda")
    drawn = torch.zeros((4, B), dtype=torch.int64, device="cuda")
    for c in range(c0, c0 + 4):
        ops.kitti_sample_pairs(ds.frames, ds.frame_latents, ds.cumlens_dev, ds.seq_start, ds.seq_len, order, B, mdt, seed, state, images, labels, drawn)
        want = KS.draw(order_h, cum, seq_start, seq_len, B, c, seed, mdt)
        assert np.array_equal(drawn.cpu().numpy(), np.stack(want)), c
        ref_img, ref_lab = _expect_batch(raw, cum, want[0], want[1])
        assert np.array_equal(images.cpu().numpy(), ref_img) and np.array_equal(labels.cpu().numpy(), ref_lab), c
        assert state.tolist() == [c + 1, 0]
    assert state.tolist() == [2 ** 32 + 2, 0]
    assert (KS.time_step(seed, np.arange(B), 2 ** 32, mdt) != KS.time_step(seed, np.arange(B), 0, mdt)).all()     # (the block word matters)
    assert (2 ** 32) % 3 != 0


# ====================================================================================================================== shapes
@pytest.mark.parametrize("hw,B", [(34, 5), (4, 3)])
def test_frame_sizes(hw, B):
    """34 x 34 = 289 quads: a second pass of the 256-thread copy loop with 33 threads; 4 x 4 = 4 quads; B is no multiple of 4."""
    _stream(_raw([3, 4, 2, 5, 3], hw=hw, seed=hw), B, max_delta_t=3, seed=11, draws=4)


@pytest.mark.parametrize("n_lat", [1, 2, 128])
def test_label_widths(n_lat):
    _stream(_raw([3, 4, 2, 5, 3], hw=4, n_lat=n_lat, seed=n_lat), 5, max_delta_t=3, seed=13, draws=3)


def test_label_width_129_is_refused_before_any_launch():
    from cl_ica_amd._lib import ClicaError
    from cl_ica_amd.kitti_masks import dataset as D
    ds = D.KittiMasks(data=_raw([3, 4], hw=4, n_lat=129, seed=1), max_delta_t=3)
    s = D.StreamPairSampler(ds, 2, seed=1)
    images = torch.full(s.image_shape, SENTINEL, device="cuda")
    labels = torch.full(s.label_shape, SENTINEL, device="cuda")
    with pytest.raises(ClicaError, match="latent table of 1..128 columns"):
        s.draw_into(images, labels)
    torch.cuda.synchronize()
    assert s.state.tolist() == [0, 0] and bool((images == SENTINEL).all()) and bool((labels == SENTINEL).all())
    s.draw_into(images)                                                              # images alone: the width does not enter
    assert s.state.tolist() == [1, 0] and float(images.min()) >= 0.0 and bool((labels == SENTINEL).all())


@pytest.mark.parametrize("n_seq", [1, 2, 7, 8, 9, 64, 65])
def test_binary_search_at_every_boundary(n_seq):
    """Sequences of two frames: one item each, so every index sits on a cumlens boundary; search_steps changes at the powers of two.  One
    pair per batch, one whole epoch: every item exactly once."""
    drawn = _stream(_raw([2] * n_seq, hw=2, seed=n_seq), 1, max_delta_t=5, seed=17, draws=n_seq)
    assert sorted(int(i[0]) for i, _ in drawn) == list(range(n_seq))


# ====================================================================================================================== the grid cap
def test_gathers_stride_past_the_grid_cap():
    """90 000 pairs / 180 000 single 4 x 4 frames: 2813 workgroups' worth of quads and 2110 of label words against the cap of 2048, so
    the image loop and the label loop (n_lat = 3) both stride."""
    from cl_ica_amd import ops
    rng = np.random.default_rng(4)
    F, P = 50, 90000
    table = (rng.random((F, 4, 4)) < 0.5).astype(np.uint8)
    lat = rng.normal(size=(F, 3)).astype(np.float32)
    assert len(np.unique(table.reshape(F, -1), axis=0)) == F
    frames, latents = torch.tensor(table, device="cuda"), torch.tensor(lat, device="cuda")
    first, second = rng.integers(0, F, size=P), rng.integers(0, F, size=P)
    assert 2 * P * 4 > 2048 * 256 and 2 * P * 3 > 2048 * 256
    images, labels = ops.kitti_gather_pairs(frames, torch.tensor(first), torch.tensor(second), latents)
    ids = np.stack([first, second], 1).reshape(-1)                                   # interleaved, as the batch
    want_img = table[ids][:, None].astype(np.float32)                                # (0 / 1 bytes: 255 / 255.0 is exactly 1)
    assert images.shape == (2 * P, 1, 4, 4) and labels.shape == (2 * P, 3)
    assert np.array_equal(images.cpu().numpy(), want_img) and np.array_equal(labels.cpu().numpy(), lat[ids])
    images, labels = ops.kitti_gather_frames(frames, torch.tensor(ids), latents)
    assert images.shape == (2 * P, 1, 4, 4) and labels.shape == (2 * P, 3)
    assert np.array_equal(images.cpu().numpy(), want_img) and np.array_equal(labels.cpu().numpy(), lat[ids])


# ====================================================================================================================== bytes and ids
def _byte_formula(v):
    return (v.astype(np.uint8) * np.uint8(255)).astype(np.float32) / 255.0


def test_all_byte_values_through_all_three_kernels():
    """Masks hold 0 / 1; every other byte follows the reference's uint8 wrap-around, astype(uint8) * 255 -> float32 / 255."""
    from cl_ica_amd import ops
    table = np.arange(256, dtype=np.uint8).reshape(4, 8, 8)
    want = _byte_formula(table)
    assert want[0, 0, 1] == 1.0 and want[0, 0, 2] == np.float32(254) / np.float32(255) and len(np.unique(want)) == 256
    lat = np.arange(12, dtype=np.float32).reshape(4, 3)
    frames = torch.tensor(table, device="cuda")
    images, _ = ops.kitti_gather_pairs(frames, torch.tensor([0, 2]), torch.tensor([1, 3]))
    assert np.array_equal(images.cpu().numpy(), want[:, None])
    images, _ = ops.kitti_gather_frames(frames, torch.tensor([3, 2, 1, 0]))
    assert np.array_equal(images.cpu().numpy(), want[::-1][:, None])
    # one sequence of the four frames: items 0, 1, 2, all drawn by every batch of three; item 2 always ends on frame 3
    raw = {"pedestrians": [table], "pedestrians_latents": [lat]}
    item = O.kitti_getitem([table], [lat], np.array([3]), 1, 2)
    assert np.array_equal(item[0][0], want[1]) and np.array_equal(item[1][0], want[3])      # the oracle _stream compares with IS the formula
    seen = set()
    for index, t in _stream(raw, 3, max_delta_t=3, seed=19, draws=2):
        seen |= set(index.tolist()) | set(np.minimum(index + t, 3).tolist())
    assert seen == {0, 1, 2, 3}


def test_device_ids_outside_the_table_are_clamped():
    """ops.kitti_gather_frames: ids that already live on the device are not checked on the host; the kernel gives the nearest frame."""
    from cl_ica_amd import ops
    rng = np.random.default_rng(6)
    F = 9
    table = (rng.random((F, 4, 4)) < 0.5).astype(np.uint8)
    lat = rng.normal(size=(F, 3)).astype(np.float32)
    ids = torch.tensor([-3, F + 2, 4, -1, F], device="cuda")
    images, labels = ops.kitti_gather_frames(torch.tensor(table, device="cuda"), ids, torch.tensor(lat, device="cuda"))
    near = np.array([0, F - 1, 4, 0, F - 1])
    assert np.array_equal(images.cpu().numpy(), table[near][:, None].astype(np.float32)) and np.array_equal(labels.cpu().numpy(), lat[near])
