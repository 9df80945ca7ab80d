"""clica_kitti_sample_pairs / StreamPairSampler and clica_kitti_gather_frames on the GPU, at the smallest shapes where they can go
wrong.  Expected batches come from oracle.np_oracle.kitti_getitem / kitti_collate for the (index, t) every launch reports; the stream
itself (permutation walk, epochs, counter, seeds, replay) is checked from those reports."""
import numpy as np
import pytest
import torch

from oracle import np_oracle as O

pytestmark = pytest.mark.gpu

E_INVALID = -1          # include/clica.h


def _tiny(hw=8, lens=(2, 2, 3), seed=2):
    """Three sequences of 2, 2 and 3 frames: 4 start items; the length-2 sequences clamp every time step."""
    rng = np.random.default_rng(seed)
    data = [rng.random((T, hw, hw)) < 0.3 for T in lens]
    lat = [rng.normal(size=(T, 3)).astype(np.float32) for T in lens]
    return {"pedestrians": data, "pedestrians_latents": lat}


def _synthetic_kitti(rng, n_seq=17, hw=64):
    """The 17-sequence set of test_gpu_next_rows (restated)."""
    lens = rng.integers(2, 40, size=n_seq)
    data = [rng.random((int(T), hw, hw)) < 0.1 for T in lens]
    lat = [rng.normal(size=(int(T), 3)).astype(np.float32) for T in lens]
    return {"pedestrians": data, "pedestrians_latents": lat}


def _cum(raw):
    return np.cumsum([len(s) - 1 for s in raw["pedestrians"]])


def _walk(raw, B, max_delta_t, seed, epochs=3):
    """`epochs` epochs of draws; every draw against the oracle; returns (per-draw (index, t), the permutation of every epoch)."""
    from cl_ica_amd.kitti_masks import dataset as D
    ds = D.KittiMasks(data=raw, max_delta_t=max_delta_t)
    cum = _cum(raw)
    n = len(ds)
    seq_start = np.concatenate([[0], np.cumsum([len(s) for s in raw["pedestrians"]])[:-1]])
    s = D.StreamPairSampler(ds, B, seed=seed)
    assert len(s) == n // B and s.issued == 0
    drawn, orders = [], []
    for k in range(epochs * len(s)):
        images, labels = s.draw()
        index, t, first, second = (v.cpu().numpy() for v in s.last_draw())
        order = s.order.cpu().numpy()
        r = k % len(s)
        if r == 0:
            orders.append(order.copy())
        assert np.array_equal(order, orders[-1])                                     # untouched within the epoch
        assert np.array_equal(index, order[r * B:(r + 1) * B]), (k, index)           # consecutive positions of the permutation
        assert t.min() >= 1 and t.max() <= max_delta_t
        items = [O.kitti_getitem(raw["pedestrians"], raw["pedestrians_latents"], cum, int(i), int(tt)) for i, tt in zip(index, t)]
        ref_img, ref_lab = O.kitti_collate(items)
        assert images.shape == ref_img.shape and images.dtype == torch.float32 and labels.shape == ref_lab.shape
        assert np.array_equal(images.cpu().numpy(), ref_img) and np.array_equal(labels.cpu().numpy(), ref_lab)      # bit-equal
        seq = np.searchsorted(cum, index, side="right")
        start = index - np.where(seq > 0, cum[np.maximum(seq - 1, 0)], 0)
        end = np.minimum(start + t, np.array([len(raw["pedestrians"][q]) for q in seq]) - 1)
        assert np.array_equal(first, seq_start[seq] + start) and np.array_equal(second, seq_start[seq] + end)
        drawn.append((index, t))
        assert s.issued == k + 1
        state = s.state.cpu().numpy()
        assert state[0] == k + 1 and state[1] == 0                                   # device counter = draws, ticket back at zero
    for e, order in enumerate(orders):
        assert np.array_equal(np.sort(order), np.arange(n))                          # a permutation of 0 .. n_items - 1
        seen = np.concatenate([d[0] for d in drawn[e * len(s):(e + 1) * len(s)]])
        assert len(set(seen.tolist())) == len(seen) == len(s) * B                    # no repeat within an epoch (the tail is dropped)
    assert len(orders) == epochs
    return drawn, orders


@pytest.mark.parametrize("max_delta_t", [1, 5])
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_tiny_table_every_draw(B, max_delta_t):
    """8 x 8 frames, n_items = 4: B = 3 drops a tail, B = 4 is one batch per epoch; three epochs, every draw against the oracle.
    (The permutations come from the seeded device generator: with 24 of them two consecutive ones CAN coincide for some seed; for the
    seed used here they do not.)"""
    drawn, orders = _walk(_tiny(), B, max_delta_t, seed=5)
    assert not np.array_equal(orders[0], orders[1]) and not np.array_equal(orders[1], orders[2])
    if max_delta_t == 1:
        assert all((t == 1).all() for _, t in drawn)


def test_synthetic_set_every_draw():
    """17 sequences of 64 x 64 frames, 32 pairs per batch, time steps 1 .. 3, three epochs."""
    raw = _synthetic_kitti(np.random.default_rng(5))
    drawn, orders = _walk(raw, 32, 3, seed=11)
    assert not np.array_equal(orders[0], orders[1]) and not np.array_equal(orders[1], orders[2])
    assert {int(v) for _, t in drawn for v in t} == {1, 2, 3}


def test_seed_determines_the_stream():
    from cl_ica_amd.kitti_masks import dataset as D
    ds = D.KittiMasks(data=_synthetic_kitti(np.random.default_rng(5)), max_delta_t=3)
    a, b, c = D.StreamPairSampler(ds, 32, seed=3), D.StreamPairSampler(ds, 32, seed=3), D.StreamPairSampler(ds, 32, seed=4)
    differs_index = differs_t = False
    for _ in range(len(a) + 2):                                                      # across an epoch boundary
        (ia, la), (ib, lb), (ic, lc) = a.draw(), b.draw(), c.draw()
        assert torch.equal(ia, ib) and torch.equal(la, lb)
        da, db, dc = a.last_draw(), b.last_draw(), c.last_draw()
        assert all(torch.equal(x, y) for x, y in zip(da, db))
        differs_index |= not torch.equal(da[0], dc[0])
        differs_t |= not torch.equal(da[1], dc[1])
    assert differs_index and differs_t


@pytest.mark.parametrize("case", ["tiny", "synthetic"])
def test_replayed_graph_walks_the_same_stream(case):
    """k eager draws and k replays of ONE captured draw_into give bit-equal batches, k crossing an epoch boundary: the launch advances
    its own counter, replayed() keeps the host count and the refill in step."""
    from cl_ica_amd.kitti_masks import dataset as D
    if case == "tiny":
        ds, B = D.KittiMasks(data=_tiny(), max_delta_t=5), 2
    else:
        ds, B = D.KittiMasks(data=_synthetic_kitti(np.random.default_rng(5)), max_delta_t=3), 32
    eager, graphed = D.StreamPairSampler(ds, B, seed=9), D.StreamPairSampler(ds, B, seed=9)
    k = len(eager) + 3
    want = []
    for _ in range(k):
        img, lab = eager.draw()
        want.append((img, lab, eager.last_draw()))
    images = torch.zeros(graphed.image_shape, device="cuda")
    labels = torch.zeros(graphed.label_shape, device="cuda")
    graphed.prepare()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.draw_into(images, labels)
    assert graphed.issued == 0 and int(graphed.state[0]) == 0                        # the capture executed and counted nothing
    for j in range(k):
        graph.replay()
        graphed.replayed()
        assert torch.equal(images, want[j][0]) and torch.equal(labels, want[j][1]), j
        assert all(torch.equal(x, y) for x, y in zip(graphed.last_draw(), want[j][2])), j
    assert graphed.issued == k and int(graphed.state[0]) == k and int(eager.state[0]) == k


def test_time_steps_are_uniform():
    """2 x 2 frames, 1000 pairs per batch, max_delta_t = 4, 20 draws: N = 20 000 time steps, each class frequency within
    5 sqrt(1/4 3/4 / N) = 0.0153 of 1/4 (five standard deviations of a binomial share; the seed is fixed, the outcome deterministic)."""
    from cl_ica_amd.kitti_masks import dataset as D
    rng = np.random.default_rng(1)
    raw = {"pedestrians": [rng.random((126, 2, 2)) < 0.5 for _ in range(8)],
           "pedestrians_latents": [rng.normal(size=(126, 3)).astype(np.float32) for _ in range(8)]}
    ds = D.KittiMasks(data=raw, max_delta_t=4)
    assert len(ds) == 1000
    s = D.StreamPairSampler(ds, 1000, seed=7)
    images = torch.empty(s.image_shape, device="cuda")
    ts = []
    for _ in range(20):
        s.draw_into(images)
        ts.append(s.last_draw()[1].cpu().numpy())
    ts = np.concatenate(ts)
    N = ts.size
    assert N == 20000 and ts.min() == 1 and ts.max() == 4
    bound = 5.0 * np.sqrt(0.25 * 0.75 / N)
    freq = np.array([(ts == v).mean() for v in (1, 2, 3, 4)])
    print("time-step frequencies", freq, "bound", bound)
    assert np.all(np.abs(freq - 0.25) <= bound), (freq, bound)


def test_refusals_before_any_launch():
    from cl_ica_amd import _lib
    from cl_ica_amd.kitti_masks import dataset as D
    lib = _lib.load()
    ds = D.KittiMasks(data=_tiny(), max_delta_t=5)
    n = len(ds)
    order = torch.arange(n, device="cuda")
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    images = torch.full((2 * n, 1, 8, 8), -7.0, device="cuda")
    labels = torch.full((2 * n, 3), -7.0, device="cuda")

    def call(**over):
        a = dict(frames=ds.frames.data_ptr(), frame_elems=64, n_frames=ds.frames.shape[0], latents=ds.frame_latents.data_ptr(), n_lat=3,
                 cumlens=ds.cumlens_dev.data_ptr(), seq_start=ds.seq_start.data_ptr(), seq_len=ds.seq_len.data_ptr(), n_seq=3, n_items=n,
                 order=order.data_ptr(), B=2, mdt=5, seed=1, state=state.data_ptr(), images=images.data_ptr(), labels=labels.data_ptr())
        a.update(over)
        return lib.clica_kitti_sample_pairs(a["frames"], a["frame_elems"], a["n_frames"], a["latents"], a["n_lat"], a["cumlens"], a["seq_start"],
                                            a["seq_len"], a["n_seq"], a["n_items"], a["order"], a["B"], a["mdt"], a["seed"], a["state"],
                                            a["images"], a["labels"], None, None, None, None, _lib.stream_ptr())

    assert call(B=n + 1) == E_INVALID and b"no full batch" in lib.clica_last_error()
    assert call(mdt=0) == E_INVALID
    assert call(frame_elems=6) == E_INVALID
    assert call(B=0) == E_INVALID
    for name in ("frames", "cumlens", "seq_start", "seq_len", "order", "state", "images"):
        assert call(**{name: None}) == E_INVALID, name
    assert call(latents=None) == E_INVALID                                           # labels requested without a latent table
    assert call(images=images.data_ptr() + 4) == E_INVALID                           # 16-byte alignment
    torch.cuda.synchronize()
    assert int(state[0]) == 0 and float(images.max()) == -7.0 and float(labels.max()) == -7.0      # nothing ran
    with pytest.raises(ValueError):
        D.StreamPairSampler(ds, n + 1)
    assert call() == 0                                                               # and the accepted call runs
    torch.cuda.synchronize()
    assert int(state[0]) == 1 and float(images[:4].min()) >= 0.0 and float(images[4:].max()) == -7.0      # two pairs written, no more


def test_gather_frames_matches_host_indexing():
    from cl_ica_amd import ops
    from cl_ica_amd.kitti_masks import dataset as D
    raw = _synthetic_kitti(np.random.default_rng(5))
    ds = D.KittiMasks(data=raw, max_delta_t=3)
    table = np.concatenate([np.asarray(s).astype(np.uint8) for s in raw["pedestrians"]], 0)
    lat = np.concatenate(raw["pedestrians_latents"], 0)
    F = table.shape[0]
    ids = np.concatenate([[0, F - 1, F - 1, 0], np.random.default_rng(1).integers(0, F, size=61)]).astype(np.int64)
    images, labels = ops.kitti_gather_frames(ds.frames, torch.as_tensor(ids), ds.frame_latents)
    assert images.shape == (65, 1, 64, 64) and labels.shape == (65, 3)
    assert np.array_equal(images.cpu().numpy(), (table[ids] * np.uint8(255))[:, None].astype(np.float32) / 255.0)
    assert np.array_equal(labels.cpu().numpy(), lat[ids])
    only_images, none = ops.kitti_gather_frames(ds.frames, torch.as_tensor(ids[:3]))
    assert none is None and torch.equal(only_images, images[:3])
    for bad in ([0, F], [-1, 0]):                                                    # host ids outside the table are refused
        with pytest.raises(ValueError):
            ops.kitti_gather_frames(ds.frames, torch.as_tensor(bad))
    # the items' first frames, as the evaluation asks for them
    items = np.arange(len(ds))
    first, _ = ds.pair_frames(torch.as_tensor(items), torch.ones(len(ds), dtype=torch.int64))
    assert np.array_equal(ds.first_frame_ids(items), first.cpu().numpy())
