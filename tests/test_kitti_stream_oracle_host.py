"""tests/kitti_stream_oracle.py pinned on the host (no GPU): the generator to the published Philox4x32-10 known answers, the
multiply-high map at its ends, and the index walk to oracle.np_oracle.kitti_getitem."""
import numpy as np
import pytest

import kitti_stream_oracle as KS
from oracle import np_oracle as O

# Random123's kat_vectors for philox4x32 with 10 rounds: counter, key -> output
KNOWN_ANSWERS = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("counter,key,want", KNOWN_ANSWERS)
def test_philox_known_answers(counter, key, want):
    assert tuple(int(w) for w in KS.philox4x32_10(counter, key)) == want


def test_philox_arrays_equal_scalars():
    """The vectorised form (what draw() uses) word for word against the scalar form, high bits of every word set."""
    i = np.array([0, 1, 2, 1026, 2048, 0xFFFFFFFF], np.int64)
    got = KS.philox4x32_10((i, 0xFFFFFFFE, 0x80000001, KS.STREAM_TIME_STEP), (0x80000005, 0xC0000001))
    for j, iv in enumerate(i):
        one = KS.philox4x32_10((int(iv), 0xFFFFFFFE, 0x80000001, KS.STREAM_TIME_STEP), (0x80000005, 0xC0000001))
        assert [int(w[j]) for w in got] == [int(w) for w in one]
    known = KS.philox4x32_10(tuple(np.array([w, w]) for w in KNOWN_ANSWERS[2][0]), KNOWN_ANSWERS[2][1])
    assert [int(w[1]) for w in known] == list(KNOWN_ANSWERS[2][2])


@pytest.mark.parametrize("max_delta_t", [1, 5, 2 ** 31 - 1])
def test_multiply_high_map_ends(max_delta_t):
    assert int(KS.mulhi_step(0, max_delta_t)) == 1
    assert int(KS.mulhi_step(0xFFFFFFFF, max_delta_t)) == max_delta_t
    words = np.arange(0, 2 ** 32, 2 ** 32 // 4099, dtype=np.int64)
    t = KS.mulhi_step(words, max_delta_t)
    assert t.min() >= 1 and t.max() <= max_delta_t and (np.diff(t) >= 0).all()
    assert np.array_equal(t, 1 + np.array([(int(w) * max_delta_t) >> 32 for w in words]))        # against Python's unbounded integers


def test_time_step_reads_every_word_of_counter_and_seed():
    """time_step = the map of output word 0 of the documented counter / key; pair, both counter words and both seed words all enter."""
    seed, c, mdt = (0xC0000001 << 32) | 0x80000005, (7 << 32) | 0x80000001, 2 ** 31 - 1
    i = np.arange(5)
    w0 = KS.philox4x32_10((i, 7, 0x80000001, 0x4B495454), (0x80000005, 0xC0000001))[0]
    base = KS.time_step(seed, i, c, mdt)
    assert np.array_equal(base, KS.mulhi_step(w0, mdt))
    assert int(KS.time_step(seed, 3, c, mdt)) == int(base[3])
    assert len(set(base.tolist())) == 5
    for other in (KS.time_step(seed ^ 1, i, c, mdt), KS.time_step(seed ^ (1 << 32), i, c, mdt), KS.time_step(seed, i, c ^ 1, mdt),
                  KS.time_step(seed, i, c ^ (1 << 32), mdt)):
        assert (other != base).all()
    assert (KS.time_step(seed, i, c, 1) == 1).all()


@pytest.mark.parametrize("B", [1, 2, 3, 4])
@pytest.mark.parametrize("max_delta_t", [1, 5])
def test_draw_equals_getitem_on_the_tiny_set(B, max_delta_t):
    """draw() item by item against oracle.np_oracle.kitti_getitem on the three-sequence set of test_gpu_kitti_sampler (every frame and
    latent row of it is distinct, so equal images and labels mean equal frames), across two epochs and at a counter beyond 2^32."""
    from test_gpu_kitti_sampler import _tiny
    raw = _tiny()
    data, lat = raw["pedestrians"], raw["pedestrians_latents"]
    frames = np.concatenate([np.asarray(s).astype(np.uint8) for s in data], 0)
    flat = np.concatenate(lat, 0)
    assert len(np.unique(frames.reshape(len(frames), -1), axis=0)) == len(frames) and len(np.unique(flat, axis=0)) == len(flat)
    seq_len = np.array([len(s) for s in data])
    seq_start = np.concatenate([[0], np.cumsum(seq_len)[:-1]])
    cum = np.cumsum(seq_len - 1)
    n = int(cum[-1])
    rng = np.random.default_rng(B)
    steps = n // B
    for c in list(range(2 * steps)) + [2 ** 32 + 1]:
        order = rng.permutation(n)
        index, t, first, second = KS.draw(order, cum, seq_start, seq_len, B, c, seed=2 ** 32 + 5, max_delta_t=max_delta_t)
        assert np.array_equal(index, order[(c % steps) * B:(c % steps) * B + B])
        assert t.min() >= 1 and t.max() <= max_delta_t
        for j in range(B):
            f, s, l1, l2 = O.kitti_getitem(data, lat, cum, int(index[j]), int(t[j]))
            assert np.array_equal(f[0], frames[first[j]].astype(np.float32)) and np.array_equal(s[0], frames[second[j]].astype(np.float32))
            assert np.array_equal(l1, flat[first[j]]) and np.array_equal(l2, flat[second[j]])
