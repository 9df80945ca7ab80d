"""The stream of clica_kitti_sample_pairs (csrc/kitti_pairs.hip: sample_pairs_k) restated on the host in integer arithmetic only.

philox4x32_10 is the published Philox4x32 with ten rounds (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11;
multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85), pinned to its known answers by
test_kitti_stream_oracle_host.py.  The counter and key of the time-step draw are those of the kernel's header comment and of the Philox
constructor in csrc/sampler_dev.h:  counter = (pair i, c >> 32, c & 0xffffffff, "KITT"),  key = (seed low word, seed high word),  and the
time step is the multiply-high map of the first output word onto 1 .. max_delta_t.  Every function takes scalars or arrays."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
STREAM_TIME_STEP = 0x4B495454          # "KITT"


def _u64(x):
    return x.astype(np.uint64) if isinstance(x, np.ndarray) else np.asarray(int(x), dtype=np.uint64)


def philox4x32_10(counter, key):
    """counter: four 32-bit words, key: two (ints or equally shaped integer arrays) -> the four output words (np.uint64 holding 32 bits)."""
    a0, a1, a2, a3 = (_u64(w) & M32 for w in counter)
    k0, k1 = (_u64(w) & M32 for w in key)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * a0          # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(0xCD9E8D57) * a2
        a0, a1, a2, a3 = (p1 >> np.uint64(32)) ^ a1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ a3 ^ k1, p0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return a0, a1, a2, a3


def mulhi_step(word, max_delta_t):
    """1 + ((word * max_delta_t) >> 32): a 32-bit word onto 1 .. max_delta_t (max_delta_t < 2^31: the product fits 64 bits)."""
    return (np.uint64(1) + ((_u64(word) * np.uint64(max_delta_t)) >> np.uint64(32))).astype(np.int64)


def time_step(seed, i, c, max_delta_t):
    """Time step of pair `i` (int or array) of batch `c` (the 64-bit batch counter) under the 64-bit `seed`."""
    seed, c = int(seed) & (2 ** 64 - 1), int(c) & (2 ** 64 - 1)
    i = np.asarray(i, np.int64).astype(np.uint64) & M32
    word0 = philox4x32_10((i, c >> 32, c & 0xFFFFFFFF, STREAM_TIME_STEP), (seed & 0xFFFFFFFF, seed >> 32))[0]
    return mulhi_step(word0, max_delta_t)


def draw(order, cumlens, seq_start, seq_len, B, c, seed, max_delta_t):
    """Batch `c` of the stream -> (index, t, first, second), int64 [B] each: the `% steps_per_epoch` walk over the epoch's permutation
    `order`, searchsorted(side="right") over the cumulative item counts, and the clamp at the sequence's last frame."""
    order, cumlens = np.asarray(order, np.int64), np.asarray(cumlens, np.int64)
    seq_start, seq_len = np.asarray(seq_start, np.int64), np.asarray(seq_len, np.int64)
    n_items = int(cumlens[-1])
    assert order.shape == (n_items,) and 1 <= B <= n_items
    steps_per_epoch = n_items // B
    r0 = (int(c) % steps_per_epoch) * B
    index = order[r0:r0 + B]
    t = time_step(seed, np.arange(B), c, max_delta_t)
    seq = np.searchsorted(cumlens, index, side="right")
    start = index - np.where(seq > 0, cumlens[np.maximum(seq - 1, 0)], 0)
    end = np.minimum(start + t, seq_len[seq] - 1)
    return index, t, seq_start[seq] + start, seq_start[seq] + end
