"""The cases of the channels-last BatchNorm2d unit (csrc/bn2d_nhwc.hip), shared by tests/test_bn2d_nhwc_host.py (CPU: every case
satisfies the oracle's caps) and tests/test_gpu_bn2d_nhwc.py.  A case's rows [M = N H W, C] (tests/bn2d_oracle.py) ARE the NHWC tensor.

The table: all of bn2d_oracle.SHAPES at their recorded attempts, then shapes for what the NCHW table does not reach in the "rows"
geometry of csrc/bn2d.h (rows_geometry): VEC = 4 | 1 channels per lane, lpr lanes per row, chunks of 64 lanes along C, S row splits,
mg merging threads per channel, T row tiles."""
import functools

import numpy as np

import bn2d_oracle as B

# (N, C, H, W) -> what it reaches
EXTRA_SHAPES = [(3, 320, 5, 7),        # C > 256, a multiple of 64: two chunks, the second partial (80 lanes of 4 channels)
                (7, 6, 9, 11),         # C % 4 = 2: a channel per lane, lpr = 8
                (33, 128, 4, 4),       # lpr = 32: two rows per wave
                (5, 516, 3, 3),        # C % 4 = 0 but not % 64: three chunks, one lane in the last
                (1, 4, 1, 2),          # M = 2, one lane per row
                (130, 12, 8, 8),       # M = 8320: S = 5 with 16 merging threads per channel (ranges past S are empty), 17 tiles (ragged)
                # the geometry's own boundaries
                (5, 260, 6, 6),        # two chunks AND S = 2, one merging thread per channel (mg = 1, ms = 2)
                (11, 64, 10, 10)]      # C = 64: four rows per wave, S = 3 ragged (367 + 367 + 366 rows, no multiple of the 16-row step), 9 tiles
# (N, C, H, W, cls, residual) -> attempt, where the first draw misses a cap (found from the inputs and the fp64 oracle alone;
# asserted by tests/test_bn2d_nhwc_host.py)
EXTRA_ATTEMPT = {(1, 4, 1, 2, 1, False): 1, (1, 4, 1, 2, 1, True): 1,
                 (130, 12, 8, 8, 0, False): 3, (130, 12, 8, 8, 0, True): 1, (130, 12, 8, 8, 1, True): 1,
                 (11, 64, 10, 10, 0, False): 1}
SHAPES = list(B.SHAPES) + EXTRA_SHAPES
EVAL_SHAPES = [(3, 7, 2, 2), (5, 516, 3, 3), (11, 64, 10, 10)]
# C % 4 == 0: the scalar accesses keep the lanes' channels and the reduction order, so the same bits
UNALIGNED_SHAPES = [(8, 512, 2, 2), (3, 320, 5, 7), (130, 12, 8, 8), (11, 64, 10, 10)]
# The cap on S (64 splits with one merging thread per channel at C = 256) is reached from M = 8193 on; with that many rows a draw with a
# kink leaves out too many of 256 channels: this shape runs at slope 1 (no kink) only.
CAPPED_SHAPE = (33, 256, 20, 25)       # M = 16500: S = 64 of 258 rows (the last 246), 516 ragged tiles


def attempt_of(N, C, H, W, cls, residual):
    key = (N, C, H, W, cls, bool(residual))
    return EXTRA_ATTEMPT.get(key, B.SEED_ATTEMPT.get(key, 0))


@functools.lru_cache(maxsize=None)
def reference(N, C, H, W, cls, residual, slope):
    """(inputs, forward, backward) of one case, computed once and shared; treat as read-only.  Cases of bn2d_oracle.SHAPES are
    bn2d_oracle.reference's own objects."""
    if (N, C, H, W) in B.SHAPES:
        return B.reference(N, C, H, W, cls, residual, slope)
    c = B.make_case(N, C, H, W, cls, residual, attempt=attempt_of(N, C, H, W, cls, residual))
    fw = B.forward(c, slope)
    return c, fw, B.backward(fw, c, slope)


def sweep():
    for shape in SHAPES:
        for cls in range(len(B.CLASSES)):
            for residual in (False, True):
                yield shape, cls, residual


def rows_of(t):
    """The rows [N H W, C] of a channels-last tensor [N, C, H, W] (a view of its memory)."""
    N, C, H, W = t.shape
    return np.asarray(t.permute(0, 2, 3, 1).reshape(N * H * W, C).detach().cpu().numpy())


# csrc/bn2d.h rows_geometry, restated: the test of the planner compares the library's workspace size with it
def rows_splits(M, C):
    vec = 4 if C % 4 == 0 else 1
    U = C // vec
    lpr = 1
    while lpr < U and lpr < 64:
        lpr *= 2
    rps = 256 // lpr
    mg = 256 // (lpr * vec)
    s = max(1, min(-(-M // (32 * rps)), min(64 * mg, 256)))
    per = -(-M // s)
    return -(-M // per)
