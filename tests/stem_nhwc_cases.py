"""The cases of the channels-last stem unit (csrc/bn2d_nhwc.hip: BatchNorm2d + (leaky) ReLU + max-pool 3/2/1 on x[N, H, W, C]), shared by
tests/test_stem_nhwc_host.py (CPU) and tests/test_gpu_stem_nhwc.py.  The inputs and the fp64 oracle are those of tests/pool2d_oracle.py:
its make_case yields x as rows [N H W, C], which is the NHWC memory.  The shapes are the smallest that reach each path of the kernels;
a draw that misses one of the oracle's three caps takes the attempt named in ATTEMPT (found from the inputs and the oracle alone;
tests/test_stem_nhwc_host.py asserts the caps for every case)."""
import functools

import pool2d_oracle as Q

# (N, C, H, W)
SHAPES = [(2, 3, 1, 1),          # M = 2: dx not compared
          (1, 2, 3, 3),          # scalar lanes, odd plane
          (2, 4, 2, 2),          # one window, one quad lane
          (3, 5, 7, 9),          # odd, non-square, scalar
          (2, 8, 5, 5),          # odd square plane, quads
          (2, 68, 8, 8),         # partly filled chunk of lanes
          (1, 260, 4, 4),        # two channel chunks, the second nearly empty
          (2, 128, 7, 7),        # a layer-like width
          (6, 64, 32, 32),       # stem geometry: 12 row splits that cut planes, 2 x 2 tiles per plane
          (5, 8, 33, 31),        # 2 splits, odd plane crossing bands
          (3, 4, 48, 48),        # one split, many bands
          (1, 4, 112, 112)]      # the largest plane of the contract, 2 splits
TIE_SHAPES = [(1, 2, 3, 3), (3, 5, 7, 9), (2, 68, 8, 8), (6, 64, 32, 32)]
EVAL_SHAPES = [(3, 5, 7, 9), (2, 68, 8, 8), (1, 4, 112, 112)]
UNALIGNED_SHAPES = [(2, 68, 8, 8), (6, 64, 32, 32), (3, 4, 48, 48)]      # C % 4 == 0: the 16-byte path when aligned
GRAPH_SHAPE = (6, 64, 32, 32)
CLASSES, SLOPES, TIE_CLASS = Q.CLASSES, Q.SLOPES, Q.TIE_CLASS
# (N, C, H, W, class) -> attempt, where attempt 0 misses a cap
ATTEMPT = {(2, 4, 2, 2, 2): 1, (1, 4, 112, 112, 0): 1}


def attempt(shape, cls):
    return ATTEMPT.get(tuple(shape) + (cls,), 0)


def make_case(shape, cls):
    return Q.make_case(*shape, cls, attempt(shape, cls))


@functools.lru_cache(maxsize=None)
def reference(shape, cls, slope):
    """(inputs, forward, backward) of one case, computed once and shared; treat as read-only."""
    c = make_case(shape, cls)
    fw = Q.forward(c, shape, slope)
    return c, fw, Q.backward(fw, c, shape, slope)


def sweep():
    for shape in SHAPES:
        for cls in range(len(CLASSES)):
            yield shape, cls
