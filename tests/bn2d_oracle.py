"""NumPy fp64 oracle of the fused BatchNorm2d unit of csrc/bn2d.hip, built on tests/norm_oracle.py:

    z = gamma xhat + beta (+ r),   y = lrelu(z, slope)          slope = 0: ReLU, slope = 1: no activation
    dz = dy gate(z),  dr = dz,  (dx, dgamma, dbeta) = norm_oracle.bn_backward on that dz

An NCHW case is norm_oracle.make_case("bn", N H W, C, cls) -- seeded rows [N H W, C] -- viewed as x[N, C, H, W], plus a residual
r ~ N(0, 1).  Also the two BasicBlock cases of the block test and their near-kink count.
Shared by tests/test_bn2d_host.py (CPU) and tests/test_gpu_bn2d.py."""
import functools
import zlib

import numpy as np

import norm_oracle as O

EPS, MOMENTUM = O.EPS, O.MOMENTUM
KINK_REL, MAX_LEFT_OUT, MAX_KAPPA = O.KINK_REL, O.MAX_LEFT_OUT, O.MAX_KAPPA
SLOPES = (0.0, 0.01, 1.0)
CLASSES = O.CLASSES
# (N, C, H, W): the smallest shapes that reach each code path of the kernels
SHAPES = [(2, 3, 1, 1),        # M = 2 (dx not compared: ill-conditioned, as in the BatchNorm1d sweep)
          (1, 5, 3, 3),        # N = 1; odd HW
          (3, 7, 2, 2),        # HW = 4 (lane = channel piece), C < 64
          (8, 512, 2, 2),      # layer-4 geometry
          (2, 64, 4, 4),       # HW = 16: four pieces per channel
          (4, 128, 8, 8),      # HW = 64: planes of 256 bytes
          (5, 65, 3, 5),       # HW = 15; C not a multiple of 64
          (3, 24, 17, 13),     # HW = 221: scalar path, several waves per plane
          (2, 257, 7, 9),      # shape coverage
          (16, 64, 16, 16),    # layer-1 geometry (one split: 16 images)
          (6, 40, 32, 32),     # stem geometry, HW = 1024 (one split: 6144 values per channel)
          # S > 1 (bn2d.h's geometry()): the later launch merges several partials in split order
          (9, 3, 48, 48),      # plane, quads, S = 2: 5 + 4 images (ragged)
          (5, 2, 63, 65),      # plane, scalar path, S = 2: 3 + 2 images
          (37, 24, 4, 4),      # small, four pieces per channel, S = 3: 13 + 13 + 11 images
          (18, 33, 2, 4),      # small, HW = 8: 66 pieces (a partial chunk), S = 2
          (40, 70, 2, 2)]      # small, one piece per channel, partial chunk, S = 3: 14 + 14 + 12 images
EVAL_SHAPES = [(3, 7, 2, 2), (5, 65, 3, 5), (4, 128, 8, 8)]
# HW % 4 == 0: the scalar accesses keep the reduction order, so the same bits
UNALIGNED_SHAPES = [(8, 512, 2, 2), (4, 128, 8, 8), (9, 3, 48, 48), (37, 24, 4, 4)]

# A case whose first draw leaves out more than MAX_LEFT_OUT of its channels (at slope 0 / 0.01: the same z), or is conditioned worse than
# MAX_KAPPA, takes the next attempt that is not: (N, C, H, W, cls, residual) -> attempt.  Found once by `python tests/bn2d_oracle.py`
# from the inputs and the fp64 oracle alone; both properties are asserted by tests/test_bn2d_host.py.
SEED_ATTEMPT = {(2, 3, 1, 1, 1, False): 1, (2, 3, 1, 1, 1, True): 1, (6, 40, 32, 32, 0, False): 1, (6, 40, 32, 32, 1, False): 1,
                (9, 3, 48, 48, 1, False): 1, (9, 3, 48, 48, 1, True): 1}
MAX_ATTEMPTS = 6

# seeds of the BasicBlock cases (inplanes, planes, stride) -> seed: the first for which the fp64 block has no pre-activation within
# KINK_REL max|z| in either of its ReLUs (found by `python tests/bn2d_oracle.py`, asserted by tests/test_bn2d_host.py)
BLOCK_CASES = [(64, 64, 1), (64, 128, 2)]
BLOCK_SEED = {(64, 64, 1): 0, (64, 128, 2): 0}


def to_nchw(rows, N, C, H, W):
    return np.ascontiguousarray(np.asarray(rows).reshape(N, H * W, C).transpose(0, 2, 1).reshape(N, C, H, W))


def to_rows(t):
    t = np.asarray(t)
    N, C, H, W = t.shape
    return t.reshape(N, C, H * W).transpose(0, 2, 1).reshape(N * H * W, C)


def make_case(N, C, H, W, cls, residual, attempt=None):
    """fp32 inputs of one case as rows [N H W, C]: norm_oracle's batch-norm draw for (N H W, C, cls) plus r ~ N(0, 1)."""
    if attempt is None:
        attempt = SEED_ATTEMPT.get((N, C, H, W, cls, bool(residual)), 0)
    M = N * H * W
    c = dict(O.make_case("bn", M, C, cls, attempt=attempt))
    rng = np.random.default_rng(zlib.crc32(f"bn2d-r:{N}:{C}:{H}:{W}:{cls}".encode()) + 7919 * attempt)
    c["r"] = np.ascontiguousarray(rng.normal(size=(M, C)), dtype=np.float32) if residual else None
    return c


def forward(c, slope):
    fw = O.bn_forward(c["x"], c["gamma"], c["beta"], 1.0, running_mean=c["running_mean"], running_var=c["running_var"])
    z = fw["z"] if c["r"] is None else fw["z"] + np.asarray(c["r"], np.float64)
    return dict(fw, z=z, y=O.lrelu(z, slope))


def backward(fw, c, slope):
    bw = O.bn_backward(fw, c["gamma"], c["dy"], slope)           # (its gate comes from fw["z"]: the sum with the residual)
    bw["dr"] = np.asarray(c["dy"], np.float64) * O.gate(fw["z"], slope)
    return bw


def evaluate(c, rm, rv, slope):
    z = O.bn_eval(c["x"], c["gamma"], c["beta"], rm, rv, 1.0)["z"]
    if c["r"] is not None:
        z = z + np.asarray(c["r"], np.float64)
    return O.lrelu(z, slope)


@functools.lru_cache(maxsize=None)
def reference(N, C, H, W, cls, residual, slope):
    """(inputs, forward, backward) of one case, computed once and shared; treat as read-only."""
    c = make_case(N, C, H, W, cls, residual)
    fw = forward(c, slope)
    return c, fw, backward(fw, c, slope)


def left_out(z, slope):
    """Channels holding an element with |z| <= KINK_REL max|z|: left out of dx / dr / dgamma / dbeta."""
    return O.left_out("bn", z, slope)[0]


def case_ok(N, C, H, W, cls, residual, attempt=None):
    """(left-out fraction at slope 0 / 0.01, kappa) of a draw, from the oracle alone."""
    c = make_case(N, C, H, W, cls, residual, attempt)
    return float(left_out(forward(c, 0.0)["z"], 0.0).mean()), O.kappa("bn", c["x"])


def sweep():
    for shape in SHAPES:
        for cls in range(len(CLASSES)):
            for residual in (False, True):
                yield shape, cls, residual


# ------------------------------------------------------------------------------------------------ BasicBlock cases
def make_block(inplanes, planes, stride, seed=None):
    """(fp32 CPU BasicBlock in training mode with non-trivial BatchNorm parameters, x [4, inplanes, 8, 8], objective weights c)."""
    import torch
    from cl_ica_amd import resnet
    seed = BLOCK_SEED.get((inplanes, planes, stride), 0) if seed is None else seed
    gen = torch.Generator().manual_seed(1000 * seed + inplanes + planes + stride)
    blk = resnet.BasicBlock(inplanes, planes, stride)
    with torch.no_grad():
        for name, prm in blk.named_parameters():
            if prm.dim() == 4:
                prm.copy_(torch.randn(prm.shape, generator=gen) * (2.0 / (prm.shape[1] * prm.shape[2] * prm.shape[3])) ** 0.5)
            elif name.endswith("weight"):
                prm.copy_(1.0 + 0.3 * torch.randn(prm.shape, generator=gen))
            else:
                prm.copy_(0.3 * torch.randn(prm.shape, generator=gen))
    x = torch.randn(4, inplanes, 8, 8, generator=gen)
    Ho = 8 // stride
    c = torch.randn(4, planes, Ho, Ho, generator=gen)
    return blk.train(), x, c


def block_preactivations(blk64, x64):
    """The inputs of the two ReLUs of an fp64 CPU block (the modules' own forward)."""
    import torch
    zs = []
    hook = blk64.relu.register_forward_pre_hook(lambda m, inp: zs.append(inp[0].detach().clone()))
    with torch.no_grad():
        blk64(x64)
    hook.remove()
    assert len(zs) == 2
    return zs


def block_near_kink(inplanes, planes, stride, seed=None):
    import copy
    blk, x, _ = make_block(inplanes, planes, stride, seed)
    zs = block_preactivations(copy.deepcopy(blk).double(), x.double())
    return sum(int((z.abs() <= KINK_REL * z.abs().max()).sum()) for z in zs)


if __name__ == "__main__":      # seed search: prints the tables the tests need
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    SEED_ATTEMPT.clear(); BLOCK_SEED.clear()
    found = {}
    for (shape, cls, residual) in sweep():
        for attempt in range(MAX_ATTEMPTS):
            frac, kap = case_ok(*shape, cls, residual, attempt)
            if frac <= MAX_LEFT_OUT and kap <= MAX_KAPPA:
                break
        else:
            raise SystemExit(f"no draw for {(shape, cls, residual)} within {MAX_ATTEMPTS} attempts")
        if attempt:
            found[shape + (cls, residual)] = attempt
    print("SEED_ATTEMPT =", found)
    seeds = {}
    for case in BLOCK_CASES:
        seeds[case] = next(s for s in range(100) if block_near_kink(*case, seed=s) == 0)
    print("BLOCK_SEED =", seeds)
