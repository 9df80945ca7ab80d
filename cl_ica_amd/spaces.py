"""Latent spaces with on-device samplers: same class/method surface as /root/reference/spaces.py
(``NRealSpace`` / ``NSphereSpace`` / ``NBoxSpace`` x ``uniform / normal / laplace /
generalized_normal / von_mises_fisher``), but every draw is one Philox kernel launch on the GPU --
no torch.distributions on the host, no NumPy vMF + H2D copy, no ``.item()`` per rejection round.

Each call consumes a fresh counter ("draw id") of the module-level generator, so successive calls
are independent; ``manual_seed`` resets it.  RNG streams differ from torch's, parity with the
reference is distributional (tests/test_gpu_samplers.py against tests/golden/g9_samplers.npz), and
every kind is held to its exact distribution (tests/test_gpu_sampler_distributions.py: fp64 CDFs,
2^20 draws, Kolmogorov-Smirnov bound sqrt(N) D < 2.6).  Range covered there: n = 1..10 for the box and
R^n kinds (scales from 1e-3 to 5 box widths, generalized-normal p from 0.5 to 8), n = 2..40 on the
sphere, von Mises-Fisher kappa from 0.01 to 1e4 (n = 1 is refused: S^0 has no tangent direction).
"""
from __future__ import annotations

import contextlib
from abc import ABC, abstractmethod

import torch

from . import ops

__all__ = ["Space", "NRealSpace", "NSphereSpace", "NBoxSpace", "manual_seed", "DeviceClock"]

_state = {"seed": 0, "draw": 0}
_clock = None      # the DeviceClock whose ``iteration()`` scope is open, else None

CLOCK_STREAM_BASE = 1 << 31      # Philox stream ids of clocked draws: this + the draw's ordinal within its iteration


def manual_seed(seed: int) -> None:
    _state["seed"] = int(seed)
    _state["draw"] = 0


class DeviceClock:
    """Draw numbering that a captured graph can replay: the iteration counter lives on the device.

    The module-level generator numbers its draws with a host counter (``stream_id`` = 1, 2, ... at Philox step 0), so a recorded
    launch would replay the same stream for ever.  Inside ``with clock.iteration():`` every draw of this module (through
    ``LatentSpace`` / ``ProductLatentSpace`` and every kind, vMF and tensor scales included: they all reach ``_draw``) instead uses
    Philox seed = the clock's `seed`, step = ``*clock.step`` (an ``int32[1]`` on the device, read by the kernel: ``step_dev`` of
    ``clica_sample`` / ``clica_sample_scaled``) and stream id = ``CLOCK_STREAM_BASE`` + the ordinal of the draw within the iteration;
    the ordinal restarts at every ``with``.  ``clock.tick()`` advances the counter by one with a stream-ordered one-thread kernel
    (``clica_tick``): no host read, capturable.  The module-level counter is not touched inside a scope, so the draws outside are
    what they would have been without it.

    Two properties follow:
      * an eager iteration and a replayed one at the same counter value draw the same numbers, bit for bit: host state enters only
        through the ordinals, which the recorded iteration fixed in the same order an eager one assigns them;
      * clocked draws never coincide with draws of the module-level generator under the same user seed: the Philox counter holds
        (element, draw, step, stream id), clocked stream ids have bit 31 set (``CLOCK_STREAM_BASE + ordinal``, ordinal < 2^31) and
        module-level ones are the draw numbers 1, 2, ... below 2^31 (``_draw`` refuses to count further), so the two ranges are
        disjoint whatever the seed and the counter are.  The evaluation batches a driver draws between training steps therefore
        never repeat a training batch.
    """

    def __init__(self, seed: int = 0, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"DeviceClock lives on the GPU only (device={device!r})")
        self.seed = int(seed)
        self.device = device
        self.step = torch.zeros(1, dtype=torch.int32, device=device)
        self._ordinal = 0

    @contextlib.contextmanager
    def iteration(self):
        """Scope of ONE iteration: the draws inside are clocked, their ordinals start at 0."""
        global _clock
        if _clock is not None:
            raise RuntimeError("DeviceClock.iteration: a clock scope is already open (scopes do not nest)")
        _clock, self._ordinal = self, 0
        try:
            yield self
        finally:
            _clock = None

    def tick(self) -> None:
        """``*step += 1`` on the current stream."""
        ops.tick(self.step)

    def _next(self) -> int:
        if self._ordinal >= CLOCK_STREAM_BASE:
            raise RuntimeError("DeviceClock: more than 2^31 draws in one iteration")
        self._ordinal += 1
        return CLOCK_STREAM_BASE + self._ordinal - 1


def _draw(space, dist, n, size, device, **kw):
    if device is None or torch.device(device).type != "cuda":
        raise RuntimeError(f"cl_ica_amd.spaces samples on the GPU only (device={device!r}); there is no host fallback")
    if _clock is not None:
        return ops.sample(space, dist, n, size, torch.device(device), seed=_clock.seed, stream_id=_clock._next(), step_dev=_clock.step,
                          **kw)
    if _state["draw"] + 1 >= CLOCK_STREAM_BASE:
        raise RuntimeError("cl_ica_amd.spaces: 2^31 draws since manual_seed (the stream ids above belong to DeviceClock)")
    _state["draw"] += 1
    return ops.sample(space, dist, n, size, torch.device(device), seed=_state["seed"], stream_id=_state["draw"], **kw)


def _mean2d(mean, n, size, device):
    mean = torch.as_tensor(mean, dtype=torch.float32)
    if mean.dim() == 1:
        mean = mean.unsqueeze(0)
    assert mean.dim() == 2 and mean.shape[-1] == n and mean.shape[0] in (1, size)
    return mean.to(device)


class Space(ABC):
    @abstractmethod
    def uniform(self, size, device):
        ...

    @abstractmethod
    def normal(self, mean, std, size, device):
        ...

    @abstractmethod
    def laplace(self, mean, lbd, size, device):
        ...

    @abstractmethod
    def generalized_normal(self, mean, lbd, p, size, device):
        ...

    @property
    @abstractmethod
    def dim(self):
        ...


class _Base(Space):
    kind = "real"
    box = (0.0, 1.0)

    def __init__(self, n):
        self.n = n

    @property
    def dim(self):
        return self.n

    def _cond(self, dist, mean, scale, size, device, shape_p=2.0):
        if torch.is_tensor(scale) and scale.numel() > 1:
            # spaces.py:60-72, 157-166, 297: `std` of normal() may be a (n,), (1, n) or (size, n) tensor (laplace and
            # generalized_normal assert a float there, spaces.py:87, 112; accepted here for all three location-scale kinds)
            return _draw(self.kind, dist, self.n, size, device, mean=_mean2d(mean, self.n, size, device), scale=1.0,
                         shape_p=float(shape_p), box=self.box, scale_vec=scale.to(device=device, dtype=torch.float32))
        return _draw(self.kind, dist, self.n, size, device, mean=_mean2d(mean, self.n, size, device), scale=float(scale),
                     shape_p=float(shape_p), box=self.box)

    def normal(self, mean, std, size, device="cuda"):
        return self._cond("normal", mean, std, size, device)

    def laplace(self, mean, lbd, size, device="cuda"):
        return self._cond("laplace", mean, lbd, size, device)

    def generalized_normal(self, mean, lbd, p, size, device="cuda"):
        return self._cond("gennorm", mean, lbd, size, device, shape_p=p)


class NRealSpace(_Base):
    """Unconstrained space R^N (spaces.py:35-119)."""
    kind = "real"

    def uniform(self, size, device="cuda"):
        raise NotImplementedError("Not defined on R^n")


class NSphereSpace(_Base):
    """Unit hypersphere (spaces.py:122-257); like the reference, ``r`` is stored but samples are unit norm."""
    kind = "sphere"

    def __init__(self, n, r=1):
        super().__init__(n)
        self._n_sub = n - 1
        self.r = r

    def uniform(self, size, device="cuda"):
        return _draw("sphere", "uniform", self.n, size, device)

    def von_mises_fisher(self, mean, kappa, size, device="cuda"):
        return self._cond("vmf", mean, kappa, size, device)


class NBoxSpace(_Base):
    """Box [min_, max_]^N (spaces.py:260-351); conditionals are truncated per element."""
    kind = "box"

    def __init__(self, n, min_=-1, max_=1):
        super().__init__(n)
        self.min_, self.max_ = min_, max_
        self.box = (float(min_), float(max_))

    def uniform(self, size, device="cuda"):
        return _draw("box", "uniform", self.n, size, device, box=self.box)
