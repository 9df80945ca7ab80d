"""Adam and SGD over ONE flat parameter arena, one HIP launch per step (csrc/adam.hip: ``clica_adam_step``, csrc/sgd.hip:
``clica_sgd_step``).

Counterpart of the ``torch.optim.Adam(f.parameters(), lr=...)`` the reference's drivers build (main_mlp.py:312,
main_3dident.py:447-448, kitti_masks/solver.py:36-40) with the same update rule (bias-corrected, eps outside the square
root, no weight decay / amsgrad) and the same ``state_dict()`` layout (``state[i] = {step, exp_avg, exp_avg_sq}``,
``param_groups``), so optimizer checkpoints interchange with the reference's.

Construction re-points every parameter's ``.data`` into a 16-byte aligned slice of one contiguous fp32 arena and installs
``.grad`` views into a matching gradient arena (autograd accumulates into them in place), so ``zero_grad()`` is one memset,
``step()`` one kernel launch, and a data-parallel run all-reduces ONE buffer (``all_reduce_grads``).

``SGD`` is the counterpart of the ``torch.optim.SGD(f.parameters(), lr=...)`` behind the 3DIdent driver's ``--optimizer sgd``
(main_3dident.py:453-454, 582-583), on the same arenas, with ``torch.optim.SGD``'s options and ``state_dict()`` layout
(``state[i] = {momentum_buffer}``).
"""
from __future__ import annotations

import weakref
from typing import Iterable, Optional

import torch
import torch.distributed as dist

from . import lazy, ops
from ._lib import require_cuda

__all__ = ["Adam", "SGD"]


class _FlatArena:
    """What the flat optimizers share: the parameter and gradient arenas, the ``.data`` / ``.grad`` views into them, the device step
    counter with the ticket of the fused tick, and the gradient bookkeeping of the ``torch.optim`` surface."""

    def _build_arenas(self, params: Iterable[torch.nn.Parameter], process_group: Optional[dist.ProcessGroup]):
        self.params = [p for p in params]
        if not self.params:
            raise ValueError("optimizer got an empty parameter list")
        for p in self.params:
            require_cuda(p.data, "parameter")
        dev = self.params[0].device
        offs, total = [], 0
        for p in self.params:
            offs.append(total)
            total += (p.numel() + 3) // 4 * 4
        self.offsets, self.total = offs, total
        self.param_arena = torch.zeros(total, dtype=torch.float32, device=dev)
        self.grad_arena = torch.zeros(total, dtype=torch.float32, device=dev)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self._ticket = torch.zeros(1, dtype=torch.int32, device=dev)       # clica_*_step_tick: the update's last workgroup advances step_dev
        for p, off in zip(self.params, offs):
            view = self.param_arena[off:off + p.numel()].view(p.shape)
            view.copy_(p.data)
            p.data = view
            p.grad = self.grad_arena[off:off + p.numel()].view(p.shape)
            # the drop-in encoder's backward (encoders._MLPFusedFn) adds its dW / db straight into this view (and hands autograd
            # None) when it finds it installed: no per-parameter gradient tensors, no AccumulateGrad launches
            p._clica_grad_view = p.grad
            p._clica_flat_opt = weakref.ref(self)      # (encoders._s16_ctx: the f16x2 arithmetic needs THIS optimizer to apply the step)
        self._s16 = None
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        return dev

    # ------------------------------------------------------------------ torch.optim surface
    def zero_grad(self, set_to_none: bool = False):
        """One memset of the gradient arena (the ``.grad`` views stay installed; ``set_to_none`` is ignored on purpose)."""
        self.grad_arena.zero_()
        for p, off in zip(self.params, self.offsets):
            if p.grad is None or p.grad.data_ptr() != self.grad_arena.data_ptr() + 4 * off:
                p.grad = self.grad_arena[off:off + p.numel()].view(p.shape)      # someone set it to None / replaced it
                p._clica_grad_view = p.grad

    def _bind_s16(self, ctx) -> bool:
        """An encoder's f16x2 context asks to ride in this optimizer's launch.  Only Adam's launch carries it."""
        return False

    def all_reduce_grads(self):
        """Data parallel: sum the gradient arena over the ranks (the 1/world average is applied inside ``step``)."""
        self._adopt_foreign_grads()      # `model.zero_grad()` (set_to_none) makes autograd allocate .grad OUTSIDE the arena: bring
        if self.world > 1:               # those back BEFORE the exchange, or the stale arena is what gets summed
            dist.all_reduce(self.grad_arena, op=dist.ReduceOp.SUM, group=self.pg)

    def _adopt_foreign_grads(self):
        """``nn.Module.zero_grad()`` / ``zero_grad(set_to_none=True)`` drop the arena views, after which autograd allocates
        fresh ``.grad`` tensors outside the arena.  Bring those back (copy + re-install the view) so the launch below
        reads the gradients autograd produced; a parameter that received no gradient this step contributes zeros."""
        base = self.grad_arena.data_ptr()
        for p, off in zip(self.params, self.offsets):
            g = p.grad
            if g is not None and g.data_ptr() == base + 4 * off:
                continue                                   # the installed view (the common case: no tensor is built for it)
            view = self.grad_arena[off:off + p.numel()].view(p.shape)
            if g is None:
                view.zero_()
            else:
                view.copy_(g)
            p.grad = view
            p._clica_grad_view = view


class Adam(_FlatArena):
    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 process_group: Optional[dist.ProcessGroup] = None):
        dev = self._build_arenas(params, process_group)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.param_groups = [dict(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=0, amsgrad=False,
                                  params=list(range(len(self.params))))]
        self.exp_avg = torch.zeros(self.total, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(self.total, dtype=torch.float32, device=dev)

    def _bind_s16(self, ctx) -> bool:
        """An encoder's f16x2 context asks to ride in this optimizer's launch (scale update + guard).  One at a time: the launch takes one."""
        cur = self._s16() if self._s16 is not None else None
        if cur is None or cur is ctx:
            self._s16 = weakref.ref(ctx)
            return True
        return False

    def step(self, closure=None):
        """One launch over the whole arena.  Differences from ``torch.optim.Adam`` (none of the reference's drivers can
        observe them): ONE parameter group; one global step count; a parameter without a gradient is updated with g = 0
        (its moments decay) where torch would skip it."""
        loss = closure() if closure is not None else None
        lazy.flush_all()          # a deferred encoder call (cl_ica_amd/lazy.py) is computed with the parameters it was made with
        if len(self.param_groups) != 1:
            raise ValueError("the flat Adam supports exactly one parameter group")
        self._adopt_foreign_grads()
        g = self.param_groups[0]
        s16 = self._s16() if self._s16 is not None else None
        if s16 is not None:
            # the encoder runs in the f16x2 arithmetic: its scale update rides in this launch, and a step whose producers met a value
            # beyond its scale (the guard, include/clica.h) leaves parameters and moments untouched and takes the step count back
            # (one launch: update, scale update, guard, and -- its last workgroup -- the counter's tick)
            ops.adam_step(self.param_arena, self.grad_arena, self.exp_avg, self.exp_avg_sq, self.step_dev, float(g["lr"]),
                          float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), grad_scale=1.0, t_offset=1, s16=s16.state,
                          ticket=self._ticket)
        else:
            ops.adam_step(self.param_arena, self.grad_arena, self.exp_avg, self.exp_avg_sq, self.step_dev, float(g["lr"]),
                          float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), grad_scale=1.0 / self.world, ticket=self._ticket)
        lazy.after_step()         # e.g. the encoder's fragment-order weight copies, re-packed now rather than in front of the next forward
        return loss

    # ------------------------------------------------------------------ checkpoints (torch.optim.Adam layout)
    def state_dict(self):
        step = int(self.step_dev.item())
        state = {}
        if step > 0:
            for i, (p, off) in enumerate(zip(self.params, self.offsets)):
                sl = slice(off, off + p.numel())
                state[i] = dict(step=torch.tensor(float(step)), exp_avg=self.exp_avg[sl].view(p.shape).clone(),
                                exp_avg_sq=self.exp_avg_sq[sl].view(p.shape).clone())
        return dict(state=state, param_groups=[dict(self.param_groups[0])])

    def load_state_dict(self, sd):
        g = sd["param_groups"][0]
        self.param_groups[0].update(lr=float(g["lr"]), betas=tuple(g["betas"]), eps=float(g["eps"]))
        steps = set()
        for i, st in sd["state"].items():
            p, off = self.params[int(i)], self.offsets[int(i)]
            sl = slice(off, off + p.numel())
            self.exp_avg[sl].view(p.shape).copy_(st["exp_avg"])
            self.exp_avg_sq[sl].view(p.shape).copy_(st["exp_avg_sq"])
            steps.add(int(float(st["step"])))
        if len(steps) > 1:
            raise ValueError("per-parameter step counts differ; the flat Adam keeps one step counter")
        self.step_dev.fill_(steps.pop() if steps else 0)


class SGD(_FlatArena):
    """``torch.optim.SGD`` over the flat arena: one ``clica_sgd_step_tick`` launch per step.  The device counter only tells the first
    update (the momentum buffer takes the gradient as it is) from the later ones."""

    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False, *, maximize: bool = False,
                 process_group: Optional[dist.ProcessGroup] = None):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        dev = self._build_arenas(params, process_group)
        self.param_groups = [dict(lr=float(lr), momentum=float(momentum), dampening=float(dampening), weight_decay=float(weight_decay),
                                  nesterov=bool(nesterov), maximize=bool(maximize), params=list(range(len(self.params))))]
        # plain SGD keeps two arenas, not three (a momentum that arrives later, through param_groups or load_state_dict, brings its buffer)
        self.momentum_buffer = torch.zeros(self.total, dtype=torch.float32, device=dev) if momentum != 0 else None

    def step(self, closure=None):
        """One launch over the whole arena.  As the flat Adam: ONE parameter group, and a parameter without a gradient is updated
        with g = 0 (its buffer decays) where torch would skip it."""
        loss = closure() if closure is not None else None
        lazy.flush_all()          # a deferred encoder call (cl_ica_amd/lazy.py) is computed with the parameters it was made with
        if len(self.param_groups) != 1:
            raise ValueError("the flat SGD supports exactly one parameter group")
        self._adopt_foreign_grads()
        g = self.param_groups[0]
        if float(g["momentum"]) != 0 and self.momentum_buffer is None:      # the momentum was switched on through param_groups
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("flat SGD: no momentum buffer yet -- run the step once eagerly before capturing it")
            self.momentum_buffer = torch.zeros(self.total, dtype=torch.float32, device=self.param_arena.device)
            self.step_dev.zero_()
        ops.sgd_step(self.param_arena, self.grad_arena, self.momentum_buffer if float(g["momentum"]) != 0 else None, self.step_dev,
                     float(g["lr"]), momentum=float(g["momentum"]), dampening=float(g["dampening"]), weight_decay=float(g["weight_decay"]),
                     nesterov=bool(g["nesterov"]), maximize=bool(g["maximize"]), grad_scale=1.0 / self.world, ticket=self._ticket)
        lazy.after_step()
        return loss

    # ------------------------------------------------------------------ checkpoints (torch.optim.SGD layout)
    def state_dict(self):
        state = {}
        if float(self.param_groups[0]["momentum"]) != 0 and self.momentum_buffer is not None and int(self.step_dev.item()) > 0:
            for i, (p, off) in enumerate(zip(self.params, self.offsets)):
                state[i] = dict(momentum_buffer=self.momentum_buffer[off:off + p.numel()].view(p.shape).clone())
        return dict(state=state, param_groups=[dict(self.param_groups[0])])

    def load_state_dict(self, sd):
        g = sd["param_groups"][0]
        self.param_groups[0].update({k: type(self.param_groups[0][k])(g[k]) for k in ("lr", "momentum", "dampening", "weight_decay",
                                                                                      "nesterov", "maximize") if k in g})
        bufs = {int(i): st["momentum_buffer"] for i, st in sd["state"].items() if st.get("momentum_buffer") is not None}
        if bufs and len(bufs) != len(self.params):
            raise ValueError("momentum buffers for some parameters only; the flat SGD keeps one counter for all of them")
        if bufs:
            if self.momentum_buffer is None:
                self.momentum_buffer = torch.zeros(self.total, dtype=torch.float32, device=self.param_arena.device)
            for i, b in bufs.items():
                p, off = self.params[i], self.offsets[i]
                self.momentum_buffer[off:off + p.numel()].view(p.shape).copy_(b)
        self.step_dev.fill_(1 if bufs else 0)
