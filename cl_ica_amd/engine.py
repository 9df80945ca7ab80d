"""Fused, HBM-resident contrastive train step: the counterpart of ``train_step`` in
/root/reference/main_mlp.py:258-285 plus the sampling at :328, without autograd and without a
host sync.

One step enqueues, on one HIP stream:
    tick -> sample z, z~ (Philox) -> mixing net g -> 7 fused Linear(+LeakyReLU) GEMMs over the
    stacked 2B rows -> [head] -> tiled Lp-InfoNCE forward -> its backward (dz1 += dz3: the
    reference's z3_rec = roll(z1_rec) is, up to a row permutation the row-wise log-sum-exp cannot
    see, "all z1_rec of the batch") -> [head bwd] -> wgrad/dgrad GEMMs into one flat gradient arena
    -> [bucketed RCCL all-reduce] -> one fused Adam launch over the flat parameter arena.
All buffers are preallocated, so the whole step can be captured in a HIP graph (``capture()``).

Data parallel (one process per GPU): every rank samples its own B pairs, all-gathers z1_rec
(B*n*4 bytes per rank) to form the global negatives pool, reduce-scatters d/dz3, and all-reduces the
flat gradient arena; semantics = the single-process loss on the concatenated batch.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import torch
import torch.distributed as dist
from torch import nn

from . import _lib, ops
from . import layers as ls
from contextlib import nullcontext as _nullctx

from .distributed import GradBuckets

__all__ = ["SamplerSpec", "ContrastiveTrainer", "SupervisedTrainer"]


@dataclass
class SamplerSpec:
    """Ground-truth latent distribution (main_mlp.py:136-200)."""
    space: str = "box"              # box | sphere | real  (--space-type, "unbounded" -> real)
    n: int = 10
    box: tuple = (0.0, 1.0)         # --box-min / --box-max
    marginal: str = "uniform"       # uniform | normal | laplace | gennorm   (--m-p 0/2/1/k)
    m_param: float = 1.0
    m_p: float = 2.0
    conditional: str = "normal"     # normal | laplace | gennorm | vmf        (--c-p 2/1/k/0)
    c_param: float = 0.05
    c_p: float = 2.0
    seed: int = 0


def _abort_capture(graph, stream, others=()) -> None:
    """Leave stream-capture mode after a failed capture, whatever state torch's CUDAGraph object is in (clica_abort_capture
    runs inside the HIP runtime instance torch and the kernels share; a ctypes handle to libamdhip64 may be another copy)."""
    try:
        graph.capture_end()
    except Exception:
        pass
    lib = _lib.load()
    for st in (stream,) + tuple(o for o in others if o is not None):       # the origin stream first, then forked side streams
        lib.clica_abort_capture(C.c_void_p(st.cuda_stream))


class StepHandoffs:
    """What one piece of a step leaves for a later piece of the SAME step (a misspelt field raises).  Idle between steps; a piece called
    outside _step_body finds every fold off.  field: written by -> consumed by
        in_step        _step_body, around loss / backward  -> loss_forward_backward: may the objective be left to the backward chain?
        fold_adam      _step_body, behind the loss         -> backward_chain (tail), weight_grads (Adam in the slab reduction)
        ticked         loss_forward_backward               -> weight_grads (Adam's t), optimizer_step (clears it; ticks if unset)
        adam_done      weight_grads                        -> optimizer_step (clears it; nothing left to launch)
        tail_ready     backward_chain                      -> weight_grads (clears it; the n-wide layers' slabs are in the workspace)
        scales_updated optimizer_step                      -> _step_body (did the Adam launch update the f16x2 scales?)
        dy_parts       ContrastiveTrainer.loss_forward_backward -> backward_chain (clears it; dy still lacks the sweep's partials)
        mse            SupervisedTrainer.loss_forward_backward  -> backward_chain (clears it; the chain's prologue forms dY and the loss)"""
    IDLE = dict(in_step=False, fold_adam=False, ticked=False, adam_done=False, tail_ready=False, scales_updated=False,
                dy_parts=None, mse=None)
    __slots__ = tuple(IDLE)

    def __init__(self):
        self.reset()

    def reset(self, *fields):
        """Back to idle: every field (load_state_dict), or only the named ones (the end of a step, a calibration pass)."""
        for name in fields or self.IDLE:
            setattr(self, name, self.IDLE[name])


@dataclass(frozen=True)
class StepPlan:
    """The launch structure of a step inside _step_body, fixed by what the trainer was constructed with (the class-attribute test
    hooks included: they are read once, at the end of construction)."""
    adam_in_wgrad: bool        # the weight gradients' slab reduction applies Adam as well
    chain_tail: bool           # the backward chain leaves the n-wide layers' weight-gradient slabs (needs adam_in_wgrad)
    dy_from_partials: bool     # ... and its prologue finishes dy from the loss sweep's partials (contrastive, p >= 1)
    mse_in_chain: bool         # ... or forms the MSE objective (supervised)
    guard_rides: bool          # data parallel: the f16x2 guard's verdict rides in the first gradient bucket
    wgrad_halves: bool         # data parallel: the grouped weight gradients go out in two halves


@dataclass(frozen=True)
class EncoderPlan:
    """Which encoder pipeline a trainer runs, decided once by plan_encoder() from host facts; the trainer's flags of the same names are
    copies of these fields, and nothing assigns them afterwards."""
    path: str                  # "whole-stack": one launch for the stack (widths <= 512, <= 8 layers) | "per-layer": one GEMM per layer
    arith: str                 # "native_fp32" | "bf16x3" | "f16x2": what the matrix cores multiply (per-layer: in the split layers only)
    fused_forward: bool        # the forward is the whole-stack launch (= path "whole-stack")
    fused_backward: bool       # ... and so are the data-gradient chain and the grouped weight gradients (more than one Linear; a
                               #     single-Linear encoder runs its backward through the per-layer body)
    mix_in_forward: bool       # the mixing net g runs in the whole-stack forward's prologue
    split_bf16: bool           # whole-stack forward and chain in a split arithmetic (bf16x3, or f16x2 with split_f16)
    split_f16: bool            # ... in f16x2
    split_wgrad: bool          # ... and the grouped weight gradients of the MFMA-sized layers on plane copies
    split_wgrad_wide: bool     # per-layer path: the weight gradients of the MFMA-sized layers on plane copies
    split_f16_wide: bool       # ... in f16x2
    kinds: tuple               # mlp_wgrad_split_kind per layer, whole-stack family (() unless split_bf16)
    wide_kinds: tuple          # ... per-layer family (() unless split_wgrad_wide)
    chain: frozenset           # per-layer path: the layers whose forward and data gradient run on the split GEMMs as well
    chain_min: int             # ... the least width, on both sides, that puts a layer there (0: no split weight gradients)
    acts_planes_only: tuple    # per layer: the forward writes this activation as planes only (acts_out[l] is None)
    dz_planes_only: tuple      # per chain link (fused_backward): dZ_l is written as planes only (dz_out[l] is None)

    def __post_init__(self):
        assert self.fused_forward == (self.path == "whole-stack") and (self.fused_forward or not self.fused_backward)
        assert self.fused_backward or not (self.split_bf16 or self.split_wgrad), "the split whole-stack kernels need the fused backward"
        assert self.split_bf16 or not (self.split_f16 or self.split_wgrad)
        assert not (self.fused_forward and self.split_wgrad_wide) and (self.split_wgrad_wide or not (self.split_f16_wide or self.chain))
        assert self.arith == ("f16x2" if self.split_f16 or self.split_f16_wide else
                              "bf16x3" if self.split_bf16 or self.split_wgrad_wide else "native_fp32")


def plan_encoder(shapes, slope: float, gpu: bool, fused_forward: bool, want_split: bool, arith_f16: bool, keep_fp32_copies: bool = False,
                 mix_ok: bool = True) -> EncoderPlan:
    """The encoder path of a Linear / LeakyReLU stack with weight shapes `shapes` = [(out, in), ...]: host logic over the library's host
    planners, no launch, no allocation.  `want_split` / `arith_f16`: the resolved split_bf16 / split_arith requests (environment
    included); `mix_ok`: the mixing net is one the whole-stack prologue can run."""
    L = len(shapes)
    widths = [s[0] for s in shapes]
    fused_fwd = bool(fused_forward) and ops.mlp_fwd_fusable([torch.empty(s, device="meta") for s in shapes])
    fused_bwd = fused_fwd and L > 1
    # whole-stack kernels and weight gradients on the bf16 matrix cores with exact 3-way bf16 operand splits (fp32 emulation: six bf16
    # products per fp32 product, fp32 accumulate, fp32-grade error) -- the default where the encoder fits them
    split = fused_bwd and want_split and sum((w + 31) // 32 * 32 for w in widths) <= 3456       # on-chip bias table (fused_mlp.hip)
    # f16x2: two fp16 pieces per operand with per-tensor power-of-two scales, three MFMA products (half the matrix work, 4 B/element;
    # include/clica.h "f16x2 arithmetic"); bf16x3 (full fp32 exponent range) stays for a slope outside (0, 1) and off the GPU
    f16 = bool(arith_f16 and 0.0 < slope < 1.0 and gpu)
    # split weight gradients (csrc/wgrad_split.hip): the MFMA-sized layers read BOTH operands as planes that the split forward /
    # backward-chain kernels write instead of the fp32 copies (nobody else reads a hidden activation or dZ); the tiny first / last
    # layer keeps the fp32 VALU kernel, so the tensors next to them stay fp32 as well
    kinds = tuple(ops.mlp_wgrad_split_kind(*s) for s in shapes) if split else ()
    split_wgrad = bool(split and L >= 3 and kinds[0] == 1 and kinds[-1] == 1)
    only = split_wgrad and not keep_fp32_copies
    # Per-layer path (a width beyond 512, BASELINE config 3): forward and data gradients on the fp32-MFMA kernels, the WEIGHT gradients
    # of the MFMA-sized layers in the split arithmetic on plane copies that an HBM-bound conversion kernel makes of the fp32
    # activations / gradients (clica_mlp_planes_from_f32); f16x2 keeps its per-tensor scales in the Split16 state (at most 8 layers)
    wide = bool(want_split and not fused_fwd)
    f16_wide = wide and f16 and L <= 8
    wide_kinds = tuple(ops.mlp_wgrad_split_kind(*s) for s in shapes) if wide else ()
    # ... and, for the layers that are wide on BOTH sides (config 3's three 2000 x 2000 layers), forward and data gradient too: split
    # GEMMs with fused epilogues on T-plane operands (csrc/wgrad_split.hip: gemm_split_k; 1.7x the fp32-MFMA kernels at
    # 12288 x 2000 x 2000).  bf16x3: from 1024 -- with the 400-wide layers in the chain one p = 1 gradient check of G13 measures 1.1e-5;
    # f16x2: from 384 -- all of config 3's checks hold 1e-5 and the step gains 13 %: 198 -> 225 steps/s
    cmin = (384 if f16_wide else 1024) if wide else 0
    chain = frozenset(l for l in range(1, L - 1) if wide and wide_kinds[l] == 0 and min(shapes[l]) >= cmin)
    return EncoderPlan(path="whole-stack" if fused_fwd else "per-layer",
                       arith="f16x2" if f16 and (split or f16_wide) else "bf16x3" if split or wide else "native_fp32",
                       fused_forward=fused_fwd, fused_backward=fused_bwd, mix_in_forward=fused_fwd and mix_ok,
                       split_bf16=bool(split), split_f16=bool(split and f16), split_wgrad=split_wgrad, split_wgrad_wide=wide,
                       split_f16_wide=f16_wide, kinds=kinds, wide_kinds=wide_kinds, chain=chain, chain_min=cmin,
                       acts_planes_only=tuple(only and l < L - 1 and kinds[l + 1] == 0 for l in range(L)),
                       dz_planes_only=tuple(only and kinds[l] == 0 for l in range(L - 1)) if fused_bwd else ())


class _FusedTrainer:
    """What the contrastive and the supervised step share: the encoder paths (EncoderPlan: one forward and one backward body each),
    arenas, sampler and mixing net, pack, forward, heads, backward chain, weight gradients, optimizer, calibration and guard bookkeeping
    of the f16x2 arithmetic, checkpoints, capture and step / step_injected.  A subclass brings the objective: _enc_rows, _allocate_loss,
    loss_forward_backward, _objective_folds, _result, inject, plan_summary and what its loss carries into a checkpoint."""
    p = tau = alpha = None           # (the contrastive objective's; checkpoints carry them as None otherwise)
    keep_fp32_copies = False         # (inspection, set on the class before construction: the split path also writes every fp32 copy)

    def __init__(self, f: nn.Sequential, g_weights: torch.Tensor, sampler: SamplerSpec, batch_size: int,
                 lr: float = 1e-4, g_slope: float = 0.2, betas=(0.9, 0.999), eps: float = 1e-8, device=None,
                 process_group: Optional[dist.ProcessGroup] = None, bucket_bytes: int = 8 << 20,
                 force_collectives: bool = False, overlap_backward: bool = True, fused_forward: bool = True,
                 split_bf16: Optional[bool] = None, g_act_kind: int = 0, emulate_pool_ranks: int = 1, dry_ranks: int = 1,
                 split_arith: Optional[str] = None):
        self.device = torch.device(device if device is not None else "cuda")
        self.f = f.to(self.device)
        self.B = int(batch_size)
        self.n = sampler.n
        self.sampler = sampler
        self.lr, self.betas, self.eps = float(lr), betas, float(eps)
        self.g_slope = float(g_slope)
        self.g_act_kind = int(g_act_kind)     # hidden activation of g (ops.MIX_ACT); the fused prologue handles LeakyReLU / ReLU only
        self.overlap_backward = bool(overlap_backward)
        self.gW = g_weights.detach().to(self.device, torch.float32).contiguous()
        assert self.gW.shape[1:] == (self.n, self.n)
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(process_group) if self.world > 1 else 0
        # run the collectives even at world size 1 (test hook: exercises the DP code path on one GPU)
        self.force_collectives = bool(force_collectives)
        self.dp = self.world > 1 or (force_collectives and dist.is_initialized())
        # measurement aid (bench.py `secondary` leg): ONE rank's compute of an R-rank data-parallel job on one GPU -- the negatives
        # pool holds R copies of the local embeddings (R x B rows, device-to-device copies stand in for the two all-gathers), so
        # the pair sweeps do the work they do on an R-GPU node.  Not a training mode: every negative counts R times.
        self.emulate_pool = int(emulate_pool_ranks) if (self.world == 1 and not self.dp) else 1
        # DRY RUN of an R-rank job on one GPU (bench.py --dry-ranks R, tests/test_gpu_engine.py): this process plans and runs exactly
        # what rank 0 of an R-rank data-parallel job would -- pool of R x B rows, loss workspaces and stream splits for that pool, the
        # two-half weight-gradient launch, the gradient buckets, 1 / R gradient scale, every collective issued on the (world-1) RCCL
        # group and captured into the step graph -- with the other ranks' contributions stood in for by copies of its own (all-gather
        # results replicated, all-reduce over one rank).  Whatever an 8-GPU run can trip over on the host side (a workspace sized for
        # the wrong plan, a capture RCCL refuses, a bucket boundary off by one) trips here; what it cannot show is the wire.
        self.dry_ranks = int(dry_ranks) if (self.world == 1 and self.dp) else 1
        if int(dry_ranks) > 1 and self.dry_ranks == 1:
            raise ValueError("dry_ranks needs an initialised one-rank process group and force_collectives=True")
        self.handoff = StepHandoffs()
        self.stamps = None                     # bench.py: device time stamps around the encoder launches, valid inside the graph
        self._dy_parts_taken = self._mse_taken = 0      # (tests: how many steps left their objective to the backward chain)
        self._planes_on_current_scales = False
        # the marginal's mean (main_mlp.py:148-150: the first unit vector on the sphere)
        self._eta = None
        if sampler.marginal != "uniform":
            self._eta = torch.zeros(1, self.n, device=self.device)
            if sampler.space == "sphere":
                self._eta[0, 0] = 1.0

        mods = list(self.f)
        for idx, m in enumerate(mods):
            # the fused step runs the Linear / LeakyReLU stack only: with a normalisation in between it would train another network
            if isinstance(m, (nn.modules.batchnorm._BatchNorm, nn.GroupNorm, nn.LayerNorm)):
                raise ValueError(f"{type(self).__name__}: the encoder holds a normalisation module ({idx}: {m}); the fused step runs plain "
                                 "Linear / LeakyReLU stacks only -- train get_mlp(layer_normalization=...) through autograd")
            if isinstance(m, nn.Linear) and m.bias is None:
                raise ValueError(f"{type(self).__name__}: the encoder holds a Linear without bias ({idx}: {m}); every kernel of the fused "
                                 "step computes a bias and its gradient")
        self.linears: List[nn.Linear] = [m for m in mods if isinstance(m, nn.Linear)]
        slopes = {m.negative_slope for m in mods if isinstance(m, nn.LeakyReLU)}
        self.slope = slopes.pop() if slopes else 0.01
        heads = [m for m in mods if isinstance(m, (ls.RescaleLayer, ls.SoftclipLayer))]
        self.head = heads[0] if heads else None
        self._flatten_parameters()
        # the encoder path (EncoderPlan).  split_bf16=False / CLICA_SPLIT_BF16=0: native fp32 MFMA; split_arith / CLICA_SPLIT_ARITH: "f16"
        # (f16x2, the default) or "bf16" (the bf16x3 scheme: six products, 6 B/element, full fp32 exponent range)
        want_split = (os.environ.get("CLICA_SPLIT_BF16", "1") == "1") if split_bf16 is None else bool(split_bf16)
        arith = (split_arith or os.environ.get("CLICA_SPLIT_ARITH", "f16")).lower()
        if arith not in ("f16", "bf16"):
            raise ValueError(f"split_arith must be 'f16' or 'bf16', got {arith!r}")
        # (the mixing net inside the whole-stack forward's prologue: n <= 16, LeakyReLU)
        self.encoder_plan = ep = plan_encoder([tuple(lin.weight.shape) for lin in self.linears], self.slope, self.device.type == "cuda",
                                              fused_forward, want_split, arith == "f16", keep_fp32_copies=bool(self.keep_fp32_copies),
                                              mix_ok=self.n <= 16 and self.g_act_kind == 0)
        for name in ("fused_forward", "fused_backward", "mix_in_forward", "split_bf16", "split_f16", "split_f16_wide", "split_wgrad",
                     "split_wgrad_wide", "chain"):
            setattr(self, name, getattr(ep, name))
        self.grouped_wgrad = ep.fused_backward        # (one grouped launch for every layer's weight gradient: bench.py reads the name)
        self.wide_kinds = list(ep.wide_kinds)
        self.packed = self.packed_t = None
        self._x_pending = self._packed_current = self._s16_calibrated = False
        if self.world > 1:
            # identical replicas by construction: rank 0's parameters and mixing weights win (callers that seed every rank
            # identically are unaffected; callers that do not would otherwise train `world` different models silently)
            src = dist.get_global_rank(process_group, 0) if process_group is not None else 0
            dist.broadcast(self.param_arena, src=src, group=process_group)
            dist.broadcast(self.gW, src=src, group=process_group)
        self.s16 = ops.Split16(len(self.linears), self.device) if ep.arith == "f16x2" else None
        if self.s16 is not None and self.dp:      # all ranks must take the guard's decision together: the verdict is all-reduced with the gradients
            self.s16.set_dp_poison(self._guard_slot)
        self._allocate()
        self._watch_versions = True           # step(): parameters written from outside (load_state_dict, copy_) -> recalibrate the f16x2 scales
        self._versions_seen = self._param_versions()
        self._guard_skipped_seen = 0
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        # data parallel + grouped weight gradients: the grouped launch is issued in TWO halves (layers L-1 .. h, then h-1 .. 0) and
        # the first half's slice of the gradient arena is all-reduced on the communication stream while the second half's GEMMs run
        L = len(self.linears)
        self.wgrad_halves = bool(self.dp and self.fused_backward and L >= 4)
        self._half = L // 2
        if self.wgrad_halves:
            # each half's launch plans its own contraction splits (fewer tiles -> more splits per layer -> larger slabs than in the
            # all-layer plan the workspace was sized for: 59.3 MB against 58.5 MB for the n = 10 stack at B = 6144)
            shapes = [tuple(lin.weight.shape) for lin in self.linears]
            mk = ops.mlp_wgrad_split_workspace if self.split_wgrad else ops.mlp_wgrad_workspace
            for part in (shapes[self._half:], shapes[:self._half]):
                w = mk(self._enc_rows(), part, self.device)
                if w.numel() > self.group_ws.numel():
                    self.group_ws = w
        slices = list(self._layer_slices)
        self._guard_rides = bool(self.dp and self.s16 is not None and self.fused_backward and slices)
        if self._guard_rides:
            # whole-stack path: every producer of the step has run when the first bucket (the last layer's slice: the arena's tail) goes
            # out, so the verdict slot behind the arena rides in that bucket; the per-layer path reduces the slot on its own at the end
            total = self.grad_arena.numel()
            k = max(range(len(slices)), key=lambda i: slices[i][1])
            if k == 0 and slices[k][1] >= total - 3:
                slices[k] = (slices[k][0], total + 4)
            else:
                self._guard_rides = False
        self.buckets = GradBuckets(self._grad_buf if self._guard_rides else self.grad_arena, slices, self.world, process_group, bucket_bytes,
                                   force=self.dp, boundaries=(L - 1 - self._half,) if self.wgrad_halves else ()) if self.dp else None
        self.plan = self._plan_step()

    # Test hook (class attribute, tests/test_gpu_engine.py): both the folded and the unfolded launch structures are product paths -- the
    # unfolded ones run under data parallelism and behind a head -- and the equivalence tests compare them on ONE trainer configuration.
    chain_tail = True            # the backward chain's tail writes the n-wide layers' weight-gradient slabs (clica_mlp_dgrad_split_tail)

    def _plan_step(self) -> StepPlan:
        """Decided once, when everything the decisions depend on is constructed (StepPlan)."""
        # The optimizer can ride in the weight-gradient reduction when ONE whole-stack split launch produces every gradient of the
        # arena and nothing has to happen between gradient and update (no data-parallel all-reduce, no gradient scaling).
        ep = self.encoder_plan
        lin_ids = {id(q) for lin in self.linears for q in (lin.weight, lin.bias)}
        adam = bool(ep.split_wgrad and self.buckets is None and self.world * self.dry_ranks == 1
                    and all(id(q) in lin_ids for q in self.f.parameters()))
        tail = bool(adam and self.chain_tail and not ep.dz_planes_only[0] and
                    ops.mlp_chain_tail_supported([tuple(lin.weight.shape) for lin in self.linears]))
        # the chain runs with its tail directly on dy: no pool beyond this rank's rows, no output head -- then it can finish dy itself
        on_dy = tail and not self.dp and self.emulate_pool <= 1 and self.head is None
        dy_parts, mse = self._objective_folds(on_dy)
        return StepPlan(adam_in_wgrad=adam, chain_tail=tail, dy_from_partials=bool(dy_parts), mse_in_chain=bool(mse),
                        guard_rides=self._guard_rides, wgrad_halves=self.wgrad_halves)

    # -------------------------------------------------------------------------------- arenas
    def _flatten_parameters(self):
        """Re-point every parameter of f into one 16-byte aligned flat arena (Parameter objects and
        state-dict keys are unchanged) and create matching grad / exp_avg / exp_avg_sq arenas."""
        params = list(self.f.parameters())
        offs, total = [], 0
        for prm in params:
            offs.append(total)
            total += (prm.numel() + 3) // 4 * 4
        dev = self.device
        self.param_arena = torch.zeros(total, dtype=torch.float32, device=dev)
        # (+ 4 floats behind the gradients: the f16x2 guard's verdict slot, which rides through the data-parallel all-reduce of the
        #  last layer's bucket -- include/clica.h, "THE GUARD of the f16x2 arithmetic")
        self._grad_buf = torch.zeros(total + 4, dtype=torch.float32, device=dev)
        self.grad_arena = self._grad_buf[:total]
        self._guard_slot = self._grad_buf[total:total + 1]
        self.exp_avg = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(total, dtype=torch.float32, device=dev)
        self._views, self._gviews = {}, {}
        for prm, off in zip(params, offs):
            view = self.param_arena[off:off + prm.numel()].view(prm.shape)
            view.copy_(prm.data.to(dev))
            prm.data = view
            gview = self.grad_arena[off:off + prm.numel()].view(prm.shape)
            prm.grad = gview
            self._views[id(prm)] = view
            self._gviews[id(prm)] = gview
        # slices per Linear layer in BACKWARD completion order (last layer first) for bucketing
        self._layer_slices = []
        pid = {id(prm): (off, prm.numel()) for prm, off in zip(params, offs)}
        for lin in reversed(self.linears):
            o_w, n_w = pid[id(lin.weight)]
            o_b, n_b = pid[id(lin.bias)]
            self._layer_slices.append((min(o_w, o_b), max(o_w + n_w, o_b + n_b)))
        # parameters that are not Linear weights/biases (a learnable head: RescaleLayer.r / SoftclipLayer.max_abs_bound) get their
        # gradient at the very start of backward(): they ride in the first slice to complete, so the data-parallel all-reduce
        # covers them too (otherwise every rank would train its own head parameter)
        lin_ids = {id(q) for lin in self.linears for q in (lin.weight, lin.bias)}
        for prm in params:
            if id(prm) not in lin_ids and self._layer_slices:
                o, k = pid[id(prm)]
                lo, hi = self._layer_slices[0]
                self._layer_slices[0] = (min(lo, o), max(hi, o + (k + 3) // 4 * 4))
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)

    def _allocate(self):
        """What every path has (latents, encoder input, fp32 activations, output, head, objective), then the path's own buffers."""
        dev, B, n = self.device, self.B, self.n
        R = self._enc_rows()
        f32 = dict(dtype=torch.float32, device=dev)
        self.z = torch.empty((2 * B, n), **f32)        # rows [0,B): z ; [B,2B): z~  (the sampler draws the pair)
        self.x = torch.empty((R, n), **f32)            # g(z), g(z~): the encoder's input rows
        L = len(self.linears)
        self.acts = [torch.empty((R, lin.out_features), **f32) for lin in self.linears]     # post-activation outputs; last = pre-head
        self.y = torch.empty((R, n), **f32) if self.head is not None else self.acts[-1]
        self.inv_norm = torch.empty((R,), **f32) if isinstance(self.head, ls.RescaleLayer) else None
        self.side_stream = torch.cuda.Stream(device=dev) if (dev.type == "cuda" and self.overlap_backward) else None
        self._allocate_loss(R)
        # what the forward writes as fp32 (None: planes only), the plane copies, and -- whole-stack path -- the same for every dZ_l
        self.acts_out = [None if only else a for a, only in zip(self.acts, self.encoder_plan.acts_planes_only)]
        self.act_planes, self.dz_planes = [None] * L, [None] * L
        self.dz = self.dz_out = self.signmasks = self.group_ws = None
        if self.fused_backward:
            self._allocate_whole_stack(R)
        else:
            self._allocate_per_layer(R)
        if self.head is not None:
            self.head_part = torch.empty(((R + 255) // 256, n if isinstance(self.head, ls.SoftclipLayer) else 1), **f32)
            self._head_src = hp = self.head.r if isinstance(self.head, ls.RescaleLayer) else self.head.max_abs_bound
            self.head_param = hp.data if isinstance(hp, nn.Parameter) else hp.to(dev).contiguous()
            self.head_learnable = isinstance(hp, nn.Parameter)
            self.dpre = torch.empty((R, n), **f32)

    def _allocate_whole_stack(self, R):
        """Buffers of the one-launch backward chain and the grouped weight gradients."""
        dev, ep = self.device, self.encoder_plan
        widths = [lin.out_features for lin in self.linears]
        shapes = [tuple(lin.weight.shape) for lin in self.linears]
        self.dz = [torch.empty((R, w), dtype=torch.float32, device=dev) for w in widths[:-1]]       # dZ_l for the weight gradients
        self.dz_out = [None if only else d for d, only in zip(self.dz, ep.dz_planes_only)]
        # sign bits of every hidden activation, written by the fused forward, read by the fused backward chain
        self.signmasks = ops.mlp_signmask_alloc(R, len(widths) - 1, dev) + [None]
        if not ep.split_wgrad:
            self.group_ws = ops.mlp_wgrad_workspace(R, shapes, dev)
            return
        for l, kind in enumerate(ep.kinds):
            if kind == 0:                                # dW_l = dZ_l^T acts_{l-1} on the bf16 / fp16 matrix cores
                self.act_planes[l - 1] = ops.mlp_planes_alloc(R, widths[l - 1], True, dev, f16=ep.split_f16)
                self.dz_planes[l] = ops.mlp_planes_alloc(R, widths[l], False, dev, f16=ep.split_f16)
        self.group_ws = ops.mlp_wgrad_split_workspace(R, shapes, dev)

    def _allocate_per_layer(self, R):
        """Buffers of the per-layer backward body: the rotating dZ buffers and the fp32 weight-gradient workspace; with split weight
        gradients the plane copies of their operands; for the chain layers T-plane operands and plane copies of the weights."""
        dev, ep = self.device, self.encoder_plan
        L = len(self.linears)
        widths, in_w = [lin.out_features for lin in self.linears], [lin.in_features for lin in self.linears]
        self.dbuf = [torch.empty((R, max(widths + [self.n])), dtype=torch.float32, device=dev) for _ in range(3)]
        nb = C.c_size_t(); need = 0
        for lin in self.linears:
            _lib.check(_lib.load().clica_linear_wgrad_workspace_bytes(R, lin.out_features, lin.in_features, C.byref(nb)), "wgrad ws")
            need = max(need, nb.value)
        self.wgrad_ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        if not ep.split_wgrad_wide:
            return
        # (f16x2: a tensor of the Split16 state = (family, layer): activations by the layer they feed, gradients and weights by their layer)
        f16w, split = ep.split_f16_wide, [k == 0 for k in ep.wide_kinds]
        self.xin_planes = [ops.mlp_planes_alloc(R, in_w[l], True, dev, f16=f16w) if split[l] else None for l in range(L)]
        self.dzw_planes = [ops.mlp_planes_alloc(R, widths[l], False, dev, f16=f16w) if split[l] else None for l in range(L)]
        self.wide_ws = max((ops.mlp_wgrad_split_workspace(R, [tuple(self.linears[l].weight.shape)], dev) for l in range(L) if split[l]),
                           key=lambda t: t.numel(), default=None)
        if not ep.chain:
            return
        # A chain layer reads its input as T-planes (planes of the transposed activation), written by the previous chain layer's epilogue
        # or converted from fp32 at the chain's head, and writes T-planes for the next chain layer, N-planes for the next layer's weight
        # gradient, fp32 only where an fp32 kernel follows.
        self.wT = {l: ops.mlp_planes_alloc(in_w[l], widths[l], False, dev, f16=f16w) for l in ep.chain}      # planes of W^T
        self.wN = {l: ops.mlp_planes_alloc(widths[l], in_w[l], False, dev, f16=f16w) for l in ep.chain}      # planes of W
        self.xT = {l: ops.mlp_planes_alloc(in_w[l], R, False, dev, f16=f16w) for l in ep.chain}              # T-planes of the layer input
        self.dzT = {l: ops.mlp_planes_alloc(widths[l], R, False, dev, f16=f16w) for l in ep.chain}           # T-planes of dZ_l
        self._wide_packed = False
        # the fused epilogues of the chain never touch the constant-1 column of the N-planes they fill: written once here
        for l in ep.chain:
            if split[l + 1]:
                ops.mlp_planes_from_f32(torch.zeros((R, widths[l]), dtype=torch.float32, device=dev), True, out=self.xin_planes[l + 1],
                                        **self._s16w(0, l + 1))

    def _s16w(self, family: int, index: int) -> dict:
        """Keyword arguments that name a tensor of the f16x2 state for the per-layer producers (empty in the bf16x3 arithmetic)."""
        return dict(state=self.s16, tensor=(family, index)) if self.split_f16_wide else {}

    def _s16l(self, l: int) -> dict:
        """... that name a chain layer of the f16x2 state for the split GEMMs (linear_split_fwd / linear_split_dgrad)."""
        return dict(state=self.s16, layer=l) if self.split_f16_wide else {}

    # -------------------------------------------------------------------------------- data
    def sample(self):
        """z ~ marginal, z~ ~ conditional(z) on device (main_mlp.py:196-200), then x = g(z)."""
        s, B, n = self.sampler, self.B, self.n
        z, zt = self.z[:B], self.z[B:]
        sid = 2 * self.rank
        # both draws in one launch for the coordinate-wise kinds (box, R^n); two for the sphere / vMF
        ops.sample_pair(s.space, s.marginal, s.conditional, n, B, z, zt, marginal_mean=self._eta, m_scale=s.m_param, m_p=s.m_p,
                        c_scale=s.c_param, c_p=s.c_p, box=s.box, seed=s.seed, stream_id=sid, step_dev=self.step_dev)
        self._mix()

    def _mix(self):
        """x = g(z): its own launch, unless the fused forward runs the mixing net in its prologue."""
        self._x_pending = self.mix_in_forward
        if not self.mix_in_forward:
            ops.mixing_fwd(self.z[:self.x.shape[0]], self.gW, self.g_slope, out=self.x, act_kind=self.g_act_kind)

    # -------------------------------------------------------------------------------- step pieces
    def _pack_sample_merged(self) -> bool:
        """The step's two independent front launches -- weight pack and latent pair draw -- in ONE (clica_mlp_pack_split16_both_sample):
        f16x2 arithmetic, packed buffers already allocated, the one-launch sampler path.  False: the caller runs them separately."""
        if self.s16 is None or not self.split_bf16 or self.packed is None or self.packed_t is None:
            return False
        s, B, n = self.sampler, self.B, self.n
        ops.mlp_pack_split16_sample([lin.weight for lin in self.linears], self.packed, self.packed_t, self.s16, s.space, s.marginal,
                                    s.conditional, n, B, self.z[:B], self.z[B:], marginal_mean=self._eta, m_scale=s.m_param, m_p=s.m_p,
                                    c_scale=s.c_param, c_p=s.c_p, box=s.box, seed=s.seed, stream_id=2 * self.rank, step_dev=self.step_dev)
        self._packed_current = True
        self._mix()
        return True

    def pack(self):
        """Fragment-order copies of the CURRENT weights for the fused forward / backward-chain kernels (one launch
        for both layouts when both are used).  Valid until the next optimizer step."""
        ws = [lin.weight for lin in self.linears]
        if self.split_bf16:
            self.packed, self.packed_t = ops.mlp_pack_split_both(ws, self.packed, self.packed_t, state=self.s16)
        elif self.fused_backward:
            self.packed, self.packed_t = ops.mlp_pack_both(ws, self.packed, self.packed_t)
        elif self.fused_forward:
            self.packed = ops.mlp_pack_weights(ws, self.packed)
        self._packed_current = True

    def forward(self):
        self._planes_on_current_scales = True      # (saved_activation: the plane copies this pass writes are scaled by the scales in force NOW)
        if self.fused_forward:
            self._forward_whole_stack()
        else:
            self._forward_per_layer()
        cur = self.acts[-1]
        if self.head is not None:
            lib, st = _lib.load(), _lib.stream_ptr()
            R, n = cur.shape
            if isinstance(self.head, ls.RescaleLayer):
                _lib.check(lib.clica_rescale_fwd(cur.data_ptr(), n, self.head_param.data_ptr(), self.y.data_ptr(), n,
                                                 self.inv_norm.data_ptr(), R, n, st), "clica_rescale_fwd")
            else:
                _lib.check(lib.clica_softclip_fwd(cur.data_ptr(), n, self.head_param.data_ptr(), self.y.data_ptr(), n, R, n, st),
                           "clica_softclip_fwd")

    def _forward_whole_stack(self):
        """One launch for the whole stack, activation panel resident in LDS (csrc/fused_mlp.hip)."""
        cur, mix = self.x, None
        ws = [lin.weight for lin in self.linears]
        if not self._packed_current:
            self.pack()
        if self._x_pending:          # latents in, x = g(z) computed in the kernel prologue and stored to self.x
            cur, mix, self._x_pending = self.z[:self.x.shape[0]], (self.gW, self.g_slope, self.x), False
        if self.split_bf16:
            ops.mlp_fwd_split(cur, ws, [lin.bias for lin in self.linears], self.acts_out, self.packed, self.slope,
                              signmasks=self.signmasks, mix=mix, planes=self.act_planes if self.split_wgrad else None, state=self.s16)
        else:
            ops.mlp_fwd(cur, ws, [lin.bias for lin in self.linears], self.acts, self.slope, packed=self.packed,
                        signmasks=self.signmasks, mix=mix)

    def _forward_per_layer(self):
        """One GEMM per layer: fp32 MFMA, or -- chain layers -- the split GEMM on T-plane operands; the inputs of the split weight
        gradients are converted to planes on the way."""
        cur, chain = self.x, self.chain
        L, R = len(self.linears), self.x.shape[0]
        split = [k == 0 for k in self.wide_kinds] or [False] * L      # layers whose weight gradient reads plane copies
        if chain and not (self._wide_packed and self._packed_current):
            for l in chain:                             # plane copies of the CURRENT weights, both orientations
                ops.mlp_planes_from_f32_t(self.linears[l].weight, out=self.wT[l], **self._s16w(2, l))
                ops.mlp_planes_from_f32(self.linears[l].weight, False, out=self.wN[l], **self._s16w(2, l))
            self._wide_packed = self._packed_current = True
        for l, lin in enumerate(self.linears):
            fed = (l - 1) in chain                      # the previous layer's epilogue already wrote this layer's plane operands
            if split[l] and not fed:                    # this layer's input as planes for its weight gradient
                ops.mlp_planes_from_f32(cur, True, out=self.xin_planes[l], **self._s16w(0, l))
            if l in chain:
                if not fed:
                    ops.mlp_planes_from_f32_t(cur, out=self.xT[l], **self._s16w(0, l))
                nxt = (l + 1) in chain
                cur = None if nxt else self.acts[l]
                ops.linear_split_fwd(self.xT[l], self.wT[l], lin.bias, R, lin.out_features, lin.in_features, l < L - 1, self.slope,
                                     yT=self.xT[l + 1] if nxt else None, yN=self.xin_planes[l + 1] if split[l + 1] else None, yN_ones=True,
                                     y=cur, **self._s16l(l))
            else:
                ops.linear_fwd(cur, lin.weight, lin.bias, leaky=(l < L - 1), slope=self.slope, out=self.acts[l])
                cur = self.acts[l]

    def _head_backward(self):
        """d loss / d (pre-head output): the head's backward (and its parameter gradient), or dy itself."""
        lib, st = _lib.load(), _lib.stream_ptr()
        g = self.dy
        R, n = g.shape
        if self.head is not None:
            pre = self.acts[-1]
            part = self.head_part if self.head_learnable else None
            if isinstance(self.head, ls.RescaleLayer):
                _lib.check(lib.clica_rescale_bwd(pre.data_ptr(), n, self.head_param.data_ptr(), self.inv_norm.data_ptr(),
                                                 g.data_ptr(), n, self.dpre.data_ptr(), n, _lib.ptr(part), R, n, st), "clica_rescale_bwd")
            else:
                _lib.check(lib.clica_softclip_bwd(pre.data_ptr(), n, self.head_param.data_ptr(), g.data_ptr(), n,
                                                  self.dpre.data_ptr(), n, _lib.ptr(part), R, n, st), "clica_softclip_bwd")
            if self.head_learnable:
                torch.sum(self.head_part, dim=0, out=self._gviews[id(self._head_src)])
            g = self.dpre
        return g

    def backward_chain(self, g):
        """Whole data-gradient chain dZ_{L-1} -> ... -> dZ_0 in ONE launch (dZ panel resident in LDS, transposed
        fragment-order weights); every dZ_l is also written to HBM (fp32 and / or bf16 planes) for the weight gradients."""
        L = len(self.linears)
        chain = list(range(L - 1, 0, -1))
        ws = [self.linears[l].weight for l in chain]
        if not self._packed_current:
            self.pack()
        if self.split_bf16:
            h, tail = self.handoff, None
            h.tail_ready = False
            if h.fold_adam and self.plan.chain_tail:
                # inside a training step (N = 1): the chain's workgroups also leave the n-wide first / last layer's weight-gradient
                # slabs (clica_mlp_dgrad_split_tail) -- weight_grads() then needs no tiny-dimension launch
                tail = dict(a_last=self.acts_out[L - 2], x=self.x, shapes=[tuple(lin.weight.shape) for lin in self.linears], ws=self.group_ws,
                            dy_parts=h.dy_parts, mse=h.mse)
                h.tail_ready = True
            if h.dy_parts is not None and (tail is None or g is not self.dy):
                raise _lib.ClicaError("engine: the loss left its partials for the backward chain, but the chain does not run with its tail on dy")
            if h.mse is not None and (tail is None or g is not self.dy):
                raise _lib.ClicaError("engine: the MSE objective was left to the backward chain, but the chain does not run with its tail on dy")
            h.dy_parts = h.mse = None
            ops.mlp_dgrad_chain_split(g, ws, self.packed_t, [self.dz_out[l - 1] for l in chain], self.slope,
                                      masks_chain=[self.signmasks[l - 1] for l in chain],
                                      planes=[self.dz_planes[l - 1] for l in chain] if self.split_wgrad else None, state=self.s16, tail=tail)
        else:
            ops.mlp_dgrad_chain(g, ws, self.packed_t, [self.acts[l - 1] for l in chain], [self.dz[l - 1] for l in chain], self.slope,
                                masks_chain=[self.signmasks[l - 1] for l in chain])

    def weight_grads(self, g, layers=None):
        """dW / db of `layers` (default: every layer): tiny-layer launch + one grouped split-K GEMM of equal-length work items +
        one grouped slab reduction (fp32 MFMA on the fp32 copies, or bf16x3 MFMA on the plane copies in split mode)."""
        L = len(self.linears)
        R = g.shape[0]
        order = list(range(L)) if layers is None else list(layers)
        dWs = [self._gviews[id(self.linears[l].weight)] for l in order]
        dbs = [self._gviews[id(self.linears[l].bias)] for l in order]
        if self.split_wgrad:
            h, adam = self.handoff, None
            if h.fold_adam and layers is None:
                # inside a training step (N = 1): the reduction launch that ends the weight gradients applies the optimizer as well
                # (clica_mlp_wgrad_split_adam) -- optimizer_step() then has nothing left to launch
                adam = dict(param=self.param_arena, grad=self.grad_arena, exp_avg=self.exp_avg, exp_avg_sq=self.exp_avg_sq,
                            step_dev=self.step_dev, lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps,
                            grad_scale=1.0, t_offset=0 if h.ticked else 1, s16=self.s16)
            ops.mlp_wgrad_split(R, [self.dz_planes[l] for l in order], [self.act_planes[l - 1] if l > 0 else None for l in order],
                                [g if l == L - 1 else self.dz_out[l] for l in order],
                                [self.acts_out[l - 1] if l > 0 else self.x for l in order], dWs, dbs, ws=self.group_ws,
                                state=self.s16, a_index=order, d_index=[L - 1 - l for l in order], adam=adam,
                                tail_slabs=adam is not None and h.tail_ready)
            h.tail_ready = False
            if adam is not None:
                h.adam_done = True
        else:
            ops.mlp_wgrad([g if l == L - 1 else self.dz[l] for l in order],
                          [self.acts[l - 1] if l > 0 else self.x for l in order], dWs, dbs, ws=self.group_ws)

    def saved_activation(self, l):
        """fp32 values of layer l's output as saved for the backward pass.  Where a split-bf16 kernel wrote the activation only as
        bf16 planes (no fp32 copy: nobody but the matrix cores reads it) the planes are decoded -- exactly, hi + mid + lo is the
        fp32 value.  Inspection / tests."""
        R, w = self.x.shape[0], self.linears[l].out_features
        # f16x2: the planes are scaled by the activation scale the pass that WROTE them ran with -- the scales in force if no update has run
        # since (a bare forward(), a calibration pass), the previous ones (kept by the update) after a full step
        which = "scales_a" if self._planes_on_current_scales else "last_scales_a"
        if l in self.chain and (l + 1) in self.chain:
            if self.split_f16_wide:
                return ops.mlp_planes16_to_f32(self.xin_planes[l + 1], R, w, True, self.s16.read()[which][l + 1])
            return ops.mlp_planes_to_f32(self.xin_planes[l + 1], R, w, True)
        if self.acts_out[l] is None:
            if self.split_f16:
                return ops.mlp_planes16_to_f32(self.act_planes[l], R, w, True, self.s16.read()[which][l + 1])
            return ops.mlp_planes_to_f32(self.act_planes[l], R, w, True)
        return self.acts[l]

    def _wgrad_layer(self, l, g, inp, ws, planes_ready=False):
        """dW_l / db_l of one layer on the per-layer path: fp32 MFMA GEMM, or -- wide encoders in split mode -- the split-bf16
        kernel on plane copies (dZ converted here, the layer input converted in forward())."""
        lin = self.linears[l]
        dW, db = self._gviews[id(lin.weight)], self._gviews[id(lin.bias)]
        if self.split_wgrad_wide and self.wide_kinds[l] == 0:
            if not planes_ready:                            # (a split data-gradient epilogue has written dZ_l's planes already)
                ops.mlp_planes_from_f32(g, False, out=self.dzw_planes[l], **self._s16w(1, l))
            ops.mlp_wgrad_split(self.x.shape[0], [self.dzw_planes[l]], [self.xin_planes[l]], [None], [None], [dW], [db], ws=self.wide_ws,
                                **(dict(state=self.s16, a_index=[l], d_index=[l]) if self.split_f16_wide else {}))
        else:
            ops.linear_wgrad(g, inp, dW=dW, db=db, accumulate=False, ws=ws)

    def backward(self):
        g = self._head_backward()
        if self.fused_backward:
            self._backward_whole_stack(g)
        else:
            self._backward_per_layer(g)

    def _backward_whole_stack(self, g):
        """(1) the data-gradient chain in one launch; (2) the grouped weight gradients -- under data parallelism with the layers'
        slices of the gradient arena handed to the buckets, in two halves where that is planned."""
        L, st, buckets = len(self.linears), self.stamps, self.buckets
        if st:
            ops.stamp(st["mlp_dgrad"], 0)
        self.backward_chain(g)
        if self._guard_rides:                      # this rank's verdict into the slot the first gradient bucket carries
            self.s16.poison_export(self._guard_slot)
        if st:
            ops.stamp(st["mlp_dgrad"], 1)
        if buckets is None:
            if st:
                ops.stamp(st["mlp_wgrad"], 0)
            self.weight_grads(g)
            if st:
                ops.stamp(st["mlp_wgrad"], 1)
            return
        if self.wgrad_halves:
            h = self._half
            self.weight_grads(g, layers=range(h, L))          # the head parameter's slot rides in the first slice
            for i in range(0, L - h):
                buckets.layer_done(i)                         # completion index i = layer L - 1 - i: all-reduce starts now ...
            self.weight_grads(g, layers=range(0, h))          # ... and runs under this launch
            for i in range(L - h, L):
                buckets.layer_done(i)
        else:
            self.weight_grads(g)
            for i in range(L):
                buckets.layer_done(i)
        buckets.wait()

    def _backward_per_layer(self, g):
        """Two streams: wgrad_l (weight / bias gradients into the arena, + bucket all-reduce) runs on the side stream while the main
        stream continues the dZ chain with dgrad_l -- the two GEMMs are independent given dZ_l, and each hides the other's prologue /
        epilogue-store bubbles.  Three dZ buffers rotate; a buffer is rewritten only after the wgrad that read it has finished."""
        L, R, chain, side = len(self.linears), self.x.shape[0], self.chain, self.side_stream
        main = torch.cuda.current_stream(self.device) if self.device.type == "cuda" else None
        two = side is not None and main is not None
        reader_done = {}        # dZ buffer index -> event of the wgrad that reads it
        buf_of_g = None         # index into self.dbuf holding the current dZ (None: self.dy / self.dpre, or planes only)
        nxt = 0
        dzN_ready = dzT_ready = False       # dZ_l already sits in dzw_planes[l] / dzT[l] (written by a split data-gradient epilogue)

        def take():             # the next dZ buffer, cut to dZ_{l-1}, once the wgrad that read it last is done (WAR)
            if two and nxt in reader_done:
                main.wait_event(reader_done.pop(nxt))
            return self.dbuf[nxt][:, :lin.in_features]
        for l in reversed(range(L)):
            lin = self.linears[l]
            inp = self.acts[l - 1] if l > 0 else self.x
            if two:
                side.wait_stream(main)                      # dZ_l is complete on main
            with torch.cuda.stream(side) if two else _nullctx():
                self._wgrad_layer(l, g, inp, self.wgrad_ws, planes_ready=dzN_ready)
                if self.buckets is not None:
                    self.buckets.layer_done(L - 1 - l)
                if two and buf_of_g is not None:
                    ev = torch.cuda.Event(); ev.record(side); reader_done[buf_of_g] = ev
            if l == 0:
                break
            if l in chain:
                # dZ_{l-1} = (dZ_l W_l) * LeakyReLU'(acts_{l-1}) on the split bodies: T-planes in, gate from the T-planes of the
                # layer input, T-planes out for the next chain layer, N-planes out for the weight gradient of layer l - 1
                if not dzT_ready:
                    ops.mlp_planes_from_f32_t(g, out=self.dzT[l], **self._s16w(1, l))
                prev = (l - 1) in chain                     # dZ_{l-1} goes on as T-planes: no fp32 copy
                out = None if prev else take()
                dxN = self.dzw_planes[l - 1] if self.wide_kinds[l - 1] == 0 else None
                ops.linear_split_dgrad(self.dzT[l], self.wN[l], self.xT[l], self.slope, R, lin.out_features, lin.in_features,
                                       dxT=self.dzT[l - 1] if prev else None, dxN=dxN, dx=out, **self._s16l(l))
                dzT_ready, dzN_ready = prev, dxN is not None
            else:
                out = take()
                ops.linear_dgrad(g, lin.weight, inp, self.slope, out=out)
                dzN_ready = dzT_ready = False
            g, buf_of_g = out, (nxt if out is not None else None)
            if out is not None:
                nxt = (nxt + 1) % len(self.dbuf)
        if two:
            main.wait_stream(side)
        if self.buckets is not None:
            self.buckets.wait()
        if self.dp and self.s16 is not None:
            # producers run until the last layer's gradient, so the verdict is reduced on its own (4 bytes) behind them
            self.s16.poison_export(self._guard_slot)
            dist.all_reduce(self._guard_slot, op=dist.ReduceOp.SUM, group=self.pg)

    def _adam_folds_into_wgrad(self) -> bool:
        """Does the weight-gradient reduction of a step apply the optimizer as well (StepPlan.adam_in_wgrad)?"""
        return self.plan.adam_in_wgrad

    def optimizer_step(self):
        self._packed_current = False
        h = self.handoff
        ticked, h.ticked = h.ticked, False
        if h.adam_done:       # applied by the weight-gradient reduction of this step (weight_grads)
            h.adam_done = False
            h.scales_updated = self.s16 is not None
        else:
            fused_update = ops.adam_step(self.param_arena, self.grad_arena, self.exp_avg, self.exp_avg_sq, self.step_dev, self.lr,
                                         self.betas[0], self.betas[1], self.eps, grad_scale=1.0 / (self.world * self.dry_ranks),
                                         t_offset=0 if ticked else 1, s16=self.s16)
            h.scales_updated = bool(fused_update)
        if not ticked:
            ops.tick(self.step_dev)

    # -------------------------------------------------------------------------------- whole step
    def _step_body(self, sample: bool):
        # The fragment-order weight copies only depend on the parameters; they are packed IN LINE in front of the forward -- merged with the
        # latent pair draw into one launch where that exists.  (Rounds 2-5 packed on a side stream beside the samplers: the fork / join of
        # a HIP graph costs more than the 9 us of sampling it hid, profiles/r4_DESIGN_history.md.)
        if self.s16 is not None and not self._s16_calibrated:
            self.calibrate_scales(sample)
        self._packed_current = False          # a step always re-packs (parameters may have been set from outside)
        fused = self.fused_forward and self.device.type == "cuda"
        if not (sample and fused and self._pack_sample_merged()):
            if sample:
                self.sample()
            if fused:
                self.pack()                    # (here, not inside forward(): bench.py's stamps bracket the encoder launch alone)
        st = self.stamps
        if st:
            ops.stamp(st["null"], 0); ops.stamp(st["null"], 1)      # empty bracket: the stamp pair's own cost, subtracted by the reader
            ops.stamp(st["mlp_fwd"], 0)
        self.forward()
        if st:
            ops.stamp(st["mlp_fwd"], 1)
        h = self.handoff
        h.in_step = True                       # (loss_forward_backward may leave dy to be finished by this step's backward chain)
        try:
            self.loss_forward_backward()
            h.fold_adam = self.plan.adam_in_wgrad
            self.backward()
        finally:
            h.reset("fold_adam", "in_step")
        self.optimizer_step()
        if self.s16 is not None and not h.scales_updated:
            self.s16.update()                  # this step's recorded maxima -> the next step's scales (normally inside the Adam launch)
        self._planes_on_current_scales = False     # (an update has run behind the forward that wrote the planes)

    def calibrate_scales(self, sample: bool = True, passes: Optional[int] = None):
        """f16x2 arithmetic: a launch runs on the scales derived from the PREVIOUS step's maxima, so before the first step (and after
        parameters were replaced from outside) the scales are brought up to the data by un-applied passes: pack, forward, loss and
        backward on the current batch (sampled when `sample`), scale update, no optimizer step; the device step / RNG counter is put
        back, so the first real step draws the very batch it would have drawn.  L + 1 passes: a producer measures its output in fp32
        BEFORE it is cut to fp16, so a pass on scales of 1 gets every activation right, but a gradient of 1e-8 is flushed on its way into
        the next chain link and that link then measures nothing -- each pass settles (at least) one more link of the chain."""
        if self.s16 is None:
            return
        passes = len(self.linears) + 1 if passes is None else int(passes)
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("calibrate_scales() inside a graph capture: call capture(), which calibrates first")
        self._s16_calibrated = True
        tick = self.step_dev.clone()
        for _ in range(passes):
            self._packed_current = False
            if sample:
                self.sample()
            elif self.mix_in_forward:
                self._x_pending = True           # the injected latents go through the mixing prologue again
            self.forward()
            self.loss_forward_backward()
            self.backward()
            self.s16.update()
            self._planes_on_current_scales = False
            self.step_dev.copy_(tick)
            self.handoff.reset("ticked")
        self.s16.clear_flags()                   # the first pass ran on scales of 1: whatever it flagged is not a finding
        self._versions_seen = self._param_versions()
        self._guard_skipped_seen = self.s16.guard()["skipped"]      # (calibration passes the guard withheld are not training steps)

    def _param_versions(self) -> int:
        """Changes when somebody writes the parameters through torch (load_state_dict, copy_, an optimizer of their own): the kernels write
        the arena through raw pointers and leave the version counters alone."""
        return int(self.param_arena._version) + sum(int(q._version) for q in self.f.parameters())

    def _check_external_writes(self):
        """f16x2: parameters replaced from outside since the last look -> the scales are re-measured before the next step.
        Without this the device-side guard would still keep a step on stale scales away from the parameters; this saves its redo steps."""
        if self.s16 is None or not self._watch_versions:
            return
        v = self._param_versions()
        if v != self._versions_seen:
            self._versions_seen = v
            self._s16_calibrated = False
            if self.graph is not None and not torch.cuda.is_current_stream_capturing():
                self.calibrate_scales(True)

    def check_arith(self, raise_on_bug: bool = True) -> dict:
        """LOG-POINT check of the f16x2 arithmetic (host read + sync; a no-op dict for the other arithmetics): the guard's flags, how many
        steps it has withheld so far (`skipped`; `new_skipped` since the last call) and whether the last step is poisoned.  A withheld step
        left parameters, moments and the step / RNG counter untouched and the next step redid its batch on fresh scales, so training has
        lost replays, not correctness; callers that count steps compare with `steps_done`.  Flag bit 2 -- an overflow the update saw but no
        producer announced -- would be a hole in the guard and raises."""
        if self.s16 is None:
            return dict(flags=0, skipped=0, new_skipped=0, poisoned=False, updates=0)
        g = self.s16.guard()
        g["new_skipped"] = g["skipped"] - self._guard_skipped_seen
        self._guard_skipped_seen = g["skipped"]
        if raise_on_bug and (g["flags"] & 4):
            raise _lib.ClicaError("f16x2 arithmetic: the scale update saw an overflow that no producer had announced (flags bit 2): a "
                                  "producer kernel without the guard -- results since the last check are not to be trusted")
        return g

    def arith_state(self) -> dict:
        """Which encoder arithmetic runs and, for f16x2, the state of its scales (host read + sync: log points, tests).  A non-zero
        `flags` means a tensor outgrew its scale by more than 64 x within one step: the step that raised it is not to be trusted."""
        if self.s16 is not None:
            return dict(arith=self._arith_name(), **self.s16.read())
        return dict(arith=self._arith_name())

    def _arith_name(self) -> str:
        """The `arith` string of arith_state() (no device read)."""
        ep = self.encoder_plan
        return ep.arith + (" (per-layer wide path; narrow layers native fp32 MFMA)" if ep.split_f16_wide else "")

    # -------------------------------------------------------------------------------- checkpoints
    STATE_FORMAT, STATE_VERSION = "cl_ica_amd.trainer", 1

    def _head_name(self) -> str:
        if self.head is None:
            return "none"
        return f"{type(self.head).__name__}({'learnable' if self.head_learnable else 'fixed'})"

    def _config(self) -> dict:
        """Everything that decides the trajectory of a run besides its state (state_dict()["config"]; load_state_dict(strict=True)
        compares it field by field)."""
        samp = dataclasses.asdict(self.sampler)
        samp["box"] = [float(v) for v in samp["box"]]
        return dict(sampler=samp, batch_size=self.B, p=self.p, tau=self.tau, alpha=self.alpha, g_weights=self.gW.detach().cpu().clone(),
                    g_slope=self.g_slope, g_act_kind=self.g_act_kind, world=self.world, dry_ranks=self.dry_ranks,
                    layer_shapes=[[int(lin.out_features), int(lin.in_features)] for lin in self.linears], head=self._head_name())

    def _loss_state(self):
        """What the objective's workspace carries from step to step, as the library's opaque blob (None: nothing)."""
        return None

    def _load_loss_state(self, blob):
        pass

    def _not_in_capture(self, what: str):
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{what} inside a graph capture: it reads / writes the trainer's state from the host")

    def state_dict(self) -> dict:
        """Everything the next step depends on, as a plain dict of CPU tensors, numbers, strings, lists and dicts (survives torch.save /
        torch.load(weights_only=True)): the encoder's state dict (`f`: the reference's keys, what {sup,unsup}_f.pth holds), the Adam
        moments in torch.optim.Adam's layout (`optimizer`: interchangeable with cl_ica_amd.optim.Adam and torch.optim.Adam over
        f.parameters()), the device step / RNG counter (`step`), the configuration the trajectory depends on (`config`) and what the
        arithmetic carries from step to step (`arith`: the f16x2 scales and guard words, the matrix-core loss sweeps' grid and guard
        words -- opaque blobs written by the library, None where the trainer has no such state).  Between steps only: one
        synchronisation, never inside a capture."""
        self._not_in_capture("state_dict()")
        cuda = self.device.type == "cuda"
        s16_blob = self.s16.export_state() if self.s16 is not None else None
        loss_blob = self._loss_state() if cuda else None
        f_sd = self.f.state_dict()
        dev = [self.exp_avg, self.exp_avg_sq, self.step_dev] + list(f_sd.values()) + [b for b in (s16_blob, loss_blob) if b is not None]
        if cuda:        # every read queued behind the step's launches, one wait for all of them
            host = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True).copy_(t.detach(), non_blocking=True) for t in dev]
            torch.cuda.current_stream(self.device).synchronize()
            host = [t.clone() for t in host]
        else:
            host = [t.detach().clone() for t in dev]
        exp_avg, exp_avg_sq, step = host[0], host[1], int(host[2].item())
        f_host = dict(zip(f_sd.keys(), host[3:3 + len(f_sd)]))
        blobs = host[3 + len(f_sd):]
        state, params, off = {}, list(self.f.parameters()), 0
        for i, prm in enumerate(params):
            if step > 0:      # (cl_ica_amd.optim.Adam and torch.optim.Adam: no state before the first step)
                sl = slice(off, off + prm.numel())
                state[i] = dict(step=torch.tensor(float(step)), exp_avg=exp_avg[sl].view(prm.shape).clone(),
                                exp_avg_sq=exp_avg_sq[sl].view(prm.shape).clone())
            off += (prm.numel() + 3) // 4 * 4
        group = dict(lr=self.lr, betas=(float(self.betas[0]), float(self.betas[1])), eps=self.eps, weight_decay=0, amsgrad=False,
                     params=list(range(len(params))))
        arith = dict(arith=self._arith_name(), clica_version=int(_lib.load().clica_version()), s16_calibrated=bool(self._s16_calibrated),
                     split16=blobs.pop(0) if s16_blob is not None else None, loss=blobs.pop(0) if loss_blob is not None else None)
        return dict(format=self.STATE_FORMAT, version=self.STATE_VERSION, kind=self._kind, f=f_host,
                    optimizer=dict(state=state, param_groups=[group]), step=step, config=self._config(), arith=arith)

    def _check_config(self, sd: dict, strict: bool):
        """ValueError naming the first field of a checkpoint that does not fit this trainer (shapes and kind always; with `strict`
        everything that changes the trajectory)."""
        def differ(field, saved, mine):
            raise ValueError(f"load_state_dict: `{field}` of the checkpoint ({saved!r}) differs from this trainer's ({mine!r})")
        if sd.get("format") != self.STATE_FORMAT or int(sd.get("version", -1)) != self.STATE_VERSION:
            raise ValueError(f"load_state_dict: not a {self.STATE_FORMAT} checkpoint of version {self.STATE_VERSION} "
                             f"(format {sd.get('format')!r}, version {sd.get('version')!r})")
        if sd["kind"] != self._kind:
            differ("kind", sd["kind"], self._kind)
        saved, mine = sd["config"], self._config()
        if [list(s) for s in saved["layer_shapes"]] != mine["layer_shapes"]:
            differ("layer_shapes", saved["layer_shapes"], mine["layer_shapes"])
        want = {k: tuple(v.shape) for k, v in self.f.state_dict().items()}
        got = {k: tuple(v.shape) for k, v in sd["f"].items()}
        if want != got:
            differ("f", got, want)
        if not strict:
            return
        for key in ("head", "batch_size", "p", "tau", "alpha", "g_slope", "g_act_kind", "world", "dry_ranks"):
            if saved[key] != mine[key]:
                differ(key, saved[key], mine[key])
        for key, val in mine["sampler"].items():
            sv = saved["sampler"].get(key)
            if (list(sv) if isinstance(sv, (list, tuple)) else sv) != val:
                differ(f"sampler.{key}", sv, val)
        if tuple(saved["g_weights"].shape) != tuple(mine["g_weights"].shape) or not torch.equal(saved["g_weights"], mine["g_weights"]):
            differ("g_weights", tuple(saved["g_weights"].shape), tuple(mine["g_weights"].shape))
        group = sd["optimizer"]["param_groups"][0]
        for key, val in (("lr", self.lr), ("eps", self.eps)):      # (kernel arguments of a captured step: they cannot follow the file)
            if float(group[key]) != val:
                differ(f"optimizer.{key}", group[key], val)
        if tuple(float(b) for b in group["betas"]) != (float(self.betas[0]), float(self.betas[1])):
            differ("optimizer.betas", group["betas"], self.betas)

    def load_state_dict(self, sd: dict, strict: bool = True) -> str:
        """Continue the run a `state_dict()` was taken from.  Written IN PLACE (copy_ into the arenas and the step counter: every
        data_ptr() stays, a captured graph stays valid and is not captured again), before or after capture(), on a fresh trainer or one
        that has stepped.  `strict`: a difference in anything that changes the trajectory -- kind, layer shapes, head, batch size, p / tau /
        alpha, any SamplerSpec field (seed included), the mixing weights, world, dry_ranks, the optimizer's constants -- raises ValueError
        naming the field; otherwise only kind and shapes bind.  Returns the domain that applied: "exact" -- the arithmetic and the library
        version are the saved ones, the blobs of `arith` are installed and the continuation is bit-identical to the uninterrupted run --
        or "portable": parameters, moments and step are restored exactly, the blobs are ignored and the f16x2 scales are calibrated anew
        (the counter is put back, so the batch sequence is still the saved run's); agreement within the arithmetic's tolerance."""
        self._not_in_capture("load_state_dict()")
        self._check_config(sd, strict)
        cuda = self.device.type == "cuda"
        with torch.no_grad():
            for key, dst in self.f.state_dict().items():          # (views of the parameter arena, and the head's buffers)
                dst.copy_(sd["f"][key])
            params, off = list(self.f.parameters()), 0
            ostate = sd["optimizer"]["state"]
            for i, prm in enumerate(params):
                st = ostate.get(i, ostate.get(str(i)))
                sl = slice(off, off + prm.numel())
                if st is None:
                    self.exp_avg[sl].zero_(); self.exp_avg_sq[sl].zero_()
                else:
                    self.exp_avg[sl].view(prm.shape).copy_(st["exp_avg"])
                    self.exp_avg_sq[sl].view(prm.shape).copy_(st["exp_avg_sq"])
                off += (prm.numel() + 3) // 4 * 4
            self.step_dev.fill_(int(sd["step"]))
        arith = sd["arith"]
        exact = (arith["arith"] == self._arith_name() and int(arith["clica_version"]) == int(_lib.load().clica_version())
                 and (arith["split16"] is not None) == (self.s16 is not None))
        if exact:
            if self.s16 is not None:
                self.s16.import_state(arith["split16"])
                self._s16_calibrated = bool(arith["s16_calibrated"])
                self._guard_skipped_seen = self.s16.guard()["skipped"]
            if arith["loss"] is not None and cuda:
                self._load_loss_state(arith["loss"])
        else:
            self._s16_calibrated = False
        # the load is not an "external write": what the kernels derive from the parameters is marked stale, nothing is re-measured
        self._versions_seen = self._param_versions()
        self._packed_current = False
        self._x_pending = False
        self.handoff.reset()
        ops.PARAM_EPOCH += 1
        if not exact and self.s16 is not None and self.graph is not None:
            self.calibrate_scales(True)        # a replayed graph cannot calibrate on its own (as _check_external_writes does)
        return "exact" if exact else "portable"

    def step(self):
        """One unsupervised step with on-device sampling.  Returns the device tensor
        ``[loss_mean, pos_mean, neg_mean]`` of this rank's rows (no host sync)."""
        self._check_external_writes()
        if self.graph is not None:
            self.graph.replay()
            self._planes_on_current_scales = False
            # a replay updates the parameter arena without passing through ops.adam_step: caches derived from the weights
            # (the drop-in encoder's fragment-order packs, encoders._MLPFusedFn) key on this epoch and must see the change
            ops.PARAM_EPOCH += 1
        else:
            self._step_body(True)
        return self._result()

    def step_injected(self, z1, z2=None):
        self._check_external_writes()
        self.inject(z1, z2)
        self._step_body(False)
        ops.PARAM_EPOCH += 1
        return self._result()

    def capture(self, warmup: int = 3):
        """Capture the step into a HIP graph (counters and RNG offsets live on device, so replays
        advance them).  With data parallelism the RCCL collectives (all-gather, reduce-scatter, bucketed
        all-reduce on the side stream) are captured into the same graph; every rank must call capture()
        and then replay in lock-step."""
        # warm-up launches (lazy kernel-attribute setup, allocator) must not count as training: snapshot
        # and restore parameters, optimizer state and the device step / RNG counter around them
        if self.s16 is not None and not self._s16_calibrated:
            self.calibrate_scales(True)
        # (also what makes a step depend on its predecessors besides the parameters: the f16x2 scales, and the loss workspace -- the
        #  matrix-core sweeps build their planes on the grid the previous call measured, csrc/lp_mfma.h)
        state = (self.param_arena, self.exp_avg, self.exp_avg_sq, self.step_dev, self.loss_ws) + ((self.s16.buf,) if self.s16 is not None else ())
        snap = [t.clone() for t in state]
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            for _ in range(warmup):
                self._step_body(True)
        torch.cuda.current_stream(self.device).wait_stream(s)
        torch.cuda.synchronize(self.device)
        for dst, src in zip(state, snap):
            dst.copy_(src)
        self._versions_seen = self._param_versions()      # (the restore wrote the arena through torch: not an external write)
        graph = torch.cuda.CUDAGraph()
        # with collectives in the step, other threads (the process group's watchdog) may legitimately touch the HIP runtime
        # during capture: "thread_local" keeps their calls from invalidating it
        mode = "thread_local" if (self.dp or self.force_collectives) else "global"
        # Explicit begin / end instead of the `torch.cuda.graph` context manager: when the body fails (a collective backend that
        # cannot be captured), that manager raises from capture_end() inside its __exit__ and never restores the stream -- the
        # process is left on a stream that is still capturing and every later CUDA call fails.  Here a failed capture is always
        # terminated (through the HIP runtime if torch refuses), the stream context is always left, and the caller gets the
        # original exception with the device in a usable state (bench.py / train_mlp then run eager launches).
        cap = torch.cuda.Stream(device=self.device)
        cap.wait_stream(torch.cuda.current_stream(self.device))
        try:
            with torch.cuda.stream(cap):
                graph.capture_begin(capture_error_mode=mode)
                try:
                    self._step_body(True)
                    graph.capture_end()
                except BaseException:
                    _abort_capture(graph, cap, (self.side_stream,))
                    if self.side_stream is not None:      # a forked stream cannot be taken out of an invalidated capture: drop it
                        self.side_stream = torch.cuda.Stream(device=self.device)
                    raise
        finally:
            torch.cuda.current_stream(self.device).wait_stream(cap)
        self.graph = graph
        return graph

    @property
    def steps_done(self) -> int:
        return int(self.step_dev.item())


class ContrastiveTrainer(_FusedTrainer):
    """The fused step with the pair's InfoNCE objective (the module's docstring); keywords beyond `device` are _FusedTrainer's."""
    fold_dy_reduce = True        # test hook, as chain_tail: the chain's prologue finishes dy from the loss sweep's partials (no reduction launch)
    _kind = "contrastive"

    def __init__(self, f: nn.Sequential, g_weights: torch.Tensor, sampler: SamplerSpec, batch_size: int,
                 p: float = 2, tau: float = 1.0, alpha: float = 0.5, lr: float = 1e-4, g_slope: float = 0.2,
                 betas=(0.9, 0.999), eps: float = 1e-8, device=None, **engine):
        self.p, self.tau, self.alpha = float(p), float(tau), float(alpha)
        # p = 0: SimCLRLoss(normalize=False, tau, alpha) -- InfoNCE on dot products (losses.py:162-202), the objective of the
        # reference's hypersphere experiment; the loss runs on the dot kind's training pair (csrc/dot_train.hip)
        self.dot = self.p == 0
        super().__init__(f, g_weights, sampler, batch_size, lr=lr, g_slope=g_slope, betas=betas, eps=eps, device=device, **engine)

    def _enc_rows(self) -> int:
        """Rows the encoder runs on per step: the pair z, z~ stacked."""
        return 2 * self.B

    def _allocate_loss(self, R):
        """Buffers of the objective: the InfoNCE loss of the pair -- Lp distances for p >= 1, dot products for p = 0 (the dot kind's
        training pair) -- with its outputs, its workspace and the negatives pool under data parallelism."""
        dev, B, n = self.device, self.B, self.n
        f32 = dict(dtype=torch.float32, device=dev)
        self.dy = torch.empty((R, n), **f32)
        self.loss_out = torch.empty(3 * B + 3, **f32)
        Bg = B * self.world * self.emulate_pool * self.dry_ranks
        pooled = self.dp or self.emulate_pool > 1
        self.z_all = torch.empty((Bg, n), **f32) if pooled else None
        self.lse_all = torch.empty((Bg,), **f32) if pooled else None
        if self.dot:
            # dot-product InfoNCE: one training pair (forward with its tile finisher, symmetric backward + reduction); its workspace
            # holds arrival counters that must start at zero
            self.desc = _lib.DotLossDesc(B=B, B3=Bg, n=n, tau=self.tau, alpha=self.alpha, normalize=0)
            tb = C.c_size_t()
            _lib.check(_lib.load().clica_dot_loss_train_workspace_bytes(C.byref(self.desc), C.byref(tb)), "dot train workspace")
            self.loss_ws = torch.zeros(tb.value, dtype=torch.uint8, device=dev)
            self.loss_train = self.early_tick = True
            return
        self.desc = _lib.LpLossDesc(B=B, B3=Bg, n=n, p=self.p, tau=self.tau, alpha=self.alpha, compat=1, pow=1)
        fb, bb = C.c_size_t(), C.c_size_t()
        _lib.check(_lib.load().clica_lp_loss_workspace_bytes(C.byref(self.desc), C.byref(fb), C.byref(bb)), "workspace")
        tb = C.c_size_t()
        self.loss_train = self.p >= 1                  # fused training pair of loss entry points
        if self.loss_train:
            _lib.check(_lib.load().clica_lp_loss_train_workspace_bytes(C.byref(self.desc), C.byref(tb)), "train workspace")
        self.loss_ws = torch.zeros(max(fb.value, bb.value, tb.value), dtype=torch.uint8, device=dev)
        # the step / RNG counter is advanced by the loss backward's reduction launch (all samplers of the step have run by then)
        # instead of a separate one-thread launch at the end; Adam then takes t = counter
        self.early_tick = self.loss_train

    def _objective_folds(self, on_dy: bool):
        return on_dy and self.fold_dy_reduce and self.loss_train and not self.dot, False

    def inject(self, z1: torch.Tensor, z2: torch.Tensor):
        """Use caller-provided latents instead of the device sampler (parity tests)."""
        self.z[:self.B].copy_(z1); self.z[self.B:].copy_(z2)
        self._mix()

    def _result(self) -> torch.Tensor:
        return self.loss_out[3 * self.B:]

    def _pooled(self, rows: torch.Tensor, pool: Optional[torch.Tensor]) -> torch.Tensor:
        """This rank's `rows` (B of them) as every rank's: all-gathered into `pool` under data parallelism -- in a dry run the other
        ranks' rows are copies of this rank's --, replicated into it for the emulated pool, themselves otherwise."""
        B = self.B
        if self.dp:
            dry = self.dry_ranks > 1
            dist.all_gather_into_tensor(pool[:B * self.world] if dry else pool, rows.contiguous(), group=self.pg)
            if dry:
                pool.view(self.dry_ranks, *rows.shape)[1:].copy_(pool[:B].unsqueeze(0))
        elif self.emulate_pool > 1:
            pool.view(self.emulate_pool, *rows.shape).copy_(rows.unsqueeze(0))
        else:
            return rows
        return pool

    def loss_forward_backward(self):
        """Loss forward + its backward w.r.t. the embeddings.  The negatives are "all z1_rec of the (global)
        batch" (the reference's roll, main_mlp.py:272, up to a permutation), so the pair matrix is symmetric
        and ONE backward sweep with both rows' softmax statistics gives dz1 complete: no row pass, no column
        pass, and under data parallelism no reduce-scatter of d/dz3 -- only an all-gather of the B
        log-sum-exp values next to the all-gather of the embeddings."""
        lib, st = _lib.load(), _lib.stream_ptr()
        B, n, o, h = self.B, self.n, self.loss_out, self.handoff
        y1, y2 = self.y[:B], self.y[B:]
        lse = o[2 * B:3 * B]
        pool = self._pooled(y1, self.z_all)
        tick = self.step_dev.data_ptr() if self.early_tick else None
        if self.dot:
            self._dot_forward_backward(y1, y2, pool, lse, tick)
            return
        if self.loss_train:
            # forward + coefficient step (finalize), then -- after the all-gather of the row statistics under DP -- pair sweep +
            # reduction (+ the forward's means): 5 launches instead of 8
            _lib.check(lib.clica_lp_loss_fwd_train(C.byref(self.desc), y1.data_ptr(), n, y2.data_ptr(), n, pool.data_ptr(), n,
                                                   o[:B].data_ptr(), o[B:2 * B].data_ptr(), lse.data_ptr(),
                                                   self.dy[:B].data_ptr(), n, self.dy[B:].data_ptr(), n,
                                                   self.loss_ws.data_ptr(), self.loss_ws.numel(), st), "clica_lp_loss_fwd_train")
            pool_lse = self._pooled(lse, self.lse_all)
            h.dy_parts = None
            if h.in_step and self.plan.dy_from_partials:
                # N = 1 training step: no reduction launch -- the backward chain's prologue sums the pair sweep's partials into dy, leaves
                # the forward's means and ticks the counter (clica_lp_dy_parts; same sums in the same order)
                h.dy_parts = _lib.DyParts()
                self._dy_parts_taken += 1
                _lib.check(lib.clica_lp_loss_bwd_sym_train_parts(C.byref(self.desc), y1.data_ptr(), n, pool.data_ptr(), n,
                                                                 lse.data_ptr(), pool_lse.data_ptr(), o[3 * B:].data_ptr(), tick,
                                                                 self.loss_ws.data_ptr(), self.loss_ws.numel(), C.byref(h.dy_parts), st),
                           "clica_lp_loss_bwd_sym_train_parts")
            else:
                _lib.check(lib.clica_lp_loss_bwd_sym_train(C.byref(self.desc), y1.data_ptr(), n, pool.data_ptr(), n,
                                                           lse.data_ptr(), pool_lse.data_ptr(), self.dy[:B].data_ptr(), n, o[3 * B:].data_ptr(),
                                                           tick, self.loss_ws.data_ptr(), self.loss_ws.numel(), st), "clica_lp_loss_bwd_sym_train")
            h.ticked = self.early_tick
            return
        _lib.check(lib.clica_lp_loss_fwd(C.byref(self.desc), y1.data_ptr(), n, y2.data_ptr(), n, pool.data_ptr(), n,
                                         o[:B].data_ptr(), o[B:2 * B].data_ptr(), lse.data_ptr(), o[3 * B:].data_ptr(),
                                         None, 0, self.loss_ws.data_ptr(), self.loss_ws.numel(), st), "clica_lp_loss_fwd")
        pool_lse = self._pooled(lse, self.lse_all)
        _lib.check(lib.clica_lp_loss_bwd_sym(C.byref(self.desc), y1.data_ptr(), n, y2.data_ptr(), n, pool.data_ptr(), n,
                                             lse.data_ptr(), pool_lse.data_ptr(), None, None, None,
                                             self.dy[:B].data_ptr(), n, self.dy[B:].data_ptr(), n,
                                             self.loss_ws.data_ptr(), self.loss_ws.numel(), st), "clica_lp_loss_bwd_sym")

    def _dot_forward_backward(self, y1, y2, pool, lse, tick):
        """p = 0: the dot kind's training pair.  Forward (one launch: pair sweep + tile finisher; writes loss_i, pos_i, lse_i and the
        positive-pair part of dy), the all-gather of the row log-sum-exps under data parallelism, then the symmetric sweep and the
        reduction launch that adds it into dy[:B], writes the three means and advances the step counter."""
        lib, st = _lib.load(), _lib.stream_ptr()
        B, n, o = self.B, self.n, self.loss_out
        _lib.check(lib.clica_dot_loss_fwd_train(C.byref(self.desc), y1.data_ptr(), n, y2.data_ptr(), n, pool.data_ptr(), n,
                                                o[:B].data_ptr(), o[B:2 * B].data_ptr(), lse.data_ptr(),
                                                self.dy[:B].data_ptr(), n, self.dy[B:].data_ptr(), n,
                                                self.loss_ws.data_ptr(), self.loss_ws.numel(), st), "clica_dot_loss_fwd_train")
        pool_lse = self._pooled(lse, self.lse_all)
        self.handoff.dy_parts = None
        _lib.check(lib.clica_dot_loss_bwd_sym_train(C.byref(self.desc), y1.data_ptr(), n, pool.data_ptr(), n,
                                                    lse.data_ptr(), pool_lse.data_ptr(), self.dy[:B].data_ptr(), n, o[3 * B:].data_ptr(),
                                                    tick, self.loss_ws.data_ptr(), self.loss_ws.numel(), st), "clica_dot_loss_bwd_sym_train")
        self.handoff.ticked = self.early_tick

    def _loss_state(self):
        return ops.lp_loss_train_state_export(self.desc, self.loss_ws) if (self.loss_train and not self.dot) else None

    def _load_loss_state(self, blob):
        if self.loss_train and not self.dot:
            ops.lp_loss_train_state_import(self.desc, self.loss_ws, blob)


    def loss_spread(self) -> float:
        """M = log2(e)/tau max_i |y_i - y_0|^2 of the largest embedding cloud the p = 2 matrix-core loss sweeps have seen in this
        trainer (0 on the VALU sweeps): their logit error scales with it (include/clica.h).  Host read + sync -- for
        log points, not for the step."""
        if not self.loss_train or self.dot:        # (p = 0: the dot sweeps need no spread guard)
            return 0.0
        v = C.c_float(0.0)
        _lib.check(_lib.load().clica_lp_loss_train_spread(C.byref(self.desc), self.loss_ws.data_ptr(), self.loss_ws.numel(), C.byref(v),
                                                          _lib.stream_ptr()), "clica_lp_loss_train_spread")
        return float(v.value)

    def loss_guard(self) -> dict:
        """State of the device-side guard of the p = 2 matrix-core loss sweeps (include/clica.h, "THE GUARD"): the largest spread M seen, the
        last step's M, the limit in force and how many steps fell back to the coordinate-difference sweeps.  The decision itself is made
        per step by the kernels (also inside graph replays); this is a host read + sync for log points."""
        if not self.loss_train or self.dot:        # (p = 0: the logits need no guard)
            return dict(max_spread=0.0, last_spread=0.0, limit=0.0, fallback_steps=0)
        v = (C.c_float * 4)()
        _lib.check(_lib.load().clica_lp_loss_train_guard(C.byref(self.desc), self.loss_ws.data_ptr(), self.loss_ws.numel(), v,
                                                         _lib.stream_ptr()), "clica_lp_loss_train_guard")
        return dict(max_spread=float(v[0]), last_spread=float(v[1]), limit=float(v[2]), fallback_steps=int(v[3]))

    def set_loss_matrix_cores(self, on):
        """Switch the p = 2 loss sweeps between the matrix cores for every pool (True) and the coordinate-difference sweeps (False); None = back
        to the default policy (matrix cores only against a pool of >= 4 x the local rows: include/clica.h).  Process-wide (clica_lp_loss_set_matrix_cores); a captured step graph is captured again."""
        _lib.check(_lib.load().clica_lp_loss_set_matrix_cores(-1 if on is None else (2 if on else 0)), "clica_lp_loss_set_matrix_cores")
        if self.graph is not None:
            self.graph = None
            self.capture()

    def plan_summary(self) -> dict:
        """What this rank has planned for its data-parallel step: pool size, workspaces, weight-gradient halves, gradient buckets,
        collectives per step.  bench.py prints it (`ranks` / `dry_ranks`), the dry-run tests assert it."""
        B, n = self.B, self.n
        ranks = self.world * self.dry_ranks
        coll = []
        if self.dp:
            coll.append(dict(op="all_gather", what="embeddings z1_rec", bytes_per_rank=4 * B * n, gathered_bytes=4 * B * n * ranks))
            coll.append(dict(op="all_gather", what="row log-sum-exp", bytes_per_rank=4 * B, gathered_bytes=4 * B * ranks))
            for lo, hi in (self.buckets.buckets if self.buckets is not None else []):
                coll.append(dict(op="all_reduce", what="gradient arena [%d, %d)" % (lo, hi), bytes=4 * (hi - lo)))
        return dict(world=self.world, dry_ranks=self.dry_ranks, planned_ranks=ranks, batch_per_rank=B, pool_rows=int(self.desc.B3),
                    loss_workspace_bytes=int(self.loss_ws.numel()), loss_entry_points=("dot train pair" if self.dot else "train pair") if self.loss_train else "generic",
                    wgrad_halves=bool(self.wgrad_halves), wgrad_group_workspace_bytes=int(self.group_ws.numel()) if self.group_ws is not None else 0,
                    gradient_buckets=[list(b) for b in (self.buckets.buckets if self.buckets is not None else [])],
                    gradient_arena_elements=int(self.grad_arena.numel()), grad_scale=1.0 / ranks, collectives_per_step=coll,
                    encoder_path=self.encoder_plan.path, split_bf16=self.split_bf16,
                    graph_captured=self.graph is not None)



class SupervisedTrainer(_FusedTrainer):
    """Fused, HBM-resident step of the SUPERVISED phase of main_mlp.py (the first of the default ``test_list = [True, False]``,
    :249-255): ``F.mse_loss(f(g(z1)), z1)`` (:274-276), backward, Adam -- no autograd, no host sync.

    The contrastive step's machinery on the B rows of z1 only (the reference also evaluates h(z2) and never reads it: not computed
    here): the same sampler launch (merged with the weight pack in f16x2), the mixing net in the forward's prologue, the whole-stack
    forward, the backward chain with its tail, the weight gradients with Adam folded in, the f16x2 scales and their guard, capture.
    The objective is row-local, dY = 2 (y - z1) / (B n): where the chain runs with its tail on dY (whole-stack split path, no output
    head) the chain's prologue forms dY and the loss itself (clica_mse_target), otherwise one launch of clica_mse_loss_fwd_bwd sits
    between the forward (and head) and the backward.  Either launch advances the step / RNG counter, as the loss backward does in
    the contrastive step.  One rank only."""

    # test hook (class attribute, tests/test_gpu_supervised.py): the chain's prologue forms dY (False: the stand-alone launch)
    fold_mse = True
    _kind = "supervised"

    def __init__(self, f: nn.Sequential, g_weights: torch.Tensor, sampler: SamplerSpec, batch_size: int, lr: float = 1e-4, **engine):
        world = dist.get_world_size(engine.get("process_group")) if dist.is_initialized() else 1
        if world > 1 or engine.get("force_collectives") or max(int(engine.get(k, 1)) for k in ("dry_ranks", "emulate_pool_ranks")) > 1:
            raise NotImplementedError("SupervisedTrainer runs on one rank: data parallelism of the supervised step is not implemented "
                                      "(train_mlp runs that phase through autograd_train_step when world > 1)")
        super().__init__(f, g_weights, sampler, batch_size, lr=lr, **engine)

    def _enc_rows(self) -> int:
        return self.B

    def _allocate_loss(self, R):
        f32 = dict(dtype=torch.float32, device=self.device)
        self.dy = torch.empty((R, self.n), **f32)
        self.loss_out = torch.zeros(1, **f32)
        self.loss_ws = ops.mse_loss_workspace(R, self.n, self.device)     # arrival counter + partials (zero between launches)
        self.early_tick = True           # the objective's launch (or the chain's prologue) advances the step / RNG counter

    def _objective_folds(self, on_dy: bool):
        return False, on_dy and self.fold_mse

    def inject(self, z1: torch.Tensor, z2: Optional[torch.Tensor] = None):
        """Use caller-provided latents z1 (parity tests); `z2` is accepted for symmetry with the contrastive step and not used."""
        self.z[:self.B].copy_(z1)
        self._mix()

    def _result(self) -> torch.Tensor:
        return self.loss_out

    def loss_forward_backward(self):
        """loss = mean((y - z1)^2), dY = 2 (y - z1) / (B n): left to the backward chain's prologue, or one launch here."""
        target, h = self.z[:self.B], self.handoff
        tick = self.step_dev if self.early_tick else None
        h.mse = None
        if h.in_step and self.plan.mse_in_chain:
            h.mse = dict(y=self.y, target=target, loss_out=self.loss_out, ws=self.loss_ws, tick=tick)
            self._mse_taken += 1
        else:
            ops.mse_loss_fwd_bwd(self.y, target, dy=self.dy, loss_out=self.loss_out, ws=self.loss_ws, tick_counter=tick)
        h.ticked = self.early_tick

    def loss_spread(self) -> float:
        """(train_mlp asks every trainer at its log points: the MSE objective has no spread guard)"""
        return 0.0

    def plan_summary(self) -> dict:
        return dict(world=1, batch_per_rank=self.B, encoder_rows=self._enc_rows(), objective="mse",
                    encoder_path=self.encoder_plan.path, split_bf16=self.split_bf16,
                    graph_captured=self.graph is not None)
