"""3DIdent experiment: encoder head, loss selection and ``train_step`` of /root/reference/main_3dident.py on the HIP path.

What runs where (BASELINE.json configs[3]: "ResNet-18 encoder ... conv path via PyTorch-ROCm + HIP loss"):
  * the backbone (``torchvision.models.resnet*`` in the reference, :287-292) is ANY ``nn.Module`` mapping images to
    ``(B, 10 * n_latents)`` features and stays on PyTorch-ROCm / MIOpen -- torchvision is not part of this image, so
    ``setup_f`` takes the backbone constructor as an argument and only falls back to torchvision when it is importable;
  * everything behind it is HIP: ``LeakyReLU`` (``clica_leaky_relu_*``), ``Linear(10 n_lat -> n_lat)``
    (``clica_linear_*``), the rescaling layer (``clica_rescale_*`` / ``clica_softclip_*``), the losses on column slices
    ``z[:, :k]`` (strided views, no copies) and -- optionally -- Adam (``cl_ica_amd.optim.Adam``).

Both halves of the driver are mirrored: ``make_unsupervised_loss`` / ``train_step`` (``train_unsupervised``) and
``make_supervised_loss`` / ``train_step_supervised`` (``train_supervised``, the driver's default ``--mode``).

``setup_f`` reproduces the module layout of :365-371 (``nn.Sequential(backbone, LeakyReLU, Linear, rescaling)``), i.e.
the reference's state-dict keys ``0.*`` (backbone), ``2.weight``, ``2.bias``, ``3.r`` / ``3.max_abs_bound``.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch
from torch import nn

from . import _lib, encoders, layers, lazy, losses, ops, optim, spaces
from .encoders import _MLPStackFn

__all__ = ["setup_f", "make_unsupervised_loss", "train_step", "HipLinear", "unpack_item_list", "make_supervised_loss",
           "train_step_supervised", "batch_format", "clocked_iteration", "capture_iteration", "CapturedIteration"]


class HipLinear(nn.Linear):
    """``nn.Linear`` (same parameters / state-dict entries / default init) computed by the HIP GEMM kernels."""

    def forward(self, x):
        x = lazy.plain(x)
        return _MLPStackFn.apply(x if x.is_contiguous() else x.contiguous(), 0.0, self.weight, self.bias)


def _identity(x):
    return x


def make_rescaling(args, n_non_angular_latents: int, n_angular_latents: int) -> nn.Module:
    """The ``rescaling`` module of ``setup_f`` (main_3dident.py:311-345) for the given mode flags."""
    periodic_rescale_layer = layers.RescaleLayer(fixed_r=False, mode="eq")
    if getattr(args, "box_constraint", None) is not None:
        non_periodic_rescale_layer = layers.SoftclipLayer(n=n_non_angular_latents, fixed_abs_bound=args.box_constraint == "fix")
    elif getattr(args, "sphere_constraint", None) is not None:
        non_periodic_rescale_layer = layers.RescaleLayer(fixed_r=args.sphere_constraint == "fix", mode="eq")
    else:
        non_periodic_rescale_layer = layers.Lambda(_identity)
    np_rc = getattr(args, "non_periodic_rotation_and_color", False)
    if getattr(args, "position_only", False):
        return non_periodic_rescale_layer
    if getattr(args, "rotation_and_color_only", False) or getattr(args, "rotation_only", False) or getattr(args, "color_only", False):
        return non_periodic_rescale_layer if np_rc else periodic_rescale_layer
    if np_rc:
        return non_periodic_rescale_layer
    k = n_non_angular_latents
    return layers.Lambda(lambda x: torch.cat((non_periodic_rescale_layer(x[:, :k]), periodic_rescale_layer(x[:, k:])), dim=1))


def setup_f(args, n_non_angular_latents: int, n_angular_latents: int,
            base_encoder: Optional[Callable[..., nn.Module]] = None) -> nn.Module:
    """``nn.Sequential(backbone(num_classes=10 n_lat), LeakyReLU, Linear(10 n_lat, n_lat), rescaling)`` (:365-370).
    ``base_encoder(pretrained, num_classes=...)`` builds the backbone; default: ``torchvision.models.<args.encoder>``."""
    if getattr(args, "identity_solution", False):
        return nn.Sequential(layers.Flatten())
    n_latents = n_non_angular_latents + n_angular_latents
    rescaling = make_rescaling(args, n_non_angular_latents, n_angular_latents)
    if getattr(args, "dummy_mixing", False):      # the encoder of main_mlp on the mixed latents instead of a backbone on images (:348-364)
        n = n_latents
        return nn.Sequential(encoders.get_mlp(n_in=n, n_out=n, layers=[n * 10, n * 50, n * 50, n * 50, n * 50, n * 10],
                                              output_normalization=None), rescaling)
    if base_encoder is None:
        try:
            from torchvision import models       # not in this image; present in the reference's environment
            base_encoder = {"rn18": models.resnet18, "rn50": models.resnet50, "rn101": models.resnet101,
                            "rn152": models.resnet152}[args.encoder]
        except ImportError as e:
            if getattr(args, "encoder", "rn18") != "rn18":
                raise ImportError("torchvision is not installed: pass base_encoder=<callable building the backbone> "
                                  "(only the default rn18 has a stand-in, cl_ica_amd/resnet.py)") from e
            from .resnet import resnet18 as base_encoder      # same architecture and state-dict keys as torchvision's
    return nn.Sequential(base_encoder(False, num_classes=n_latents * 10), layers.LeakyReLU(),
                         HipLinear(n_latents * 10, n_latents), rescaling)


def make_unsupervised_loss(args, n_non_angular_latents: int):
    """Loss selection of ``train_unsupervised`` (main_3dident.py:402-445)."""
    spherical_loss = losses.SimCLRLoss(normalize=False, tau=1.0)
    kind = getattr(args, "unsupervised_loss", "l2")
    if kind in ("l1", "l2", "l3"):
        nonspherical_loss = losses.LpSimCLRLoss(p=int(kind[1]), tau=1.0, simclr_compatibility_mode=True, pow=True)
    elif kind == "vmf":
        nonspherical_loss = losses.SimCLRLoss(normalize=True, tau=1.0)
    else:
        raise ValueError(f"unsupervised_loss {kind!r}")
    k = n_non_angular_latents

    def loss(z1, z2_con_z1, z3, z1_rec, z2_con_z1_rec, z3_rec):
        # the combined objective; the reference slices z3_rec at a hard-coded 3 (:431,439)
        nsl = nonspherical_loss(z1, z2_con_z1, z3, z1_rec[:, :k], z2_con_z1_rec[:, :k], z3_rec[:, :3])
        sl = spherical_loss(z1, z2_con_z1, z3, z1_rec[:, k:], z2_con_z1_rec[:, k:], z3_rec[:, 3:])
        return sl[0] + nsl[0], [(sl[0], sl[1])] + [(nsl[0], nsl[1])]

    if getattr(args, "position_only", False):
        loss = nonspherical_loss
    elif getattr(args, "rotation_and_color_only", False) or getattr(args, "rotation_only", False) or getattr(args, "color_only", False):
        loss = spherical_loss
    if getattr(args, "non_periodic_rotation_and_color", False):
        loss = nonspherical_loss
    return loss


def unpack_item_list(lst):
    if isinstance(lst, tuple):
        lst = list(lst)
    return [unpack_item_list(it) if isinstance(it, (tuple, list)) else it.item() for it in lst]


AMP_MODES = (None, "bf16")


def encode(f, x, amp=None):
    """``f(x)``; with ``amp="bf16"`` under ``torch.autocast("cuda", dtype=torch.bfloat16)``: the backbone's convolutions run in bf16 (and,
    with resnet.BF16_MODE "hip", the units between them on the bf16 kernels), its head and everything behind it in fp32.  No loss
    scaling: bf16 has fp32's exponent range."""
    if amp is None:
        return f(x)
    if amp != "bf16":
        raise ValueError(f"amp={amp!r} (one of {AMP_MODES})")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        return f(x)


def train_step(data, loss, optimizer, f, sync: bool = True, amp=None):
    """One unsupervised step (main_3dident.py:467-503): two encoder passes, ``z3_rec = roll(z1_rec)`` inside the graph,
    the loss with ``None`` latents, backward, optimizer step.  Returns ``(total, per_item, [pos_mean, neg_mean])`` as python
    floats like the reference when ``sync`` (3 host syncs), device tensors otherwise.  ``amp``: see ``encode`` (the encoder passes
    only; the loss and the optimizer stay fp32)."""
    (_z1, _z2), (x1, x2_con_x1) = data
    optimizer.zero_grad()
    z1_rec = encode(f, x1, amp)
    z2_con_z1_rec = encode(f, x2_con_x1, amp)
    del x1, x2_con_x1
    z3_rec = torch.roll(z1_rec, 1, 0)
    total_loss_value, total_loss_per_item_value, losses_value = loss(None, None, None, z1_rec, z2_con_z1_rec, z3_rec)
    total_loss_value.backward()
    if hasattr(optimizer, "all_reduce_grads"):
        optimizer.all_reduce_grads()
    optimizer.step()
    if not sync:
        return total_loss_value, total_loss_per_item_value, losses_value
    return total_loss_value.item(), total_loss_per_item_value, unpack_item_list(losses_value)


class _MSELossFn(torch.autograd.Function):
    """``F.mse_loss(y_pred, y)`` (mean over all elements) on clica_mse_loss_fwd_bwd: the loss and d loss / d y_pred come from ONE launch;
    the backward only scales that gradient by the upstream scalar."""

    @staticmethod
    def forward(ctx, y_pred, y):
        loss, dy = ops.mse_loss_fwd_bwd(y_pred.detach(), y.detach(), ws=_mse_workspace(y_pred.shape[0], y_pred.shape[1], y_pred.device))
        ctx.save_for_backward(dy)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None
        (dy,) = ctx.saved_tensors
        return dy * g, None


_MSE_WS = {}      # (device, M, n) -> zeroed workspace, never replaced or freed (as ops.r2_loss_workspace: a captured graph keeps its pointer)


def _mse_workspace(M: int, n: int, device) -> torch.Tensor:
    key = (device.index if device.index is not None else torch.cuda.current_device(), int(M), int(n))
    ws = _MSE_WS.get(key)
    if ws is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"mse loss: no workspace for shape ({M}, {n}) yet -- run the step once eagerly before capturing it")
        ws = _MSE_WS[key] = ops.mse_loss_workspace(M, n, device)
    _lib.note_graph_use(ws)
    return ws


class HipMSELoss:
    """``torch.nn.MSELoss(reduction="mean")`` for 2-D fp32 device tensors; differentiates with respect to ``y_pred``."""

    reduction = "mean"

    def forward(self, y_pred, y):
        y_pred, y = lazy.plain(y_pred), lazy.plain(y)
        if y_pred.dim() != 2 or y.shape != y_pred.shape:
            raise ValueError(f"shape mismatch: y_pred {tuple(y_pred.shape)}, y {tuple(y.shape)} (2-D, equal shapes)")
        if y.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("the HIP MSE objective differentiates with respect to y_pred only: the target requires grad")
        return _MSELossFn.apply(y_pred, y)

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)


def make_supervised_loss(args):
    """Loss selection of ``train_supervised`` (main_3dident.py:574-577): ``args.supervised_loss`` is "r2" (negative mean R2 score) or
    "mse"; called as ``loss(hz1, z1)``."""
    kind = getattr(args, "supervised_loss", "r2")
    if kind == "r2":
        return losses.R2Loss(reduction="mean", mode="negative_r2")
    if kind == "mse":
        return HipMSELoss()
    raise ValueError(f"supervised_loss {kind!r}")


def train_step_supervised(data, loss, optimizer, f, sync: bool = True, amp=None):
    """One supervised step (main_3dident.py:585-601): one encoder pass on the first view, the loss against its true latents,
    backward, optimizer step.  Returns the loss as a python float like the reference when ``sync`` (one host sync), the device
    scalar otherwise.  ``amp``: see ``encode``."""
    (z1, _), (x1, _) = data
    optimizer.zero_grad()
    hz1 = lazy.plain(encode(f, x1, amp))
    del x1
    total_loss_value = loss(hz1, z1.to(hz1.device))
    total_loss_value.backward()
    if hasattr(optimizer, "all_reduce_grads"):
        optimizer.all_reduce_grads()
    optimizer.step()
    if not sync:
        return total_loss_value
    return total_loss_value.item()


# ------------------------------------------------------------------------------------------------ the iteration as one HIP graph
def batch_format(f, amp=None):
    """``(memory_format, dtype)`` of the image batch the model takes without a copy in front of it: channels-last bf16 under
    ``amp="bf16"`` (what ``conv1`` under autocast computes on), else float32 in the memory format of the model's first 4-D parameter."""
    if amp == "bf16":
        return torch.channels_last, torch.bfloat16
    if amp is not None:
        raise ValueError(f"amp={amp!r} (one of {AMP_MODES})")
    for p in f.parameters():
        if p.dim() == 4:
            if p.is_contiguous(memory_format=torch.channels_last) and not p.is_contiguous():
                return torch.channels_last, torch.float32
            break
    return torch.contiguous_format, torch.float32


def clocked_iteration(dataset, loss, optimizer, f, batch_size: int, clock, *, supervised: bool = False, amp=None, latents=None,
                      images=None):
    """ONE training iteration with its batch drawn under `clock` (``spaces.DeviceClock``): the clocked pair draw, ``snap``, one gather of
    both views, ``train_step`` (``train_step_supervised`` when `supervised`) without host reads, ``clock.tick()``.  `latents`
    ``(z, z~)`` / `images` ``(2 B, C, H, W)``: buffers the batch is written into (the captured iteration's static ones); ``None``: fresh
    tensors in ``batch_format(f, amp)``.  Returns ``((total, per_item, parts), (z, z~), images)``; the supervised step has no per-item
    vector and no parts (``None``).  Every launch is stream-ordered and reads its counters on the device: the call can be captured
    once its workspaces exist."""
    B = int(batch_size)
    memory_format, dtype = batch_format(f, amp)
    with clock.iteration():
        index_z, index_zt, z, zt = dataset.pairs.sample(B)
    if latents is not None:
        latents[0].copy_(z); latents[1].copy_(zt)
        z, zt = latents
    x = dataset.images.gather(torch.cat([index_z, index_zt]), dataset.normalize, images, memory_format=memory_format, dtype=dtype)
    data = ((z, zt), (x[:B], x[B:]))
    if supervised:
        out = (train_step_supervised(data, loss, optimizer, f, sync=False, amp=amp), None, None)
    else:
        out = tuple(train_step(data, loss, optimizer, f, sync=False, amp=amp))
        if len(out) == 2:                  # the combined objective returns (total, parts)
            out = (out[0], None, out[1])
    clock.tick()
    return out, (z, zt), x


def _scale_layers(module):
    """The ``RescaleLayer`` / ``SoftclipLayer`` instances under `module`, those held in the closure of a ``layers.Lambda`` (the
    combined rescaling of ``make_rescaling``) included."""
    for m in module.modules():
        if isinstance(m, (layers.RescaleLayer, layers.SoftclipLayer)):
            yield m
        elif isinstance(m, layers.Lambda):
            for cell in getattr(m.f, "__closure__", None) or ():
                if isinstance(cell.cell_contents, nn.Module):
                    yield from _scale_layers(cell.cell_contents)


def _scales_to_device(f, device) -> None:
    """A fixed radius / bound is a plain host tensor, neither parameter nor buffer (as in the reference), and its layer copies it to the
    device in every forward: a host copy that cannot be recorded.  Put those tensors (and a learnable one held only in a closure) on
    `device` once, ahead of the capture; the layers' ``.to(x.device)`` is then the tensor itself.  State dicts do not hold them."""
    for m in _scale_layers(f):
        name = "r" if isinstance(m, layers.RescaleLayer) else "max_abs_bound"
        t = getattr(m, name)
        if t.device != device:
            if isinstance(t, nn.Parameter):
                t.data = t.data.to(device)
            else:
                setattr(m, name, t.to(device))


class CapturedIteration:
    """What ``capture_iteration`` returns: ``step()`` replays the graph (one launch) and returns ``(total, per_item, parts)``, device
    tensors owned by the graph and rewritten by every replay.  ``latents`` ``(z, z~)`` and ``images`` ``(2 B, C, H, W)`` are the static
    batch of the last replay, ``graph`` the ``torch.cuda.CUDAGraph``, ``clock`` the device clock, ``owned`` the buffers of the package's
    caches that the recorded launches use (kept alive and kept from other owners through ``_lib.pin`` while this object lives)."""

    def __init__(self, graph, result, latents, images, clock, owned):
        self.graph, self.result, self.latents, self.images, self.clock, self.owned = graph, result, latents, images, clock, owned
        self.replays = 0

    def __call__(self):
        self.graph.replay()
        self.replays += 1
        return self.result


def capture_iteration(dataset, loss, optimizer, f, batch_size: int, *, supervised: bool = False, amp=None, warmup: int = 3, clock=None,
                      on_warmup=None):
    """The whole 3DIdent training iteration -- clocked pair draw, ``snap``, image gather, encoder passes, loss, ``backward()``,
    ``all_reduce_grads`` if present, ``optimizer.step()``, ``clock.tick()`` (``clocked_iteration``) -- recorded into ONE HIP graph on
    static buffers; returns ``step`` (``CapturedIteration``).

    `warmup` (at least 1) ordinary eager iterations run first on the capture stream, inside the clock scope, and they TRAIN: the MIOpen
    find step, the growth of the workspaces and the allocations of the graph's pool happen there (the fused units of ``resnet`` raise
    when they are captured without one).  ``on_warmup(result)`` is called after each with its ``(total, per_item, parts)``.  A run of
    ``warmup`` eager iterations followed by replays visits the batch sequence of an all-eager run of ``clocked_iteration`` under the
    same clock: iteration k draws with the counter at k either way.  Fixed radii / bounds of the rescaling layers (plain host
    tensors) are moved to the device first (``_scales_to_device``).  `clock`: default ``spaces.DeviceClock`` seeded with the module-level
    generator's seed.  Capture is on one stream, no forked branches.

    The optimizer must be ``optim.Adam`` or ``optim.SGD`` (flat arenas, step counter on the device); a dataset of ``dummy_images`` has
    no image batch to gather and is refused (``--dummy-mixing`` and ``--identity-mixing-and-solution`` of the driver, whose steps run
    eagerly), and so is a model without parameters (``--identity-solution``).  Evaluation, other batch sizes and other encoders may
    run eagerly between replays: the cache-held buffers of the recorded launches are owned by the returned object."""
    if not isinstance(optimizer, (optim.Adam, optim.SGD)):
        raise TypeError(f"capture_iteration: the optimizer must be cl_ica_amd.optim.Adam or optim.SGD (flat arenas, step counter on the "
                        f"device), got {type(optimizer).__name__}")
    if getattr(dataset, "dummy_images", False) or getattr(dataset, "images", None) is None:
        raise ValueError("capture_iteration: the dataset has no images (dummy_images): there is no image batch to capture")
    if not any(p.requires_grad for p in f.parameters()):
        raise ValueError("capture_iteration: the model has no trainable parameters (identity solution): there is nothing to capture")
    if optimizer.world > 1:
        raise RuntimeError("capture_iteration: the data-parallel step (collectives issued from Python) is not captured")
    if _lib._CAPTURE_NOTES is not None:
        raise RuntimeError("capture_iteration: another capture is in progress")
    device = dataset.device
    B = int(batch_size)
    if clock is None:
        clock = spaces.DeviceClock(spaces._state["seed"], device)
    memory_format, dtype = batch_format(f, amp)
    _scales_to_device(f, device)
    _N, H, W, Cn = dataset.images.shape
    images = torch.empty((2 * B, Cn, H, W), dtype=dtype, device=device, memory_format=memory_format)
    d = dataset.latents.shape[1]
    latents = (torch.empty((B, d), dtype=torch.float32, device=device), torch.empty((B, d), dtype=torch.float32, device=device))
    kw = dict(supervised=supervised, amp=amp, latents=latents, images=images)

    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        for _ in range(max(1, int(warmup))):
            out, _z, _x = clocked_iteration(dataset, loss, optimizer, f, B, clock, **kw)
            if on_warmup is not None:
                on_warmup(out)
    torch.cuda.current_stream(device).wait_stream(side)
    torch.cuda.synchronize(device)

    graph = torch.cuda.CUDAGraph()
    notes = _lib._CAPTURE_NOTES = []
    try:
        with torch.cuda.graph(graph, stream=side):
            result, _z, _x = clocked_iteration(dataset, loss, optimizer, f, B, clock, **kw)
    finally:
        _lib._CAPTURE_NOTES = None
    owned = list({id(t): t for t in notes}.values())
    step = CapturedIteration(graph, result, latents, images, clock, owned)
    _lib.pin(step, owned)
    return step
