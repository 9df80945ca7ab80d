"""ResNet-18 in plain ``torch.nn`` with torchvision's module names.

The 3DIdent driver builds its encoder as ``torchvision.models.resnet18(False, num_classes=10 * n_latents)``
(/root/reference/main_3dident.py:287-292, 365-370).  torchvision is not part of the MI355X image, so ``threedident.setup_f`` falls
back to this module when the import fails: the same architecture (7x7 stem, max-pool, four stages of two basic blocks, global
average pool, fc) and the same attribute names -- ``conv1, bn1, layer1..4[.i].{conv1,bn1,conv2,bn2,downsample.{0,1}}, fc`` -- so a
state dict written by torchvision's model loads here and vice versa.  The convolutions run on PyTorch-ROCm / MIOpen, as BASELINE
config 4 prescribes ("conv path via PyTorch-ROCm + HIP loss").

Everything between the convolutions -- BatchNorm2d, the shortcut add, the ReLU -- is one call of the fused kernels of csrc/bn2d.hip per
unit (``bn1 + relu``, ``bn2 (+ shortcut) + relu``, ``downsample[1]``) whenever ``_bn2d_on_hip`` holds: NORM_MODE "hip", a contiguous
(NCHW) fp32 CUDA input, an affine module that tracks running statistics with a momentum, in training or in inference outside autograd.
Anything else -- channels-last inputs among it, by default -- runs the modules' own forward and torch's ``relu`` / ``+``.  The modules
stay plain ``nn.BatchNorm2d`` objects that own weight, bias, running_mean, running_var and num_batches_tracked: the state dict does not
change.

With POOL_MODE "hip" (and NORM_MODE "hip") the two pools run on csrc/pool2d.hip as well: the stem's ``bn1 + relu + maxpool`` is one
unit that never writes the 32 x 32 activation, pooling indices or their sparse gradient (``_stem_pool_on_hip``: a plain
``nn.MaxPool2d(3, 2, 1)`` and a plane within the kernels' limit), and ``avgpool + flatten`` is one launch (``_avgpool_on_hip``).

With NHWC_MODE "hip" (and NORM_MODE "hip") a dense channels-last input -- ``model.to(memory_format=torch.channels_last)`` -- takes the
same units on the kernels of csrc/bn2d_nhwc.hip, whose outputs and gradients are channels-last again, so the backbone stays NHWC between
MIOpen's convolutions; the average pool follows under POOL_MODE "hip".  A residual in the other layout runs torch's path (no hidden
copy).  The default is "torch": channels-last inputs run the modules' own forward, as they always did.

The channels-last stem is the unit followed by ``nn.MaxPool2d`` unless NHWC_STEM_MODE is "hip" (with NORM_MODE, POOL_MODE and NHWC_MODE
all "hip"): then ``bn1 + relu + maxpool`` is the fused stem unit of csrc/bn2d_nhwc.hip, which tiles the plane instead of holding it in
LDS and, as the NCHW one, writes neither the activation nor indices.  Its default is "torch".

With BF16_MODE "hip" (and NHWC_MODE "hip") the channels-last units, the fused stem (under NHWC_STEM_MODE and POOL_MODE "hip") and the
average pool also take bf16 activations -- what ``torch.autocast("cuda", dtype=torch.bfloat16)`` makes of the convolutions' outputs -- on
the ``_bf16`` entry points of csrc/bn2d_nhwc.hip: bf16 in and out, fp32 parameters, statistics and parameter gradients.  The pooled
features are fp32 and ``fc`` then runs outside autocast, so everything behind the backbone is fp32.  Its default is "torch": bf16
inputs run the modules' own forward, as they always did.  NCHW bf16 inputs do so in either mode.

Both layouts share the code here: ``_layout(x)`` names the layout once per unit, and ``_unit``, ``_stem``, ``_BN2dActFn``,
``_BN2dActPoolFn`` and ``_GlobalAvgPoolFn`` take it as an argument that picks the ``ops`` function (``name`` or ``name_nhwc``) and the
memory format of the incoming gradient.
"""
from __future__ import annotations

import os

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import ops

__all__ = ["resnet18", "ResNet18", "BasicBlock"]

# "hip": the fused kernels where they apply; "torch": the modules' own forward everywhere (the A/B leg).  Read at call time.
NORM_MODE = os.environ.get("CLICA_RESNET_NORM", "hip")
if NORM_MODE not in ("hip", "torch"):
    raise ValueError(f"CLICA_RESNET_NORM={NORM_MODE!r} (one of 'hip', 'torch')")

# "hip": the stem's max-pool inside its bn2d unit and the global average pool on csrc/pool2d.hip, where NORM_MODE is "hip" and they
# apply; "torch": nn.MaxPool2d / nn.AdaptiveAvgPool2d as before (the A/B leg).  Read at call time.
POOL_MODE = os.environ.get("CLICA_RESNET_POOL", "hip")
if POOL_MODE not in ("hip", "torch"):
    raise ValueError(f"CLICA_RESNET_POOL={POOL_MODE!r} (one of 'hip', 'torch')")

# "hip": dense channels-last inputs take the bn2d units (and, under POOL_MODE "hip", the average pool) on csrc/bn2d_nhwc.hip where
# NORM_MODE is "hip"; "torch": they run the modules' own forward, as before.  Read at call time.
NHWC_MODE = os.environ.get("CLICA_RESNET_NHWC", "torch")
if NHWC_MODE not in ("hip", "torch"):
    raise ValueError(f"CLICA_RESNET_NHWC={NHWC_MODE!r} (one of 'hip', 'torch')")

# "hip": a channels-last stem runs bn1 + relu + maxpool as the fused unit of csrc/bn2d_nhwc.hip, where NORM_MODE, POOL_MODE and NHWC_MODE
# are all "hip" and it applies; "torch": the bn2d unit followed by nn.MaxPool2d, as before.  Read at call time.
NHWC_STEM_MODE = os.environ.get("CLICA_RESNET_NHWC_STEM", "torch")
if NHWC_STEM_MODE not in ("hip", "torch"):
    raise ValueError(f"CLICA_RESNET_NHWC_STEM={NHWC_STEM_MODE!r} (one of 'hip', 'torch')")

# "hip": dense channels-last bf16 inputs (autocast's) take the units and pools on the bf16 instances of csrc/bn2d_nhwc.hip where
# NHWC_MODE -- and for the fused stem NHWC_STEM_MODE and POOL_MODE -- are "hip"; "torch": they run the modules' own forward, as before.
# Read at call time.
BF16_MODE = os.environ.get("CLICA_RESNET_BF16", "torch")
if BF16_MODE not in ("hip", "torch"):
    raise ValueError(f"CLICA_RESNET_BF16={BF16_MODE!r} (one of 'hip', 'torch')")

_NHWC = torch.channels_last
# A layout ("nchw" / "nhwc", what _layout gives) picks the memory format of a gradient and the ops function of a name, looked up on the
# module at call time.
_FORMAT = {"nchw": torch.contiguous_format, "nhwc": _NHWC}


def _op(name, layout):
    return getattr(ops, name if layout == "nchw" else name + "_nhwc")


def _grad_like(g, out, layout):
    """The incoming gradient in the unit's layout and in its output's element type (autograd hands a bf16 output a bf16 gradient; one
    that arrives in fp32 is cast)."""
    return g.to(out.dtype).contiguous(memory_format=_FORMAT[layout])


class _BN2dActFn(torch.autograd.Function):
    """nn.BatchNorm2d in training mode + the shortcut add + the ReLU behind it (slope = 1: none) on clica_bn2d_act_fwd_train / _bwd or,
    for `layout` "nhwc" (dense channels-last x and r; output and input gradients channels-last again), on clica_bn2d_nhwc_act_fwd_train /
    _bwd.  `mod` is the module itself: its running statistics are updated in place by the forward's second launch, as its own forward does."""

    @staticmethod
    def forward(ctx, x, r, weight, bias, mod, slope, layout):
        y, save_mean, save_invstd = _op("batchnorm2d_act_fwd", layout)(x, weight, bias, mod.running_mean, mod.running_var, mod.eps,
                                                                       mod.momentum, slope, residual=r)
        ctx.save_for_backward(x, y, weight, save_mean, save_invstd)
        ctx.slope, ctx.layout = slope, layout
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, y, weight, save_mean, save_invstd = ctx.saved_tensors
        dx, dr, dw, db = _op("batchnorm2d_act_bwd", ctx.layout)(x, y, _grad_like(gy, y, ctx.layout), weight, save_mean, save_invstd, ctx.slope,
                                                                need_dr=ctx.needs_input_grad[1])
        return dx, dr, dw, db, None, None, None


class _BN2dActPoolFn(torch.autograd.Function):
    """The stem: nn.BatchNorm2d in training mode + ReLU + nn.MaxPool2d(3, 2, 1) on clica_bn2d_act_maxpool_fwd_train / _bwd or, for `layout`
    "nhwc" (a dense channels-last x; output and input gradient channels-last again), on clica_bn2d_nhwc_act_maxpool_fwd_train / _bwd.  The
    backward recomputes the activation from x, so nothing of its size is saved but x itself."""

    @staticmethod
    def forward(ctx, x, weight, bias, mod, slope, layout):
        p, save_mean, save_invstd = _op("batchnorm2d_act_maxpool_fwd", layout)(x, weight, bias, mod.running_mean, mod.running_var, mod.eps,
                                                                               mod.momentum, slope)
        ctx.save_for_backward(x, weight, bias, save_mean, save_invstd)
        ctx.slope, ctx.layout = slope, layout
        return p

    @staticmethod
    @once_differentiable
    def backward(ctx, gp):
        x, weight, bias, save_mean, save_invstd = ctx.saved_tensors
        dx, dw, db = _op("batchnorm2d_act_maxpool_bwd", ctx.layout)(x, _grad_like(gp, x, ctx.layout), weight, bias, save_mean, save_invstd,
                                                                    ctx.slope)
        return dx, dw, db, None, None, None


class _GlobalAvgPoolFn(torch.autograd.Function):
    """flatten(nn.AdaptiveAvgPool2d(1)(x), 1) on clica_avgpool2d_global_fwd / _bwd or, for `layout` "nhwc" (a dense channels-last x), on
    clica_avgpool2d_global_nhwc_fwd / _bwd.  The output and its gradient are matrices in both."""

    @staticmethod
    def forward(ctx, x, layout):
        ctx.hw, ctx.layout, ctx.dtype = (x.shape[2], x.shape[3]), layout, x.dtype
        return _op("avgpool2d_global_fwd", layout)(x)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        if ctx.dtype == torch.float32:
            return _op("avgpool2d_global_bwd", ctx.layout)(gy.contiguous(), *ctx.hw), None
        return _op("avgpool2d_global_bwd", ctx.layout)(gy.float().contiguous(), *ctx.hw, ctx.dtype), None      # (fp32 [N, C] in, bf16 out)


def _layout(x):
    """"nchw" for a contiguous tensor (those with C = 1 or H = W = 1, the same memory in both layouts, among them), "nhwc" for any other
    dense channels-last tensor when NHWC_MODE is "hip", else None: not the kernels' input."""
    if x.dtype == torch.bfloat16 and BF16_MODE == "hip" and NHWC_MODE == "hip" and x.numel() > 0 and x.is_contiguous(memory_format=_NHWC):
        return "nhwc"                                       # (1 x 1 planes too: the bf16 kernels are channels-last only)
    if x.is_contiguous():
        return "nchw"
    if NHWC_MODE == "hip" and x.numel() > 0 and x.is_contiguous(memory_format=_NHWC):
        return "nhwc"
    return None


def _same_layout(r, layout) -> bool:
    return r.is_contiguous() if layout == "nchw" else r.is_contiguous(memory_format=_NHWC)


def _act_dtype_on_hip(x, layout) -> bool:
    """fp32 in either layout; bf16 channels-last under BF16_MODE "hip" (layout "nhwc" already says NHWC_MODE "hip")."""
    return x.dtype == torch.float32 or (x.dtype == torch.bfloat16 and BF16_MODE == "hip" and layout == "nhwc")


def _bn2d_on_hip(m, x, layout, r=None) -> bool:
    """Do the bn2d kernels cover this module on this input of `layout` (= _layout(x)) and residual?  Anything else runs the module's own
    forward, as before."""
    if NORM_MODE != "hip" or not x.is_cuda or not _act_dtype_on_hip(x, layout) or x.dim() != 4 or layout is None:
        return False
    if r is not None and not (r.is_cuda and r.dtype == x.dtype and r.shape == x.shape and _same_layout(r, layout)):
        return False
    if not (isinstance(m, nn.BatchNorm2d) and m.affine and m.track_running_stats and m.momentum is not None and x.shape[1] == m.num_features):
        return False
    if m.training:
        if x.shape[0] * x.shape[2] * x.shape[3] < 2:        # (the module's own error to raise)
            return False
    elif torch.is_grad_enabled():                           # inference inside autograd: the module's own forward
        return False
    return m.weight.is_cuda and m.weight.dtype == torch.float32


def _unit(bn, relu, x, r=None):
    """relu(bn(x) + r) -- `relu` None: no activation, `r` None: no shortcut -- as one fused call where the kernels apply."""
    layout = _layout(x)
    if not _bn2d_on_hip(bn, x, layout, r):
        y = bn(x)
        if r is not None:
            y = y + r
        return y if relu is None else relu(y)
    slope = 1.0 if relu is None else 0.0
    if bn.training:
        N, C, H, W = x.shape
        if layout == "nchw":                                # (raises while capturing without a warm-up: before anything is counted)
            ops.bn2d_workspace(N, C, H * W, x.device)
        else:
            ops.bn2d_nhwc_workspace(N * H * W, C, x.device)
        bn.num_batches_tracked.add_(1)                      # in place on the device: capturable
        return _BN2dActFn.apply(x, r, bn.weight, bn.bias, bn, slope, layout)
    return _op("batchnorm2d_act_eval", layout)(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, float(bn.eps), slope, residual=r)


def _stem_pool_on_hip(bn, pool, x) -> bool:
    """Does the fused stem unit cover bn + relu + `pool` on this input?  Otherwise: the unfused unit, then the module."""
    layout = _layout(x)
    if POOL_MODE != "hip" or (layout == "nhwc" and NHWC_STEM_MODE != "hip") or not _bn2d_on_hip(bn, x, layout):
        return False
    one = lambda v, k: v == k or v == (k, k)
    if not (type(pool) is nn.MaxPool2d and one(pool.kernel_size, 3) and one(pool.stride, 2) and one(pool.padding, 1) and one(pool.dilation, 1)
            and not pool.ceil_mode and not pool.return_indices):
        return False
    if layout == "nhwc":
        return ops.bn2d_nhwc_maxpool_fits(x.shape[2], x.shape[3], x.shape[1])
    return ops.bn2d_maxpool_fits(x.shape[2], x.shape[3])


def _stem(bn, relu, pool, x):
    """pool(relu(bn(x))) as one fused call where the kernels apply."""
    if not _stem_pool_on_hip(bn, pool, x):
        return pool(_unit(bn, relu, x))
    layout = _layout(x)
    if bn.training:
        workspace = ops.bn2d_maxpool_workspace if layout == "nchw" else ops.bn2d_nhwc_maxpool_workspace
        workspace(x.shape[0], x.shape[1], x.shape[2], x.shape[3], x.device)      # (raises while capturing without a warm-up)
        bn.num_batches_tracked.add_(1)
        return _BN2dActPoolFn.apply(x, bn.weight, bn.bias, bn, 0.0, layout)
    return _op("batchnorm2d_act_maxpool_eval", layout)(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, float(bn.eps), 0.0)


def _avgpool_on_hip(pool, x) -> bool:
    if POOL_MODE != "hip" or NORM_MODE != "hip":
        return False
    if not (x.is_cuda and x.dim() == 4 and _layout(x) is not None and _act_dtype_on_hip(x, _layout(x)) and x.numel() > 0):
        return False
    return type(pool) is nn.AdaptiveAvgPool2d and pool.output_size in (1, (1, 1)) and x.shape[2] * x.shape[3] <= ops.AVGPOOL_MAX_HW


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes: int, planes: int, stride: int = 1):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = None
        if stride != 1 or inplanes != planes:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes, 1, stride, bias=False), nn.BatchNorm2d(planes))

    def forward(self, x):
        if NORM_MODE != "hip":
            y = self.relu(self.bn1(self.conv1(x)))
            y = self.bn2(self.conv2(y))
            return self.relu(y + (x if self.downsample is None else self.downsample(x)))
        y = _unit(self.bn1, self.relu, self.conv1(x))
        identity = x if self.downsample is None else _unit(self.downsample[1], None, self.downsample[0](x))
        return _unit(self.bn2, self.relu, self.conv2(y), identity)


class ResNet18(nn.Module):
    def __init__(self, num_classes: int = 1000):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = nn.Sequential(BasicBlock(64, 64, 1), BasicBlock(64, 64, 1))
        self.layer2 = nn.Sequential(BasicBlock(64, 128, 2), BasicBlock(128, 128, 1))
        self.layer3 = nn.Sequential(BasicBlock(128, 256, 2), BasicBlock(256, 256, 1))
        self.layer4 = nn.Sequential(BasicBlock(256, 512, 2), BasicBlock(512, 512, 1))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512, num_classes)
        for m in self.modules():                      # torchvision's initialisation (models/resnet.py)
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def forward(self, x):
        if NORM_MODE != "hip":
            x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        else:
            x = _stem(self.bn1, self.relu, self.maxpool, self.conv1(x))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        if _avgpool_on_hip(self.avgpool, x):
            feats = _GlobalAvgPoolFn.apply(x, _layout(x))
            if x.dtype == torch.bfloat16:                 # fp32 features of the bf16 pool: the head stays fp32 inside an autocast region
                with torch.autocast("cuda", enabled=False):
                    return self.fc(feats)
            return self.fc(feats)
        return self.fc(torch.flatten(self.avgpool(x), 1))


def resnet18(pretrained: bool = False, num_classes: int = 1000, **_unused) -> ResNet18:
    """Call-compatible with ``torchvision.models.resnet18(pretrained, num_classes=...)`` as the reference uses it (weights are never
    downloaded here: ``pretrained=True`` raises)."""
    if pretrained:
        raise ValueError("no pretrained weights in this image (the reference trains from scratch: main_3dident.py:365 passes False)")
    return ResNet18(num_classes)
