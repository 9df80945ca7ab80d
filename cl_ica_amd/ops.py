"""Thin functional wrappers over the C ABI (include/clica.h).  Every function launches HIP
kernels on torch's current stream and returns torch tensors; there is no other code path."""
from __future__ import annotations

import ctypes as C
from typing import Callable, NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._lib import check, load, ptr, require_cuda, rowmajor, stream_ptr, workspace, ClicaError


def _mat(name: str, t: torch.Tensor) -> Tuple[torch.Tensor, int]:
    if t.dim() != 2:
        raise ValueError(f"{name} must be 2-D, got {tuple(t.shape)}")
    require_cuda(t, name)
    return rowmajor(t.detach())


# ------------------------------------------------------------------------------- Linear
def linear_fwd(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], leaky: bool,
               slope: float = 0.01, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Y = act(x W^T + b); act = LeakyReLU(slope) if `leaky` (encoders.py:38-48)."""
    (x, ldx), (w, ldw) = _mat("x", x), _mat("weight", weight)
    M, K = x.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError(f"weight {tuple(w.shape)} does not match input {tuple(x.shape)}")
    if bias is not None:
        require_cuda(bias, "bias")
        bias = bias.detach().contiguous()
    y = out if out is not None else torch.empty((M, N), dtype=torch.float32, device=x.device)
    check(load().clica_linear_fwd(x.data_ptr(), ldx, w.data_ptr(), ldw, ptr(bias), y.data_ptr(), y.stride(0),
                                  M, N, K, int(leaky), float(slope), stream_ptr()), "clica_linear_fwd")
    return y


def linear_dgrad(dy: torch.Tensor, weight: torch.Tensor, xact: Optional[torch.Tensor], slope: float = 0.01,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dX = (dY W) * act'(xact)  (xact = saved activation output feeding this layer, or None)."""
    (dy, lddy), (w, ldw) = _mat("dy", dy), _mat("weight", weight)
    M, N = dy.shape
    K = w.shape[1]
    xa, ldxa = (None, 0)
    if xact is not None:
        xa, ldxa = _mat("xact", xact)
    dx = out if out is not None else torch.empty((M, K), dtype=torch.float32, device=dy.device)
    check(load().clica_linear_dgrad(dy.data_ptr(), lddy, w.data_ptr(), ldw, ptr(xa), ldxa, float(slope),
                                    dx.data_ptr(), dx.stride(0), M, N, K, stream_ptr()), "clica_linear_dgrad")
    return dx


def linear_wgrad(dy: torch.Tensor, x: torch.Tensor, dW: Optional[torch.Tensor] = None,
                 db: Optional[torch.Tensor] = None, accumulate: bool = False, want_bias: bool = True,
                 ws: Optional[torch.Tensor] = None):
    """dW = dY^T X, db = column sums of dY."""
    (dy, lddy), (x, ldx) = _mat("dy", dy), _mat("x", x)
    M, N = dy.shape
    K = x.shape[1]
    if dW is None:
        dW = torch.empty((N, K), dtype=torch.float32, device=dy.device)
    if db is None and want_bias:
        db = torch.empty((N,), dtype=torch.float32, device=dy.device)
    if ws is None:
        nbytes = C.c_size_t()
        check(load().clica_linear_wgrad_workspace_bytes(M, N, K, C.byref(nbytes)), "clica_linear_wgrad_workspace_bytes")
        ws = workspace("wgrad", nbytes.value, dy.device)
    check(load().clica_linear_wgrad(dy.data_ptr(), lddy, x.data_ptr(), ldx, dW.data_ptr(), dW.stride(0), ptr(db),
                                    M, N, K, int(accumulate), ws.data_ptr(), ws.numel(), stream_ptr()),
          "clica_linear_wgrad")
    return dW, db


def mlp_wgrad_workspace(M: int, shapes, device) -> torch.Tensor:
    """Workspace for `mlp_wgrad` over layers with weight shapes `shapes` = [(N_l, K_l), ...]."""
    n = len(shapes)
    I32 = C.c_int32 * n
    nbytes = C.c_size_t()
    check(load().clica_mlp_wgrad_workspace_bytes(int(M), n, I32(*[s[0] for s in shapes]), I32(*[s[1] for s in shapes]), C.byref(nbytes)),
          "clica_mlp_wgrad_workspace_bytes")
    return torch.zeros(nbytes.value, dtype=torch.uint8, device=device)


def mlp_wgrad(dzs, xs, dWs, dbs, ws: Optional[torch.Tensor] = None, accumulate: bool = False):
    """All layers' dW[l] = dZ[l]^T X[l], db[l] = column sums of dZ[l] in two launches (clica_mlp_wgrad)."""
    n = len(dzs)
    dz = [_mat(f"dz[{l}]", t) for l, t in enumerate(dzs)]
    xx = [_mat(f"x[{l}]", t) for l, t in enumerate(xs)]
    M = dz[0][0].shape[0]
    shapes = [(d.shape[1], x.shape[1]) for (d, _), (x, _) in zip(dz, xx)]
    if ws is None:
        ws = mlp_wgrad_workspace(M, shapes, dz[0][0].device)
    VP, I64, I32 = C.c_void_p * n, C.c_int64 * n, C.c_int32 * n
    check(load().clica_mlp_wgrad(M, n, VP(*[d.data_ptr() for d, _ in dz]), I64(*[ld for _, ld in dz]),
                                 VP(*[x.data_ptr() for x, _ in xx]), I64(*[ld for _, ld in xx]),
                                 VP(*[w.data_ptr() for w in dWs]), I64(*[w.stride(0) for w in dWs]),
                                 VP(*[ptr(b) for b in dbs]), I32(*[s[0] for s in shapes]), I32(*[s[1] for s in shapes]),
                                 int(accumulate), ws.data_ptr(), ws.numel(), stream_ptr()), "clica_mlp_wgrad")
    return dWs, dbs


MLP_FUSED_MAX_WIDTH = 512
MLP_FUSED_MAX_LAYERS = 8


def mlp_fwd_fusable(weights) -> bool:
    return len(weights) <= MLP_FUSED_MAX_LAYERS and all(max(w.shape) <= MLP_FUSED_MAX_WIDTH for w in weights)


def mlp_pack_weights(weights, packed: Optional[torch.Tensor] = None, transpose: bool = False) -> torch.Tensor:
    """Weights in MFMA fragment order for `mlp_fwd(..., packed=...)` (clica_mlp_pack), or -- with
    ``transpose`` and the layers given in chain order (last layer first) -- for `mlp_dgrad_chain`.
    Re-run after every parameter update; `packed` is reused when given."""
    L = len(weights)
    ws = [_mat(f"weight[{l}]", w) for l, w in enumerate(weights)]
    I32 = C.c_int32 * L
    Ns, Ks = I32(*[w.shape[0] for w, _ in ws]), I32(*[w.shape[1] for w, _ in ws])
    if packed is None:
        nb = C.c_size_t()
        check(load().clica_mlp_pack_bytes(L, Ns, Ks, int(transpose), C.byref(nb)), "clica_mlp_pack_bytes")
        packed = torch.zeros(nb.value // 4, dtype=torch.float32, device=ws[0][0].device)   # zero padding written once
    check(load().clica_mlp_pack(L, (C.c_void_p * L)(*[w.data_ptr() for w, _ in ws]), (C.c_int64 * L)(*[ld for _, ld in ws]),
                                Ns, Ks, int(transpose), packed.data_ptr(), stream_ptr()), "clica_mlp_pack")
    return packed


def mlp_pack_both(weights, packed: Optional[torch.Tensor] = None, packed_t: Optional[torch.Tensor] = None):
    """Both fragment-order copies a training step needs in ONE launch (clica_mlp_pack_both): `packed` for
    `mlp_fwd` (layers 0..L-1) and `packed_t` for `mlp_dgrad_chain` (layers L-1..1, transposed)."""
    L = len(weights)
    ws = [_mat(f"weight[{l}]", w) for l, w in enumerate(weights)]
    I32 = C.c_int32 * L
    Ns, Ks = I32(*[w.shape[0] for w, _ in ws]), I32(*[w.shape[1] for w, _ in ws])
    dev = ws[0][0].device
    if packed is None:
        nb = C.c_size_t()
        check(load().clica_mlp_pack_bytes(L, Ns, Ks, 0, C.byref(nb)), "clica_mlp_pack_bytes")
        packed = torch.zeros(nb.value // 4, dtype=torch.float32, device=dev)
    if packed_t is None:
        nb = C.c_size_t()
        chain = list(range(L - 1, 0, -1))
        I32c = C.c_int32 * (L - 1)
        check(load().clica_mlp_pack_bytes(L - 1, I32c(*[ws[l][0].shape[0] for l in chain]), I32c(*[ws[l][0].shape[1] for l in chain]), 1,
                                          C.byref(nb)), "clica_mlp_pack_bytes")
        packed_t = torch.zeros(nb.value // 4, dtype=torch.float32, device=dev)
    check(load().clica_mlp_pack_both(L, (C.c_void_p * L)(*[w.data_ptr() for w, _ in ws]), (C.c_int64 * L)(*[ld for _, ld in ws]),
                                     Ns, Ks, packed.data_ptr(), packed_t.data_ptr(), stream_ptr()), "clica_mlp_pack_both")
    return packed, packed_t


# ---- opt-in split-bf16 arithmetic (clica_mlp_*_split): fp32-grade results on the bf16 matrix cores -------------------
def mlp_pack_split_both(weights, packed: Optional[torch.Tensor] = None, packed_t: Optional[torch.Tensor] = None, state=None):
    """Fragment-order piece copies for `mlp_fwd_split` (layers 0..L-1) and `mlp_dgrad_chain_split` (layers L-1..1, transposed) in one
    launch: bf16x3, or -- with a `Split16` state -- f16x2 scaled by the state's weight scales (clica_mlp_pack_split16_both)."""
    L = len(weights)
    ws = [_mat(f"weight[{l}]", w) for l, w in enumerate(weights)]
    I32 = C.c_int32 * L
    Ns, Ks = I32(*[w.shape[0] for w, _ in ws]), I32(*[w.shape[1] for w, _ in ws])
    dev = ws[0][0].device
    nb = C.c_size_t()
    nbytes = load().clica_mlp_pack_split_bytes if state is None else load().clica_mlp_pack_split16_bytes
    if packed is None:
        check(nbytes(L, Ns, Ks, 0, C.byref(nb)), "clica_mlp_pack_split_bytes")
        packed = torch.zeros(nb.value, dtype=torch.uint8, device=dev)
    if packed_t is None:
        chain = list(range(L - 1, 0, -1))
        I32c = C.c_int32 * (L - 1)
        check(nbytes(L - 1, I32c(*[ws[l][0].shape[0] for l in chain]), I32c(*[ws[l][0].shape[1] for l in chain]), 1, C.byref(nb)),
              "clica_mlp_pack_split_bytes")
        packed_t = torch.zeros(nb.value, dtype=torch.uint8, device=dev)
    Wp, ldp = (C.c_void_p * L)(*[w.data_ptr() for w, _ in ws]), (C.c_int64 * L)(*[ld for _, ld in ws])
    if state is None:
        check(load().clica_mlp_pack_split_both(L, Wp, ldp, Ns, Ks, packed.data_ptr(), packed_t.data_ptr(), stream_ptr()), "clica_mlp_pack_split_both")
    else:
        check(load().clica_mlp_pack_split16_both(L, Wp, ldp, Ns, Ks, packed.data_ptr(), packed_t.data_ptr(), state.buf.data_ptr(), stream_ptr()),
              "clica_mlp_pack_split16_both")
    return packed, packed_t


class Split16:
    """Device state of the f16x2 encoder arithmetic of ONE encoder (include/clica.h, "f16x2 arithmetic"): per-tensor scales in force and
    the running maxima the producer kernels record.  `update()` (one tiny launch, once per training step after its last producer) turns
    the maxima into the next step's scales; `read()` synchronises and reports flags / scales (log points, tests)."""

    def __init__(self, n_layers: int, device):
        nb = C.c_size_t()
        check(load().clica_split16_state_bytes(C.byref(nb)), "clica_split16_state_bytes")
        self.n_layers = int(n_layers)
        self.buf = torch.zeros(nb.value, dtype=torch.uint8, device=device)
        check(load().clica_split16_state_init(self.buf.data_ptr(), stream_ptr()), "clica_split16_state_init")

    def update(self):
        check(load().clica_split16_update(self.buf.data_ptr(), self.n_layers, stream_ptr()), "clica_split16_update")

    def clear_flags(self):
        check(load().clica_split16_clear_flags(self.buf.data_ptr(), stream_ptr()), "clica_split16_clear_flags")

    def guard(self) -> dict:
        """State of the device-side guard (include/clica.h, "THE GUARD of the f16x2 arithmetic"): sticky flags, steps withheld so far, scale
        updates so far, and whether the step whose producers ran last is poisoned.  Host read + sync: log points, tests."""
        fl, sk, up, po = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        check(load().clica_split16_guard(self.buf.data_ptr(), C.byref(fl), C.byref(sk), C.byref(up), C.byref(po), stream_ptr()), "clica_split16_guard")
        return dict(flags=int(fl.value), skipped=int(sk.value), updates=int(up.value), poisoned=bool(po.value))

    def set_dp_poison(self, slot: Optional[torch.Tensor]):
        """Data parallel: the optimizer launches take the step's verdict from the device float `slot` (all-reduced by the caller)."""
        check(load().clica_split16_set_dp_poison(self.buf.data_ptr(), ptr(slot), stream_ptr()), "clica_split16_set_dp_poison")
        self._dp_slot = slot

    def poison_export(self, slot: torch.Tensor):
        check(load().clica_split16_poison_export(self.buf.data_ptr(), slot.data_ptr(), stream_ptr()), "clica_split16_poison_export")

    def export_state(self) -> torch.Tensor:
        """The portable part of the state at a step boundary as an opaque device blob (include/clica.h, "CHECKPOINTS": scales, flags,
        generation, the guard's words -- no addresses, no capacities).  One tiny launch, no sync; `import_state` of another `Split16`
        of the same number of layers, in this process or another, takes it."""
        nb = C.c_size_t()
        check(load().clica_split16_export_bytes(C.byref(nb)), "clica_split16_export_bytes")
        blob = torch.zeros(nb.value, dtype=torch.uint8, device=self.buf.device)
        check(load().clica_split16_export(self.buf.data_ptr(), self.n_layers, blob.data_ptr(), blob.numel(), stream_ptr()), "clica_split16_export")
        return blob

    def import_state(self, blob: torch.Tensor):
        """Install a blob of `export_state` (a uint8 tensor, any device): the data-parallel verdict slot and the capacities stay this
        process's, the slot counts go to their between-steps condition.  Synchronises; not inside a graph capture."""
        if blob.dtype != torch.uint8 or blob.dim() != 1:
            raise ClicaError(f"Split16.import_state: the blob is a 1-D uint8 tensor (got {blob.dtype}, {blob.dim()} dimensions)")
        blob = blob.to(self.buf.device).contiguous()
        check(load().clica_split16_import(self.buf.data_ptr(), blob.data_ptr(), blob.numel(), self.n_layers, stream_ptr()), "clica_split16_import")

    def read(self) -> dict:
        fl, up = C.c_int32(), C.c_int32()
        a, d, w, pa, pd = (C.c_float * 9)(), (C.c_float * 9)(), (C.c_float * 9)(), (C.c_float * 9)(), (C.c_float * 9)()
        check(load().clica_split16_read(self.buf.data_ptr(), C.byref(fl), C.byref(up), a, d, w, pa, pd, stream_ptr()), "clica_split16_read")
        L = self.n_layers
        return dict(flags=int(fl.value), updates=int(up.value), scales_a=list(a)[:L + 1], scales_d=list(d)[:L], scales_w=list(w)[:L],
                    last_scales_a=list(pa)[:L + 1], last_scales_d=list(pd)[:L])


_PLANES_BYTES = {}


def mlp_planes_alloc(M: int, width: int, ones: bool, device, zero: bool = True, f16: bool = False) -> torch.Tensor:
    """Opaque buffer for the bf16-plane copy of an [M, width] layer output (operand format of `mlp_wgrad_split`).
    `zero=False`: uninitialised -- for buffers a producer kernel writes completely (the whole-stack kernels and
    `mlp_planes_from_f32` write every piece of every 16-row group, padding and ones column included; pinned by the NaN-fill in
    tests/test_gpu_mlp.py::test_split_bf16_wgrad_matches_fp64).  The drop-in path allocates per call: zeroing was two ~160 MB
    memsets per training step."""
    key = (int(M), int(width), bool(ones), bool(f16))
    nbytes = _PLANES_BYTES.get(key)
    if nbytes is None:
        nb = C.c_size_t()
        fn = load().clica_mlp_planes16_bytes if f16 else load().clica_mlp_planes_bytes      # f16x2: two pieces per unit
        check(fn(int(M), int(width), 1 if ones else 0, C.byref(nb)), "clica_mlp_planes_bytes")
        nbytes = _PLANES_BYTES[key] = nb.value
    return (torch.zeros if zero else torch.empty)(nbytes, dtype=torch.uint8, device=device)


def mlp_planes_from_f32(x: torch.Tensor, ones: bool, out: Optional[torch.Tensor] = None, state=None, tensor=None) -> torch.Tensor:
    """Plane copy (operand format of `mlp_wgrad_split`) of a fp32 [M, width] tensor: bf16x3 (clica_mlp_planes_from_f32), or -- with a
    `Split16` state and `tensor` = (family, index) in it -- f16x2 on that tensor's scale (clica_mlp_planes16_from_f32)."""
    (x, ldx) = _mat("x", x)
    M, width = x.shape
    if out is None:
        out = mlp_planes_alloc(M, width, ones, x.device, zero=False, f16=state is not None)
    if state is None:
        check(load().clica_mlp_planes_from_f32(x.data_ptr(), ldx, M, width, 1 if ones else 0, out.data_ptr(), stream_ptr()), "clica_mlp_planes_from_f32")
    else:
        check(load().clica_mlp_planes16_from_f32(x.data_ptr(), ldx, M, width, 1 if ones else 0, out.data_ptr(), state.buf.data_ptr(),
                                                 int(tensor[0]), int(tensor[1]), stream_ptr()), "clica_mlp_planes16_from_f32")
    return out


def mlp_planes_to_f32(buf: torch.Tensor, rows: int, feats: int, ones: bool) -> torch.Tensor:
    """Decode a bf16 plane buffer (csrc/planes.h) back into the fp32 [rows, feats] matrix it holds (hi + mid + lo is exact in fp32).
    Inspection / tests only -- plain tensor ops, no kernel of ours."""
    units = (feats + (1 if ones else 0) + 31) // 32
    raw = buf.view(torch.int16)
    groups = raw.numel() // (units * 3 * 512)
    a = (raw.view(groups, units, 3, 4, 2, 4, 16).to(torch.int32) << 16).view(torch.float32)      # [g][u][plane][k/4][f/16][k%4][f%16]
    v = (a[:, :, 0] + a[:, :, 1]) + a[:, :, 2]
    return v.permute(0, 2, 4, 1, 3, 5).reshape(groups * 16, units * 32)[:rows, :feats].contiguous()


def mlp_planes16_to_f32(buf: torch.Tensor, rows: int, feats: int, ones: bool, scale: float) -> torch.Tensor:
    """Decode an f16x2 plane buffer (two fp16 pieces per unit, scaled by `scale`) into the fp32 [rows, feats] matrix it represents:
    (hi + lo) / scale.  Inspection / tests only."""
    units = (feats + (1 if ones else 0) + 31) // 32
    raw = buf.view(torch.float16)
    groups = raw.numel() // (units * 2 * 512)
    a = raw.view(groups, units, 2, 4, 2, 4, 16).to(torch.float32)       # [g][u][piece][k/4][f/16][k%4][f%16]
    v = (a[:, :, 0] + a[:, :, 1]) / float(scale)
    return v.permute(0, 2, 4, 1, 3, 5).reshape(groups * 16, units * 32)[:rows, :feats].contiguous()


def mlp_planes_from_f32_t(x: torch.Tensor, out: Optional[torch.Tensor] = None, state=None, tensor=None) -> torch.Tensor:
    """T-planes of a fp32 [M, width] tensor = planes of its transpose (rows = feature, features = batch row): the A operand of
    `linear_split_fwd` / `linear_split_dgrad` (clica_mlp_planes_from_f32_t; f16x2 with `state` / `tensor` as in mlp_planes_from_f32)."""
    (x, ldx) = _mat("x", x)
    M, width = x.shape
    if out is None:
        out = mlp_planes_alloc(width, M, False, x.device, f16=state is not None)
    if state is None:
        check(load().clica_mlp_planes_from_f32_t(x.data_ptr(), ldx, M, width, out.data_ptr(), stream_ptr()), "clica_mlp_planes_from_f32_t")
    else:
        check(load().clica_mlp_planes16_from_f32_t(x.data_ptr(), ldx, M, width, out.data_ptr(), state.buf.data_ptr(), int(tensor[0]), int(tensor[1]),
                                                   stream_ptr()), "clica_mlp_planes16_from_f32_t")
    return out


def _pp(t):
    return t.data_ptr() if t is not None else None


def linear_split_fwd(xT, wT, bias, M: int, N: int, K: int, leaky: bool, slope: float, yT=None, yN=None, yN_ones: bool = True, y=None,
                     state=None, layer=None):
    """One wide nn.Linear (+ LeakyReLU) forward in split-bf16 arithmetic from T-plane operands (clica_linear_split_fwd)."""
    ldy = 0
    if y is not None:
        require_cuda(y, "y")
        if y.dim() != 2 or y.stride(1) != 1:
            raise ValueError("y must be a 2-D tensor with contiguous rows")
        ldy = y.stride(0)
    args = (xT.data_ptr(), wT.data_ptr(), _pp(bias), int(M), int(N), int(K), 1 if leaky else 0, float(slope), _pp(yT), _pp(yN),
            1 if yN_ones else 0, _pp(y), ldy)
    if state is None:
        check(load().clica_linear_split_fwd(*args, stream_ptr()), "clica_linear_split_fwd")
    else:      # f16x2: operands are the state's tensors A[layer] / W[layer], the output is A[layer + 1]
        check(load().clica_linear_split_fwd16(*args, state.buf.data_ptr(), int(layer), stream_ptr()), "clica_linear_split_fwd16")


def linear_split_dgrad(dzT, wN, actT, slope: float, M: int, N: int, K: int, dxT=None, dxN=None, dx=None, state=None, layer=None):
    """dX = (dZ W) * LeakyReLU'(layer input) of one wide layer in split-bf16 arithmetic (clica_linear_split_dgrad)."""
    ldd = 0
    if dx is not None:
        require_cuda(dx, "dx")
        if dx.dim() != 2 or dx.stride(1) != 1:
            raise ValueError("dx must be a 2-D tensor with contiguous rows")
        ldd = dx.stride(0)
    args = (dzT.data_ptr(), wN.data_ptr(), _pp(actT), float(slope), int(M), int(N), int(K), _pp(dxT), _pp(dxN), _pp(dx), ldd)
    if state is None:
        check(load().clica_linear_split_dgrad(*args, stream_ptr()), "clica_linear_split_dgrad")
    else:      # f16x2: operands D[layer] / W[layer], the output is D[layer - 1]
        check(load().clica_linear_split_dgrad16(*args, state.buf.data_ptr(), int(layer), stream_ptr()), "clica_linear_split_dgrad16")


def mlp_wgrad_split_kind(N: int, K: int) -> int:
    """0: the layer's weight gradient runs on the bf16 matrix cores from plane copies; 1: fp32 tiny-dimension kernel."""
    k = C.c_int32()
    check(load().clica_mlp_wgrad_split_kind(int(N), int(K), C.byref(k)), "clica_mlp_wgrad_split_kind")
    return int(k.value)


def mlp_fwd_split(x: torch.Tensor, weights, biases, outs, packed_split: torch.Tensor, slope: float = 0.01, signmasks=None, mix=None,
                  planes=None, state=None):
    """`mlp_fwd` on the bf16 matrix cores with exact 3-way bf16 splits (clica_mlp_fwd_split); `weights` only give the shapes.
    `planes[l]` (from mlp_planes_alloc(M, width_l, True), or None) receives layer l's output as bf16 planes for
    `mlp_wgrad_split`; `outs[l]` may then be None (no fp32 copy of that hidden activation)."""
    (x, ldx) = _mat("x", x)
    L = len(weights)
    bs = [None if b is None else b.detach().contiguous() for b in biases]
    VP, I64, I32 = C.c_void_p * L, C.c_int64 * L, C.c_int32 * L
    gW, gslope, xout = mix if mix is not None else (None, 0.0, None)
    if gW is not None:
        gW = gW.detach().contiguous()
    args = (x.data_ptr(), ldx, x.shape[0], ptr(gW), 0 if gW is None else gW.shape[0], float(gslope),
            ptr(xout), 0 if xout is None else xout.stride(0), L,
            VP(*[None if b is None else b.data_ptr() for b in bs]),
            VP(*[ptr(o) for o in outs]), I64(*[0 if o is None else o.stride(0) for o in outs]),
            I32(*[w.shape[0] for w in weights]), I32(*[w.shape[1] for w in weights]),
            packed_split.data_ptr(), None if signmasks is None else VP(*[ptr(m) for m in signmasks]),
            None if planes is None else VP(*[ptr(q) for q in planes]), float(slope))
    if state is None:
        check(load().clica_mlp_fwd_split(*args, stream_ptr()), "clica_mlp_fwd_split")
    else:      # f16x2 arithmetic on `state`'s scales (ops.Split16)
        check(load().clica_mlp_fwd_split16(*args, state.buf.data_ptr(), stream_ptr()), "clica_mlp_fwd_split16")
    return outs[-1]


def mlp_chain_tail_supported(shapes) -> bool:
    """Can the backward chain leave the weight-gradient slabs of the first / last layer of an encoder with these (out, in) shapes
    (forward order) itself?  (clica_mlp_chain_tail_supported)"""
    L = len(shapes)
    I32 = C.c_int32 * L
    ok = C.c_int32()
    check(load().clica_mlp_chain_tail_supported(L, I32(*[s[0] for s in shapes]), I32(*[s[1] for s in shapes]), C.byref(ok)),
          "clica_mlp_chain_tail_supported")
    return bool(ok.value)


def mlp_dgrad_chain_split(dy: torch.Tensor, weights_chain, packed_split_t: torch.Tensor, outs, slope: float = 0.01, masks_chain=None,
                          planes=None, state=None, tail: Optional[dict] = None):
    """`mlp_dgrad_chain` on the bf16 matrix cores (clica_mlp_dgrad_split); sign bits from `mlp_fwd_split`.  `planes[j]`
    (mlp_planes_alloc(M, width, False) or None) receives link j's dZ as bf16 planes; `outs[j]` may then be None.
    `tail` = dict(a_last, x, shapes, ws): the launch also leaves the weight-gradient slabs of the encoder's n-wide first and last
    layer in `ws`, the workspace of the `mlp_wgrad_split(..., adam=..., tail_slabs=True)` call that follows
    (clica_mlp_dgrad_split_tail)."""
    (dy, lddy) = _mat("dy", dy)
    n = len(weights_chain)
    I32, I64, VP = C.c_int32 * n, C.c_int64 * n, C.c_void_p * n
    args = (dy.data_ptr(), lddy, dy.shape[0], n,
            I32(*[w.shape[1] for w in weights_chain]), I32(*[w.shape[0] for w in weights_chain]),
            packed_split_t.data_ptr(), None if masks_chain is None else VP(*[ptr(m) for m in masks_chain]),
            VP(*[ptr(o) for o in outs]), I64(*[0 if o is None else o.stride(0) for o in outs]),
            None if planes is None else VP(*[ptr(q) for q in planes]), float(slope))
    if tail is not None:
        (al, lda), (xx, ldx) = _mat("a_last", tail["a_last"]), _mat("x", tail["x"])
        shapes = [tuple(sh) for sh in tail["shapes"]]
        Le = len(shapes)
        N32, K32 = (C.c_int32 * Le)(*[sh[0] for sh in shapes]), (C.c_int32 * Le)(*[sh[1] for sh in shapes])
        parts = tail.get("dy_parts")          # _lib.DyParts filled by clica_lp_loss_bwd_sym_train_parts: the chain's prologue finishes dy
        mse = tail.get("mse")                 # dict(y, target, loss_out, ws[, tick]): the chain's prologue forms dy from the MSE objective
        mse_desc = None
        if mse is not None:
            (yy, ldy), (tt, ldt) = _mat("y", mse["y"]), _mat("target", mse["target"])
            mse_desc = _lib.MseTarget(y=yy.data_ptr(), ldy=ldy, target=tt.data_ptr(), ldt=ldt, loss_out=mse["loss_out"].data_ptr(),
                                      tick=ptr(mse.get("tick")), workspace=mse["ws"].data_ptr(), workspace_bytes=mse["ws"].numel())
        desc = _lib.ChainTail(a_last=al.data_ptr(), lda=lda, x=xx.data_ptr(), ldx=ldx, n_layers=Le, N=N32, K=K32,
                              wgrad_workspace=tail["ws"].data_ptr(), wgrad_workspace_bytes=tail["ws"].numel(),
                              dy_parts=C.pointer(parts) if parts is not None else None,
                              mse=C.pointer(mse_desc) if mse_desc is not None else None)
        check(load().clica_mlp_dgrad_split_tail(*args, None if state is None else state.buf.data_ptr(), C.byref(desc), stream_ptr()),
              "clica_mlp_dgrad_split_tail")
    elif state is None:
        check(load().clica_mlp_dgrad_split(*args, stream_ptr()), "clica_mlp_dgrad_split")
    else:
        check(load().clica_mlp_dgrad_split16(*args, state.buf.data_ptr(), stream_ptr()), "clica_mlp_dgrad_split16")
    return outs


def mlp_wgrad_split_workspace(M: int, shapes, device) -> torch.Tensor:
    L = len(shapes)
    I32 = C.c_int32 * L
    nb = C.c_size_t()
    check(load().clica_mlp_wgrad_split_workspace_bytes(int(M), L, I32(*[s[0] for s in shapes]), I32(*[s[1] for s in shapes]), C.byref(nb)),
          "clica_mlp_wgrad_split_workspace_bytes")
    return torch.zeros(nb.value, dtype=torch.uint8, device=device)


def mlp_wgrad_split(M: int, dz_planes, x_planes, dzs, xs, dWs, dbs, ws: Optional[torch.Tensor] = None, accumulate: bool = False,
                    state=None, a_index=None, d_index=None, adam: Optional[dict] = None, tail_slabs: bool = False):
    """Every layer's dW / db in the split-bf16 arithmetic (clica_mlp_wgrad_split).  Per layer EITHER the two plane buffers
    (`dz_planes[l]`, `x_planes[l]`: layers with `mlp_wgrad_split_kind` 0) OR the fp32 operands (`dzs[l]`, `xs[l]`: kind 1).
    `adam` = dict(param, grad, exp_avg, exp_avg_sq, step_dev, lr, beta1, beta2, eps, grad_scale, t_offset, s16): the trailing
    reduction launch also applies the optimizer to the arenas the dW / db views live in (clica_mlp_wgrad_split_adam)."""
    L = len(dWs)
    VP, I64, I32 = C.c_void_p * L, C.c_int64 * L, C.c_int32 * L
    dzm = [None if t is None else _mat("dz", t) for t in dzs]
    xm = [None if t is None else _mat("x", t) for t in xs]
    shapes = [tuple(w.shape) for w in dWs]
    if ws is None:
        ws = mlp_wgrad_split_workspace(M, shapes, dWs[0].device)
    args = (int(M), L, VP(*[ptr(q) for q in dz_planes]), VP(*[ptr(q) for q in x_planes]),
            VP(*[None if m is None else m[0].data_ptr() for m in dzm]), I64(*[0 if m is None else m[1] for m in dzm]),
            VP(*[None if m is None else m[0].data_ptr() for m in xm]), I64(*[0 if m is None else m[1] for m in xm]),
            VP(*[w.data_ptr() for w in dWs]), I64(*[w.stride(0) for w in dWs]),
            VP(*[ptr(b) for b in dbs]), I32(*[s[0] for s in shapes]), I32(*[s[1] for s in shapes]), 1 if accumulate else 0)
    if tail_slabs and adam is None:
        raise ValueError("mlp_wgrad_split(tail_slabs=True) needs adam=...: the slabs the chain left are consumed by clica_mlp_wgrad_split_adam")
    if adam is not None:
        global PARAM_EPOCH
        PARAM_EPOCH += 1
        if accumulate:
            raise ValueError("mlp_wgrad_split(adam=...): accumulate is not supported")
        s16 = adam.get("s16")
        desc = _lib.AdamDesc(param=adam["param"].data_ptr(), grad=adam["grad"].data_ptr(), exp_avg=adam["exp_avg"].data_ptr(),
                             exp_avg_sq=adam["exp_avg_sq"].data_ptr(), count=adam["param"].numel(), lr=float(adam["lr"]),
                             beta1=float(adam["beta1"]), beta2=float(adam["beta2"]), eps=float(adam["eps"]),
                             grad_scale=float(adam.get("grad_scale", 1.0)), step_dev=adam["step_dev"].data_ptr(),
                             t_offset=int(adam.get("t_offset", 1)), split16_state=None if s16 is None else s16.buf.data_ptr(),
                             n_layers=0 if s16 is None else s16.n_layers)
        check(load().clica_mlp_wgrad_split_adam(*args[:-1], None if state is None else state.buf.data_ptr(),
                                                None if state is None else I32(*[int(i) for i in a_index]),
                                                None if state is None else I32(*[int(i) for i in d_index]), C.byref(desc),
                                                1 if tail_slabs else 0, ws.data_ptr(), ws.numel(), stream_ptr()), "clica_mlp_wgrad_split_adam")
    elif state is None:
        check(load().clica_mlp_wgrad_split(*args, ws.data_ptr(), ws.numel(), stream_ptr()), "clica_mlp_wgrad_split")
    else:      # f16x2 plane copies: per layer the positions of its operands' scales in the state (include/clica.h)
        check(load().clica_mlp_wgrad_split16(*args, state.buf.data_ptr(), I32(*[int(i) for i in a_index]), I32(*[int(i) for i in d_index]),
                                             ws.data_ptr(), ws.numel(), stream_ptr()), "clica_mlp_wgrad_split16")
    return ws


def mlp_signmask_alloc(M: int, n_layers: int, device, zero: bool = True) -> list:
    """Per-layer opaque sign-bit buffers for mlp_fwd(signmasks=...) / mlp_dgrad_chain(masks_chain=...).  The forward writes every
    word of a buffer it is given (all waves and lanes of every workgroup), so `zero=False` (no fill launches) is safe for a buffer
    that goes straight into a forward call."""
    nbytes = C.c_size_t()
    check(load().clica_mlp_signmask_bytes(int(M), C.byref(nbytes)), "clica_mlp_signmask_bytes")
    mk = torch.zeros if zero else torch.empty
    return [mk(nbytes.value // 8, dtype=torch.int64, device=device) for _ in range(n_layers)]


def mlp_fwd(x: torch.Tensor, weights, biases, outs, slope: float = 0.01, packed: Optional[torch.Tensor] = None,
            signmasks=None, mix=None):
    """Whole Linear(+LeakyReLU) stack in one launch (clica_mlp_fwd); `outs[l]` receives layer l's output
    (saved activations; the last one is the result).  Widths <= 512, <= 8 layers.  `packed` = the same
    weights from `mlp_pack_weights` (faster weight streaming).  `signmasks[l]` (from mlp_signmask_alloc, or
    None) receives the (out > 0) bits of layer l for the one-launch backward.
    `mix = (gW [L, n, n], slope, x_out)`: `x` holds the LATENTS and the mixing net g runs in the kernel's prologue
    (clica_mlp_fwd_mixed); x_out receives g(x)."""
    (x, ldx) = _mat("x", x)
    L = len(weights)
    ws = [_mat(f"weight[{l}]", w) for l, w in enumerate(weights)]
    bs = [None if b is None else b.detach().contiguous() for b in biases]
    for o in outs:
        require_cuda(o, "out")
    VP = C.c_void_p * L
    I64 = C.c_int64 * L
    I32 = C.c_int32 * L
    common = (L, VP(*[w.data_ptr() for w, _ in ws]), I64(*[ld for _, ld in ws]),
              VP(*[None if b is None else b.data_ptr() for b in bs]),
              VP(*[o.data_ptr() for o in outs]), I64(*[o.stride(0) for o in outs]),
              I32(*[w.shape[0] for w, _ in ws]), I32(*[w.shape[1] for w, _ in ws]),
              ptr(packed), None if signmasks is None else VP(*[ptr(m) for m in signmasks]),
              float(slope), stream_ptr())
    if mix is None:
        check(load().clica_mlp_fwd(x.data_ptr(), ldx, x.shape[0], *common), "clica_mlp_fwd")
    else:
        gW, gslope, xout = mix
        gW = gW.detach().contiguous()
        check(load().clica_mlp_fwd_mixed(x.data_ptr(), ldx, x.shape[0], gW.data_ptr(), gW.shape[0], float(gslope),
                                         xout.data_ptr(), xout.stride(0), *common), "clica_mlp_fwd_mixed")
    return outs[-1]


def mlp_dgrad_chain(dy: torch.Tensor, weights_chain, packed_t: torch.Tensor, acts_chain, outs, slope: float = 0.01,
                    masks_chain=None):
    """Backward data chain in one launch (clica_mlp_dgrad).  `weights_chain` = encoder weights in chain order
    (layer L-1 first ... layer 1), `packed_t` = mlp_pack_weights(weights_chain, transpose=True), `acts_chain[j]`
    = saved activation that fed layer j of the chain, `outs[j]` = dZ of the layer below (written).
    `masks_chain[j]` = that activation's sign bits from mlp_fwd (used instead of re-reading the activation)."""
    (dy, lddy) = _mat("dy", dy)
    n = len(weights_chain)
    I32, I64, VP = C.c_int32 * n, C.c_int64 * n, C.c_void_p * n
    acts = [None if a is None else _mat("act", a) for a in acts_chain]
    check(load().clica_mlp_dgrad(dy.data_ptr(), lddy, dy.shape[0], n,
                                 I32(*[w.shape[1] for w in weights_chain]), I32(*[w.shape[0] for w in weights_chain]),
                                 packed_t.data_ptr(),
                                 VP(*[None if a is None else a[0].data_ptr() for a in acts]), I64(*[0 if a is None else a[1] for a in acts]),
                                 None if masks_chain is None else VP(*[ptr(m) for m in masks_chain]),
                                 VP(*[o.data_ptr() for o in outs]), I64(*[o.stride(0) for o in outs]),
                                 float(slope), stream_ptr()), "clica_mlp_dgrad")
    return outs


def linear_plan(op: str, M: int, N: int, K: int):
    """(tile_m, tile_n, waves, splits) of the kernel instance a Linear launch of this shape uses."""
    v = [C.c_int32() for _ in range(4)]
    check(load().clica_linear_plan({"fwd": 0, "dgrad": 1, "wgrad": 2}[op], M, N, K, *[C.byref(x) for x in v]), "clica_linear_plan")
    return tuple(x.value for x in v)


# ------------------------------------------------------------------------------- heads
def rescale_fwd(x, r):
    (x, ldx) = _mat("x", x)
    M, n = x.shape
    y = torch.empty((M, n), dtype=torch.float32, device=x.device)
    inv = torch.empty((M,), dtype=torch.float32, device=x.device)
    check(load().clica_rescale_fwd(x.data_ptr(), ldx, r.data_ptr(), y.data_ptr(), n, inv.data_ptr(), M, n, stream_ptr()),
          "clica_rescale_fwd")
    return y, inv


def rescale_bwd(x, r, inv, dy, need_dx=True, need_dr=True):
    (x, ldx), (dy, lddy) = _mat("x", x), _mat("dy", dy)
    M, n = x.shape
    dx = torch.empty((M, n), dtype=torch.float32, device=x.device) if need_dx else None
    part = torch.empty(((M + 255) // 256,), dtype=torch.float32, device=x.device) if need_dr else None
    check(load().clica_rescale_bwd(x.data_ptr(), ldx, r.data_ptr(), inv.data_ptr(), dy.data_ptr(), lddy, ptr(dx), n,
                                   ptr(part), M, n, stream_ptr()), "clica_rescale_bwd")
    return dx, (part.sum().reshape(1) if need_dr else None)


def softclip_fwd(x, bound):
    (x, ldx) = _mat("x", x)
    M, n = x.shape
    y = torch.empty((M, n), dtype=torch.float32, device=x.device)
    check(load().clica_softclip_fwd(x.data_ptr(), ldx, bound.data_ptr(), y.data_ptr(), n, M, n, stream_ptr()),
          "clica_softclip_fwd")
    return y


def softclip_bwd(x, bound, dy, need_dx=True, need_db=True):
    (x, ldx), (dy, lddy) = _mat("x", x), _mat("dy", dy)
    M, n = x.shape
    dx = torch.empty((M, n), dtype=torch.float32, device=x.device) if need_dx else None
    part = torch.empty(((M + 255) // 256, n), dtype=torch.float32, device=x.device) if need_db else None
    check(load().clica_softclip_bwd(x.data_ptr(), ldx, bound.data_ptr(), dy.data_ptr(), lddy, ptr(dx), n, ptr(part),
                                    M, n, stream_ptr()), "clica_softclip_bwd")
    return dx, (part.sum(0) if need_db else None)


def leaky_relu_fwd(x, slope: float = 0.01):
    (x, ldx) = _mat("x", x)
    M, n = x.shape
    y = torch.empty((M, n), dtype=torch.float32, device=x.device)
    check(load().clica_leaky_relu_fwd(x.data_ptr(), ldx, y.data_ptr(), n, M, n, float(slope), stream_ptr()), "clica_leaky_relu_fwd")
    return y


def leaky_relu_bwd(yact, dy, slope: float = 0.01):
    (yact, ldy), (dy, lddy) = _mat("yact", yact), _mat("dy", dy)
    M, n = yact.shape
    dx = torch.empty((M, n), dtype=torch.float32, device=dy.device)
    check(load().clica_leaky_relu_bwd(yact.data_ptr(), ldy, dy.data_ptr(), lddy, dx.data_ptr(), n, M, n, float(slope), stream_ptr()),
          "clica_leaky_relu_bwd")
    return dx


# ------------------------------------------------------------------------------- mixing / adam / sampler
MIX_ACT = {"leaky_relu": 0, "relu": 0, "elu": 1, "smooth_leaky_relu": 2, "softplus": 3}


def mixing_fwd(z: torch.Tensor, weights: torch.Tensor, slope: float = 0.2, out: Optional[torch.Tensor] = None, act_kind: int = 0):
    """x = W_L phi(... phi(W_1 z)); `weights` is a contiguous [L, n, n] stack (nn.Linear layout).  `act_kind` / `slope`:
    0 LeakyReLU(slope) (slope 0 = ReLU), 1 ELU(alpha = slope), 2 SmoothLeakyReLU(alpha = slope), 3 Softplus(beta = slope)."""
    (z, ldz) = _mat("z", z)
    require_cuda(weights, "weights")
    M, n = z.shape
    if weights.dim() != 3 or weights.shape[1:] != (n, n) or not weights.is_contiguous():
        raise ValueError(f"weights must be contiguous [L,{n},{n}], got {tuple(weights.shape)}")
    x = out if out is not None else torch.empty((M, n), dtype=torch.float32, device=z.device)
    check(load().clica_mixing_fwd_act(z.data_ptr(), ldz, weights.data_ptr(), weights.shape[0], int(act_kind), float(slope), x.data_ptr(),
                                      x.stride(0), M, n, stream_ptr()), "clica_mixing_fwd_act")
    return x


PARAM_EPOCH = 0     # bumped by every raw-pointer parameter update (adam_step): caches derived from weights (fragment-order packs) key on it,
                    # because a kernel writing through data_ptr() does not advance torch's per-tensor version counters


def adam_step(param, grad, exp_avg, exp_avg_sq, step_dev, lr, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0,
              ticket: Optional[torch.Tensor] = None, t_offset: int = 1, s16=None):
    """In-place Adam on flat fp32 arenas; `step_dev` int32[1] = updates already applied.  With `ticket` (device
    int32[1], zero) the same launch also advances `step_dev` by one (clica_adam_step_tick)."""
    global PARAM_EPOCH
    PARAM_EPOCH += 1
    for nm, t in (("param", param), ("grad", grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        require_cuda(t, nm)
        if not t.is_contiguous():
            raise ValueError(f"{nm} must be contiguous")
    if s16 is not None and ticket is not None:     # ... and so does the counter's tick (the drop-in optimizer's step)
        if t_offset != 1:
            raise ValueError("adam_step(s16=..., ticket=...): the fused tick advances the counter AFTER the update (t_offset = 1)")
        check(load().clica_adam_step_s16_tick(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                                              param.numel(), float(lr), float(beta1), float(beta2), float(eps), float(grad_scale),
                                              step_dev.data_ptr(), ticket.data_ptr(), s16.buf.data_ptr(), s16.n_layers, stream_ptr()),
              "clica_adam_step_s16_tick")
        return True
    if s16 is not None and ticket is None:     # the f16x2 arithmetic's scale update rides in the optimizer launch (clica_adam_step_s16)
        check(load().clica_adam_step_s16(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                                         param.numel(), float(lr), float(beta1), float(beta2), float(eps), float(grad_scale),
                                         step_dev.data_ptr(), int(t_offset), s16.buf.data_ptr(), s16.n_layers, stream_ptr()), "clica_adam_step_s16")
        return True
    if ticket is None and t_offset != 1:       # the counter was already advanced earlier in the step
        check(load().clica_adam_step_at(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                                        param.numel(), float(lr), float(beta1), float(beta2), float(eps), float(grad_scale),
                                        step_dev.data_ptr(), int(t_offset), stream_ptr()), "clica_adam_step_at")
    elif ticket is None:
        check(load().clica_adam_step(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                                     param.numel(), float(lr), float(beta1), float(beta2), float(eps), float(grad_scale),
                                     step_dev.data_ptr(), stream_ptr()), "clica_adam_step")
    else:
        check(load().clica_adam_step_tick(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                                          param.numel(), float(lr), float(beta1), float(beta2), float(eps), float(grad_scale),
                                          step_dev.data_ptr(), ticket.data_ptr(), stream_ptr()), "clica_adam_step_tick")


def sgd_step(param, grad, momentum_buf, step_dev, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False,
             grad_scale=1.0, ticket: Optional[torch.Tensor] = None, count: Optional[int] = None):
    """In-place torch.optim.SGD update on the first `count` (default: all) elements of flat fp32 arenas; `step_dev` int32[1] = updates
    already applied (0: the momentum buffer takes the gradient as it is).  `momentum_buf` may be None when momentum == 0.  With `ticket` (device int32[1], zero) the same launch also
    advances `step_dev` by one (clica_sgd_step_tick)."""
    global PARAM_EPOCH
    PARAM_EPOCH += 1
    for nm, t in (("param", param), ("grad", grad), ("momentum_buf", momentum_buf)):
        if t is None and nm == "momentum_buf":
            continue
        require_cuda(t, nm)
        if not t.is_contiguous():
            raise ValueError(f"{nm} must be contiguous")
    count = param.numel() if count is None else int(count)
    if count > min(t.numel() for t in (param, grad, momentum_buf) if t is not None):
        raise ValueError("sgd_step: an arena is shorter than count")
    args = (param.data_ptr(), grad.data_ptr(), ptr(momentum_buf), count, float(lr), float(momentum), float(dampening),
            float(weight_decay), int(bool(nesterov)), int(bool(maximize)), float(grad_scale), step_dev.data_ptr())
    if ticket is None:
        check(load().clica_sgd_step(*args, stream_ptr()), "clica_sgd_step")
    else:
        check(load().clica_sgd_step_tick(*args, ticket.data_ptr(), stream_ptr()), "clica_sgd_step_tick")


def publish_host(src: torch.Tensor, host_dst: torch.Tensor, seq_dev: torch.Tensor, host_seq: torch.Tensor):
    """src (device fp32, <= 64 values) -> host_dst (pinned fp32), then ++seq_dev (device int32) -> host_seq (pinned int32) behind a
    system-scope release: a host read from the middle of a captured step (clica_publish_host)."""
    assert src.is_cuda and src.dtype == torch.float32 and src.is_contiguous() and 1 <= src.numel() <= 64
    assert host_dst.is_pinned() and host_dst.dtype == torch.float32 and host_dst.numel() >= src.numel()
    assert seq_dev.is_cuda and seq_dev.dtype == torch.int32 and host_seq.is_pinned() and host_seq.dtype == torch.int32
    check(load().clica_publish_host(src.data_ptr(), src.numel(), host_dst.data_ptr(), seq_dev.data_ptr(), host_seq.data_ptr(), stream_ptr()),
          "clica_publish_host")


def stamp(slot: torch.Tensor, which: int):
    """Device-side begin (0) / end (1) time stamp into `slot` (int64 [1 + 2 * capacity], zeros): usable inside graph capture."""
    check(load().clica_stamp(slot.data_ptr(), int(which), (slot.numel() - 1) // 2, stream_ptr()), "clica_stamp")


def clock_probe(n: int, period_us: float, stream: "torch.cuda.Stream") -> torch.Tensor:
    """Start the one-wave shader-clock probe on `stream` (a SIDE stream): n samples, `period_us` apart; returns the device buffer
    int64 [n, 2] = (wall clock in 100 MHz ticks, core-clock counter), complete once `stream` is (clica_clock_probe)."""
    buf = torch.zeros((int(n), 2), dtype=torch.int64, device="cuda")
    check(load().clica_clock_probe(buf.data_ptr(), int(n), max(1, int(round(period_us * 100))), stream.cuda_stream), "clica_clock_probe")
    return buf


def clock_between(samples_cpu, t0: int, t1: int) -> Optional[float]:
    """Shader clock in GHz over the wall-clock window [t0, t1] (100 MHz ticks) from the probe's samples (numpy int64 [n, 2], sorted):
    cycles between the first and the last sample inside the window / their distance in time; None with fewer than two samples."""
    import numpy as np
    w = samples_cpu[:, 0]
    lo, hi = int(np.searchsorted(w, t0, "left")), int(np.searchsorted(w, t1, "right")) - 1
    if hi - lo < 1 or w[lo] == 0:
        return None
    return float(samples_cpu[hi, 1] - samples_cpu[lo, 1]) / (float(w[hi] - w[lo]) * 10.0)       # cycles per 10 ns tick -> GHz


def stamp_brackets(slot: torch.Tensor):
    """Completed (begin, end) pairs of a stamp slot as absolute wall-clock ticks (100 MHz)."""
    v = slot.cpu()
    n = min(int(v[0]), (v.numel() - 1) // 2)
    return [(int(v[1 + 2 * i]), int(v[2 + 2 * i])) for i in range(n)]


def stamp_intervals_us(slot: torch.Tensor):
    """Completed (begin, end) pairs of a stamp slot as microseconds (100 MHz counter)."""
    v = slot.cpu()
    n = min(int(v[0]), (v.numel() - 1) // 2)
    return [(int(v[2 + 2 * i]) - int(v[1 + 2 * i])) / 100.0 for i in range(n)]


# ------------------------------------------------------------------------------- loss workspace state (checkpoints)
def lp_loss_train_state_export(desc, ws: torch.Tensor) -> torch.Tensor:
    """What the training pair's workspace `ws` carries from call to call (include/clica.h, "CHECKPOINTS": the guard / grid words of the
    p = 2 matrix-core sweeps) as an opaque device blob; all zero where the calls of `desc` run the VALU sweeps only or `desc` is the dot
    pair's (nothing carried).  One tiny launch, no sync."""
    nb = C.c_size_t()
    check(load().clica_lp_loss_train_state_bytes(C.byref(nb)), "clica_lp_loss_train_state_bytes")
    blob = torch.zeros(nb.value, dtype=torch.uint8, device=ws.device)
    if isinstance(desc, _lib.LpLossDesc):
        check(load().clica_lp_loss_train_state_export(C.byref(desc), ws.data_ptr(), ws.numel(), blob.data_ptr(), blob.numel(), stream_ptr()),
              "clica_lp_loss_train_state_export")
    return blob


def lp_loss_train_state_import(desc, ws: torch.Tensor, blob: torch.Tensor):
    """Install a blob of `lp_loss_train_state_export` into the workspace `ws` of the same loss description (a no-op for an all-zero
    blob, the VALU-only shapes and the dot pair).  Synchronises; not inside a graph capture."""
    if blob.dtype != torch.uint8 or blob.dim() != 1:
        raise ClicaError(f"lp_loss_train_state_import: the blob is a 1-D uint8 tensor (got {blob.dtype}, {blob.dim()} dimensions)")
    if not isinstance(desc, _lib.LpLossDesc):
        return
    blob = blob.to(ws.device).contiguous()
    check(load().clica_lp_loss_train_state_import(C.byref(desc), ws.data_ptr(), ws.numel(), blob.data_ptr(), blob.numel(), stream_ptr()),
          "clica_lp_loss_train_state_import")


# ------------------------------------------------------------------------------- MSE objective
def mse_loss_workspace(M: int, n: int, device) -> torch.Tensor:
    """Zeroed workspace of clica_mse_loss_fwd_bwd / the backward chain's MSE prologue for M x n (its arrival counter must start at zero)."""
    nb = C.c_size_t()
    check(load().clica_mse_loss_workspace_bytes(int(M), int(n), C.byref(nb)), "clica_mse_loss_workspace_bytes")
    return torch.zeros(nb.value, dtype=torch.uint8, device=device)


def mse_loss_fwd_bwd(y: torch.Tensor, target: torch.Tensor, dy: Optional[torch.Tensor] = None, loss_out: Optional[torch.Tensor] = None,
                     ws: Optional[torch.Tensor] = None, tick_counter: Optional[torch.Tensor] = None):
    """loss = mean((y - target)^2) (F.mse_loss) and dy = 2 (y - target) / y.numel() in one launch, deterministic
    (clica_mse_loss_fwd_bwd).  Strided row views pass without a copy.  Returns (loss_out [1] device tensor, dy)."""
    (y, ldy), (target, ldt) = _mat("y", y), _mat("target", target)
    if target.shape != y.shape:
        raise ValueError(f"target {tuple(target.shape)} does not match y {tuple(y.shape)}")
    M, n = y.shape
    dy = torch.empty((M, n), dtype=torch.float32, device=y.device) if dy is None else dy
    loss_out = torch.empty(1, dtype=torch.float32, device=y.device) if loss_out is None else loss_out
    if ws is None:
        nb = C.c_size_t()
        check(load().clica_mse_loss_workspace_bytes(M, n, C.byref(nb)), "clica_mse_loss_workspace_bytes")
        ws = workspace("mse_loss", nb.value, y.device)
    (dyv, lddy) = _mat("dy", dy)
    if dyv.data_ptr() != dy.data_ptr():
        raise ValueError("dy must be a row-major (strided) view")
    check(load().clica_mse_loss_fwd_bwd(y.data_ptr(), ldy, target.data_ptr(), ldt, M, n, dy.data_ptr(), lddy, loss_out.data_ptr(),
                                        ptr(tick_counter), ws.data_ptr(), ws.numel(), stream_ptr()), "clica_mse_loss_fwd_bwd")
    return loss_out, dy


# ------------------------------------------------------------------------------- R2 objective
R2_REDUCTIONS = {"none": 0, "mean": 1, "sum": 2}       # CLICA_R2_REDUCE_*
R2_MODES = {"r2": 0, "negative_r2": 1}                 # CLICA_R2_MODE_*

# zeroed workspaces of clica_r2_loss_fwd per (device, M, n).  An entry is never replaced or freed (a few KB each), so a captured graph
# that recorded its pointer stays valid whatever runs afterwards; one entry serves one launch at a time (one stream per shape).
_R2_WS = {}


def r2_loss_workspace(M: int, n: int, device) -> torch.Tensor:
    """The cached zeroed workspace of clica_r2_loss_fwd for M x n on `device` (its arrival counter must start at zero)."""
    device = torch.device(device)
    key = (device.index if device.index is not None else torch.cuda.current_device(), int(M), int(n))
    ws = _R2_WS.get(key)
    if ws is None:
        nb = C.c_size_t()
        check(load().clica_r2_loss_workspace_bytes(int(M), int(n), C.byref(nb)), "clica_r2_loss_workspace_bytes")
        if torch.cuda.is_current_stream_capturing():
            # (memory allocated while capturing belongs to the graph's pool and its zeroing would be replayed: not something to cache)
            raise ClicaError(f"r2_loss: no workspace for shape ({M}, {n}) yet -- run the step once eagerly before capturing it")
        ws = _R2_WS[key] = torch.zeros(nb.value, dtype=torch.uint8, device=device)
    _lib.note_graph_use(ws)
    return ws


def _r2_codes(reduction: str, mode: str) -> Tuple[int, int]:
    if reduction not in R2_REDUCTIONS:
        raise ValueError(f"reduction {reduction!r} (one of {sorted(R2_REDUCTIONS)})")
    if mode not in R2_MODES:
        raise ValueError(f"mode {mode!r} (one of {sorted(R2_MODES)})")
    return R2_REDUCTIONS[reduction], R2_MODES[mode]


def r2_loss_fwd(y_pred: torch.Tensor, y: torch.Tensor, reduction: str = "mean", mode: str = "negative_r2",
                out: Optional[torch.Tensor] = None, r2_cols: Optional[torch.Tensor] = None, inv_var: Optional[torch.Tensor] = None,
                ws: Optional[torch.Tensor] = None):
    """(Negative) R2 score per column of y_pred against the target y (reference losses.py:489-500) in one deterministic launch
    (clica_r2_loss_fwd).  Strided row views pass without a copy.  Returns (out: [n] for "none" else [1], r2_cols [n], inv_var [n]);
    inv_var is what r2_loss_bwd needs."""
    red, md = _r2_codes(reduction, mode)
    (y_pred, ldp), (y, ldy) = _mat("y_pred", y_pred), _mat("y", y)
    if y.shape != y_pred.shape:
        raise ValueError(f"target {tuple(y.shape)} does not match y_pred {tuple(y_pred.shape)}")
    M, n = y_pred.shape
    dev = y_pred.device
    out = torch.empty(n if red == 0 else 1, dtype=torch.float32, device=dev) if out is None else out
    r2_cols = torch.empty(n, dtype=torch.float32, device=dev) if r2_cols is None else r2_cols
    inv_var = torch.empty(n, dtype=torch.float32, device=dev) if inv_var is None else inv_var
    ws = r2_loss_workspace(M, n, dev) if ws is None else ws
    check(load().clica_r2_loss_fwd(y_pred.data_ptr(), ldp, y.data_ptr(), ldy, M, n, red, md, out.data_ptr(), r2_cols.data_ptr(),
                                   inv_var.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr()), "clica_r2_loss_fwd")
    return out, r2_cols, inv_var


def r2_loss_bwd(y_pred: torch.Tensor, y: torch.Tensor, inv_var: torch.Tensor, g: torch.Tensor, reduction: str = "mean",
                mode: str = "negative_r2", dy: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d out / d y_pred of r2_loss_fwd times the upstream gradient g (a device tensor: n values for "none", else one) in one
    element-wise launch (clica_r2_loss_bwd); inv_var is the forward's."""
    red, md = _r2_codes(reduction, mode)
    (y_pred, ldp), (y, ldy) = _mat("y_pred", y_pred), _mat("y", y)
    if y.shape != y_pred.shape:
        raise ValueError(f"target {tuple(y.shape)} does not match y_pred {tuple(y_pred.shape)}")
    M, n = y_pred.shape
    require_cuda(inv_var, "inv_var"); require_cuda(g, "g")
    if inv_var.numel() != n or not inv_var.is_contiguous():
        raise ValueError(f"inv_var must hold n = {n} contiguous values, got {tuple(inv_var.shape)}")
    if g.numel() != (n if red == 0 else 1) or not g.is_contiguous():
        raise ValueError(f"g must hold {n if red == 0 else 1} contiguous value(s) for reduction {reduction!r}, got {tuple(g.shape)}")
    dy = torch.empty((M, n), dtype=torch.float32, device=y_pred.device) if dy is None else dy
    (dyv, lddy) = _mat("dy", dy)
    if dyv.data_ptr() != dy.data_ptr() or tuple(dy.shape) != (M, n):
        raise ValueError(f"dy must be a row-major (strided) {M} x {n} view")
    check(load().clica_r2_loss_bwd(y_pred.data_ptr(), ldp, y.data_ptr(), ldy, M, n, red, md, inv_var.data_ptr(), g.data_ptr(),
                                   dy.data_ptr(), lddy, stream_ptr()), "clica_r2_loss_bwd")
    return dy


# ------------------------------------------------------------------------------- BatchNorm1d / GroupNorm(1, C) + LeakyReLU
NORM_KINDS = {"bn": 0, "gn": 1}                        # CLICA_NORM_BATCH / CLICA_NORM_GROUP

# Partial-sum workspaces of the norm, bn2d and stem-unit kernels per (family, device, shape); as _R2_WS an entry is never replaced or
# freed, so a pointer a captured graph recorded stays valid.  No initial contents are needed; one entry serves one launch at a time on
# one stream.
_PARTIAL_WS = {}


def _partial_workspace(family: str, shape, device, size_fn: str, size_args, what: str) -> torch.Tensor:
    """The cached workspace of `family` for `shape` on `device`.  The library's size_fn(*size_args, &bytes) gives its size (and validates
    the shape); `what` names the workspace in the error of a first use under capture."""
    device = torch.device(device)
    key = (family, device.index if device.index is not None else torch.cuda.current_device()) + tuple(shape)
    ws = _PARTIAL_WS.get(key)
    if ws is None:
        nb = C.c_size_t()
        check(getattr(load(), size_fn)(*size_args, C.byref(nb)), size_fn)
        if torch.cuda.is_current_stream_capturing():
            # (memory allocated while capturing belongs to the graph's pool: not something to cache)
            raise ClicaError(f"{what} yet -- run the step once eagerly before capturing it")
        ws = _PARTIAL_WS[key] = torch.empty(max(nb.value, 16), dtype=torch.uint8, device=device)
    _lib.note_graph_use(ws)
    return ws


def norm_workspace(kind: str, M: int, C_: int, device) -> torch.Tensor:
    """The cached workspace of clica_bn_lrelu_fwd_train / _bwd ("bn") or clica_gn_lrelu_bwd ("gn") for M x C on `device`."""
    if kind not in NORM_KINDS:
        raise ValueError(f"kind {kind!r} (one of {sorted(NORM_KINDS)})")
    return _partial_workspace("norm", (kind, int(M), int(C_)), device, "clica_norm_workspace_bytes",
                              (NORM_KINDS[kind], int(M), int(C_), 1.0), f"norm: no {kind} workspace for shape ({M}, {C_})")


# Every wrapper of the family validates in one order: the maps / matrices (layout, then shape against x), the vectors, device and dtype
# of everything, then the workspace.  The three helpers below and the map checks are all of it; None stands for an argument not given.
def _norm_mat(name: str, t: torch.Tensor) -> torch.Tensor:
    if t.dim() != 2 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous [M, C] matrix, got shape {tuple(t.shape)} strides {t.stride()}")
    return t


def _norm_vecs(n: int, **vecs) -> None:
    for name, t in vecs.items():
        if t is not None and (t.numel() != n or not t.is_contiguous()):
            raise ValueError(f"{name} must hold {n} contiguous values, got {tuple(t.shape)}")


def _running_pair(running_mean, running_var) -> None:
    """The optional running statistics of a training forward: both or neither."""
    if (running_mean is None) != (running_var is None):
        raise ValueError("running_mean and running_var come together")


def _on_gpu(**tensors) -> None:
    for name, t in tensors.items():
        if t is not None:
            require_cuda(t, name)


def batchnorm_lrelu_fwd(x, weight, bias, running_mean=None, running_var=None, eps: float = 1e-5, momentum: float = 0.1,
                        slope: float = 0.01):
    """Training BatchNorm1d over the rows of x [M, C] (M >= 2) fused with LeakyReLU(slope) (slope = 1: none) in two launches
    (clica_bn_lrelu_fwd_train); running_mean / running_var, when given, are updated in place as nn.BatchNorm1d does.
    Returns (y, save_mean [C], save_invstd [C]); the last two are what batchnorm_lrelu_bwd needs."""
    x = _norm_mat("x", x)
    M, n = x.shape
    _running_pair(running_mean, running_var)
    _norm_vecs(n, weight=weight, bias=bias, running_mean=running_mean, running_var=running_var)
    _on_gpu(x=x, weight=weight, bias=bias, running_mean=running_mean, running_var=running_var)
    y = torch.empty_like(x)
    save_mean = torch.empty(n, dtype=torch.float32, device=x.device)
    save_invstd = torch.empty(n, dtype=torch.float32, device=x.device)
    nb = C.c_size_t()        # (validates M, C and the slope before a workspace is looked up)
    check(load().clica_norm_workspace_bytes(0, M, n, float(slope), C.byref(nb)), "clica_norm_workspace_bytes")
    ws = norm_workspace("bn", M, n, x.device)
    check(load().clica_bn_lrelu_fwd_train(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), M, n, float(eps), float(momentum), float(slope),
                                          y.data_ptr(), save_mean.data_ptr(), save_invstd.data_ptr(), ptr(running_mean), ptr(running_var),
                                          ws.data_ptr(), ws.numel(), stream_ptr()), "clica_bn_lrelu_fwd_train")
    return y, save_mean, save_invstd


def batchnorm_lrelu_eval(x, weight, bias, running_mean, running_var, eps: float = 1e-5, slope: float = 0.01):
    """Inference BatchNorm1d on the running statistics fused with LeakyReLU(slope): one element-wise launch (clica_bn_lrelu_fwd_eval)."""
    x = _norm_mat("x", x)
    M, n = x.shape
    _norm_vecs(n, weight=weight, bias=bias, running_mean=running_mean, running_var=running_var)
    _on_gpu(x=x, weight=weight, bias=bias, running_mean=running_mean, running_var=running_var)
    y = torch.empty_like(x)
    check(load().clica_bn_lrelu_fwd_eval(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), running_mean.data_ptr(), running_var.data_ptr(),
                                         M, n, float(eps), float(slope), y.data_ptr(), stream_ptr()), "clica_bn_lrelu_fwd_eval")
    return y


def batchnorm_lrelu_bwd(x, y, dy, weight, save_mean, save_invstd, slope: float = 0.01):
    """(dx, dweight, dbias) of batchnorm_lrelu_fwd from its input x, its OUTPUT y (the gate) and the saved statistics: two launches
    (clica_bn_lrelu_bwd)."""
    x, y, dy = _norm_mat("x", x), _norm_mat("y", y), _norm_mat("dy", dy)
    M, n = x.shape
    if y.shape != x.shape or dy.shape != x.shape:
        raise ValueError(f"x {tuple(x.shape)}, y {tuple(y.shape)} and dy {tuple(dy.shape)} must agree")
    _norm_vecs(n, weight=weight, save_mean=save_mean, save_invstd=save_invstd)
    _on_gpu(x=x, y=y, dy=dy, weight=weight, save_mean=save_mean, save_invstd=save_invstd)
    dx = torch.empty_like(x)
    dw = torch.empty(n, dtype=torch.float32, device=x.device)
    db = torch.empty(n, dtype=torch.float32, device=x.device)
    ws = norm_workspace("bn", M, n, x.device)
    check(load().clica_bn_lrelu_bwd(x.data_ptr(), y.data_ptr(), dy.data_ptr(), weight.data_ptr(), save_mean.data_ptr(),
                                    save_invstd.data_ptr(), M, n, float(slope), dx.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                    ws.numel(), stream_ptr()), "clica_bn_lrelu_bwd")
    return dx, dw, db


def groupnorm_lrelu_fwd(x, weight, bias, eps: float = 1e-5, slope: float = 0.01):
    """GroupNorm(1, C) over each row of x [M, C] fused with LeakyReLU(slope) in one launch (clica_gn_lrelu_fwd).
    Returns (y, mean [M], rstd [M]); the last two are what groupnorm_lrelu_bwd needs."""
    x = _norm_mat("x", x)
    M, n = x.shape
    _norm_vecs(n, weight=weight, bias=bias)
    _on_gpu(x=x, weight=weight, bias=bias)
    y = torch.empty_like(x)
    mean = torch.empty(M, dtype=torch.float32, device=x.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x.device)
    check(load().clica_gn_lrelu_fwd(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), M, n, float(eps), float(slope), y.data_ptr(),
                                    mean.data_ptr(), rstd.data_ptr(), stream_ptr()), "clica_gn_lrelu_fwd")
    return y, mean, rstd


def groupnorm_lrelu_bwd(x, y, dy, weight, mean, rstd, slope: float = 0.01):
    """(dx, dweight, dbias) of groupnorm_lrelu_fwd: two launches (clica_gn_lrelu_bwd)."""
    x, y, dy = _norm_mat("x", x), _norm_mat("y", y), _norm_mat("dy", dy)
    M, n = x.shape
    if y.shape != x.shape or dy.shape != x.shape:
        raise ValueError(f"x {tuple(x.shape)}, y {tuple(y.shape)} and dy {tuple(dy.shape)} must agree")
    _norm_vecs(n, weight=weight); _norm_vecs(M, mean=mean, rstd=rstd)
    _on_gpu(x=x, y=y, dy=dy, weight=weight, mean=mean, rstd=rstd)
    dx = torch.empty_like(x)
    dw = torch.empty(n, dtype=torch.float32, device=x.device)
    db = torch.empty(n, dtype=torch.float32, device=x.device)
    nb = C.c_size_t()
    check(load().clica_norm_workspace_bytes(1, M, n, float(slope), C.byref(nb)), "clica_norm_workspace_bytes")
    ws = norm_workspace("gn", M, n, x.device)
    check(load().clica_gn_lrelu_bwd(x.data_ptr(), y.data_ptr(), dy.data_ptr(), weight.data_ptr(), mean.data_ptr(), rstd.data_ptr(), M, n,
                                    float(slope), dx.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr()),
          "clica_gn_lrelu_bwd")
    return dx, dw, db


# ------------------------------------------------------------------------------- BatchNorm2d (+ residual) + (leaky) ReLU and the global
# average pool, on contiguous NCHW or on dense channels-last activations
AVGPOOL_MAX_HW = 1 << 14                   # csrc/pool2d.hip avgpool::kMaxHW


def bn2d_workspace(N: int, C_: int, HW: int, device) -> torch.Tensor:
    """The cached workspace of clica_bn2d_act_fwd_train / _bwd for x[N, C, H, W] with H W = HW on `device`."""
    shape = (int(N), int(C_), int(HW))
    return _partial_workspace("bn2d", shape, device, "clica_bn2d_workspace_bytes", shape, f"bn2d: no workspace for shape ({N}, {C_}, {HW})")


def bn2d_nhwc_workspace(M: int, C_: int, device) -> torch.Tensor:
    """The cached workspace of clica_bn2d_nhwc_act_fwd_train / _bwd for a channels-last x[N, C, H, W] with N H W = M on `device`."""
    shape = (int(M), int(C_))
    return _partial_workspace("bn2d_nhwc", shape, device, "clica_bn2d_nhwc_workspace_bytes", shape,
                              f"bn2d (channels-last): no workspace for shape ({M}, {C_})")


def _bn2d_map(name: str, t: torch.Tensor, shape=None) -> torch.Tensor:
    if t.dim() != 4 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous NCHW tensor [N, C, H, W], got shape {tuple(t.shape)} strides {t.stride()}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} {tuple(t.shape)} must have the shape of x {tuple(shape)}")
    return t


def _bn2d_nhwc_map(name: str, t: torch.Tensor, shape=None) -> torch.Tensor:
    """A 4-D tensor whose memory is the dense row-major [N, H, W, C] (with C = 1 or H = W = 1 that is also the memory of a contiguous
    NCHW tensor, whatever its strides say)."""
    if t.dim() != 4 or t.numel() == 0 or not t.is_contiguous(memory_format=torch.channels_last):
        raise ValueError(f"{name} must be a dense channels-last tensor [N, C, H, W] (strides (H W C, 1, W C, C)), got shape {tuple(t.shape)} "
                         f"strides {t.stride()}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} {tuple(t.shape)} must have the shape of x {tuple(shape)}")
    return t


class _Bn2dLayout(NamedTuple):
    """All that differs between the two memory layouts of the units and of the average pool."""
    map: Callable                               # (name, t, shape=None) -> t: the layout, then the shape against x; no device check
    memory_format: torch.memory_format          # of the outputs shaped like x
    unit_dims: Callable                         # (N, C, H, W) -> the leading integers of the units' ABI calls and of `workspace`
    pool_dims: Callable                         # (N, C, H, W) -> those of the average pool's
    workspace: Callable                         # (*unit_dims, device) -> the cached partial-sum workspace
    fwd_train: str                              # the entry points
    fwd_eval: str
    bwd: str
    pool_fwd: str
    pool_bwd: str
    bf16: bool                                  # are there `name + "_bf16"` entry points for bf16 activations?

    def empty(self, shape, device, dtype=torch.float32) -> torch.Tensor:
        return torch.empty(tuple(shape), dtype=dtype, device=device, memory_format=self.memory_format)


_NCHW = _Bn2dLayout(_bn2d_map, torch.contiguous_format, lambda N, n, H, W: (N, n, H * W), lambda N, n, H, W: (N * n, H * W), bn2d_workspace,
                    "clica_bn2d_act_fwd_train", "clica_bn2d_act_fwd_eval", "clica_bn2d_act_bwd",
                    "clica_avgpool2d_global_fwd", "clica_avgpool2d_global_bwd", False)
_NHWC = _Bn2dLayout(_bn2d_nhwc_map, torch.channels_last, lambda N, n, H, W: (N * H * W, n), lambda N, n, H, W: (N, H * W, n), bn2d_nhwc_workspace,
                    "clica_bn2d_nhwc_act_fwd_train", "clica_bn2d_nhwc_act_fwd_eval", "clica_bn2d_nhwc_act_bwd",
                    "clica_avgpool2d_global_nhwc_fwd", "clica_avgpool2d_global_nhwc_bwd", True)


def _acts_on_gpu(L, **acts) -> torch.dtype:
    """The activations of one call (None: absent) live on the GPU and share one element type, which is returned: float32, or bfloat16
    where the layout has kernels for it.  Anything else raises before any launch -- a bf16 x with an fp32 residual or dy among it."""
    named = [(name, t) for name, t in acts.items() if t is not None]
    lead, dtype = named[0][0], named[0][1].dtype
    if not (L.bf16 and dtype == torch.bfloat16):
        _on_gpu(**acts)
        return torch.float32
    for name, t in named:
        if not t.is_cuda:
            raise ClicaError(f"{name} must live on the GPU (got device {t.device}); cl_ica_amd runs only through its HIP kernels")
        if t.dtype != dtype:
            raise ClicaError(f"{name} must be {dtype} as {lead} is (got {t.dtype}): the activations of a call share one element type")
    return dtype


def _entry(name: str, dtype: torch.dtype):
    """The entry point `name` for activations of `dtype` (what _acts_on_gpu returned)."""
    name = name + "_bf16" if dtype == torch.bfloat16 else name
    return getattr(load(), name), name


def _bn2d_act_fwd(L, x, weight, bias, running_mean, running_var, eps, momentum, slope, residual):
    x = L.map("x", x)
    n = x.shape[1]
    if residual is not None:
        L.map("residual", residual, x.shape)
    _running_pair(running_mean, running_var)
    _norm_vecs(n, weight=weight, bias=bias, running_mean=running_mean, running_var=running_var)
    dtype = _acts_on_gpu(L, x=x, residual=residual)
    _on_gpu(weight=weight, bias=bias, running_mean=running_mean, running_var=running_var)
    dims = L.unit_dims(*x.shape)
    ws = L.workspace(*dims, x.device)       # (validates the shape; one value per channel is the training call's to refuse)
    y = L.empty(x.shape, x.device, dtype)
    save_mean = torch.empty(n, dtype=torch.float32, device=x.device)
    save_invstd = torch.empty(n, dtype=torch.float32, device=x.device)
    fn, name = _entry(L.fwd_train, dtype)
    check(fn(x.data_ptr(), ptr(residual), weight.data_ptr(), bias.data_ptr(), *dims, float(eps), float(momentum), float(slope), y.data_ptr(),
             save_mean.data_ptr(), save_invstd.data_ptr(), ptr(running_mean), ptr(running_var), ws.data_ptr(), ws.numel(), stream_ptr()), name)
    return y, save_mean, save_invstd


def _bn2d_act_eval(L, x, weight, bias, running_mean, running_var, eps, slope, residual):
    x = L.map("x", x)
    if residual is not None:
        L.map("residual", residual, x.shape)
    _norm_vecs(x.shape[1], weight=weight, bias=bias, running_mean=running_mean, running_var=running_var)
    dtype = _acts_on_gpu(L, x=x, residual=residual)
    _on_gpu(weight=weight, bias=bias, running_mean=running_mean, running_var=running_var)
    y = L.empty(x.shape, x.device, dtype)
    fn, name = _entry(L.fwd_eval, dtype)
    check(fn(x.data_ptr(), ptr(residual), weight.data_ptr(), bias.data_ptr(), running_mean.data_ptr(), running_var.data_ptr(),
             *L.unit_dims(*x.shape), float(eps), float(slope), y.data_ptr(), stream_ptr()), name)
    return y


def _bn2d_act_bwd(L, x, y, dy, weight, save_mean, save_invstd, slope, need_dr):
    x = L.map("x", x)
    L.map("y", y, x.shape); L.map("dy", dy, x.shape)
    n = x.shape[1]
    _norm_vecs(n, weight=weight, save_mean=save_mean, save_invstd=save_invstd)
    dtype = _acts_on_gpu(L, x=x, y=y, dy=dy)
    _on_gpu(weight=weight, save_mean=save_mean, save_invstd=save_invstd)
    dims = L.unit_dims(*x.shape)
    ws = L.workspace(*dims, x.device)
    dx = L.empty(x.shape, x.device, dtype)
    dr = L.empty(x.shape, x.device, dtype) if need_dr else None
    dw = torch.empty(n, dtype=torch.float32, device=x.device)
    db = torch.empty(n, dtype=torch.float32, device=x.device)
    fn, name = _entry(L.bwd, dtype)
    check(fn(x.data_ptr(), y.data_ptr(), dy.data_ptr(), weight.data_ptr(), save_mean.data_ptr(), save_invstd.data_ptr(), *dims, float(slope),
             dx.data_ptr(), ptr(dr), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr()), name)
    return dx, dr, dw, db


def _avgpool2d_global_fwd(L, x):
    x = L.map("x", x)
    dtype = _acts_on_gpu(L, x=x)
    y = torch.empty(tuple(x.shape[:2]), dtype=torch.float32, device=x.device)
    fn, name = _entry(L.pool_fwd, dtype)
    check(fn(x.data_ptr(), *L.pool_dims(*x.shape), y.data_ptr(), stream_ptr()), name)
    return y


def _avgpool2d_global_bwd(L, dy, H, W, dtype=torch.float32):
    if dy.dim() != 2 or not dy.is_contiguous():
        raise ValueError(f"dy must be a contiguous matrix [N, C], got shape {tuple(dy.shape)} strides {dy.stride()}")
    _on_gpu(dy=dy)
    shape = tuple(dy.shape) + (int(H), int(W))
    if dtype != torch.float32 and not (L.bf16 and dtype == torch.bfloat16):
        raise ClicaError(f"dx can be float32{' or bfloat16' if L.bf16 else ''}, not {dtype}")
    dx = L.empty(shape, dy.device, dtype)
    fn, name = _entry(L.pool_bwd, dtype)
    check(fn(dy.data_ptr(), *L.pool_dims(*shape), dx.data_ptr(), stream_ptr()), name)
    return dx


def batchnorm2d_act_fwd(x, weight, bias, running_mean=None, running_var=None, eps: float = 1e-5, momentum: float = 0.1,
                        slope: float = 0.0, residual=None):
    """Training BatchNorm2d of contiguous NCHW x (N H W >= 2), plus `residual` when given, then LeakyReLU(slope) (0: ReLU, 1: none) in
    two launches (clica_bn2d_act_fwd_train); running_mean / running_var, when given, are updated in place as nn.BatchNorm2d does.
    Returns (y, save_mean [C], save_invstd [C]); the last two are what batchnorm2d_act_bwd needs."""
    return _bn2d_act_fwd(_NCHW, x, weight, bias, running_mean, running_var, eps, momentum, slope, residual)


def batchnorm2d_act_eval(x, weight, bias, running_mean, running_var, eps: float = 1e-5, slope: float = 0.0, residual=None):
    """Inference BatchNorm2d on the running statistics, plus `residual` when given, then LeakyReLU(slope): one element-wise launch
    (clica_bn2d_act_fwd_eval)."""
    return _bn2d_act_eval(_NCHW, x, weight, bias, running_mean, running_var, eps, slope, residual)


def batchnorm2d_act_bwd(x, y, dy, weight, save_mean, save_invstd, slope: float = 0.0, need_dr: bool = False):
    """(dx, dr, dweight, dbias) of batchnorm2d_act_fwd from its input x, its OUTPUT y (the gate) and the saved statistics: two launches
    (clica_bn2d_act_bwd).  dr, the residual's gradient dy gate(y), is None unless `need_dr`."""
    return _bn2d_act_bwd(_NCHW, x, y, dy, weight, save_mean, save_invstd, slope, need_dr)


def avgpool2d_global_fwd(x):
    """flatten(adaptive_avg_pool2d(x, 1), 1) of contiguous NCHW x: y [N, C], one launch (clica_avgpool2d_global_fwd)."""
    return _avgpool2d_global_fwd(_NCHW, x)


def avgpool2d_global_bwd(dy, H: int, W: int):
    """dx [N, C, H, W] = dy [N, C] / (H W) on every pixel: one launch (clica_avgpool2d_global_bwd)."""
    return _avgpool2d_global_bwd(_NCHW, dy, H, W)


def batchnorm2d_act_fwd_nhwc(x, weight, bias, running_mean=None, running_var=None, eps: float = 1e-5, momentum: float = 0.1,
                             slope: float = 0.0, residual=None):
    """batchnorm2d_act_fwd on a dense channels-last x (N H W >= 2) and residual: two launches (clica_bn2d_nhwc_act_fwd_train).
    Returns (y, save_mean [C], save_invstd [C]), y channels-last.  Anything but dense channels-last maps of one shape and vectors of C
    values: ValueError, before any launch.
    This and the other ``*_nhwc`` functions also take bf16 ACTIVATIONS (x, residual, y, dy, dp) -- all of one call alike, or ClicaError --
    and then run the ``_bf16`` entry points: outputs shaped like x and input gradients are bf16, rounded to nearest even from what the
    fp32 call computes on the upcast activations; parameters, statistics, their gradients and the average pool's [N, C] matrix are fp32."""
    return _bn2d_act_fwd(_NHWC, x, weight, bias, running_mean, running_var, eps, momentum, slope, residual)


def batchnorm2d_act_eval_nhwc(x, weight, bias, running_mean, running_var, eps: float = 1e-5, slope: float = 0.0, residual=None):
    """batchnorm2d_act_eval on a dense channels-last x and residual: one element-wise launch (clica_bn2d_nhwc_act_fwd_eval)."""
    return _bn2d_act_eval(_NHWC, x, weight, bias, running_mean, running_var, eps, slope, residual)


def batchnorm2d_act_bwd_nhwc(x, y, dy, weight, save_mean, save_invstd, slope: float = 0.0, need_dr: bool = False):
    """(dx, dr, dweight, dbias) of batchnorm2d_act_fwd_nhwc from dense channels-last x, y (its OUTPUT: the gate) and dy: two launches
    (clica_bn2d_nhwc_act_bwd).  dx and dr are channels-last; dr is None unless `need_dr`."""
    return _bn2d_act_bwd(_NHWC, x, y, dy, weight, save_mean, save_invstd, slope, need_dr)


def avgpool2d_global_fwd_nhwc(x):
    """flatten(adaptive_avg_pool2d(x, 1), 1) of a dense channels-last x: y [N, C], one launch (clica_avgpool2d_global_nhwc_fwd)."""
    return _avgpool2d_global_fwd(_NHWC, x)


def avgpool2d_global_bwd_nhwc(dy, H: int, W: int, dtype=torch.float32):
    """dx [N, C, H, W], dense channels-last, = dy [N, C] / (H W) on every pixel: one launch (clica_avgpool2d_global_nhwc_bwd).  dy is
    fp32; `dtype` (that of the forward's x: float32 or bfloat16) is dx's."""
    return _avgpool2d_global_bwd(_NHWC, dy, H, W, dtype)


# ------------------------------------------------------------------------------- the stem unit with its max-pool, contiguous NCHW
POOL_LDS_FLOATS = 112 * 112 + 56 * 56 + 56 * 56 // 8      # csrc/bn2d.h kPoolLdsFloats: a plane, its window gradients and argmax nibbles in LDS


def maxpool_out_hw(H: int, W: int):
    """(Ho, Wo) of max-pool 3 / stride 2 / padding 1 in floor mode."""
    return (int(H) - 1) // 2 + 1, (int(W) - 1) // 2 + 1


def bn2d_maxpool_fits(H: int, W: int) -> bool:
    """Is an H x W plane within the limit of clica_bn2d_act_maxpool_*?"""
    Ho, Wo = maxpool_out_hw(H, W)
    return H >= 1 and W >= 1 and H * W + Ho * Wo + (Ho * Wo + 7) // 8 <= POOL_LDS_FLOATS


def bn2d_maxpool_workspace(N: int, C_: int, H: int, W: int, device) -> torch.Tensor:
    """The cached workspace of clica_bn2d_act_maxpool_fwd_train / _bwd for x[N, C, H, W] on `device`."""
    shape = (int(N), int(C_), int(H), int(W))
    return _partial_workspace("pool", shape, device, "clica_bn2d_maxpool_workspace_bytes", shape,
                              f"bn2d + max-pool: no workspace for shape ({N}, {C_}, {H}, {W})")


def batchnorm2d_act_maxpool_fwd(x, weight, bias, running_mean=None, running_var=None, eps: float = 1e-5, momentum: float = 0.1,
                                slope: float = 0.0):
    """max_pool2d(leaky_relu(batch_norm(x), slope), 3, 2, 1) of contiguous NCHW x in training mode, in two launches
    (clica_bn2d_act_maxpool_fwd_train): the activation and the pooling indices are never written.  Running statistics, when given, are
    updated in place.  Returns (p [N, C, Ho, Wo], save_mean [C], save_invstd [C])."""
    x = _bn2d_map("x", x)
    N, n, H, W = x.shape
    _running_pair(running_mean, running_var)
    _norm_vecs(n, weight=weight, bias=bias, running_mean=running_mean, running_var=running_var)
    _on_gpu(x=x, weight=weight, bias=bias, running_mean=running_mean, running_var=running_var)
    ws = bn2d_maxpool_workspace(N, n, H, W, x.device)       # (validates the shape)
    p = torch.empty((N, n) + maxpool_out_hw(H, W), dtype=torch.float32, device=x.device)
    save_mean = torch.empty(n, dtype=torch.float32, device=x.device)
    save_invstd = torch.empty(n, dtype=torch.float32, device=x.device)
    check(load().clica_bn2d_act_maxpool_fwd_train(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), N, n, H, W, float(eps), float(momentum),
                                                  float(slope), p.data_ptr(), save_mean.data_ptr(), save_invstd.data_ptr(),
                                                  ptr(running_mean), ptr(running_var), ws.data_ptr(), ws.numel(), stream_ptr()),
          "clica_bn2d_act_maxpool_fwd_train")
    return p, save_mean, save_invstd


def batchnorm2d_act_maxpool_eval(x, weight, bias, running_mean, running_var, eps: float = 1e-5, slope: float = 0.0):
    """The same on the running statistics (inference): one launch (clica_bn2d_act_maxpool_fwd_eval)."""
    x = _bn2d_map("x", x)
    N, n, H, W = x.shape
    _norm_vecs(n, weight=weight, bias=bias, running_mean=running_mean, running_var=running_var)
    _on_gpu(x=x, weight=weight, bias=bias, running_mean=running_mean, running_var=running_var)
    p = torch.empty((N, n) + maxpool_out_hw(H, W), dtype=torch.float32, device=x.device)
    check(load().clica_bn2d_act_maxpool_fwd_eval(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), running_mean.data_ptr(),
                                                 running_var.data_ptr(), N, n, H, W, float(eps), float(slope), p.data_ptr(), stream_ptr()),
          "clica_bn2d_act_maxpool_fwd_eval")
    return p


def batchnorm2d_act_maxpool_bwd(x, dp, weight, bias, save_mean, save_invstd, slope: float = 0.0):
    """(dx, dweight, dbias) of batchnorm2d_act_maxpool_fwd from its input x, the pooled gradient dp and the saved statistics: two
    launches (clica_bn2d_act_maxpool_bwd); a window's gradient goes to its first maximum in scan order, as torch's does."""
    x = _bn2d_map("x", x)
    N, n, H, W = x.shape
    _bn2d_map("dp", dp, (N, n) + maxpool_out_hw(H, W))
    _norm_vecs(n, weight=weight, bias=bias, save_mean=save_mean, save_invstd=save_invstd)
    _on_gpu(x=x, dp=dp, weight=weight, bias=bias, save_mean=save_mean, save_invstd=save_invstd)
    ws = bn2d_maxpool_workspace(N, n, H, W, x.device)
    dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    dw = torch.empty(n, dtype=torch.float32, device=x.device)
    db = torch.empty(n, dtype=torch.float32, device=x.device)
    check(load().clica_bn2d_act_maxpool_bwd(x.data_ptr(), dp.data_ptr(), weight.data_ptr(), bias.data_ptr(), save_mean.data_ptr(),
                                            save_invstd.data_ptr(), N, n, H, W, float(slope), dx.data_ptr(), dw.data_ptr(), db.data_ptr(),
                                            ws.data_ptr(), ws.numel(), stream_ptr()), "clica_bn2d_act_maxpool_bwd")
    return dx, dw, db


# ------------------------------------------------------------------------------- the stem unit with its max-pool, channels-last
POOL_NHWC_MAX_SIDE = 1 << 15               # csrc/bn2d.h kPoolRowsMaxSide
BN2D_MAX_C = 1 << 20                       # csrc/bn2d.h kMaxC


def bn2d_nhwc_maxpool_fits(H: int, W: int, C_: int) -> bool:
    """Is an H x W plane of C channels within the limits of clica_bn2d_nhwc_act_maxpool_*?  (Its kernels tile the plane: no limit from LDS.)"""
    return 1 <= H <= POOL_NHWC_MAX_SIDE and 1 <= W <= POOL_NHWC_MAX_SIDE and 1 <= C_ <= BN2D_MAX_C


def bn2d_nhwc_maxpool_workspace(N: int, C_: int, H: int, W: int, device) -> torch.Tensor:
    """The cached workspace of clica_bn2d_nhwc_act_maxpool_fwd_train / _bwd for a channels-last x[N, C, H, W] on `device`."""
    shape = (int(N), int(C_), int(H), int(W))
    return _partial_workspace("pool_nhwc", shape, device, "clica_bn2d_nhwc_maxpool_workspace_bytes", shape,
                              f"bn2d + max-pool (channels-last): no workspace for shape ({N}, {C_}, {H}, {W})")


def batchnorm2d_act_maxpool_fwd_nhwc(x, weight, bias, running_mean=None, running_var=None, eps: float = 1e-5, momentum: float = 0.1,
                                     slope: float = 0.0):
    """batchnorm2d_act_maxpool_fwd on a dense channels-last x (N H W >= 2): two launches (clica_bn2d_nhwc_act_maxpool_fwd_train).
    Returns (p [N, C, Ho, Wo] channels-last, save_mean [C], save_invstd [C]); p and the statistics have the bits of
    batchnorm2d_act_fwd_nhwc followed by max_pool2d(., 3, 2, 1).  Anything but a dense channels-last map and vectors of C values:
    ValueError, before any launch."""
    x = _bn2d_nhwc_map("x", x)
    N, n, H, W = x.shape
    _running_pair(running_mean, running_var)
    _norm_vecs(n, weight=weight, bias=bias, running_mean=running_mean, running_var=running_var)
    dtype = _acts_on_gpu(_NHWC, x=x)
    _on_gpu(weight=weight, bias=bias, running_mean=running_mean, running_var=running_var)
    ws = bn2d_nhwc_maxpool_workspace(N, n, H, W, x.device)       # (validates the shape)
    p = _NHWC.empty((N, n) + maxpool_out_hw(H, W), x.device, dtype)
    save_mean = torch.empty(n, dtype=torch.float32, device=x.device)
    save_invstd = torch.empty(n, dtype=torch.float32, device=x.device)
    fn, name = _entry("clica_bn2d_nhwc_act_maxpool_fwd_train", dtype)
    check(fn(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), N, n, H, W, float(eps), float(momentum), float(slope), p.data_ptr(),
             save_mean.data_ptr(), save_invstd.data_ptr(), ptr(running_mean), ptr(running_var), ws.data_ptr(), ws.numel(), stream_ptr()), name)
    return p, save_mean, save_invstd


def batchnorm2d_act_maxpool_eval_nhwc(x, weight, bias, running_mean, running_var, eps: float = 1e-5, slope: float = 0.0):
    """The same on the running statistics (inference): one launch (clica_bn2d_nhwc_act_maxpool_fwd_eval)."""
    x = _bn2d_nhwc_map("x", x)
    N, n, H, W = x.shape
    _norm_vecs(n, weight=weight, bias=bias, running_mean=running_mean, running_var=running_var)
    dtype = _acts_on_gpu(_NHWC, x=x)
    _on_gpu(weight=weight, bias=bias, running_mean=running_mean, running_var=running_var)
    p = _NHWC.empty((N, n) + maxpool_out_hw(H, W), x.device, dtype)
    fn, name = _entry("clica_bn2d_nhwc_act_maxpool_fwd_eval", dtype)
    check(fn(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), running_mean.data_ptr(), running_var.data_ptr(), N, n, H, W, float(eps),
             float(slope), p.data_ptr(), stream_ptr()), name)
    return p


def batchnorm2d_act_maxpool_bwd_nhwc(x, dp, weight, bias, save_mean, save_invstd, slope: float = 0.0):
    """(dx, dweight, dbias) of batchnorm2d_act_maxpool_fwd_nhwc from its input x, the pooled gradient dp (both dense channels-last) and
    the saved statistics: two launches (clica_bn2d_nhwc_act_maxpool_bwd).  dx is channels-last."""
    x = _bn2d_nhwc_map("x", x)
    N, n, H, W = x.shape
    _bn2d_nhwc_map("dp", dp, (N, n) + maxpool_out_hw(H, W))
    _norm_vecs(n, weight=weight, bias=bias, save_mean=save_mean, save_invstd=save_invstd)
    dtype = _acts_on_gpu(_NHWC, x=x, dp=dp)
    _on_gpu(weight=weight, bias=bias, save_mean=save_mean, save_invstd=save_invstd)
    ws = bn2d_nhwc_maxpool_workspace(N, n, H, W, x.device)
    dx = _NHWC.empty(x.shape, x.device, dtype)
    dw = torch.empty(n, dtype=torch.float32, device=x.device)
    db = torch.empty(n, dtype=torch.float32, device=x.device)
    fn, name = _entry("clica_bn2d_nhwc_act_maxpool_bwd", dtype)
    check(fn(x.data_ptr(), dp.data_ptr(), weight.data_ptr(), bias.data_ptr(), save_mean.data_ptr(), save_invstd.data_ptr(), N, n, H, W,
             float(slope), dx.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr()), name)
    return dx, dw, db


def tick(counter: torch.Tensor):
    check(load().clica_tick(counter.data_ptr(), stream_ptr()), "clica_tick")


def _pair_descs(space, marginal, conditional, n, marginal_mean, m_scale, m_p, c_scale, c_p, box, seed, stream_id):
    mk = lambda dist, scale, p, sid: _lib.SamplerDesc(space=SPACE[space], dist=DIST[dist], n=n, box_min=float(box[0]), box_max=float(box[1]),
                                                      scale=float(scale), shape_p=float(p), seed=int(seed) & (2**64 - 1),
                                                      stream_id=int(sid) & 0xFFFFFFFF)
    dm, dc = mk(marginal, m_scale, m_p, stream_id), mk(conditional, c_scale, c_p, stream_id + 1)
    ldmm = 0
    if marginal_mean is not None:
        require_cuda(marginal_mean, "marginal_mean")
        marginal_mean = marginal_mean.reshape(1, -1) if marginal_mean.dim() == 1 else marginal_mean
        marginal_mean, ldmm = rowmajor(marginal_mean.detach())
        if marginal_mean.shape[0] == 1:
            ldmm = 0
    return dm, dc, marginal_mean, ldmm


def sample_pair(space: str, marginal: str, conditional: str, n: int, size: int, z: torch.Tensor, zt: torch.Tensor,
                marginal_mean: Optional[torch.Tensor] = None, m_scale: float = 1.0, m_p: float = 2.0,
                c_scale: float = 1.0, c_p: float = 2.0, box=(0.0, 1.0), seed: int = 0, stream_id: int = 0,
                step_dev: Optional[torch.Tensor] = None):
    """z ~ marginal, zt ~ conditional(. | z) with Philox stream ids `stream_id` and `stream_id + 1` (clica_sample_pair:
    one launch for the coordinate-wise kinds; same numbers as two `sample` calls)."""
    dm, dc, marginal_mean, ldmm = _pair_descs(space, marginal, conditional, n, marginal_mean, m_scale, m_p, c_scale, c_p, box, seed, stream_id)
    check(load().clica_sample_pair(C.byref(dm), C.byref(dc), ptr(marginal_mean), ldmm, z.data_ptr(), z.stride(0), zt.data_ptr(),
                                   zt.stride(0), size, ptr(step_dev), stream_ptr()), "clica_sample_pair")
    return z, zt


def mlp_pack_split16_sample(weights, packed: torch.Tensor, packed_t: torch.Tensor, state, space: str, marginal: str, conditional: str, n: int,
                            size: int, z: torch.Tensor, zt: torch.Tensor, marginal_mean: Optional[torch.Tensor] = None, m_scale: float = 1.0,
                            m_p: float = 2.0, c_scale: float = 1.0, c_p: float = 2.0, box=(0.0, 1.0), seed: int = 0, stream_id: int = 0,
                            step_dev: Optional[torch.Tensor] = None):
    """`mlp_pack_split_both(weights, packed, packed_t, state)` and `sample_pair(...)` in ONE launch (clica_mlp_pack_split16_both_sample):
    the training step's two independent front launches; same results bit for bit.  `packed` / `packed_t` must exist."""
    L = len(weights)
    ws = [_mat(f"weight[{l}]", w) for l, w in enumerate(weights)]
    I32 = C.c_int32 * L
    Ns, Ks = I32(*[w.shape[0] for w, _ in ws]), I32(*[w.shape[1] for w, _ in ws])
    Wp, ldp = (C.c_void_p * L)(*[w.data_ptr() for w, _ in ws]), (C.c_int64 * L)(*[ld for _, ld in ws])
    dm, dc, marginal_mean, ldmm = _pair_descs(space, marginal, conditional, n, marginal_mean, m_scale, m_p, c_scale, c_p, box, seed, stream_id)
    check(load().clica_mlp_pack_split16_both_sample(L, Wp, ldp, Ns, Ks, packed.data_ptr(), packed_t.data_ptr(), state.buf.data_ptr(),
                                                    C.byref(dm), C.byref(dc), ptr(marginal_mean), ldmm, z.data_ptr(), z.stride(0), zt.data_ptr(),
                                                    zt.stride(0), size, ptr(step_dev), stream_ptr()), "clica_mlp_pack_split16_both_sample")
    return packed, packed_t


# ------------------------------------------------------------------------------- nearest neighbours
def nn_search(table: torch.Tensor, query: torch.Tensor, k: int = 1, want_dist: bool = True):
    """Exact k nearest table rows of every query row in squared L2 (clica_nn_search; faiss.IndexFlatL2.search semantics:
    ascending distances, int64 labels).  Returns (dist (Q, k) float32 | None, idx (Q, k) int64)."""
    (tab, ldt), (qry, ldq) = _mat("table", table), _mat("query", query)
    N, n = tab.shape
    Q = qry.shape[0]
    if qry.shape[1] != n:
        raise ValueError(f"query {tuple(qry.shape)} does not match the table {tuple(tab.shape)}")
    nbytes = C.c_size_t()
    check(load().clica_nn_search_workspace_bytes(Q, N, n, int(k), C.byref(nbytes)), "clica_nn_search_workspace_bytes")
    ws = workspace("nn_search", nbytes.value, tab.device)
    idx = torch.empty((Q, k), dtype=torch.int64, device=tab.device)
    dist = torch.empty((Q, k), dtype=torch.float32, device=tab.device) if want_dist else None
    check(load().clica_nn_search(tab.data_ptr(), ldt, N, qry.data_ptr(), ldq, Q, n, int(k), idx.data_ptr(), ptr(dist),
                                 ws.data_ptr(), ws.numel(), stream_ptr()), "clica_nn_search")
    return dist, idx


def kitti_gather_pairs(frames: torch.Tensor, first: torch.Tensor, second: torch.Tensor, latents: Optional[torch.Tensor] = None,
                       image_shape=None):
    """Interleaved float32 image batch [2 B, 1, H, W] (and labels [2 B, n_lat]) of the frame pairs (first[i], second[i]) from a uint8 frame
    table [F, H, W] in HBM (clica_kitti_gather_pairs: kitti_masks/dataset.py:90-142 on the device)."""
    if not frames.is_cuda:
        raise ClicaError(f"frames must live on the GPU (got device {frames.device}); cl_ica_amd runs only through its HIP kernels")
    if frames.dtype != torch.uint8 or not frames.is_contiguous():
        raise ValueError("frames must be a contiguous uint8 tensor [F, ...]")
    F = frames.shape[0]
    elems = frames[0].numel()
    first = first.to(device=frames.device, dtype=torch.int64).contiguous()
    second = second.to(device=frames.device, dtype=torch.int64).contiguous()
    B = first.numel()
    if second.numel() != B or B == 0:
        raise ValueError("first / second must hold the same, non-zero number of frame indices")
    shape = tuple(image_shape) if image_shape is not None else (1,) + tuple(frames.shape[1:])
    images = torch.empty((2 * B,) + shape, dtype=torch.float32, device=frames.device)
    labels = lat = None
    n_lat = 0
    if latents is not None:
        require_cuda(latents, "latents")
        lat = latents.detach().to(torch.float32).contiguous()
        n_lat = lat.shape[1]
        labels = torch.empty((2 * B, n_lat), dtype=torch.float32, device=frames.device)
    check(load().clica_kitti_gather_pairs(frames.data_ptr(), elems, F, first.data_ptr(), second.data_ptr(), B, images.data_ptr(),
                                          ptr(lat), n_lat, ptr(labels), stream_ptr()), "clica_kitti_gather_pairs")
    return images, labels


def kitti_gather_frames(frames: torch.Tensor, frame_ids: torch.Tensor, latents: Optional[torch.Tensor] = None):
    """float32 images [n, 1, H, W] (and labels [n, n_lat]) of the single frames `frame_ids` of a uint8 frame table [F, H, W] in HBM
    (clica_kitti_gather_frames).  Ids handed over on the host are checked against the table here; ids that already live on the device
    are not (that would be a host sync): the kernel clamps them, so an id outside the table gives its nearest frame."""
    if not frames.is_cuda:
        raise ClicaError(f"frames must live on the GPU (got device {frames.device}); cl_ica_amd runs only through its HIP kernels")
    if frames.dtype != torch.uint8 or not frames.is_contiguous():
        raise ValueError("frames must be a contiguous uint8 tensor [F, ...]")
    F = frames.shape[0]
    ids = torch.as_tensor(frame_ids)
    if not ids.is_cuda and ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= F):
        raise ValueError(f"frame_ids must lie in 0 .. {F - 1} (got {int(ids.min())} .. {int(ids.max())})")
    ids = ids.to(device=frames.device, dtype=torch.int64).contiguous()
    n = ids.numel()
    if n == 0 or ids.dim() != 1:
        raise ValueError(f"frame_ids must be a non-empty 1-D list (got shape {tuple(ids.shape)})")
    images = torch.empty((n, 1) + tuple(frames.shape[1:]), dtype=torch.float32, device=frames.device)
    labels = lat = None
    n_lat = 0
    if latents is not None:
        require_cuda(latents, "latents")
        lat = latents.detach().to(torch.float32).contiguous()
        n_lat = lat.shape[1]
        labels = torch.empty((n, n_lat), dtype=torch.float32, device=frames.device)
    check(load().clica_kitti_gather_frames(frames.data_ptr(), frames[0].numel(), F, ids.data_ptr(), n, images.data_ptr(), ptr(lat), n_lat,
                                           ptr(labels), stream_ptr()), "clica_kitti_gather_frames")
    return images, labels


def kitti_sample_pairs(frames: torch.Tensor, latents: Optional[torch.Tensor], cumlens: torch.Tensor, seq_start: torch.Tensor,
                       seq_len: torch.Tensor, order: torch.Tensor, n_pairs: int, max_delta_t: int, seed: int, state: torch.Tensor,
                       images: torch.Tensor, labels: Optional[torch.Tensor] = None, drawn: Optional[torch.Tensor] = None) -> None:
    """The next batch of the KITTI-masks training stream, drawn and gathered by one launch into `images` [2 B, 1, H, W] (and `labels`
    [2 B, n_lat]); `state` (int64 [2]: batch counter, ticket) is advanced by the launch itself (clica_kitti_sample_pairs, include/clica.h).
    `drawn`: optional int64 [4, B] that receives (index, t, first frame, second frame) per pair.  No tensor is allocated or converted
    here: every argument is a device buffer the caller owns, so the call is capture-safe."""
    for name, t, dt in (("frames", frames, torch.uint8), ("cumlens", cumlens, torch.int64), ("seq_start", seq_start, torch.int64),
                        ("seq_len", seq_len, torch.int64), ("order", order, torch.int64), ("state", state, torch.int64),
                        ("images", images, torch.float32), ("labels", labels, torch.float32), ("latents", latents, torch.float32),
                        ("drawn", drawn, torch.int64)):
        if t is None and name in ("labels", "latents", "drawn"):
            continue
        if not (torch.is_tensor(t) and t.is_cuda):
            raise ClicaError(f"{name} must live on the GPU; cl_ica_amd runs only through its HIP kernels")
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} tensor (got {t.dtype}, contiguous={t.is_contiguous()})")
    B, elems, n_seq, n_items = int(n_pairs), frames[0].numel(), cumlens.numel(), order.numel()
    n_lat = latents.shape[1] if latents is not None else 0
    if seq_start.numel() != n_seq or seq_len.numel() != n_seq or state.numel() < 2:
        raise ValueError("cumlens / seq_start / seq_len must have one entry per sequence and state two words")
    if B >= 1 and images.numel() != 2 * B * elems:
        raise ValueError(f"images holds {images.numel()} values for {B} pairs of {elems} pixels")
    if labels is not None and (latents is None or labels.numel() != 2 * B * n_lat):
        raise ValueError(f"labels must hold 2 x {B} x {n_lat} values and needs a latent table")
    if drawn is not None and tuple(drawn.shape) != (4, max(B, 0)):
        raise ValueError(f"drawn must be int64 [4, {B}]")
    outs = [drawn[k].data_ptr() for k in range(4)] if drawn is not None else [None] * 4
    check(load().clica_kitti_sample_pairs(frames.data_ptr(), elems, frames.shape[0], ptr(latents), n_lat, cumlens.data_ptr(),
                                          seq_start.data_ptr(), seq_len.data_ptr(), n_seq, n_items, order.data_ptr(), B, int(max_delta_t),
                                          int(seed) & (2 ** 64 - 1), state.data_ptr(), images.data_ptr(), ptr(labels), *outs, stream_ptr()),
          "clica_kitti_sample_pairs")


def _image_table(table: torch.Tensor) -> Tuple[int, int, int, int]:
    if not torch.is_tensor(table):
        raise ValueError("table must be a uint8 tensor [N, H, W, C]")
    if not table.is_cuda:
        raise ClicaError(f"table must live on the GPU (got device {table.device}); cl_ica_amd runs only through its HIP kernels")
    if table.dtype != torch.uint8 or not table.is_contiguous() or table.dim() != 4:
        raise ValueError(f"table must be a contiguous uint8 tensor [N, H, W, C] (got {table.dtype}, shape {tuple(table.shape)})")
    N, H, W, Cn = table.shape
    if N == 0 or H == 0 or W == 0:
        raise ValueError(f"table of shape {tuple(table.shape)} holds no pixels")
    if not 1 <= Cn <= 4:
        raise ValueError(f"table has C={Cn} channels (1..4 supported)")
    return N, H, W, Cn


def _host_floats(name: str, v, n: int):
    v = v.detach().cpu().tolist() if torch.is_tensor(v) else list(v)
    if len(v) != n:
        raise ValueError(f"{name} has {len(v)} entries for C={n} channels")
    return (C.c_float * n)(*[float(e) for e in v])


IMAGE_LAYOUTS = {torch.contiguous_format: 0, torch.channels_last: 1}      # enum clica_image_layout
IMAGE_DTYPES = {torch.float32: 0, torch.bfloat16: 1}                      # enum clica_image_dtype


def image_format_args(memory_format=torch.contiguous_format, dtype=torch.float32) -> Tuple[int, int]:
    """(layout, dtype) codes of clica_image_gather_norm_ex for an image batch's `memory_format` / `dtype`, or ``ValueError``."""
    if memory_format not in IMAGE_LAYOUTS:
        raise ValueError(f"memory_format={memory_format!r} (torch.contiguous_format or torch.channels_last)")
    if dtype not in IMAGE_DTYPES:
        raise ValueError(f"dtype={dtype!r} (torch.float32 or torch.bfloat16)")
    return IMAGE_LAYOUTS[memory_format], IMAGE_DTYPES[dtype]


def image_gather_norm(table: torch.Tensor, index: torch.Tensor, mean=None, std=None, out: Optional[torch.Tensor] = None, *,
                      memory_format=torch.contiguous_format, dtype=torch.float32) -> torch.Tensor:
    """Batch of logical shape [len(index), C, H, W] of the rows `index` of a uint8 image table [N, H, W, C] in HBM, one launch
    (clica_image_gather_norm / _ex): ``((v / 255) - mean[c]) / std[c]``, torchvision's ToTensor + Normalize (main_3dident.py:787-796) as
    three correctly rounded fp32 operations; ``mean is std is None``: ToTensor alone.  `mean` / `std` are host sequences of C numbers,
    read at the call.  `memory_format`: ``torch.contiguous_format`` (NCHW) or ``torch.channels_last`` (dense channels-last, what
    ``x.contiguous(memory_format=torch.channels_last)`` gives); `dtype`: ``torch.float32`` or ``torch.bfloat16`` (the fp32 value narrowed
    once at the store, what ``x.to(torch.bfloat16)`` gives).  `out`: a buffer of that shape, layout, dtype and device to write into, else
    ``ValueError`` (a captured graph keeps its buffer; `index` is then read on replay).  The default format on a 16-byte aligned `out`
    (every fresh tensor) is clica_image_gather_norm's launch as before; an `out` view that is only element-aligned, which that entry
    point refuses, is served by clica_image_gather_norm_ex's scalar instance in every format, the default one included (same bits)."""
    N, H, W, Cn = _image_table(table)
    layout, dt = image_format_args(memory_format, dtype)
    if (mean is None) != (std is None):
        raise ValueError("mean and std must be given together")
    m = s = None
    if mean is not None:
        m, s = _host_floats("mean", mean, Cn), _host_floats("std", std, Cn)
    if not (torch.is_tensor(index) and index.device == table.device and index.dtype == torch.int64 and index.is_contiguous()):
        index = torch.as_tensor(index).to(device=table.device, dtype=torch.int64).contiguous()
    n = index.numel()
    if n == 0 or index.dim() != 1:
        raise ValueError(f"index must be a non-empty 1-D list of rows (got shape {tuple(index.shape)})")
    if out is None:
        out = torch.empty((n, Cn, H, W), dtype=dtype, device=table.device, memory_format=memory_format)
    else:
        if (not torch.is_tensor(out) or tuple(out.shape) != (n, Cn, H, W) or out.dtype != dtype or out.device != table.device
                or not out.is_contiguous(memory_format=memory_format)):
            got = f"{out.dtype} {tuple(out.shape)}, strides {tuple(out.stride())}, on {out.device}" if torch.is_tensor(out) else type(out).__name__
            raise ValueError(f"out must be a {dtype} tensor {(n, Cn, H, W)}, dense in {memory_format}, on {table.device} (got {got})")
    if layout == 0 and dt == 0 and out.data_ptr() % 16 == 0:      # (the one alignment the first entry point accepts for every shape)
        check(load().clica_image_gather_norm(table.data_ptr(), N, H, W, Cn, index.data_ptr(), n, m, s, out.data_ptr(), stream_ptr()),
              "clica_image_gather_norm")
    else:
        check(load().clica_image_gather_norm_ex(table.data_ptr(), N, H, W, Cn, index.data_ptr(), n, m, s, out.data_ptr(), layout, dt,
                                                stream_ptr()), "clica_image_gather_norm_ex")
    return out


def image_channel_sums(table: torch.Tensor) -> torch.Tensor:
    """Exact integer sums per image and channel of a uint8 table [N, H, W, C] (clica_image_channel_stats): int64 [N, C, 2] on the device,
    ``[..., 0]`` = sum of the bytes, ``[..., 1]`` = sum of their squares (the data pass of tools/3dident/get_mean_std.py)."""
    N, H, W, Cn = _image_table(table)
    sums = torch.empty((N, Cn, 2), dtype=torch.int64, device=table.device)      # (uint64 in the ABI; the sums stay far below 2^63)
    check(load().clica_image_channel_stats(table.data_ptr(), N, H, W, Cn, sums.data_ptr(), stream_ptr()), "clica_image_channel_stats")
    return sums


def moments(a: torch.Tensor, b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """G = [a | b | 1]^T [a | b | 1] in fp64 (clica_moments): the (da + db + 1)^2 second-moment matrix every disentanglement score is a
    function of (cl_ica_amd/disentanglement_utils.py).  a [M, da], b [M, db] fp32 on the device; returns a device fp64 tensor."""
    (a, lda) = _mat("a", a)
    M, da = a.shape
    db, ldb, bp = 0, 0, None
    if b is not None:
        (b, ldb) = _mat("b", b)
        if b.shape[0] != M:
            raise ValueError(f"row counts differ: {tuple(a.shape)} vs {tuple(b.shape)}")
        db, bp = b.shape[1], b.data_ptr()
    d = da + db + 1
    if d > 129:
        # wider than one launch of the kernel covers (2 n + 1 <= 129, i.e. n <= 64): the same kernel over 64-column blocks of
        # X = [a | b], G[I, J] = X_I^T X_J from the cross block of the launch on (X_I, X_J), sums from its last column
        X = [(a, c0, min(c0 + 64, da)) for c0 in range(0, da, 64)] + ([(b, c0, min(c0 + 64, db)) for c0 in range(0, db, 64)] if b is not None else [])
        offs, o = [], 0
        for (_, c0, c1) in X:
            offs.append(o); o += c1 - c0
        G = torch.empty((d, d), dtype=torch.float64, device=a.device)
        G[-1, -1] = float(M)
        for i, (ti, i0, i1) in enumerate(X):
            for j in range(i, len(X)):
                tj, j0, j1 = X[j]
                blk = moments(ti[:, i0:i1], tj[:, j0:j1])
                ni, nj = i1 - i0, j1 - j0
                G[offs[i]:offs[i] + ni, offs[j]:offs[j] + nj] = blk[:ni, ni:ni + nj]
                G[offs[j]:offs[j] + nj, offs[i]:offs[i] + ni] = blk[:ni, ni:ni + nj].t()
                if j == i:
                    G[offs[i]:offs[i] + ni, offs[i]:offs[i] + ni] = blk[:ni, :ni]
                    G[offs[i]:offs[i] + ni, -1] = blk[:ni, -1]
                    G[-1, offs[i]:offs[i] + ni] = blk[-1, :ni]
        return G
    nbytes = C.c_size_t()
    check(load().clica_moments_workspace_bytes(M, d, C.byref(nbytes)), "clica_moments_workspace_bytes")
    ws = workspace("moments", nbytes.value, a.device)
    out = torch.empty((d, d), dtype=torch.float64, device=a.device)
    check(load().clica_moments(a.data_ptr(), lda, da, bp, ldb, db, M, out.data_ptr(), ws.data_ptr(), ws.numel(), stream_ptr()), "clica_moments")
    return out


SPACE = {"real": 0, "box": 1, "sphere": 2}
DIST = {"uniform": 0, "normal": 1, "laplace": 2, "gennorm": 3, "vmf": 4}


def sample(space: str, dist: str, n: int, size: int, device, mean: Optional[torch.Tensor] = None,
           scale: float = 1.0, shape_p: float = 2.0, box=(0.0, 1.0), seed: int = 0, stream_id: int = 0,
           step_dev: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
           scale_vec: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`scale_vec`: optional (n,), (1, n) or (size, n) tensor of per-coordinate scales multiplying `scale` (clica_sample_scaled)."""
    d = _lib.SamplerDesc(space=SPACE[space], dist=DIST[dist], n=n, box_min=float(box[0]), box_max=float(box[1]),
                         scale=float(scale), shape_p=float(shape_p), seed=int(seed) & (2**64 - 1),
                         stream_id=int(stream_id) & 0xFFFFFFFF)
    ldm = 0
    if mean is not None:
        require_cuda(mean, "mean")
        if mean.dim() == 1:
            mean = mean.reshape(1, -1)
        mean, ldm = rowmajor(mean.detach())
        if mean.shape[0] == 1:
            ldm = 0
        elif mean.shape[0] != size:
            raise ValueError(f"mean has {mean.shape[0]} rows, expected 1 or {size}")
    o = out if out is not None else torch.empty((size, n), dtype=torch.float32, device=device)
    if scale_vec is not None:
        require_cuda(scale_vec, "scale_vec")
        sv = scale_vec.detach().to(torch.float32)
        sv = sv.reshape(1, -1) if sv.dim() == 1 else sv
        if sv.dim() != 2 or sv.shape[1] != n or sv.shape[0] not in (1, size):
            raise ValueError(f"scale tensor of shape {tuple(scale_vec.shape)}: expected ({n},), (1, {n}) or ({size}, {n})")
        sv, lds = rowmajor(sv)
        check(load().clica_sample_scaled(C.byref(d), ptr(mean), ldm, sv.data_ptr(), 0 if sv.shape[0] == 1 else lds, o.data_ptr(),
                                         o.stride(0), size, ptr(step_dev), stream_ptr()), "clica_sample_scaled")
        return o
    check(load().clica_sample(C.byref(d), ptr(mean), ldm, o.data_ptr(), o.stride(0), size, ptr(step_dev), stream_ptr()),
          "clica_sample")
    return o
