"""Every conv-stage entry point of the C ABI on its own, through ctypes, against the fp64 oracle of tests/conv_stage_oracle.py
(torch.nn.functional.conv2d in float64 and its autograd, carried into the kernels' layouts): csrc/conv16.hip (f16x2) and the conv
section of csrc/linear.hip (fp32).  tests/test_gpu_conv.py drives the same kernels through conv_stack() at ONE geometry (64 x 64,
32/32/64/64 channels), where launch_conv16 only ever picks fwd_tile16_k and stream16_k and every grid is square; here each row of
the tables names the kernel its shape is meant to reach (read from the dispatch conditions: whoever changes the dispatch updates the
table), hs != ws throughout, and per case:

  values      PARITY.check at 1e-5 against fp64 for the whole tensor AND for the border ring alone (first / last output row and column;
              first / last valid row and column of dPrev); weight gradients per (dy, dx) block as well
  gate bits   forward: every written word == (stored output > 0) exactly; data gradient: words supplied by the test
  footprint   destinations, gate arrays and workspaces sit between 4 KB guard zones, everything pre-filled with a finite sentinel and
              compared bit for bit afterwards: padding slots of the next S, non-output rows, dPrev outside its valid part, the zero tail
  contract    memory behind S's zero tail and in front of dO's zero rows is NaN (same allocation): a kernel that consumes it shows NaN
  maxima      conv16: the output's 256 slots hold exactly the float bits of max |stored output|; amax_in comes from clica_conv16_amax

Primary inputs are one-signed (the sums do not cancel; one zero-mean case per weight-gradient entry point, whose allowance -- if ATen's own
fp32 convolution misses 1e-5 against fp64 on the same data -- is 4 x that measured error, passed as tol= with a note).  The forward's bias
puts the ReLU's edge through the middle of the outputs; ReLU outputs are compared by value, no element is excluded anywhere.

The table keys name the conv16 kernel (launch_conv16: fwd_tile16_k for the 32 -> 32 stage on a 16-wide output grid with hs - 1 a multiple
of 8; stream16_k where N % 32 == 0, K % 128 == 0, the run length % 32 == 0 and the weight columns fit LDS in 1, 2 or 4 blocks; gemm16_k
otherwise -- Cout = 96, C = 128, data gradients with Cout = 8 / 16 / 24).  The fp32 entry points take the same rows through conv_gemm_k's
128 x 32 / 128 x 64 / 64 x 128 / 64 x 64 tiles by Cout (ragged at Cout = 20 and 96), the data gradient through the tiled kernel below
2048 rows of the 32 <- 32 stage and conv_dgrad32_stream_k from there on.  Dummy-pointer refusal checks live in tests/test_cabi_symbols.py.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_stage_oracle as O
from conftest import PARITY

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 1024                                  # 4-byte elements: 4 KB on either side
SENT = -12345.678
SENT_BITS = int(np.float32(SENT).view(np.int32))
SENT_WORD = 0x5A5A5A5A
E_INVALID, E_WORKSPACE = -1, -2
SLOTS = 256


def _lib():
    from cl_ica_amd import _lib
    return _lib.load()


def _st():
    from cl_ica_amd._lib import stream_ptr
    return stream_ptr()


def _ok(rc, what):
    assert rc == 0, (what, rc, _lib().clica_last_error())


class Guarded:
    """`n` elements between two guard zones, all pre-filled with the sentinel."""

    def __init__(self, n, dtype=torch.float32, fill=None):
        g = GUARD if dtype != torch.uint8 else 4 * GUARD
        self.g, self.n = g, n
        self.whole = torch.empty(n + 2 * g, dtype=dtype, device=DEV)
        if dtype == torch.float32:
            self.whole.fill_(SENT); self.bits = SENT_BITS
        elif dtype == torch.int32:
            self.whole.fill_(SENT_WORD); self.bits = SENT_WORD
        else:
            self.whole.fill_(0x5A); self.bits = 0x5A
        self.t = self.whole[g:g + n]
        if fill is not None:
            self.t.copy_(fill)

    def ptr(self):
        return self.t.data_ptr()

    def raw(self, t=None):
        t = self.whole if t is None else t
        return t.view(torch.int32) if t.dtype == torch.float32 else t

    def untouched(self, t):
        return bool((self.raw(t) == self.bits).all())

    def guards_intact(self):
        return self.untouched(self.whole[:self.g]) and self.untouched(self.whole[self.g + self.n:])


def _fenced(flat):
    """An input operand with NaN on both sides, inside the same allocation.  Returns (keep-alive, view)."""
    whole = torch.full((flat.numel() + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    whole[GUARD:GUARD + flat.numel()] = flat
    return whole, whole[GUARD:GUARD + flat.numel()]


def _words32(w64):
    """int64 words in [0, 2^32) -> the int32 storage the kernels read."""
    return torch.where(w64 >= 2 ** 31, w64 - 2 ** 32, w64).to(torch.int32)


def _pack16(mats, maps=None):
    """clica_conv16_pack of fp32 matrices (contiguous, on the GPU): ([hi plane | lo plane] int16 per matrix, scales)."""
    n = len(mats)
    maps = maps or [None] * n
    counts = [m.numel() if mp is None else mp.numel() for m, mp in zip(mats, maps)]
    dst = [torch.empty(2 * c, dtype=torch.int16, device=DEV) for c in counts]
    scales = torch.zeros(n, dtype=torch.float32, device=DEV)
    VP, I32 = C.c_void_p * n, C.c_int32 * n
    _ok(_lib().clica_conv16_pack(n, VP(*[m.data_ptr() for m in mats]), I32(*[m.numel() for m in mats]),
                                 VP(*[None if mp is None else mp.data_ptr() for mp in maps]), VP(*[d.data_ptr() for d in dst]),
                                 I32(*counts), scales.data_ptr(), _st()), "clica_conv16_pack")
    return dst, scales


def _slots(k):
    s = torch.full((k * SLOTS,), 0x7F, dtype=torch.int32, device=DEV)           # (zero_slots must clear them)
    _ok(_lib().clica_conv16_zero_slots(s.data_ptr(), k, _st()), "clica_conv16_zero_slots")
    return s


def _amax_into(t, slots, i):
    _ok(_lib().clica_conv16_amax(t.data_ptr(), t.numel(), slots.data_ptr() + 4 * SLOTS * i, _st()), "clica_conv16_amax")


def _max_bits(t):
    return int(t.abs().max().to(torch.float32).view(torch.int32)) if t.numel() else 0


def _check_values(family, case, what, got, ref, ring, tol=None, note=None):
    """Whole tensor, then the border ring alone under its own norm.  `ring`: bool mask over the last two (spatial) dimensions."""
    kw = {} if tol is None else dict(tol=tol, note=note)
    PARITY.check(family, case, what, got.cpu().numpy(), ref.cpu().numpy(), **kw)
    PARITY.check(family, case, what + " (border ring)", got[..., ring].cpu().numpy(), ref[..., ring].cpu().numpy(), **kw)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------------ forward
# (images, C, Cout, hs, ws, scatter)
FWD = {
    "tile16 1 tile per image": (1, 32, 32, 9, 17, 1),
    "tile16 2 tiles per image": (3, 32, 32, 17, 17, 1),
    "tile16 3 tiles per image": (2, 32, 32, 25, 17, 1),
    "tile16 260 tiles > 256 workgroups": (130, 32, 32, 17, 17, 1),
    "stream16 32->64 9x9": (5, 32, 64, 9, 9, 1),
    "stream16 64->64 5x5 rows": (5, 64, 64, 5, 5, 2),
    "stream16 32->32 17x17 rows": (3, 32, 32, 17, 17, 2),
    "stream16 odd 3x6 grid, 18 rows": (1, 8, 128, 4, 7, 2),
    "stream16 16->64 3x9": (2, 16, 64, 3, 9, 1),
    "stream16 24->32 5x3": (7, 24, 32, 5, 3, 1),
    "stream16 more 32-row tiles than resident waves": (520, 32, 32, 17, 17, 2),
    "gemm16 64x128 tile, N = 96": (3, 8, 96, 5, 9, 1),
    "gemm16 128x32 tile, K = 2048": (2, 128, 32, 5, 5, 1),
    "gemm16 64x64 tile, rows": (2, 128, 64, 5, 5, 2),
    "gemm16 one row": (1, 8, 96, 2, 2, 2),
    "gemm16 128x64 tile (65536 rows)": (256, 128, 64, 17, 17, 1),
}
# fp32 entry point only: no gate bits possible (Cout % 32), ragged N tile
FWD_F32_ONLY = {
    "f32 C=4 Cout=20 ragged tile": (3, 4, 20, 5, 9, 1),
    "f32 C=4 Cout=20 rows": (3, 4, 20, 4, 7, 2),
}
FWD_SCALES = ["tile16 2 tiles per image", "stream16 32->64 9x9", "gemm16 64x128 tile, N = 96"]


def _fwd_inputs(shape, xscale, seed):
    images, Cc, Cout, hs, ws, scatter = shape
    H, W = 2 * (hs - 1), 2 * (ws - 1)
    g = _gen(seed)
    # one-signed: the sums do not cancel.  A pixel mask shared by the channels spreads a channel's pre-activations by ~ 15 % of their
    # mean, so that the bias below puts the ReLU's edge through the middle of most channels
    x = (torch.rand(images, Cc, H, W, generator=g) * (torch.rand(images, 1, H, W, generator=g) > 0.3) * xscale).to(DEV)
    w = ((torch.rand(Cout, Cc, 4, 4, generator=g) + 0.05) / (8 * Cc)).to(DEV)
    z0 = O.stage_reference(x, w, relu=False)["pre"]
    u = (0.8 + 0.4 * torch.rand(Cout, generator=g)).to(DEV)
    b = (-(z0.mean((0, 2, 3))) * u.double()).float()                                # about half of every channel's outputs below zero
    ref = torch.relu(z0 + b.double().view(1, -1, 1, 1))
    return x, w, b, ref


def _run_fwd(arith, name, shape, xscale=1.0):
    from cl_ica_amd import conv
    images, Cc, Cout, hs, ws, scatter = shape
    ho, wo = hs - 1, ws - 1
    x, w, b, ref = _fwd_inputs(shape, xscale, seed=1000 + 7 * hs + ws + Cc + Cout)
    S_keep, S = _fenced(O.s_flat(x).float())
    Wg = conv._wg(w).contiguous()
    if scatter == 1:
        dhs, dws = ho // 2 + 1, wo // 2 + 1
        n_out = images * dhs * dws * 4 * Cout
        out = Guarded(n_out + (dws + 2) * 4 * Cout)                                   # the next stage's S, zero tail included
    else:
        out = Guarded(images * hs * ws * Cout)
    gate = Guarded(images * hs * ws * (Cout // 32), torch.int32) if scatter == 1 and Cout % 32 == 0 else None
    entry = "clica_conv16_k4s2_fwd" if arith == "f16x2" else "clica_conv_k4s2_fwd"
    if arith == "f16x2":
        (w16,), wscale = _pack16([Wg])
        slots = _slots(2)
        _amax_into(S, slots, 0)
        _ok(_lib().clica_conv16_k4s2_fwd(S.data_ptr(), w16.data_ptr(), wscale.data_ptr(), b.data_ptr(), images, Cc, Cout, hs, ws, 1, scatter,
                                         out.ptr(), gate.ptr() if gate else None, slots.data_ptr(), slots.data_ptr() + 4 * SLOTS, _st()), entry)
    else:
        _ok(_lib().clica_conv_k4s2_fwd(S.data_ptr(), Wg.data_ptr(), b.data_ptr(), images, Cc, Cout, hs, ws, 1, scatter, out.ptr(),
                                       gate.ptr() if gate else None, _st()), entry)
    torch.cuda.synchronize()
    case = f"{name} {shape}" + (f" xscale={xscale:g}" if xscale != 1.0 else "")
    assert out.guards_intact(), case
    if scatter == 1:
        Sn = out.t[:n_out].view(images, dhs, dws, 4 * Cout)
        got, ring_cells = O.depth_to_space(Sn, Cout)
        assert out.untouched(ring_cells), f"{case}: a padding slot of the next S was written"
        assert out.untouched(out.t[n_out:]), f"{case}: the next S's zero tail was written"
    else:
        grid = out.t.view(images, hs, ws, Cout)
        got = O.from_grid(grid)
        assert out.untouched(grid[:, ho]) and out.untouched(grid[:, :, wo]), f"{case}: a non-output row was written"
    assert float(ref.max()) > 0 and 0.2 < float((ref > 0).double().mean()) < 0.8, case            # the ReLU really gates
    _check_values(f"conv_stage/{entry}", case, "output", got, ref, O.border_mask(ho, wo, DEV))
    assert bool((got >= 0).all())
    if gate is not None:
        assert gate.guards_intact(), case
        words = gate.t.view(images, hs, ws, Cout // 32)
        want = O.pack_bits(got.permute(0, 2, 3, 1) > 0)
        assert torch.equal(words[:, :ho, :wo].to(torch.int64) & 0xFFFFFFFF, want), f"{case}: gate words != (stored output > 0)"
        assert gate.untouched(words[:, ho]) and gate.untouched(words[:, :, wo]), f"{case}: a gate word of a non-output row was written"
    if arith == "f16x2":
        assert int(slots[SLOTS:].max()) == _max_bits(got), f"{case}: output maximum slots"
        assert int(slots[:SLOTS].max()) == _max_bits(S), f"{case}: clica_conv16_amax of S"


@pytest.mark.parametrize("arith", ["f16x2", "f32"])
@pytest.mark.parametrize("name", list(FWD))
def test_fwd(arith, name):
    _run_fwd(arith, name, FWD[name])


@pytest.mark.parametrize("name", list(FWD_F32_ONLY))
def test_fwd_f32_ragged(name):
    _run_fwd("f32", name, FWD_F32_ONLY[name])


@pytest.mark.parametrize("xscale", [1e-6, 3e4])
@pytest.mark.parametrize("name", FWD_SCALES)
def test_fwd_scale_extremes(name, xscale):
    """fp16 alone would flush 1e-6 and overflow at 3e4: the per-tensor power-of-two scale from the recorded maximum carries both."""
    _run_fwd("f16x2", name, FWD[name], xscale=xscale)


# ------------------------------------------------------------------------------------------------------------ data gradient
# (images, C, Cout, hs, ws, dhs, dws)
DGRAD = {
    "stream16 32<-32 17x17": (5, 32, 32, 17, 17, 32, 32),
    "stream16 32<-64 9x9": (5, 32, 64, 9, 9, 17, 17),
    "stream16 64<-64 5x5": (5, 64, 64, 5, 5, 9, 9),
    "stream16 96<-32 2x2, N split over 3": (1, 96, 32, 2, 2, 2, 2),
    "stream16 wrap": (240, 32, 32, 17, 17, 32, 32),
    "gemm16 Cout = 16": (3, 32, 16, 4, 6, 7, 12),
    "gemm16 Cout = 8, single k-tile": (2, 32, 8, 3, 3, 4, 5),
    "gemm16 Cout = 24, C = 64": (2, 64, 24, 5, 4, 8, 7),
}
DGRAD_F32_ONLY = {
    "f32 Cout = 4, non-fast operand path, no gate": (3, 8, 4, 4, 6, 6, 11),
    "f32 7 images: tiled kernel below 2048 rows": (7, 32, 32, 17, 17, 32, 32),
    "f32 8 images: persistent kernel from 2048 rows": (8, 32, 32, 17, 17, 32, 32),
}
DGRAD_SCALES = ["stream16 32<-64 9x9", "gemm16 Cout = 16"]


def _run_dgrad(arith, name, shape, gates="random", gscale=1.0):
    from cl_ica_amd import conv
    images, Cc, Cout, hs, ws, dhs, dws = shape
    ho, wo = hs - 1, ws - 1
    H, W = 2 * ho, 2 * wo
    g = _gen(2000 + 5 * hs + ws + Cc + Cout)
    dout = ((torch.rand(images, Cout, ho, wo, generator=g) + 0.1) * gscale).to(DEV)
    w = ((torch.rand(Cout, Cc, 4, 4, generator=g) + 0.05) / (4 * Cout)).to(DEV)
    dx = O.stage_reference(torch.zeros(images, Cc, H, W, device=DEV), w, None, dout)["dx"]
    use_gate = Cc % 32 == 0
    if gates == "random":
        bits = (torch.rand(images, dhs, dws, Cc, generator=g) > 0.4).to(DEV)
    else:
        bits = torch.full((images, dhs, dws, Cc), gates == "ones", dtype=torch.bool, device=DEV)
    if not use_gate:
        bits = torch.ones_like(bits)
    ref = dx.permute(0, 2, 3, 1) * bits[:, :H, :W].double()                       # [img][y][x][c]
    d_keep, dfl = _fenced(O.dO_flat(dout).float())
    dO = dfl[(ws + 1) * Cout:]
    words = _words32(O.pack_bits(bits)).contiguous() if use_gate else None
    dprev = Guarded(images * dhs * dws * Cc)
    entry = "clica_conv16_k4s2_dgrad" if arith == "f16x2" else "clica_conv_k4s2_dgrad"
    if arith == "f16x2":
        (w16,), wscale = _pack16([conv._wd(w).t().contiguous()])
        slots = _slots(2)
        _amax_into(dO, slots, 0)
        _ok(_lib().clica_conv16_k4s2_dgrad(dO.data_ptr(), w16.data_ptr(), wscale.data_ptr(), images, Cc, Cout, hs, ws, dprev.ptr(), dhs, dws,
                                           words.data_ptr(), slots.data_ptr(), slots.data_ptr() + 4 * SLOTS, _st()), entry)
    else:
        Wd = conv._wd(w).contiguous()
        _ok(_lib().clica_conv_k4s2_dgrad(dO.data_ptr(), Wd.data_ptr(), None, images, Cc, Cout, hs, ws, dprev.ptr(), dhs, dws,
                                         words.data_ptr() if use_gate else None, _st()), entry)
    torch.cuda.synchronize()
    case = f"{name} {shape} gates={gates if use_gate else 'none'}" + (f" gscale={gscale:g}" if gscale != 1.0 else "")
    assert dprev.guards_intact(), case
    grid = dprev.t.view(images, dhs, dws, Cc)
    assert dprev.untouched(grid[:, H:]) and dprev.untouched(grid[:, :, W:]), f"{case}: dPrev written outside its valid 2(hs-1) x 2(ws-1) part"
    got = grid[:, :H, :W]
    assert bool(torch.isfinite(got).all()), f"{case}: non-finite values (memory outside the contract consumed?)"
    _check_values(f"conv_stage/{entry}", case, "dPrev", got.permute(0, 3, 1, 2), ref.permute(0, 3, 1, 2), O.border_mask(H, W, DEV))
    if gates == "zeros" and use_gate:
        assert not bool(got.any())
    if arith == "f16x2":
        assert int(slots[SLOTS:].max()) == _max_bits(got), f"{case}: output maximum slots"
        assert int(slots[:SLOTS].max()) == _max_bits(dO), f"{case}: clica_conv16_amax of dO"


@pytest.mark.parametrize("arith", ["f16x2", "f32"])
@pytest.mark.parametrize("name", list(DGRAD))
def test_dgrad(arith, name):
    _run_dgrad(arith, name, DGRAD[name])


@pytest.mark.parametrize("arith", ["f16x2", "f32"])
@pytest.mark.parametrize("gates", ["ones", "zeros"])
@pytest.mark.parametrize("name", ["stream16 32<-64 9x9", "gemm16 Cout = 16"])
def test_dgrad_gate_patterns(arith, name, gates):
    _run_dgrad(arith, name, DGRAD[name], gates=gates)


@pytest.mark.parametrize("name", list(DGRAD_F32_ONLY))
def test_dgrad_f32_paths(name):
    _run_dgrad("f32", name, DGRAD_F32_ONLY[name])


@pytest.mark.parametrize("gscale", [1e-18, 1e12])
@pytest.mark.parametrize("name", DGRAD_SCALES)
def test_dgrad_scale_extremes(name, gscale):
    _run_dgrad("f16x2", name, DGRAD[name], gscale=gscale)


# ---------------------------------------------------------------------------------------------------------- weight gradient
# (images, C, Cout, hs, ws)
WGRAD = {
    "model stage 2": (5, 32, 32, 17, 17),
    "model stage 3": (5, 32, 64, 9, 9),
    "model stage 4": (5, 64, 64, 5, 5),
    "7 contraction rows": (1, 32, 32, 2, 2),
    "three column tiles, 4x7": (3, 96, 64, 4, 7),
    "174 images: split count above the old bound": (174, 32, 32, 17, 17),
    "1000 images 9x9: split count above the old bound": (1000, 32, 64, 9, 9),
}
WGRAD_F32_ONLY = {
    "f32 C=4 Cout=20 ragged": (3, 4, 20, 5, 9),
    "f32 C=8 Cout=96": (3, 8, 96, 4, 7),
}


def _wgrad_call(arith, dO, S, images, Cc, Cout, hs, ws, dWg_ptr, db_ptr, accumulate, slots, ws_ptr, ws_bytes):
    if arith == "f16x2":
        return _lib().clica_conv16_k4s2_wgrad(dO.data_ptr(), S.data_ptr(), images, Cc, Cout, hs, ws, dWg_ptr, db_ptr, accumulate,
                                              slots.data_ptr(), slots.data_ptr() + 4 * SLOTS, ws_ptr, ws_bytes, _st())
    return _lib().clica_conv_k4s2_wgrad(dO.data_ptr(), S.data_ptr(), images, Cc, Cout, hs, ws, dWg_ptr, db_ptr, accumulate, ws_ptr, ws_bytes, _st())


def _run_wgrad(arith, name, shape, mode="plain"):
    """mode: plain | zero_mean | accumulate | no_db | short (one byte less workspace than *_workspace_bytes returns)."""
    from cl_ica_amd import conv
    images, Cc, Cout, hs, ws = shape
    ho, wo = hs - 1, ws - 1
    H, W = 2 * ho, 2 * wo
    g = _gen(3000 + 3 * hs + ws + Cc + Cout)
    x = torch.rand(images, Cc, H, W, generator=g).to(DEV)
    if mode == "zero_mean":
        dout = torch.randn(images, Cout, ho, wo, generator=g).to(DEV)
    else:
        dout = (torch.rand(images, Cout, ho, wo, generator=g) + 0.1).to(DEV)
    wz = torch.zeros(Cout, Cc, 4, 4, device=DEV)
    r = O.stage_reference(x, wz, None, dout, relu=False)
    ref_w, ref_b = conv._wg(r["dw"]).contiguous(), r["db"]
    S_keep, S = _fenced(O.s_flat(x).float())
    d_keep, dfl = _fenced(O.dO_flat(dout).float())
    dO = dfl[(ws + 1) * Cout:]
    K = 16 * Cc
    entry = "clica_conv16_k4s2_wgrad" if arith == "f16x2" else "clica_conv_k4s2_wgrad"
    nb = C.c_size_t()
    _ok(getattr(_lib(), entry + "_workspace_bytes")(images * hs * ws, Cout, K, C.byref(nb)), entry + "_workspace_bytes")
    wsp = Guarded(nb.value, torch.uint8)
    pre_w = pre_b = None
    if mode == "accumulate":
        pre_w = torch.rand(Cout, K, generator=g).to(DEV) * float(ref_w.abs().max())
        pre_b = torch.rand(Cout, generator=g).to(DEV) * float(ref_b.abs().max())
    dWg = Guarded(Cout * K, fill=None if pre_w is None else pre_w.reshape(-1))
    db = Guarded(Cout, fill=pre_b)
    slots = None
    if arith == "f16x2":
        slots = _slots(2)
        _amax_into(dO, slots, 0)
        _amax_into(S, slots, 1)
    case = f"{name} {shape} {mode}"
    given = nb.value
    if mode == "short":
        # what the call itself demands (asked with workspace_bytes = 0: refused before any launch), less one byte
        import re
        assert _wgrad_call(arith, dO, S, images, Cc, Cout, hs, ws, dWg.ptr(), db.ptr(), 0, slots, wsp.ptr(), 0) == E_WORKSPACE
        given = int(re.search(rb"workspace 0 < (\d+)", _lib().clica_last_error()).group(1)) - 1
        assert given < nb.value
    rc = _wgrad_call(arith, dO, S, images, Cc, Cout, hs, ws, dWg.ptr(), None if mode == "no_db" else db.ptr(), int(mode == "accumulate"), slots,
                     wsp.ptr(), given)
    torch.cuda.synchronize()
    assert wsp.guards_intact() and dWg.guards_intact() and db.guards_intact(), case
    if mode == "short":
        assert rc == E_WORKSPACE and b"workspace" in _lib().clica_last_error(), (case, rc)
        assert dWg.untouched(dWg.t) and db.untouched(db.t) and wsp.untouched(wsp.t), f"{case}: a refused call wrote something"
        return
    _ok(rc, entry)
    got_w, got_b = dWg.t.view(Cout, K), db.t
    if mode == "accumulate":
        ref_w, ref_b = ref_w + pre_w.double(), ref_b + pre_b.double()
    tol, note = None, None
    if mode == "zero_mean":
        # a cancelling sum: the allowance is what ATen's own fp32 convolution loses against fp64 on the same data, x 4 (check_elementwise's factor)
        with torch.backends.cudnn.flags(enabled=False):
            x32 = x.clone(); w32 = wz.clone().requires_grad_(True)
            torch.nn.functional.conv2d(x32, w32, None, stride=2, padding=1).backward(dout)
        e32 = O.rel_err(conv._wg(w32.grad), conv._wg(r["dw"]))
        if e32 >= 1e-5:
            tol, note = 4 * e32, f"zero-mean upstream gradient: ATen's fp32 convolution is {e32:.2e} from fp64 on the same data; cap = 4 x that"
    kw = {} if tol is None else dict(tol=tol, note=note)
    fam = f"conv_stage/{entry}"
    assert bool(torch.isfinite(got_w).all()) and (mode == "no_db" or bool(torch.isfinite(got_b).all())), f"{case}: non-finite values"
    PARITY.check(fam, case, "dWg", got_w.cpu().numpy(), ref_w.cpu().numpy(), **kw)
    for blk in range(4):
        PARITY.check(fam, case, f"dWg block (dy, dx) = ({blk >> 1}, {blk & 1})", got_w.view(Cout, 4, 4 * Cc)[:, blk].cpu().numpy(),
                     ref_w.view(Cout, 4, 4 * Cc)[:, blk].cpu().numpy(), **kw)
    if mode == "no_db":
        assert db.untouched(db.t), f"{case}: db = NULL, yet the bias gradient buffer was written"
    else:
        PARITY.check(fam, case, "db", got_b.cpu().numpy(), ref_b.cpu().numpy(), **kw)


@pytest.mark.parametrize("arith", ["f16x2", "f32"])
@pytest.mark.parametrize("name", list(WGRAD))
def test_wgrad(arith, name):
    _run_wgrad(arith, name, WGRAD[name])


@pytest.mark.parametrize("arith", ["f16x2", "f32"])
@pytest.mark.parametrize("mode", ["zero_mean", "accumulate", "no_db", "short"])
def test_wgrad_modes(arith, mode):
    _run_wgrad(arith, "model stage 3", WGRAD["model stage 3"], mode=mode)
    if mode == "zero_mean":
        _run_wgrad(arith, "three column tiles, 4x7", WGRAD["three column tiles, 4x7"], mode=mode)


@pytest.mark.parametrize("name", list(WGRAD_F32_ONLY))
def test_wgrad_f32_ragged(name):
    _run_wgrad("f32", name, WGRAD_F32_ONLY[name])


# ------------------------------------------------------------------------------------------------ first stage (K = 16 C)
FIRST = [(1, 64, 64), (3, 8, 12), (2, 12, 8), (1, 4, 4), (5, 20, 36), (260, 64, 64)]
FIRST_SMALL = FIRST[:5]


def _patches_of(x):
    """The patch matrix clica_conv_im2col_k4s2 builds: [images * H/2 * W/2][16 C], column (ky * 4 + kx) * C + c (an exact copy of x)."""
    N, Cc = x.shape[:2]
    u = torch.nn.functional.unfold(x, 4, stride=2, padding=1)                      # [N][c * 16 + ky * 4 + kx][pixels]
    return u.view(N, Cc, 16, -1).permute(0, 3, 2, 1).reshape(-1, 16 * Cc).contiguous()


@pytest.mark.parametrize("kind", ["clica_conv16_first_fwd", "clica_conv_k4s2_fwd_image", "clica_conv_k4s2_fwd_patches", "clica_conv_k4s2_fwd_patches_amax"])
@pytest.mark.parametrize("images,H,W", FIRST)
def test_first_fwd(kind, images, H, W):
    """One input channel -> 32, into the next stage's S with gate words on the stage's own ho x wo grid: on the matrix cores straight from
    the images (fwd_first16_k), on the vector ALUs from the images (conv_fwd_image_valu_k; pixel_decode's division branch wherever ho or
    wo is no power of two) and from the patch matrix (conv_fwd_patches_valu_k).  (260, 64, 64): more work than one pass of the grid."""
    g = _gen(4000 + H + 3 * W + images)
    x = (torch.rand(images, 1, H, W, generator=g) > 0.6).float().to(DEV)
    w = ((torch.rand(32, 1, 4, 4, generator=g) + 0.05) / 8).to(DEV)
    z0 = O.stage_reference(x, w, relu=False)["pre"]
    b = (-(z0.mean((0, 2, 3))) * (0.6 + 0.8 * torch.rand(32, generator=g)).to(DEV).double()).float()
    ref = torch.relu(z0 + b.double().view(1, -1, 1, 1))
    ho, wo = H // 2, W // 2
    dhs, dws = ho // 2 + 1, wo // 2 + 1
    x_keep, xf = _fenced(x.reshape(-1))
    Wg = w.reshape(32, 16).contiguous()
    n_out = images * dhs * dws * 128
    out = Guarded(n_out + (dws + 2) * 128)
    gate = Guarded(images * ho * wo, torch.int32)
    slots = _slots(2)
    so = slots.data_ptr() + 4 * SLOTS
    L = _lib()
    if kind == "clica_conv16_first_fwd":
        (w16,), wscale = _pack16([Wg])
        _amax_into(xf, slots, 0)
        rc = L.clica_conv16_first_fwd(xf.data_ptr(), w16.data_ptr(), wscale.data_ptr(), b.data_ptr(), images, H, W, 32, 1, out.ptr(), gate.ptr(),
                                      slots.data_ptr(), so, _st())
    elif kind == "clica_conv_k4s2_fwd_image":
        rc = L.clica_conv_k4s2_fwd_image(xf.data_ptr(), Wg.data_ptr(), b.data_ptr(), images, H, W, 32, 1, out.ptr(), gate.ptr(), so, _st())
    else:
        p_keep, P = _fenced(_patches_of(x).reshape(-1))
        if kind.endswith("_amax"):
            rc = L.clica_conv_k4s2_fwd_patches_amax(P.data_ptr(), Wg.data_ptr(), b.data_ptr(), images, 16, 32, ho, wo, 1, 1, out.ptr(), gate.ptr(), so, _st())
        else:
            rc = L.clica_conv_k4s2_fwd_patches(P.data_ptr(), Wg.data_ptr(), b.data_ptr(), images, 16, 32, ho, wo, 1, 1, out.ptr(), gate.ptr(), _st())
    _ok(rc, kind)
    torch.cuda.synchronize()
    case = f"({images}, {H}, {W})"
    assert out.guards_intact() and gate.guards_intact(), case
    got, ring_cells = O.depth_to_space(out.t[:n_out].view(images, dhs, dws, 128), 32)
    assert out.untouched(ring_cells) and out.untouched(out.t[n_out:]), f"{case}: padding slot / zero tail of S written"
    assert float(ref.max()) > 0
    _check_values(f"conv_stage/{kind}", case, "output", got, ref, O.border_mask(ho, wo, DEV))
    want = O.pack_bits(got.permute(0, 2, 3, 1) > 0)
    assert torch.equal(gate.t.view(images, ho, wo, 1).to(torch.int64) & 0xFFFFFFFF, want), f"{case}: gate words != (stored output > 0)"
    if kind != "clica_conv_k4s2_fwd_patches":
        assert int(slots[SLOTS:].max()) == _max_bits(got), f"{case}: output maximum slots"
    else:
        assert not bool(slots[SLOTS:].any())
    if kind == "clica_conv16_first_fwd":
        assert int(slots[:SLOTS].max()) == _max_bits(x), case


@pytest.mark.parametrize("Cc", [1, 3])
@pytest.mark.parametrize("images,H,W", FIRST_SMALL)
def test_im2col(Cc, images, H, W):
    """clica_conv_im2col_k4s2 is a copy: bit for bit, nothing outside the matrix written."""
    x = torch.randn(images, Cc, H, W, generator=_gen(4100 + H + Cc)).to(DEV)
    x_keep, xf = _fenced(x.reshape(-1))
    want = _patches_of(x)
    out = Guarded(want.numel())
    _ok(_lib().clica_conv_im2col_k4s2(xf.data_ptr(), images, Cc, H, W, out.ptr(), _st()), "clica_conv_im2col_k4s2")
    torch.cuda.synchronize()
    assert out.guards_intact() and torch.equal(out.t.view(want.shape).view(torch.int32), want.view(torch.int32)), (Cc, images, H, W)


def test_fwd_patches_three_channels():
    """The patch-matrix forward through the GEMM path (K = 48: no whole k-tile, the generic loaders), scatter = 1 with gate words."""
    images, Cc, H, W = 3, 3, 8, 12
    g = _gen(4200)
    x = torch.rand(images, Cc, H, W, generator=g).to(DEV)
    w = ((torch.rand(32, Cc, 4, 4, generator=g) + 0.05) / 24).to(DEV)
    z0 = O.stage_reference(x, w, relu=False)["pre"]
    b = (-(z0.mean((0, 2, 3))) * (0.8 + 0.4 * torch.rand(32, generator=g)).to(DEV).double()).float()
    ref = torch.relu(z0 + b.double().view(1, -1, 1, 1))
    ho, wo = H // 2, W // 2
    dhs, dws = ho // 2 + 1, wo // 2 + 1
    p_keep, P = _fenced(_patches_of(x).reshape(-1))
    Wg = w.permute(0, 2, 3, 1).reshape(32, 16 * Cc).contiguous()
    n_out = images * dhs * dws * 128
    out = Guarded(n_out + (dws + 2) * 128)
    gate = Guarded(images * ho * wo, torch.int32)
    _ok(_lib().clica_conv_k4s2_fwd_patches(P.data_ptr(), Wg.data_ptr(), b.data_ptr(), images, 16 * Cc, 32, ho, wo, 1, 1, out.ptr(), gate.ptr(), _st()),
        "clica_conv_k4s2_fwd_patches")
    torch.cuda.synchronize()
    assert out.guards_intact() and gate.guards_intact()
    got, ring_cells = O.depth_to_space(out.t[:n_out].view(images, dhs, dws, 128), 32)
    assert out.untouched(ring_cells) and out.untouched(out.t[n_out:])
    _check_values("conv_stage/clica_conv_k4s2_fwd_patches", "nc=3 (3, 8, 12)", "output", got, ref, O.border_mask(ho, wo, DEV))
    assert torch.equal(gate.t.view(images, ho, wo, 1).to(torch.int64) & 0xFFFFFFFF, O.pack_bits(got.permute(0, 2, 3, 1) > 0))


def _first_wgrad(entry, images, Cc, Cout, H, W, mode="plain"):
    g = _gen(4300 + H + 3 * W + Cout + Cc)
    ho, wo = H // 2, W // 2
    rows = images * ho * wo
    x = (torch.rand(images, Cc, H, W, generator=g) > 0.5).float().to(DEV) if Cc == 1 else torch.rand(images, Cc, H, W, generator=g).to(DEV)
    dout = (torch.rand(images, Cout, ho, wo, generator=g) + 0.1).to(DEV) if mode != "zero_mean" else torch.randn(images, Cout, ho, wo, generator=g).to(DEV)
    r = O.stage_reference(x, torch.zeros(Cout, Cc, 4, 4, device=DEV), None, dout, relu=False)
    ref_w, ref_b = r["dw"].permute(0, 2, 3, 1).reshape(Cout, 16 * Cc), r["db"]
    d_keep, dO = _fenced(dout.permute(0, 2, 3, 1).reshape(-1))
    K = 16 * Cc
    nb = C.c_size_t()
    _ok(_lib().clica_conv_k4s2_wgrad_patches_workspace_bytes(rows, Cout, K, C.byref(nb)), "clica_conv_k4s2_wgrad_patches_workspace_bytes")
    wsp = Guarded(nb.value, torch.uint8)
    pre_w = pre_b = None
    if mode == "accumulate":
        pre_w = torch.rand(Cout, K, generator=g).to(DEV) * float(ref_w.abs().max())
        pre_b = torch.rand(Cout, generator=g).to(DEV) * float(ref_b.abs().max())
        ref_w, ref_b = ref_w + pre_w.double(), ref_b + pre_b.double()
    dWg = Guarded(Cout * K, fill=None if pre_w is None else pre_w.reshape(-1))
    db = Guarded(Cout, fill=pre_b)
    if entry == "clica_conv_k4s2_wgrad_image":
        x_keep, src = _fenced(x.reshape(-1))
        rc = _lib().clica_conv_k4s2_wgrad_image(dO.data_ptr(), src.data_ptr(), images, H, W, Cout, dWg.ptr(), db.ptr(), int(mode == "accumulate"),
                                                wsp.ptr(), nb.value, _st())
    else:
        p_keep, src = _fenced(_patches_of(x).reshape(-1))
        rc = _lib().clica_conv_k4s2_wgrad_patches(dO.data_ptr(), src.data_ptr(), rows, Cout, K, dWg.ptr(), db.ptr(), int(mode == "accumulate"),
                                                  wsp.ptr(), nb.value, _st())
    _ok(rc, entry)
    torch.cuda.synchronize()
    case = f"({images}, {Cc}, {Cout}, {H}, {W}) {mode}"
    assert wsp.guards_intact() and dWg.guards_intact() and db.guards_intact(), case
    tol, note = None, None
    if mode == "zero_mean":
        with torch.backends.cudnn.flags(enabled=False):
            w32 = torch.zeros(Cout, Cc, 4, 4, device=DEV, requires_grad=True)
            torch.nn.functional.conv2d(x, w32, None, stride=2, padding=1).backward(dout)
        e32 = O.rel_err(w32.grad, r["dw"])
        if e32 >= 1e-5:
            tol, note = 4 * e32, f"zero-mean upstream gradient: ATen's fp32 convolution is {e32:.2e} from fp64 on the same data; cap = 4 x that"
    kw = {} if tol is None else dict(tol=tol, note=note)
    PARITY.check(f"conv_stage/{entry}", case, "dWg", dWg.t.view(Cout, K).cpu().numpy(), ref_w.cpu().numpy(), **kw)
    PARITY.check(f"conv_stage/{entry}", case, "db", db.t.cpu().numpy(), ref_b.cpu().numpy(), **kw)


@pytest.mark.parametrize("Cout", [8, 16, 32, 64, 128])
@pytest.mark.parametrize("images,H,W", [(3, 8, 12), (5, 20, 36)])
def test_wgrad_image_widths(Cout, images, H, W):
    """clica_conv_k4s2_wgrad_image: conv_wgrad_image_mfma_k for Cout = 32, conv_wgrad_image_k (group sizes 4 ... 64) for the others."""
    _first_wgrad("clica_conv_k4s2_wgrad_image", images, 1, Cout, H, W)


@pytest.mark.parametrize("Cout", [8, 32])
@pytest.mark.parametrize("images,H,W", [(1, 64, 64), (2, 12, 8), (1, 4, 4), (260, 64, 64)])
def test_wgrad_image_shapes(Cout, images, H, W):
    _first_wgrad("clica_conv_k4s2_wgrad_image", images, 1, Cout, H, W)


@pytest.mark.parametrize("mode", ["zero_mean", "accumulate"])
@pytest.mark.parametrize("entry,Cc,Cout", [("clica_conv_k4s2_wgrad_image", 1, 32), ("clica_conv_k4s2_wgrad_image", 1, 16),
                                           ("clica_conv_k4s2_wgrad_patches", 1, 32), ("clica_conv_k4s2_wgrad_patches", 4, 16)])
def test_first_wgrad_modes(entry, Cc, Cout, mode):
    _first_wgrad(entry, 5, Cc, Cout, 20, 36, mode=mode)


@pytest.mark.parametrize("Cc,Cout", [(1, 32), (4, 16)])
@pytest.mark.parametrize("images,H,W", FIRST_SMALL)
def test_wgrad_patches(Cc, Cout, images, H, W):
    """clica_conv_k4s2_wgrad_patches at (Cout, K) = (32, 16) and (16, 64); (32, 48) is refused (tests/test_cabi_symbols.py)."""
    _first_wgrad("clica_conv_k4s2_wgrad_patches", images, Cc, Cout, H, W)


@pytest.mark.parametrize("Cc", [1, 2, 3, 4])
@pytest.mark.parametrize("images,H,W", FIRST_SMALL)
def test_dgrad_input(Cc, images, H, W):
    """clica_conv_k4s2_dgrad_input: d loss / d image of the first stage from dO on its ho x wo grid and Conv2d.weight as the module stores it."""
    g = _gen(4400 + H + Cc)
    ho, wo = H // 2, W // 2
    dout = (torch.rand(images, 32, ho, wo, generator=g) + 0.1).to(DEV)
    w = (torch.rand(32, Cc, 4, 4, generator=g) + 0.05).to(DEV)
    ref = O.stage_reference(torch.zeros(images, Cc, H, W, device=DEV), w, None, dout)["dx"]
    d_keep, dO = _fenced(dout.permute(0, 2, 3, 1).reshape(-1))
    dX = Guarded(images * Cc * H * W)
    _ok(_lib().clica_conv_k4s2_dgrad_input(dO.data_ptr(), w.data_ptr(), images, Cc, 32, H, W, dX.ptr(), _st()), "clica_conv_k4s2_dgrad_input")
    torch.cuda.synchronize()
    assert dX.guards_intact()
    _check_values("conv_stage/clica_conv_k4s2_dgrad_input", f"({images}, {Cc}, {H}, {W})", "dX", dX.t.view(images, Cc, H, W), ref, O.border_mask(H, W, DEV))


def test_gather():
    """clica_conv_gather: 16 segments in one launch -- permutation maps, -1 entries (-> 0), a NULL map (identity), a count of 0 (nothing
    written) -- plain and accumulating, bit for bit."""
    g = _gen(4500)
    n = 16
    counts = [0 if i == 5 else int(torch.randint(1, 3000, (1,), generator=g)) for i in range(n)]
    srcs = [torch.randn(max(c, 4), generator=g).to(DEV) for c in counts]
    maps = []
    for i, c in enumerate(counts):
        if i % 4 == 0:
            maps.append(None)
        else:
            m = torch.randperm(max(c, 4), generator=g)[:c].to(torch.int32)
            if i % 4 == 2 and c:
                m[torch.randint(0, c, (max(c // 7, 1),), generator=g)] = -1
            maps.append(m.to(DEV))
    VP, I32 = C.c_void_p * n, C.c_int32 * n
    for accumulate in (0, 1):
        pre = [torch.randn(max(c, 4), generator=g).to(DEV) for c in counts]
        dsts = [Guarded(max(c, 4), fill=p_) for c, p_ in zip(counts, pre)]
        _ok(_lib().clica_conv_gather(n, VP(*[t.data_ptr() for t in srcs]), VP(*[None if m is None else m.data_ptr() for m in maps]),
                                     VP(*[d.ptr() for d in dsts]), I32(*counts), accumulate, _st()), "clica_conv_gather")
        torch.cuda.synchronize()
        for i, (c, d) in enumerate(zip(counts, dsts)):
            m = maps[i]
            v = srcs[i][:c] if m is None else torch.where(m >= 0, srcs[i][m.clamp(min=0).long()], torch.zeros((), device=DEV))
            want = pre[i].clone()
            want[:c] = pre[i][:c] + v if accumulate else v
            assert d.guards_intact() and torch.equal(d.t.view(torch.int32), want.view(torch.int32)), (i, c, accumulate)
    # every count zero: nothing is launched
    assert _lib().clica_conv_gather(2, (C.c_void_p * 2)(srcs[0].data_ptr(), srcs[1].data_ptr()), (C.c_void_p * 2)(None, None),
                                    (C.c_void_p * 2)(srcs[2].data_ptr(), srcs[3].data_ptr()), (C.c_int32 * 2)(0, 0), 0, _st()) == 0


# ------------------------------------------------------------------------------------------------------------ pack and amax
def _split_np(v, s):
    t = (v.astype(np.float32) * np.float32(s)).astype(np.float32)                 # s is a power of two: exact
    hi = t.astype(np.float16)
    lo = (t - hi.astype(np.float32)).astype(np.float16)
    return hi.view(np.int16), lo.view(np.int16)


def test_pack_bit_for_bit():
    """clica_conv16_pack: hi = f16(v s), lo = f16(v s - hi) bit for bit against NumPy, s = 2^(8 - e) with e the exponent of max |v| over
    the source; 8 matrices, counts that are no multiples of 4 or 1024, with a map (a permutation), with -1 entries (-> 0), without a map."""
    g = _gen(50)
    srcs, maps = [], []
    for i, n in enumerate([4, 7, 1023, 1025, 4099, 32 * 512, 64 * 1024 + 3, 18]):
        v = torch.randn(n, generator=g) * float(10.0 ** (i - 3))
        srcs.append(v.to(DEV))
        if i % 3 == 0:
            maps.append(None)
        else:
            m = torch.randperm(n, generator=g).to(torch.int32)
            if i % 3 == 2:
                m = torch.cat([m, torch.full((5,), -1, dtype=torch.int32)])[torch.randperm(n + 5, generator=g)]
            maps.append(m.to(DEV))
    dst, scales = _pack16(srcs, maps)
    torch.cuda.synchronize()
    for i, (v, m, d) in enumerate(zip(srcs, maps, dst)):
        vn = v.cpu().numpy()
        e = int(np.floor(np.log2(np.abs(vn).max())))
        s = 2.0 ** (8 - e)
        assert float(scales[i]) == s, (i, float(scales[i]), s)
        assert 256 <= np.abs(vn).max() * s < 512
        if m is None:
            src = vn
        else:
            mn = m.cpu().numpy()
            src = np.where(mn >= 0, vn[np.clip(mn, 0, None)], np.float32(0))
        hi, lo = _split_np(src, s)
        dn = d.cpu().numpy()
        assert np.array_equal(dn[:src.size], hi), i
        assert np.array_equal(dn[src.size:], lo), i
    # an all-zero source: scale 1, zero planes
    (dz,), sz = _pack16([torch.zeros(12, device=DEV)])
    assert float(sz[0]) == 1.0 and not bool(dz.any())


def test_amax_slots():
    """clica_conv16_amax: exact bits of max |x| (n = 4, 1028, and beyond the 4 x CUs block cap), a negative maximum, an all-zero tensor
    (slots stay zero), inf / NaN -> a finite huge value."""
    g = _gen(60)
    for n in (4, 1028, 4 * 256 * 4 * 256 * 3 + 8):
        x = torch.randn(n, generator=g).to(DEV)
        x[n // 2] = -77.25                                      # the maximum is a negative element
        s = _slots(1)
        _amax_into(x, s, 0)
        torch.cuda.synchronize()
        assert int(s.max()) == _max_bits(x) == int(np.float32(77.25).view(np.int32)), n
    s = _slots(1)
    _amax_into(torch.zeros(1028, device=DEV), s, 0)
    assert not bool(s.any())
    for bad in (float("inf"), float("-inf"), float("nan")):
        x = torch.ones(1028, device=DEV); x[5] = bad
        s = _slots(1)
        _amax_into(x, s, 0)
        m = float(s.max().view(torch.float32))
        assert np.isfinite(m) and m >= 3.0e38, (bad, m)
