"""fp64 oracle of ONE conv stage (Conv2d(k = 4, stride 2, pad 1) + ReLU) in the layouts the stage kernels read and write
(cl_ica_amd/conv.py, csrc/conv16.hip, conv section of csrc/linear.hip).  Values come from torch.nn.functional.conv2d in
float64 and its autograd; this module only carries them into the kernels' layouts and back.  Device-agnostic (CPU or GPU tensors).

    S       padded space-to-depth input, S[img][sy][sx][(py*2+px)*C + c] = x_padded[img][c][2sy+py][2sx+px] on an hs x ws grid
            (hs = H/2 + 1, ws = W/2 + 1, one zero pixel all round), flat, with a zero tail of (ws + 2) * 4C floats
    output  pixel (y, x), y < hs - 1, x < ws - 1:  scatter = 1 -> pixel ((y+1)>>1, (x+1)>>1), slot ((y+1)&1)*2 + ((x+1)&1) of the next
            stage's S (= space_to_depth of the output);  scatter = 2 -> row (img*hs + y)*ws + x of the stage's own grid
    gate    words [(img*hs + y)*ws + x][Cout/32], bit = (stored output > 0)
    dO      on the hs x ws grid, zero on the non-output rows, (ws + 1) * Cout zero floats in front
    dPrev   on a dhs x dws pixel grid, valid part 2(hs-1) x 2(ws-1), C channels
"""
import torch
import torch.nn.functional as F

__all__ = ["space_to_depth", "depth_to_space", "s_flat", "grid_hw", "on_grid", "from_grid", "dO_flat", "written_s2d", "pack_bits", "unpack_bits",
           "row_operand", "dgrad_operand", "stage_reference", "border_mask", "rel_err"]


def grid_hw(H, W):
    """(hs, ws) of the space-to-depth grid of an H x W input."""
    return H // 2 + 1, W // 2 + 1


def space_to_depth(x):
    """x [N][C][H][W] -> S [N][hs][ws][4C] (zero pixel all round)."""
    N, C, H, W = x.shape
    hs, ws = grid_hw(H, W)
    xp = F.pad(x.permute(0, 2, 3, 1), (0, 0, 1, 1, 1, 1))
    return xp.reshape(N, hs, 2, ws, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, hs, ws, 4 * C)


def depth_to_space(S, C):
    """Inverse of space_to_depth: S [N][hs][ws][4C] -> (x [N][C][H][W], the padding ring's cells as a flat tensor)."""
    N, hs, ws, _ = S.shape
    xp = S.reshape(N, hs, ws, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * hs, 2 * ws, C)
    inner = xp[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2)
    ring = torch.cat([xp[:, 0].reshape(-1), xp[:, -1].reshape(-1), xp[:, 1:-1, 0].reshape(-1), xp[:, 1:-1, -1].reshape(-1)])
    return inner, ring


def written_s2d(N, C, H, W, device=None):
    """bool [N][hs][ws][4C]: the cells of S that hold a pixel of the image (the others are the padding slots)."""
    return space_to_depth(torch.ones(N, C, H, W, device=device)) > 0


def s_flat(x):
    """The flat S the kernels read: the grid, then the zero tail of (ws + 2) * 4C."""
    S = space_to_depth(x)
    return torch.cat([S.reshape(-1), S.new_zeros((S.shape[2] + 2) * S.shape[3])])


def on_grid(t, fill=0.0):
    """t [N][Co][ho][wo] -> [N][ho+1][wo+1][Co]: channels-last on the stage's row grid, `fill` on the non-output rows."""
    g = F.pad(t.permute(0, 2, 3, 1), (0, 0, 0, 1, 0, 1), value=fill)
    return g.contiguous()


def from_grid(g):
    """[N][hs][ws][Co] -> the output part [N][Co][hs-1][ws-1]."""
    return g[:, :-1, :-1, :].permute(0, 3, 1, 2)


def dO_flat(dout):
    """dout [N][Co][ho][wo] -> flat [(ws + 1) * Co zeros][N hs ws Co]."""
    g = on_grid(dout)
    return torch.cat([g.new_zeros((g.shape[2] + 1) * g.shape[3]), g.reshape(-1)])


def pack_bits(b):
    """bool [..., 32 k] -> int64 words [..., k] (bit i of word j = element 32 j + i), values in [0, 2^32)."""
    sh = b.shape
    w = b.reshape(*sh[:-1], sh[-1] // 32, 32).to(torch.int64) << torch.arange(32, device=b.device)
    return w.sum(-1)


def unpack_bits(w, n):
    """int words [..., n/32] (int32 or int64) -> bool [..., n]."""
    w = w.to(torch.int64) & 0xFFFFFFFF
    b = (w.unsqueeze(-1) >> torch.arange(32, device=w.device)) & 1
    return b.reshape(*w.shape[:-1], n).bool()


def row_operand(flat, rows, C, ws):
    """The forward's two-run row operand: row r = S_flat[r*4C : +8C] ++ S_flat[(r + ws)*4C : +8C]  ([rows][16 C])."""
    idx = torch.arange(8 * C, device=flat.device)
    base = torch.arange(rows, device=flat.device).unsqueeze(1) * (4 * C)
    return torch.cat([flat[base + idx], flat[base + ws * 4 * C + idx]], 1)


def dgrad_operand(dflat, rows, Co, ws):
    """The data gradient's operand on the zero-fronted dO: row r = dO_flat[r*Co : +2Co] ++ dO_flat[(r + ws)*Co : +2Co]  ([rows][4 Co])."""
    idx = torch.arange(2 * Co, device=dflat.device)
    base = torch.arange(rows, device=dflat.device).unsqueeze(1) * Co
    return torch.cat([dflat[base + idx], dflat[base + ws * Co + idx]], 1)


def stage_reference(x, w, b=None, dout=None, relu=True):
    """float64 conv2d(k = 4, stride 2, pad 1) of the given (any float dtype) tensors: returns dict with `out` (after ReLU if asked) and,
    with `dout` (gradient at the PRE-activation), `dx`, `dw`, `db`."""
    x = x.double().detach().requires_grad_(dout is not None)
    w = w.double().detach().requires_grad_(dout is not None)
    z = F.conv2d(x, w, None if b is None else b.double(), stride=2, padding=1)
    res = {"pre": z.detach(), "out": torch.relu(z).detach() if relu else z.detach()}
    if dout is not None:
        z.backward(dout.double())
        res.update(dx=x.grad, dw=w.grad, db=dout.double().sum((0, 2, 3)))
    return res


def border_mask(h, w, device=None):
    """bool [h][w]: first / last row and column."""
    m = torch.zeros(h, w, dtype=torch.bool, device=device)
    m[0, :] = m[-1, :] = True
    m[:, 0] = m[:, -1] = True
    return m


def rel_err(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))
