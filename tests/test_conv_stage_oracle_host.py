"""Pins tests/conv_stage_oracle.py (the per-stage oracle of tests/test_gpu_conv_stages.py) on the CPU in fp64 against nn.functional.conv2d
and its autograd, at hs != ws: test_conv_stack_formulation_and_layouts_on_cpu (tests/test_host_logic.py) restates the same formulation on
square grids only, and a kernel that swaps hs for ws is invisible there."""
import pytest
import torch
import torch.nn.functional as F

import conv_stage_oracle as O

SHAPES = [(8, 12), (6, 4)]


def _data(H, W, N=3, C=4, Co=6, seed=0):
    g = torch.Generator().manual_seed(seed + 17 * H + W)
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Co, C, 4, 4, generator=g, dtype=torch.float64)
    b = torch.randn(Co, generator=g, dtype=torch.float64)
    dout = torch.randn(N, Co, H // 2, W // 2, generator=g, dtype=torch.float64)
    return x, w, b, dout


@pytest.mark.parametrize("H,W", SHAPES)
def test_converters_round_trip(H, W):
    from cl_ica_amd import conv
    x, w, b, dout = _data(H, W)
    N, C = x.shape[:2]
    Co = w.shape[0]
    hs, ws = O.grid_hw(H, W)
    assert (hs, ws) == (H // 2 + 1, W // 2 + 1) and hs != ws
    S = O.space_to_depth(x)
    assert S.shape == (N, hs, ws, 4 * C)
    # the definition, element by element
    xp = F.pad(x, (1, 1, 1, 1))
    for (img, sy, sx, py, px, c) in [(0, 0, 0, 0, 0, 0), (1, 2, 1, 1, 0, 3), (2, hs - 1, ws - 1, 1, 1, 2), (1, hs - 1, 0, 0, 1, 1), (0, 1, ws - 1, 1, 0, 0)]:
        assert S[img, sy, sx, (py * 2 + px) * C + c] == xp[img, c, 2 * sy + py, 2 * sx + px]
    back, ring = O.depth_to_space(S, C)
    assert torch.equal(back, x) and ring.numel() == N * C * (2 * hs * 2 * ws - H * W) and not ring.any()
    wr = O.written_s2d(N, C, H, W)
    assert int(wr.sum()) == N * C * H * W and not S[~wr].any()
    flat = O.s_flat(x)
    assert flat.numel() == N * hs * ws * 4 * C + (ws + 2) * 4 * C and not flat[N * hs * ws * 4 * C:].any()
    # scatter = 1 is the space-to-depth of the output: pixel (y, x) -> pixel ((y+1)>>1, (x+1)>>1), slot ((y+1)&1)*2 + ((x+1)&1)
    out = torch.randn(N, Co, hs - 1, ws - 1, dtype=torch.float64)
    if (hs - 1) % 2 == 0 and (ws - 1) % 2 == 0:          # (the kernels refuse scatter = 1 on an odd output grid)
        Sn = O.space_to_depth(out)
        for (img, y, xx, co) in [(0, 0, 0, 0), (1, hs - 2, ws - 2, Co - 1), (2, 1, 0, 2), (0, 0, ws - 2, 1)]:
            assert Sn[img, (y + 1) >> 1, (xx + 1) >> 1, (((y + 1) & 1) * 2 + ((xx + 1) & 1)) * Co + co] == out[img, co, y, xx]
    # the row grid
    gr = O.on_grid(out, fill=7.0)
    assert gr.shape == (N, hs, ws, Co) and torch.equal(O.from_grid(gr), out)
    assert bool((gr[:, hs - 1] == 7.0).all()) and bool((gr[:, :, ws - 1] == 7.0).all())
    d = O.dO_flat(dout)
    assert d.numel() == (ws + 1) * Co + N * hs * ws * Co and not d[:(ws + 1) * Co].any()
    # weights
    assert torch.equal(conv._wg_to_conv(conv._wg(w), Co, C), w)
    Wg, Wd = conv._wg(w), conv._wd(w)
    assert Wg.shape == (Co, 16 * C) and Wd.shape == (4 * Co, 4 * C)
    for dy in range(2):
        for dx in range(2):
            assert torch.equal(Wd[((1 - dy) * 2 + (1 - dx)) * Co:][:Co], Wg[:, (dy * 2 + dx) * 4 * C:][:, :4 * C])
    # gate words
    bits = torch.rand(5, 3, 64, generator=torch.Generator().manual_seed(1)) > 0.5
    words = O.pack_bits(bits)
    assert words.shape == (5, 3, 2) and int(words.max()) < 2 ** 32
    assert torch.equal(O.unpack_bits(words, 64), bits)
    assert torch.equal(O.unpack_bits(words.to(torch.int32), 64), bits)          # as the kernels' int32 storage holds them
    assert int(O.pack_bits(torch.ones(32, dtype=torch.bool))[0]) == 0xFFFFFFFF
    bm = O.border_mask(hs - 1, ws - 1)
    assert int(bm.sum()) == (hs - 1) * (ws - 1) - max(hs - 3, 0) * max(ws - 3, 0)


@pytest.mark.parametrize("H,W", SHAPES)
def test_restatements_reproduce_conv2d_and_autograd(H, W):
    from cl_ica_amd import conv
    x, w, b, dout = _data(H, W, seed=3)
    N, C = x.shape[:2]
    Co = w.shape[0]
    hs, ws = O.grid_hw(H, W)
    rows = N * hs * ws
    ref = O.stage_reference(x, w, b, dout, relu=False)
    z = F.conv2d(x, w, b, stride=2, padding=1)
    assert torch.equal(ref["out"], z) and torch.equal(ref["pre"], z)
    assert torch.equal(O.stage_reference(x, w, b)["out"], torch.relu(z))
    # forward: two-run row operand x Wg^T on the whole grid; its output rows are conv2d
    flat = O.s_flat(x)
    A = O.row_operand(flat, rows, C, ws)
    assert A.shape == (rows, 16 * C)
    out = (A @ conv._wg(w).t() + b).view(N, hs, ws, Co)
    assert O.rel_err(O.from_grid(out), z) < 1e-13
    # weight / bias gradient, and the same as one pass over S against four shifted dO windows (csrc/conv16.hip: wgrad16_k)
    dflat = O.dO_flat(dout)
    dO = dflat[(ws + 1) * Co:].view(rows, Co)
    assert O.rel_err(conv._wg_to_conv(dO.t() @ A, Co, C), ref["dw"]) < 1e-13
    assert O.rel_err(dO.sum(0), ref["db"]) < 1e-13
    prows = rows + ws + 1
    Sp = flat[:prows * 4 * C].view(prows, 4 * C)
    blocks = []
    for dy in range(2):
        for dx in range(2):
            sh = dy * ws + dx
            dsh = torch.zeros(prows, Co, dtype=torch.float64)
            dsh[sh:sh + rows] = dO                                     # row p holds dO[p - shift]
            blocks.append(dsh.t() @ Sp)
    assert O.rel_err(conv._wg_to_conv(torch.cat(blocks, 1), Co, C), ref["dw"]) < 1e-13
    # data gradient: row r = gradient of S pixel r
    Ad = O.dgrad_operand(dflat, rows, Co, ws)
    assert Ad.shape == (rows, 4 * Co)
    dS = (Ad @ conv._wd(w)).view(N, hs, ws, 4 * C)
    dx, _ = O.depth_to_space(dS, C)
    assert O.rel_err(dx, ref["dx"]) < 1e-13
    # the conv16 data gradient multiplies by the packed TRANSPOSE [4C][4Cout]
    assert O.rel_err((Ad @ conv._wd(w).t().contiguous().t()).view(N, hs, ws, 4 * C), dS) < 1e-13
