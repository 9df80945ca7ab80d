"""The C-ABI library loads on a CPU-only host and exports exactly what include/clica.h declares
(no compute calls: those need the GPU)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "clica.h")
LIB = os.path.join(ROOT, "cl_ica_amd", "lib", "libclica_hip.so")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(clica_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(LIB)


def test_header_declares_functions():
    names = declared_functions()
    assert len(names) >= 20
    for must in ("clica_lp_loss_fwd", "clica_lp_loss_bwd", "clica_linear_fwd", "clica_linear_dgrad", "clica_linear_wgrad",
                 "clica_adam_step", "clica_sample", "clica_mixing_fwd", "clica_last_error"):
        assert must in names


def test_library_exports_every_declared_symbol(lib):
    missing = [n for n in declared_functions() if not hasattr(lib, n)]
    assert not missing, f"declared in clica.h but not exported: {missing}"


def test_python_binding_matches_header(lib):
    from cl_ica_amd import _lib
    declared = set(declared_functions()) - {"clica_last_error"}
    bound = set(_lib.SIGNATURES)
    assert bound == declared, (sorted(bound - declared), sorted(declared - bound))
    assert _lib.load().clica_version() >= 100


def test_host_only_entry_points(lib):
    """Planning/validation entry points are pure host code: they must work (and fail loudly) without a GPU."""
    from cl_ica_amd import _lib
    L = _lib.load()
    d = _lib.LpLossDesc(B=6144, B3=6144, n=10, p=2.0, tau=1.0, alpha=0.5, compat=1, pow=1)
    fb, bb = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.clica_lp_loss_workspace_bytes(ctypes.byref(d), ctypes.byref(fb), ctypes.byref(bb)) == 0
    assert 0 < fb.value < 64 << 20 and 0 < bb.value < 256 << 20
    bad = _lib.LpLossDesc(B=4, B3=4, n=513, p=2.0, tau=1.0, alpha=0.5, compat=1, pow=1)
    assert L.clica_lp_loss_workspace_bytes(ctypes.byref(bad), ctypes.byref(fb), ctypes.byref(bb)) == -1
    assert b"n=513" in L.clica_last_error()
    frac = _lib.LpLossDesc(B=4, B3=5, n=3, p=0.5, tau=1.0, alpha=0.5, compat=1, pow=1)
    assert L.clica_lp_loss_workspace_bytes(ctypes.byref(frac), ctypes.byref(fb), ctypes.byref(bb)) == -1
    nb = ctypes.c_size_t()
    assert L.clica_linear_wgrad_workspace_bytes(12288, 500, 500, ctypes.byref(nb)) == 0 and nb.value > 0
    assert L.clica_linear_fwd(None, 0, None, 0, None, None, 0, 1, 1, 1, 0, 0.0, None) == -1     # NULL pointers rejected
    with pytest.raises(_lib.ClicaError):
        _lib.check(-1, "probe")


def test_host_planners_on_random_shapes(lib):
    """The host-side planners behind the *_workspace_bytes entry points (stream-split planner of the loss sweeps, grouped
    weight-gradient planner, nearest-neighbour planner) on 3000 seeded random shapes: they must return, succeed, and ask for a
    sane amount of memory (no division by zero, no runaway split counts).  No GPU involved."""
    import numpy as np
    from cl_ica_amd import _lib
    rng = np.random.default_rng(0)
    fb, bb, nb = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    for _ in range(1000):
        B = int(rng.choice([1, 2, 63, 64, 65, 1000, 6144, 20000]) + rng.integers(0, 3))
        B3 = int(rng.choice([1, 7, 128, 129, 6144, 49152, 200000]) + rng.integers(0, 3))
        n = int(rng.choice([1, 2, 10, 16, 17, 40, 64, 65, 128, 300, 512]))
        p = float(rng.choice([1.0, 2.0, 2.5]))
        d = _lib.LpLossDesc(B=B, B3=B3, n=n, p=p, tau=1.0, alpha=0.5, compat=1, pow=1)
        assert lib.clica_lp_loss_workspace_bytes(ctypes.byref(d), ctypes.byref(fb), ctypes.byref(bb)) == 0, (B, B3, n)
        # partials: (splits x rows) pairs forward, (splits x rows x padded n) floats backward; splits stay <= a few dozen per row tile
        assert 0 < fb.value <= 64 * (B + B3) * 8 * 64 + (1 << 20), (B, B3, n, fb.value)
        assert 0 < bb.value <= 64 * (B + B3) * (n + 3) * 4 * 64 + (1 << 20), (B, B3, n, bb.value)
        assert lib.clica_lp_loss_train_workspace_bytes(ctypes.byref(d), ctypes.byref(nb)) == 0 and nb.value > 0
    I32 = ctypes.c_int32
    for _ in range(1000):
        L = int(rng.integers(1, 8))
        dims = [int(rng.choice([1, 3, 10, 16, 17, 100, 128, 256, 500, 512, 600, 2000])) for _ in range(L + 1)]
        M = int(rng.choice([1, 47, 48, 1000, 12288, 100000]))
        N = (I32 * L)(*dims[1:]); K = (I32 * L)(*dims[:-1])
        assert lib.clica_mlp_wgrad_workspace_bytes(M, L, N, K, ctypes.byref(nb)) == 0, (M, dims)
        dense = sum(a * b + b for a, b in zip(dims[:-1], dims[1:])) * 4
        assert 0 < nb.value <= 600 * dense + (1 << 20), (M, dims, nb.value)         # slabs: a bounded number of splits per layer
    for _ in range(1000):
        Q = int(rng.choice([1, 2, 64, 1000, 5000])); N = int(rng.choice([1, 2, 100, 250000, 3000000])); n = int(rng.integers(1, 65)); k = int(rng.integers(1, 5))
        assert lib.clica_nn_search_workspace_bytes(Q, N, n, k, ctypes.byref(nb)) == 0 and 0 < nb.value <= Q * 8 * 4 * 4096 + 4096, (Q, N, n, k, nb.value)


def _wgrad_demand(fn, images, C, Cout, hs, ws, conv16):
    """What the weight-gradient call asks for: called with workspace_bytes = 0 (and dummy aligned pointers it never touches) it returns
    CLICA_E_WORKSPACE before any launch and names the size in clica_last_error()."""
    from cl_ica_amd import _lib
    p = 4096
    rc = fn(p, p, images, C, Cout, hs, ws, p, p, 0, None, None, p, 0, None) if conv16 else fn(p, p, images, C, Cout, hs, ws, p, p, 0, p, 0, None)
    assert rc == -2, (rc, _lib.load().clica_last_error())
    m = re.search(rb"workspace 0 < (\d+)", _lib.load().clica_last_error())
    assert m, _lib.load().clica_last_error()
    return int(m.group(1))


def test_conv_wgrad_workspace_bytes_bound_the_call(lib):
    """*_wgrad_workspace_bytes(rows, ...) knows the rows, not the grid width; the call plans its contraction splits over rows + ws + 1
    (conv16) -- whatever it then demands must fit what was granted: every image count 1..4096 at the three 16C-deep stages of the KITTI
    stack, and 2000 seeded (images, hs, ws, C, Cout) with ws up to the 4095 the call admits.  (The conv16 bound used to plan with
    rows + 4096 where the call plans with rows + ws + 1, and the split count is not monotone: 174 images at the 17 x 17 stage asked for
    393 slabs against 342 granted, CLICA_E_WORKSPACE in the middle of a backward pass.)  Both arithmetics' entry points."""
    import numpy as np
    from cl_ica_amd import _lib
    L = _lib.load()
    nb = ctypes.c_size_t()
    pairs = ((L.clica_conv16_k4s2_wgrad, L.clica_conv16_k4s2_wgrad_workspace_bytes, True),
             (L.clica_conv_k4s2_wgrad, L.clica_conv_k4s2_wgrad_workspace_bytes, False))
    for call, bound, conv16 in pairs:
        for (C, Cout, hs) in ((32, 32, 17), (32, 64, 9), (64, 64, 5)):
            for images in range(1, 4097):
                assert bound(images * hs * hs, Cout, 16 * C, ctypes.byref(nb)) == 0
                need = _wgrad_demand(call, images, C, Cout, hs, hs, conv16)
                assert need <= nb.value, (conv16, images, C, Cout, hs, need, nb.value)
                assert nb.value <= 2 * need + (8 << 20), (conv16, images, C, Cout, hs, need, nb.value)      # a bound, not a blank cheque
        rng = np.random.default_rng(16)
        for _ in range(2000):
            images = int(rng.choice([1, 2, 7, 100, 174, 1000, 3000]) + rng.integers(0, 50))
            hs = int(rng.integers(2, 40))
            ws = int(rng.choice([2, 3, 5, 9, 17, 33, 100, 1000, 4095])) if rng.random() < 0.7 else int(rng.integers(2, 4096))
            C = int(rng.choice([32, 64, 96, 128]))
            Cout = int(rng.choice([32, 64])) if conv16 else int(rng.choice([4, 20, 32, 64, 96]))
            assert bound(images * hs * ws, Cout, 16 * C, ctypes.byref(nb)) == 0
            need = _wgrad_demand(call, images, C, Cout, hs, ws, conv16)
            assert need <= nb.value, (conv16, images, hs, ws, C, Cout, need, nb.value)
    # the grid width the bound does not cover is refused by the call itself, before the workspace check
    assert L.clica_conv16_k4s2_wgrad(4096, 4096, 1, 32, 32, 2, 4096, 4096, 4096, 0, None, None, 4096, 0, None) == -1


def test_conv_stage_entry_points_refuse_by_return_code(lib):
    """Shapes outside a conv-stage entry point's contract are refused by CLICA_E_INVALID in its argument checks -- host code, before any
    launch (tests/test_gpu_conv_stages.py runs the shapes they admit).  Every call here fails a check the entry point makes ahead of
    its launch; the weight-gradient calls also carry workspace_bytes = 0."""
    from cl_ica_amd import _lib
    L, p = _lib.load(), 4096
    # conv16 forward: C a multiple of 8, Cout of 32, scatter 1 | 2, an even output grid for scatter = 1, hs >= 2, gate bits only with scatter = 1
    for (C, Cout, hs, ws, scatter) in [(4, 32, 5, 5, 1), (8, 20, 5, 5, 1), (32, 32, 4, 7, 1), (32, 32, 5, 5, 3), (32, 32, 1, 5, 2)]:
        assert L.clica_conv16_k4s2_fwd(p, p, p, p, 1, C, Cout, hs, ws, 1, scatter, p, None, None, None, None) == -1, (C, Cout, hs, ws, scatter)
    assert L.clica_conv16_k4s2_fwd(p, p, p, p, 1, 32, 32, 5, 5, 1, 2, p, p, None, None, None) == -1
    assert L.clica_conv16_k4s2_fwd(p, p, p, p, 1 << 20, 32, 32, 5, 5, 1, 2, p, None, None, None, None) == -1             # 2^24 rows
    assert L.clica_conv_k4s2_fwd(p, p, p, 1, 4, 20, 5, 5, 1, 1, p, p, None) == -1                                        # gate bits need Cout % 32 == 0
    assert L.clica_conv_k4s2_fwd(p, p, p, 1, 6, 32, 5, 5, 1, 1, p, None, None) == -1                                     # C % 4
    # conv16 data gradient: C a multiple of 32, Cout of 8, gate bits required, the destination grid at least 2 (hs - 1) x 2 (ws - 1)
    for (C, Cout, hs, ws, dhs, dws) in [(16, 32, 5, 5, 8, 8), (32, 4, 5, 5, 8, 8), (32, 32, 5, 5, 7, 8), (32, 32, 5, 4, 8, 5)]:
        assert L.clica_conv16_k4s2_dgrad(p, p, p, 1, C, Cout, hs, ws, p, dhs, dws, p, None, None, None) == -1, (C, Cout, hs, ws, dhs, dws)
    assert L.clica_conv16_k4s2_dgrad(p, p, p, 1, 32, 32, 5, 5, p, 8, 8, None, None, None, None) == -1
    assert L.clica_conv_k4s2_dgrad(p, p, None, 1, 8, 4, 5, 5, p, 8, 8, p, None) == -1                                    # gate bits need C % 32 == 0
    assert L.clica_conv_k4s2_dgrad(p, p, None, 1, 8, 6, 5, 5, p, 8, 8, None, None) == -1                                 # Cout % 4
    # conv16 weight gradient: C a multiple of 32, Cout 32 or 64, ws < 4096
    for (C, Cout, hs, ws) in [(16, 32, 5, 5), (32, 96, 5, 5), (32, 32, 1, 5), (32, 32, 2, 4096)]:
        assert L.clica_conv16_k4s2_wgrad(p, p, 1, C, Cout, hs, ws, p, p, 0, None, None, p, 0, None) == -1, (C, Cout, hs, ws)
    assert L.clica_conv_k4s2_wgrad(p, p, 1, 6, 32, 5, 5, p, p, 0, p, 0, None) == -1
    # first stage on the matrix cores: Cout = 32, H and W multiples of 4
    for (H, W, Cout) in [(6, 8, 32), (8, 8, 64), (2, 8, 32)]:
        assert L.clica_conv16_first_fwd(p, p, p, p, 1, H, W, Cout, 1, p, None, None, None, None) == -1, (H, W, Cout)
    # pack: at most 8 matrices; amax: n a multiple of 4, 16-byte aligned
    VP, I32 = ctypes.c_void_p * 9, ctypes.c_int32 * 9
    assert L.clica_conv16_pack(9, VP(*[p] * 9), I32(*[4] * 9), VP(*[None] * 9), VP(*[p] * 9), I32(*[4] * 9), p, None) == -1
    assert L.clica_conv16_amax(p, 6, p, None) == -1 and L.clica_conv16_amax(p + 4, 8, p, None) == -1
    # first-stage weight gradient from the patch matrix: (Cout / 4)(K / 4) must divide 256
    nb = ctypes.c_size_t()
    assert L.clica_conv_k4s2_wgrad_patches_workspace_bytes(1024, 32, 48, ctypes.byref(nb)) == -1
    assert L.clica_conv_k4s2_wgrad_patches(p, p, 1024, 32, 48, p, p, 0, p, 0, None) == -1
    assert L.clica_conv_k4s2_wgrad_patches_workspace_bytes(1024, 32, 16, ctypes.byref(nb)) == 0 and nb.value > 0
    assert L.clica_conv_k4s2_wgrad_patches_workspace_bytes(1024, 16, 64, ctypes.byref(nb)) == 0 and nb.value > 0
