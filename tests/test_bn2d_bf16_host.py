"""The bf16 entry points of csrc/bn2d_nhwc.hip on a CPU-only host: they are exported and bound, their argument checks refuse by return
code before any launch, the rounding they use (restated here) is that of ``Tensor.to(torch.bfloat16)``, and resnet.BF16_MODE is
validated like the other switches."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

BF16_ENTRY_POINTS = ("clica_bn2d_nhwc_act_fwd_train_bf16", "clica_bn2d_nhwc_act_fwd_eval_bf16", "clica_bn2d_nhwc_act_bwd_bf16",
                     "clica_bn2d_nhwc_act_maxpool_fwd_train_bf16", "clica_bn2d_nhwc_act_maxpool_fwd_eval_bf16",
                     "clica_bn2d_nhwc_act_maxpool_bwd_bf16", "clica_avgpool2d_global_nhwc_fwd_bf16", "clica_avgpool2d_global_nhwc_bwd_bf16")


@pytest.fixture(scope="module")
def L():
    from cl_ica_amd import _lib
    return _lib.load()


def test_the_eight_entry_points_are_exported_and_bound(L):
    from cl_ica_amd import _lib
    raw = ctypes.CDLL(os.path.join(ROOT, "cl_ica_amd", "lib", "libclica_hip.so"))
    for name in BF16_ENTRY_POINTS:
        assert hasattr(raw, name), name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name[:-len("_bf16")]], name          # the fp32 twin's argument list
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name]
    assert L.clica_version() >= 102


def test_they_refuse_null_pointers_and_bad_shapes_by_return_code(L):
    """Host code ahead of every launch: the checks, messages and codes of the fp32 twins (dummy aligned pointers are never touched)."""
    p, eps, mom = 4096, 1e-5, 0.1
    nb = ctypes.c_size_t()
    assert L.clica_bn2d_nhwc_workspace_bytes(64, 8, ctypes.byref(nb)) == 0
    need = nb.value
    for sfx in ("", "_bf16"):
        fwd, ev, bwd = (getattr(L, "clica_bn2d_nhwc_act_" + k + sfx) for k in ("fwd_train", "fwd_eval", "bwd"))
        ok = [p, None, p, p, 64, 8, eps, mom, 0.0, p, p, p, None, None, p, need, None]
        for i in (0, 2, 3, 9, 10, 11, 14):                                                   # X, gamma, beta, Y, save_mean, save_invstd, workspace
            assert fwd(*[None if j == i else a for j, a in enumerate(ok)]) == -1, (sfx, i)
            assert f"clica_bn2d_nhwc_act_fwd_train{sfx}: NULL pointer".encode() in L.clica_last_error()
        for i, bad in ((4, 1), (4, 0), (5, 0), (5, (1 << 20) + 1), (8, -0.5), (15, need - 1), (14, p + 4)):
            assert fwd(*[bad if j == i else a for j, a in enumerate(ok)]) == -1, (sfx, i, bad)          # M < 2, C off limits, slope, workspace
            assert f"clica_bn2d_nhwc_act_fwd_train{sfx}:".encode() in L.clica_last_error()
        assert ev(None, None, p, p, p, p, 64, 8, eps, 0.0, p, None) == -1 and ev(p, None, p, p, p, p, 64, 8, eps, 0.0, None, None) == -1
        assert ev(p, None, p, p, p, p, 0, 8, eps, 0.0, p, None) == -1 and ev(p, None, p, p, p, p, 64, (1 << 20) + 1, eps, 0.0, p, None) == -1
        okb = [p, p, p, p, p, p, 64, 8, 0.0, p, None, p, p, p, need, None]
        for i in (0, 1, 2, 3, 4, 5, 9, 11, 12, 13):
            assert bwd(*[None if j == i else a for j, a in enumerate(okb)]) == -1, (sfx, i)
        assert bwd(*[1 if j == 6 else a for j, a in enumerate(okb)]) == -1 and bwd(*[16 if j == 14 else a for j, a in enumerate(okb)]) == -1
        # the stem: a short workspace is CLICA_E_WORKSPACE
        assert L.clica_bn2d_nhwc_maxpool_workspace_bytes(4, 8, 4, 4, ctypes.byref(nb)) == 0
        sf, se, sb = (getattr(L, "clica_bn2d_nhwc_act_maxpool_" + k + sfx) for k in ("fwd_train", "fwd_eval", "bwd"))
        oks = [p, p, p, 4, 8, 4, 4, eps, mom, 0.0, p, p, p, None, None, p, nb.value, None]
        for i in (0, 1, 2, 10, 11, 12, 15):
            assert sf(*[None if j == i else a for j, a in enumerate(oks)]) == -1, (sfx, i)
        for i, bad, rc in ((3, 0, -1), (4, (1 << 20) + 1, -1), (5, (1 << 15) + 1, -1), (9, 1.5, -1), (16, nb.value - 1, -2)):
            assert sf(*[bad if j == i else a for j, a in enumerate(oks)]) == rc, (sfx, i, bad)
        assert sf(p, p, p, 1, 8, 1, 1, eps, mom, 0.0, p, p, p, None, None, p, 1 << 20, None) == -1          # N H W < 2 in training
        assert se(p, p, p, p, None, 4, 8, 4, 4, eps, 0.0, p, None) == -1 and se(p, p, p, p, p, 4, 8, 4, 4, eps, 0.0, None, None) == -1
        assert sb(p, None, p, p, p, p, 4, 8, 4, 4, 0.0, p, p, p, p, nb.value, None) == -1
        assert sb(p, p, p, p, p, p, 4, 8, 4, 4, 0.0, p, p, p, p, 16, None) == -2
        af, ab = (getattr(L, "clica_avgpool2d_global_nhwc_" + k + sfx) for k in ("fwd", "bwd"))
        assert af(None, 4, 4, 8, p, None) == -1 and af(p, 4, 4, 8, None, None) == -1 and af(p, 0, 4, 8, p, None) == -1
        assert af(p, 4, (1 << 14) + 1, 8, p, None) == -1 and ab(None, 4, 4, 8, p, None) == -1 and ab(p, 4, 4, 0, p, None) == -1
        assert f"clica_avgpool2d_global_nhwc_bwd{sfx}:".encode() in L.clica_last_error()


def bf16_bits_rne(a):
    """csrc/bn2d.h bf16_rne on an fp32 array: the upper 16 bits after adding 0x7fff + (bit 16); a NaN becomes 0x7fc0."""
    u = np.asarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where((u & 0x7FFFFFFF) > 0x7F800000, np.uint16(0x7FC0), r)


def test_the_rounding_rule_is_torchs():
    f = lambda bits: np.array(bits, dtype=np.uint32).view(np.float32)  # noqa: E731
    edge = f([0x00000000, 0x80000000,                      # +-0
              0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000,      # halfway: to even (down, up), just above / below
              0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000,                  # the largest finite values: fp32's overflows to inf
              0x7F800000, 0xFF800000,                      # infinities
              0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807F8000, 0x00800000,      # denormals and the smallest normal
              0x3F800000, 0x40490FDB, 0x42C80000, 0x42C84000, 0x42C8C000])                 # 1, pi, 100, 100.125 (tie), 100.375 (tie)
    rng = np.random.default_rng(0)
    table = np.concatenate([edge, rng.normal(size=4096).astype(np.float32), rng.integers(0, 1 << 32, size=8192, dtype=np.uint64)
                            .astype(np.uint32).view(np.float32)])
    table = table[~np.isnan(table)]
    want = torch.from_numpy(table).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = bf16_bits_rne(table)
    assert np.array_equal(got, want), [(hex(int(a.view(np.uint32))), hex(int(g)), hex(int(w))) for a, g, w in zip(table, got, want) if g != w][:8]
    assert got[2] == 0x3F80 and got[3] == 0x3F82 and got[4] == 0x3F81 and got[8] == 0x7F80 and got[10] == 0x7F7F          # spot checks
    # a NaN stays a NaN (torch keeps a quiet NaN too; payloads are not compared)
    nan = torch.tensor([float("nan")]).to(torch.bfloat16)
    assert bool(torch.isnan(nan).all()) and bf16_bits_rne(np.float32("nan"))[()] == 0x7FC0
    # widening is the 16-bit shift
    back = (want.astype(np.uint32) << 16).view(np.float32)
    assert np.array_equal(back, torch.from_numpy(table).to(torch.bfloat16).float().numpy(), equal_nan=True)


def test_the_switch_defaults_to_torch_and_is_validated():
    from cl_ica_amd import resnet
    assert resnet.BF16_MODE == os.environ.get("CLICA_RESNET_BF16", "torch")
    assert "CLICA_RESNET_BF16" in os.environ or resnet.BF16_MODE == "torch"
    env = dict(os.environ, CLICA_RESNET_BF16="bogus", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    bad = subprocess.run([sys.executable, "-c", "from cl_ica_amd import resnet"], env=env, capture_output=True, text=True)
    assert bad.returncode != 0 and "CLICA_RESNET_BF16='bogus'" in bad.stderr, bad.stderr


def test_cpu_bf16_tensors_fall_through(monkeypatch):
    """BF16_MODE "hip" on the CPU, where no kernel applies: a channels-last bf16 block has the bits of BF16_MODE "torch"."""
    import copy
    from cl_ica_amd import resnet
    monkeypatch.setattr(resnet, "NHWC_MODE", "hip")
    torch.manual_seed(3)
    base = resnet.BasicBlock(8, 16, 2).to(memory_format=torch.channels_last).bfloat16()
    x = torch.randn(2, 8, 6, 6).contiguous(memory_format=torch.channels_last).bfloat16()
    out = {}
    for mode in ("hip", "torch"):
        monkeypatch.setattr(resnet, "BF16_MODE", mode)
        blk = copy.deepcopy(base).train()
        out[mode] = [blk(x).detach()] + [b.float() for b in blk.buffers()]
    for a, b in zip(out["hip"], out["torch"]):
        assert torch.equal(a.float(), b.float())
