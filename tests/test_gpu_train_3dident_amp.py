"""cl_ica_amd.train_3dident --amp bf16 end to end on the GPU: a synthetic root (64 seeded latents, 64 x 64 x 3 images handed over through
``main(images=...)``) and the ResNet-18 stand-in as the backbone, batches of 4 -- planes down to 2 x 2, as the real run's.  ``--amp off``
against no flag runs on 8 x 8 images and a one-layer backbone, as tests/test_gpu_train_3dident.py does: it is about the flag."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

COMMON = ["--batch-size", "4", "--n-eval-samples", "16", "--iterations", "4", "--n-log-steps", "2", "--seed", "1"]


def tiny_backbone(pretrained, num_classes):
    from cl_ica_amd import layers
    return torch.nn.Sequential(layers.Flatten(), torch.nn.Linear(192, num_classes))


def resnet_backbone(pretrained, num_classes):
    from cl_ica_amd import resnet
    return resnet.resnet18(pretrained, num_classes=num_classes)


def _root(path, d, side, n=64):
    """raw_latents.npy with `n` seeded points in [0, 1]^d and a side x side x 3 image per point."""
    os.makedirs(path, exist_ok=True)
    latents = np.random.default_rng(21).uniform(size=(n, d)).astype(np.float32)
    np.save(os.path.join(path, "raw_latents.npy"), latents)
    p = np.arange(side * side * 3, dtype=np.int64).reshape(1, side, side, 3)
    images = ((np.arange(n, dtype=np.int64).reshape(n, 1, 1, 1) * 3 + p * 5) % 256).astype(np.uint8)
    images[:, 0, 0, 0] = np.arange(n)
    return str(path), latents, images


@pytest.fixture(scope="module")
def root64(tmp_path_factory):
    return _root(tmp_path_factory.mktemp("ident64"), 3, 64)


@pytest.fixture(scope="module")
def root8(tmp_path_factory):
    return _root(tmp_path_factory.mktemp("ident8"), 3, 8)


@pytest.fixture(autouse=True)
def deterministic_convolutions(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)


def run(root, extra, backbone, capsys):
    from cl_ica_amd import train_3dident as T
    path, _latents, images = root
    out = T.main(["--offline-dataset", path] + COMMON + extra, images=images, base_encoder=backbone)
    torch.cuda.synchronize()
    return out, capsys.readouterr().out


def logged(text):
    return [(int(m.group(1)), float(m.group(2))) for m in (re.search(r"Step: (\d+) .*?Loss: (\S+)", line) for line in text.splitlines()) if m]


def spy(monkeypatch):
    """The library's bn2d / pool entry points by name, and the calls of torch's batch-norm."""
    import torch.nn.functional as F
    from cl_ica_amd import ops
    entries, torch_bn = [], []
    real_entry, real_bn = ops._entry, F.batch_norm

    def entry(name, dtype):
        fn, full = real_entry(name, dtype)
        entries.append(full)
        return fn, full

    def batch_norm(*a, **k):
        torch_bn.append(1)
        return real_bn(*a, **k)
    monkeypatch.setattr(ops, "_entry", entry)
    monkeypatch.setattr(F, "batch_norm", batch_norm)
    return entries, torch_bn


def test_unsupervised_bf16_trains_evaluates_and_saves(root64, tmp_path, capsys, monkeypatch):
    from cl_ica_amd import resnet
    switches = (resnet.NHWC_MODE, resnet.NHWC_STEM_MODE, resnet.BF16_MODE)
    plain = str(tmp_path / "fp32.pth")
    ref, ref_text = run(root64, ["--mode", "unsupervised", "--position-only", "--save-model", plain], resnet_backbone, capsys)
    assert "Mixed precision" not in ref_text
    entries, torch_bn = spy(monkeypatch)
    model = str(tmp_path / "bf16.pth")
    out, text = run(root64, ["--mode", "unsupervised", "--position-only", "--amp", "bf16", "--save-model", model], resnet_backbone, capsys)
    assert len([l for l in text.splitlines() if l.startswith("Mixed precision: --amp bf16")]) == 1
    rows = logged(text)
    assert [s for s, _ in rows] == [1, 3] and all(np.isfinite(v) for _, v in rows), text
    assert len(out["losses"]) == 4 and all(np.isfinite(v) for v in out["losses"])
    with capsys.disabled():
        print(f"first-step loss: --amp bf16 {out['losses'][0]:.6f}, fp32 {ref['losses'][0]:.6f}")
    # 4 steps x 2 views and 2 evaluations of 4 batches, 20 units and the pool each; every unit on a bf16 entry point, none on torch
    assert not torch_bn
    assert entries and all(e.endswith("_bf16") for e in entries)
    assert sum(e == "clica_bn2d_nhwc_act_maxpool_fwd_train_bf16" for e in entries) == 16
    assert sum(e == "clica_bn2d_nhwc_act_fwd_train_bf16" for e in entries) == 304
    assert sum(e == "clica_bn2d_nhwc_act_bwd_bf16" for e in entries) == 152
    assert sum(e == "clica_avgpool2d_global_nhwc_bwd_bf16" for e in entries) == 8
    assert (resnet.NHWC_MODE, resnet.NHWC_STEM_MODE, resnet.BF16_MODE) == switches          # the driver's switches end with the run
    assert all(p.dtype == torch.float32 for p in out["f"].parameters())
    sd, sd_ref = (torch.load(f, map_location="cpu", weights_only=True) for f in (model, plain))
    assert list(sd) == list(sd_ref)
    assert all(sd[k].shape == sd_ref[k].shape and sd[k].dtype == sd_ref[k].dtype for k in sd)
    assert all(bool(torch.isfinite(v).all()) for v in sd.values() if v.is_floating_point())
    # --mode test of the file just written, in both precisions
    for amp in ("bf16", "off"):
        tested, text = run(root64, ["--mode", "test", "--position-only", "--load-model", model, "--amp", amp], resnet_backbone, capsys)
        assert f"Model loaded: {model}" in text and ("Mixed precision" in text) == (amp == "bf16")
        perm, lin, mse, linfit = tested["scores"]
        assert np.isfinite(perm) and np.isfinite(lin) and mse.shape == (3,) and linfit.shape == (3,)


def test_supervised_bf16_runs(root64, capsys, monkeypatch):
    entries, torch_bn = spy(monkeypatch)
    out, text = run(root64, ["--mode", "supervised", "--position-only", "--amp", "bf16", "--lr", "1e-3"], resnet_backbone, capsys)
    assert [s for s, _ in logged(text)] == [0, 2] and all(np.isfinite(v) for _, v in logged(text)), text
    assert len(out["losses"]) == 4 and all(np.isfinite(v) for v in out["losses"])
    assert not torch_bn and sum(e == "clica_bn2d_nhwc_act_bwd_bf16" for e in entries) == 76


def test_bf16_without_a_backbone_is_refused(root8):
    from cl_ica_amd import train_3dident as T
    for flag in ("--dummy-mixing", "--identity-solution", "--identity-mixing-and-solution"):
        with pytest.raises(AssertionError, match="no backbone"):
            T.main(["--offline-dataset", root8[0]] + COMMON + ["--mode", "unsupervised", "--position-only", "--amp", "bf16", flag])


def test_amp_off_is_a_run_without_the_flag(root8, tmp_path, capsys):
    runs = []
    for k, extra in enumerate(([], ["--amp", "off"])):
        model = str(tmp_path / f"m{k}.pth")
        out, text = run(root8, ["--mode", "unsupervised", "--position-only", "--save-model", model] + extra, tiny_backbone, capsys)
        lines = [re.sub(r"^\[[^\]]*\]", "", l) for l in text.splitlines() if "Step:" in l]          # (the log lines without their time stamp)
        runs.append((out["losses"], lines, torch.load(model, map_location="cpu", weights_only=True)))
        assert "Mixed precision" not in text
    (l0, t0, s0), (l1, t1, s1) = runs
    assert l0 == l1 and t0 == t1 and len(t0) == 2
    assert list(s0) == list(s1) and all(torch.equal(s0[k], s1[k]) and s0[k].stride() == s1[k].stride() for k in s0)
