"""cl_ica_amd.train_3dident end to end on the GPU: a synthetic root (64 seeded latents, 8 x 8 x 3 images handed over through
``main(images=...)``) and a one-layer backbone, so that no MIOpen find step runs.  Every case runs
``--batch-size 16 --n-eval-samples 32 --iterations 6 --n-log-steps 3 --seed 1``."""
import argparse
import os
import random
import re

import numpy as np
import pytest
import torch

import sgd_oracle as S

pytestmark = pytest.mark.gpu

COMMON = ["--batch-size", "16", "--n-eval-samples", "32", "--iterations", "6", "--n-log-steps", "3", "--seed", "1"]


def backbone(pretrained, num_classes):
    from cl_ica_amd import layers
    return torch.nn.Sequential(layers.Flatten(), torch.nn.Linear(192, num_classes))


def _root(path, d, n=64):
    """raw_latents.npy with `n` seeded points in [0, 1]^d and an 8 x 8 x 3 image per point (as test_gpu_image_table._synthetic_root)."""
    os.makedirs(path, exist_ok=True)
    latents = np.random.default_rng(21).uniform(size=(n, d)).astype(np.float32)
    np.save(os.path.join(path, "raw_latents.npy"), latents)
    p = np.arange(8 * 8 * 3, dtype=np.int64).reshape(1, 8, 8, 3)
    images = ((np.arange(n, dtype=np.int64).reshape(n, 1, 1, 1) * 3 + p * 5) % 256).astype(np.uint8)
    images[:, 0, 0, 0] = np.arange(n)
    return str(path), latents, images


@pytest.fixture(scope="module")
def root3(tmp_path_factory):
    return _root(tmp_path_factory.mktemp("ident3"), 3)


@pytest.fixture(scope="module")
def root10(tmp_path_factory):
    return _root(tmp_path_factory.mktemp("ident10"), 10)


def run(root, extra, capsys=None):
    from cl_ica_amd import train_3dident as T
    path, _latents, images = root
    out = T.main(["--offline-dataset", path] + COMMON + extra, images=images, base_encoder=backbone)
    torch.cuda.synchronize()
    text = capsys.readouterr().out if capsys is not None else ""
    return out, text


def logged(text):
    """[(step, loss)] of the printed log lines."""
    rows = []
    for line in text.splitlines():
        m = re.search(r"Step: (\d+) .*?Loss: (\S+)", line)
        if m:
            rows.append((int(m.group(1)), float(m.group(2))))
    return rows


def numbers_after(text, label):
    return [float(v) for line in text.splitlines() if "Step:" in line for v in re.findall(re.escape(label) + r" (-?[\d.]+(?:[eE][-+]?\d+)?|nan|inf)", line)]


def hand_first_step(root, extra):
    """The first step of the unsupervised loop written out by hand on the same seeds: initial parameters and the loss."""
    from cl_ica_amd import optim, spaces, threedident
    from cl_ica_amd import train_3dident as T
    from cl_ica_amd.datasets import BatchLoader, ThreeDIdentDataset
    path, _latents, images = root
    args = T.parse_args(["--offline-dataset", path] + COMMON + extra)
    np.random.seed(args.seed); random.seed(args.seed); torch.manual_seed(args.seed); spaces.manual_seed(args.seed)
    ls, n_non_angular, n_angular = T.setup_latent_space(args)
    f = threedident.setup_f(args, n_non_angular, n_angular, base_encoder=backbone).cuda()
    ds = ThreeDIdentDataset(path, ls, latent_dimensions_to_use=T.latent_dimensions_to_use(args), normalize=T.NORMALIZE, images=images)
    loss = threedident.make_unsupervised_loss(args, n_non_angular)
    opt = optim.Adam(f.parameters(), lr=args.lr)
    p0 = [p.detach().clone() for p in f.parameters()]
    total, _per_item, _parts = threedident.train_step(next(iter(BatchLoader(ds, args.batch_size))), loss, opt, f, sync=True)
    return p0, total


def test_unsupervised_position_only(root3, capsys):
    extra = ["--mode", "unsupervised", "--position-only"]
    out, text = run(root3, extra, capsys)
    rows = logged(text)
    assert [s for s, _ in rows] == [1, 4], text                              # global steps 0 and 3, printed 1-based
    assert all(np.isfinite(v) for _, v in rows)
    for label in ("sigma(loss):", "<Loss>:", "Lin. Disentanglement:", "Perm. Disentanglement (MCC):"):
        vals = numbers_after(text, label)
        assert len(vals) >= 2 and all(np.isfinite(v) for v in vals), (label, text)      # ("<Loss>:" also ends "sigma(<Loss>):")
    assert "L2: [" in text and "lin. L2: [" in text and "Using latent dimensions: [0, 1, 2]" in text
    assert len(out["losses"]) == 6 and all(np.isfinite(v) for v in out["losses"])
    assert rows[0][1] == pytest.approx(out["losses"][0], abs=1e-6) and rows[1][1] == pytest.approx(out["losses"][3], abs=1e-6)
    from cl_ica_amd import optim
    assert isinstance(out["optimizer"], optim.Adam) and int(out["optimizer"].step_dev.item()) == 6
    p0, first = hand_first_step(root3, extra)
    assert abs(out["losses"][0] - first) <= 1e-5 * abs(first), (out["losses"][0], first)
    moved = [float((p.detach() - q).abs().max()) for p, q in zip(out["f"].parameters(), p0)]
    assert all(m > 0 for m in moved), moved


def test_unsupervised_ten_columns_l1(root10, capsys):
    out, text = run(root10, ["--mode", "unsupervised", "--non-periodic-rotation-and-color", "--unsupervised-loss", "l1"], capsys)
    assert [s for s, _ in logged(text)] == [1, 4] and all(np.isfinite(v) for _, v in logged(text))
    assert "Using latent dimensions: [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]" in text
    assert out["latent_space"].dim == 10 and out["n_non_angular_latents"] == 10 and len(out["losses"]) == 6
    assert all(np.isfinite(v) for v in out["losses"]) and out["f"][2].weight.shape == (10, 100)


@pytest.mark.parametrize("kind", ["mse", "r2"])
def test_supervised(root3, capsys, kind):
    out, text = run(root3, ["--mode", "supervised", "--position-only", "--supervised-loss", kind, "--lr", "1e-3"], capsys)
    rows = logged(text)
    assert [s for s, _ in rows] == [0, 3], text                              # the supervised loop prints the 0-based step
    assert all(np.isfinite(v) for _, v in rows) and len(out["losses"]) == 6 and all(np.isfinite(v) for v in out["losses"])
    assert "Perm. Disentanglement" not in text and "sigma(loss)" not in text
    perm, lin, mse, linfit = out["scores"]
    assert perm == np.inf and np.isfinite(lin) and mse.shape == (3,) and linfit.shape == (3,)


def test_optimizer_sgd_first_step_is_the_kernels(root3, monkeypatch):
    from cl_ica_amd import optim
    seen = []
    real_step = optim.SGD.step

    def recording_step(self, closure=None):
        self._adopt_foreign_grads()
        before = self.param_arena.clone()
        r = real_step(self, closure)
        if not seen:
            torch.cuda.synchronize()
            seen.append((before.cpu().numpy(), self.grad_arena.cpu().numpy().copy(), self.param_arena.cpu().numpy().copy()))
        return r

    monkeypatch.setattr(optim.SGD, "step", recording_step)
    out, _ = run(root3, ["--mode", "unsupervised", "--position-only", "--optimizer", "sgd", "--lr", "0.01"])
    opt = out["optimizer"]
    assert type(opt) is optim.SGD and opt.momentum_buffer is None
    g = opt.param_groups[0]
    assert (g["lr"], g["momentum"], g["dampening"], g["weight_decay"], g["nesterov"], g["maximize"]) == (0.01, 0.0, 0.0, 0.0, False, False)
    before, grad, after = seen[0]
    assert float(np.abs(grad).max()) > 0
    want, _ = S.sgd_fp32_emulation(before, grad, None, 0, dict(lr=0.01))
    assert np.array_equal(after.view(np.uint32), want.view(np.uint32))
    assert int(opt.step_dev.item()) == 6


def test_save_every_and_test_mode(root3, tmp_path, capsys):
    from cl_ica_amd import train_3dident as T
    model = str(tmp_path / "f.pth")
    out, text = run(root3, ["--mode", "unsupervised", "--position-only", "--save-model", model, "--save-every", "3"], capsys)
    assert sorted(os.listdir(tmp_path)) == ["f.pth", "f.pth.iteration_3", "f.pth.iteration_6"]
    assert f"Model saved as {model}.iteration_3" in text and f"Saving final model at: {model}" in text
    sd = torch.load(model, map_location="cpu", weights_only=True)
    assert sd and all(k.startswith("module.") for k in sd)
    assert sorted(k[len("module."):] for k in sd) == sorted(out["f"].state_dict())
    sd6 = torch.load(model + ".iteration_6", map_location="cpu", weights_only=True)
    assert all(torch.equal(sd[k], sd6[k]) for k in sd)
    sd3 = torch.load(model + ".iteration_3", map_location="cpu", weights_only=True)
    assert any(not torch.equal(sd[k], sd3[k]) for k in sd)
    tested, text = run(root3, ["--mode", "test", "--position-only", "--load-model", model], capsys)
    assert f"Model loaded: {model}" in text
    line = [l for l in text.splitlines() if l.startswith("Lin. Disentanglement:")]
    assert len(line) == 1 and all(k in line[0] for k in ("MCC:", "MSE:", "lin. fit MSE:"))
    perm, lin, mse, linfit = tested["scores"]
    assert np.isfinite(perm) and np.isfinite(lin) and mse.shape == (3,) and linfit.shape == (3,)
    x = torch.randn(16, 3, 8, 8, device="cuda")
    with torch.no_grad():
        assert torch.equal(tested["f"](x), out["f"](x))
    # a file without the prefix loads as well
    plain = str(tmp_path / "plain.pth")
    torch.save(T.strip_module_prefix(sd), plain)
    again, _ = run(root3, ["--mode", "test", "--position-only", "--load-model", plain], capsys)
    with torch.no_grad():
        assert torch.equal(again["f"](x), out["f"](x))


def test_evaluate_against_direct_computation(root3):
    from cl_ica_amd import disentanglement_utils as du
    from cl_ica_amd import train_3dident as T
    torch.manual_seed(5)
    f = backbone(False, 3).cuda()
    batches = [((torch.rand(16, 3, device="cuda"), None), (torch.randn(16, 3, 8, 8, device="cuda"), None)) for _ in range(2)]
    args = argparse.Namespace(n_eval_samples=32, batch_size=16, dummy_mixing=False, identity_mixing_and_solution=False, identity_solution=False)
    perm, lin, mse, linfit = T.evaluate(args, f, iter(batches), True)
    z = torch.cat([b[0][0] for b in batches]); x = torch.cat([b[1][0] for b in batches])
    with torch.no_grad():
        hz = f(x)
    (want_lin, _), (z2, pred) = du.linear_disentanglement(z, hz, mode="r2", train_test_split=True)
    (want_perm, _), _ = du.permutation_disentanglement(z, hz, mode="pearson", solver="munkres", rescaling=True)
    assert lin == want_lin and perm == want_perm
    want_mse = ((z.double() - hz.double()) ** 2).mean(0).cpu().numpy()
    want_fit = ((torch.as_tensor(z2).double() - torch.as_tensor(pred).double().to(z2.device)) ** 2).mean(0).cpu().numpy()
    assert mse.shape == (3,) and linfit.shape == (3,)
    assert np.abs(mse - want_mse).max() <= 1e-5 * np.abs(want_mse).max()
    assert np.abs(linfit - want_fit).max() <= 1e-5 * np.abs(want_fit).max()
    assert z2.shape[0] == 16                                                   # the fit's error is taken on the held-out half
    # no permutation score asked for, unpaired batches, and fewer samples than one batch
    perm2, lin2, _, _ = T.evaluate(args, f, iter([(b[0][0], b[1][0]) for b in batches]), False, no_pairs=True)
    assert perm2 == np.inf and lin2 == want_lin
    args.n_eval_samples = 8
    assert T.evaluate(args, f, iter(batches), True) == (np.inf, np.inf, np.inf, np.inf)


def test_dummy_mixing_runs(root3, capsys):
    path, _latents, _images = root3
    from cl_ica_amd import train_3dident as T
    argv = ["--offline-dataset", path] + COMMON + ["--mode", "unsupervised", "--position-only", "--dummy-mixing"]
    argv[argv.index("--iterations") + 1] = "2"
    out = T.main(argv)                                                        # no images: none are read
    torch.cuda.synchronize()
    assert len(out["losses"]) == 2 and all(np.isfinite(v) for v in out["losses"])
    assert [s for s, _ in logged(capsys.readouterr().out)] == [1]
    assert len(out["f"]) == 2 and sum(p.dim() == 2 for p in out["f"][0].parameters()) == 7      # get_mlp's seven layers + the rescaling


def test_identity_solution_in_test_mode(root3, capsys):
    out, text = run(root3, ["--mode", "test", "--position-only", "--identity-solution"], capsys)
    perm, lin, mse, linfit = out["scores"]
    assert perm == np.inf and mse == np.inf and np.isfinite(lin) and linfit.shape == (3,)
    assert len(list(out["f"].parameters())) == 0 and "MCC: inf" in text


def test_no_flags_with_ten_columns_raises_the_shape_assertion(root10):
    with pytest.raises(AssertionError, match="Shapes do not match"):
        run(root10, ["--mode", "unsupervised"])


def test_refusals(root3):
    from cl_ica_amd import train_3dident as T
    with pytest.raises(SystemExit, match="no CPU path"):
        T.main(["--offline-dataset", root3[0], "--no-cuda"])
    with pytest.raises(AssertionError):
        T.main(["--offline-dataset", os.path.join(root3[0], "nowhere")])
