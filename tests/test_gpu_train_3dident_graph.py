"""The 3DIdent iteration as one HIP graph (threedident.capture_iteration, ``train_3dident --graph``) on the GPU, on the synthetic root
of test_gpu_train_3dident.py: 64 latents, 8 x 8 x 3 images through ``main(images=...)``, the one-layer backbone,
``--batch-size 16 --iterations 6 --n-log-steps 3 --seed 1`` (no MIOpen find step), and one case on the real ResNet-18 in bf16.

The captured run is held to the all-eager clocked run from the same initial state: the batches bit for bit; losses and final
parameters bit for bit if two eager runs agree bit for bit, else within 4 x their largest difference."""
import random

import numpy as np
import pytest
import torch

import test_gpu_train_3dident as base

pytestmark = pytest.mark.gpu

MODE = ["--mode", "unsupervised", "--position-only"]
N_REPLAYS = 6


@pytest.fixture(scope="module")
def root3(tmp_path_factory):
    return base._root(tmp_path_factory.mktemp("ident3g"), 3)


def setup(root, extra=()):
    """Model, data set, loss and optimizer as ``main`` builds them from ``--seed 1``."""
    from cl_ica_amd import optim, spaces, threedident
    from cl_ica_amd import train_3dident as T
    from cl_ica_amd.datasets import ThreeDIdentDataset
    path, _latents, images = root
    args = T.parse_args(["--offline-dataset", path] + base.COMMON + MODE + list(extra))
    np.random.seed(args.seed); random.seed(args.seed); torch.manual_seed(args.seed); spaces.manual_seed(args.seed)
    ls, n_non_angular, n_angular = T.setup_latent_space(args)
    f = threedident.setup_f(args, n_non_angular, n_angular, base_encoder=base.backbone).cuda()
    ds = ThreeDIdentDataset(path, ls, latent_dimensions_to_use=T.latent_dimensions_to_use(args), normalize=T.NORMALIZE, images=images)
    loss = T._three_values(threedident.make_unsupervised_loss(args, n_non_angular))
    return args, ds, f, loss, optim.Adam(f.parameters(), lr=args.lr)


def snapshot(result, latents, images):
    return dict(total=result[0].detach().clone(), per_item=result[1].detach().clone(), z=latents[0].clone(), zt=latents[1].clone(),
                x=images.clone())


def eager_run(root, n):
    from cl_ica_amd import spaces, threedident
    args, ds, f, loss, opt = setup(root)
    clock = spaces.DeviceClock(args.seed, "cuda")
    steps = []
    for _ in range(n):
        result, latents, images = threedident.clocked_iteration(ds, loss, opt, f, args.batch_size, clock)
        steps.append(snapshot(result, latents, images))
    torch.cuda.synchronize()
    assert int(clock.step.item()) == n and int(opt.step_dev.item()) == n
    return steps, [p.detach().clone() for p in f.parameters()]


def captured_run(root, between=None):
    """One eager warm-up iteration and N_REPLAYS replays; ``between(args, ds, f)`` runs between replays 3 and 4."""
    from cl_ica_amd import spaces, threedident
    args, ds, f, loss, opt = setup(root)
    warm = []
    step = threedident.capture_iteration(ds, loss, opt, f, args.batch_size, warmup=1, clock=spaces.DeviceClock(args.seed, "cuda"),
                                         on_warmup=warm.append)
    assert len(warm) == 1 and step.owned and isinstance(step.graph, torch.cuda.CUDAGraph)
    steps = [dict(total=warm[0][0].detach().clone(), per_item=warm[0][1].detach().clone())]
    for k in range(N_REPLAYS):
        if k == 3 and between is not None:
            between(args, ds, f)
        result = step()
        assert step.images.shape == (32, 3, 8, 8) and step.images.dtype == torch.float32 and step.images.is_contiguous()
        steps.append(snapshot(result, step.latents, step.images))
    torch.cuda.synchronize()
    assert int(step.clock.step.item()) == N_REPLAYS + 1 and int(opt.step_dev.item()) == N_REPLAYS + 1
    return steps, [p.detach().clone() for p in f.parameters()], step


_REF = {}


def reference(root):
    """The eager clocked run (twice, computed once): its steps and final parameters, and the bound the captured run is held to -- 0
    (bit equality) if the two eager runs agree bit for bit, else 4 x their largest difference."""
    if not _REF:
        (a, pa), (b, pb) = eager_run(root, N_REPLAYS + 1), eager_run(root, N_REPLAYS + 1)
        d_loss = max(float((s["total"] - t["total"]).abs().max()) for s, t in zip(a, b))
        d_par = max(float((p - q).abs().max()) for p, q in zip(pa, pb))
        for s, t in zip(a, b):      # the batches do not depend on the training: always bit for bit
            assert all(torch.equal(s[k], t[k]) for k in ("z", "zt", "x"))
        print(f"eager against eager: largest loss difference {d_loss:.3e}, largest parameter difference {d_par:.3e}")
        _REF.update(steps=a, params=pa, loss_bound=4 * d_loss, param_bound=4 * d_par)
    return _REF


def check_trajectory(ref, steps, params, first=0):
    for k in range(first, len(steps)):
        d = float((steps[k]["total"] - ref["steps"][k]["total"]).abs().max())
        dp = float((steps[k]["per_item"] - ref["steps"][k]["per_item"]).abs().max())
        print(f"iteration {k}: loss {float(steps[k]['total']):.7f}, difference to eager {d:.3e} (per item {dp:.3e}), bound {ref['loss_bound']:.3e}")
        assert d <= ref["loss_bound"] and dp <= ref["loss_bound"], (k, d, dp, ref["loss_bound"])
    d = max(float((p - q).abs().max()) for p, q in zip(params, ref["params"]))
    print(f"final parameters: largest difference to eager {d:.3e}, bound {ref['param_bound']:.3e}")
    assert d <= ref["param_bound"], (d, ref["param_bound"])


def test_batch_stream_and_trajectory(root3):
    ref = reference(root3)
    steps, params, _step = captured_run(root3)
    for k in range(1, N_REPLAYS + 1):                      # replay k is iteration k of the eager run: the same batch, bit for bit
        for name in ("z", "zt", "x"):
            assert torch.equal(steps[k][name].view(torch.int32), ref["steps"][k][name].view(torch.int32)), (k, name)
    assert len({s["z"].cpu().numpy().tobytes() for s in steps[1:]}) == N_REPLAYS          # and a fresh one every replay
    check_trajectory(ref, steps, params)


def test_interleaved_eager_work_leaves_the_replay_correct(root3):
    from cl_ica_amd import train_3dident as T
    from cl_ica_amd.datasets import BatchLoader

    def between(args, ds, f):
        args.n_eval_samples = 32
        scores = T.evaluate(args, f, iter(BatchLoader(ds, args.batch_size)), True)
        assert np.isfinite(scores[1])
        with torch.no_grad():
            assert f(torch.randn(5, 3, 8, 8, device="cuda")).shape == (5, 3)
        (z, zt), (x, xt) = ds.batch(7)                     # another batch size through nn_search's and the gather's caches
        assert x.shape == (7, 3, 8, 8)

    ref = reference(root3)
    steps, params, step = captured_run(root3, between)
    for k in range(4, N_REPLAYS + 1):
        for name in ("z", "zt", "x"):
            assert torch.equal(steps[k][name].view(torch.int32), ref["steps"][k][name].view(torch.int32)), (k, name)
    check_trajectory(ref, steps, params)


def test_refusals(root3):
    from cl_ica_amd import threedident
    args, ds, f, loss, opt = setup(root3)
    with pytest.raises(TypeError, match="optim.Adam or optim.SGD"):
        threedident.capture_iteration(ds, loss, torch.optim.Adam(f.parameters(), lr=1e-4, capturable=True), f, 16)
    ds.dummy_images = True
    with pytest.raises(ValueError, match="no images"):
        threedident.capture_iteration(ds, loss, opt, f, 16)
    from cl_ica_amd import train_3dident as T
    for flag in ("--dummy-mixing", "--identity-solution", "--identity-mixing-and-solution"):
        with pytest.raises(AssertionError, match="nothing to capture"):
            T.main(["--offline-dataset", root3[0]] + base.COMMON + MODE + ["--graph", flag], images=root3[2], base_encoder=base.backbone)


def test_driver_graph_flag(root3, capsys):
    ref = reference(root3)
    out, text = base.run(root3, MODE + ["--graph"], capsys)
    rows = base.logged(text)
    assert [s for s, _ in rows] == [1, 4], text                                # the schedule of a run without the flag: global steps 0 and 3, printed 1-based
    assert all(np.isfinite(v) for _, v in rows) and len(out["losses"]) == 6 and all(np.isfinite(v) for v in out["losses"])
    for label in ("sigma(loss):", "<Loss>:", "Lin. Disentanglement:", "Perm. Disentanglement (MCC):"):
        vals = base.numbers_after(text, label)
        assert len(vals) >= 2 and all(np.isfinite(v) for v in vals), (label, text)
    assert rows[0][1] == pytest.approx(out["losses"][0], abs=1e-6) and rows[1][1] == pytest.approx(out["losses"][3], abs=1e-6)
    assert int(out["optimizer"].step_dev.item()) == 6
    # the driver's clocked run is the eager clocked run from --seed 1: the evaluations between the steps change nothing
    for k in range(6):
        d = abs(out["losses"][k] - float(ref["steps"][k]["total"]))
        assert d <= ref["loss_bound"], (k, d, ref["loss_bound"])
    # the flag is off by default, and a run without it draws other batches (the module-level generator's)
    plain, _ = base.run(root3, MODE, capsys)
    assert plain["args"].graph == "off" and out["args"].graph == "on" and plain["losses"][0] != out["losses"][0]


def test_driver_graph_with_sgd_and_supervised(root3, capsys):
    from cl_ica_amd import optim
    out, text = base.run(root3, MODE + ["--graph", "--optimizer", "sgd", "--lr", "0.01"], capsys)
    assert type(out["optimizer"]) is optim.SGD and int(out["optimizer"].step_dev.item()) == 6
    assert [s for s, _ in base.logged(text)] == [1, 4] and all(np.isfinite(v) for v in out["losses"]) and len(out["losses"]) == 6
    for kind in ("mse", "r2"):
        out, text = base.run(root3, ["--mode", "supervised", "--position-only", "--supervised-loss", kind, "--lr", "1e-3", "--graph"], capsys)
        assert [s for s, _ in base.logged(text)] == [0, 3], text
        assert len(out["losses"]) == 6 and all(np.isfinite(v) for v in out["losses"]) and len(set(out["losses"])) == 6


def test_driver_graph_with_fixed_constraints(root3, tmp_path_factory, capsys):
    """A fixed bound / radius is a plain host tensor that its layer copies to the device in every forward; the capture needs it on the
    device beforehand (it failed with 'operation not permitted when stream is capturing')."""
    out, text = base.run(root3, MODE + ["--graph", "--box-constraint", "fix"], capsys)
    assert [s for s, _ in base.logged(text)] == [1, 4] and len(set(out["losses"])) == 6 and all(np.isfinite(v) for v in out["losses"])
    assert out["f"][3].max_abs_bound.is_cuda and "3.max_abs_bound" not in out["f"].state_dict()
    root10 = base._root(tmp_path_factory.mktemp("ident10g"), 10)
    extra = ["--mode", "unsupervised", "--non-periodic-rotation-and-color", "--rotation-and-color-only", "--sphere-constraint", "fix", "--graph"]
    out, text = base.run(root10, extra, capsys)
    assert [s for s, _ in base.logged(text)] == [1, 4] and len(set(out["losses"])) == 6 and all(np.isfinite(v) for v in out["losses"])
    assert out["f"][3].r.is_cuda and "3.r" not in out["f"].state_dict()


def test_real_backbone_bf16_graph(tmp_path, capsys, monkeypatch):
    """ResNet-18 (cl_ica_amd.resnet) under ``--amp bf16 --graph``, batch 4, 16 x 16 x 3 images, 4 iterations: it runs, ``conv1`` is handed
    the gather's own channels-last bf16 batch (no transposing copy, no cast) and the model file's keys are what they are without."""
    from cl_ica_amd import resnet
    from cl_ica_amd import train_3dident as T
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    path = str(tmp_path / "ident16")
    import os
    os.makedirs(path)
    n, side = 64, 16
    np.save(os.path.join(path, "raw_latents.npy"), np.random.default_rng(21).uniform(size=(n, 3)).astype(np.float32))
    p = np.arange(side * side * 3, dtype=np.int64).reshape(1, side, side, 3)
    images = ((np.arange(n, dtype=np.int64).reshape(n, 1, 1, 1) * 3 + p * 5) % 256).astype(np.uint8)
    seen, copies = [], []

    def backbone(pretrained, num_classes):
        model = resnet.resnet18(pretrained, num_classes=num_classes)

        def hook(module, inputs):
            x = inputs[0]
            seen.append((torch.is_grad_enabled(), x.dtype, x.is_contiguous(memory_format=torch.channels_last), tuple(x.shape),
                         (resnet.NORM_MODE, resnet.NHWC_MODE, resnet.NHWC_STEM_MODE, resnet.BF16_MODE)))
        model.conv1.register_forward_pre_hook(hook)
        return model

    real = T._amp_batch
    monkeypatch.setattr(T, "_amp_batch", lambda x, amp: (copies.append(torch.is_grad_enabled()), real(x, amp))[1])
    argv = ["--offline-dataset", path, "--batch-size", "4", "--n-eval-samples", "8", "--iterations", "4", "--n-log-steps", "2", "--seed", "1"]
    out = T.main(argv + MODE + ["--amp", "bf16", "--graph"], images=images, base_encoder=backbone)
    torch.cuda.synchronize()
    text = capsys.readouterr().out
    assert [s for s, _ in base.logged(text)] == [1, 3], text
    assert len(out["losses"]) == 4 and all(np.isfinite(v) for v in out["losses"]), out["losses"]
    train = [s for s in seen if s[0]]
    assert len(train) == 4                                  # two views of the eager first iteration, two of the recorded one
    assert all(s[1:] == (torch.bfloat16, True, (4, 3, 16, 16), ("hip",) * 4) for s in train), train
    assert copies and not any(copies)                       # _amp_batch ran for the evaluation batches only
    keys = list(out["f"].state_dict())
    assert keys == list(T.threedident.setup_f(out["args"], 3, 0, base_encoder=resnet.resnet18).state_dict())
    assert all(p.dtype == torch.float32 for p in out["f"].parameters())
