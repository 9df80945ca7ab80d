"""SURVEY.md 8(f) "next" rows on the GPU: N3 checkpoint compatibility with reference-written state dicts (G16), N2 evaluation
metrics on device tensors (G11), plus regression tests for round-1 advisor findings."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PARITY
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu
CKPT = os.path.join(GOLDEN, "g16_ckpt")


def dev(a):
    return torch.tensor(np.asarray(a, np.float32), device="cuda")


def test_n3_reference_checkpoints_load_and_reproduce(golden, tmp_path):
    """unsup_f.pth-style state dicts torch.save'd BY THE REFERENCE's get_mlp modules (every head) and its g.pth load into
    FusedMLP / MixingMLP with strict key matching and reproduce the reference's forward on the GPU; saving them again gives
    a file with identical keys, shapes and bits (main_mlp.py:245-248, 373-381)."""
    from cl_ica_amd import encoders, invertible_network_utils as inu
    z = golden("g16_ckpt.npz").z
    x = dev(z["x"])
    for tag in [str(t) for t in z["names"]]:
        head = tag[2:]; head = None if head == "None" else head
        hidden = [int(h) for h in z[f"{tag}/hidden"]]
        sd = torch.load(os.path.join(CKPT, tag + ".pth"), map_location="cpu")
        f = encoders.get_mlp(4, 4, list(hidden), output_normalization=head)
        missing = f.load_state_dict(sd, strict=True)
        assert not missing.missing_keys and not missing.unexpected_keys
        f = f.to("cuda")
        PARITY.check("n3_checkpoints_g16", tag, "forward", f(x).detach().cpu().numpy(), z[f"{tag}/y"])
        out = tmp_path / (tag + "_resaved.pth")
        torch.save(f.state_dict(), out)
        sd2 = torch.load(out, map_location="cpu")
        assert list(sd2.keys()) == list(sd.keys())
        for k in sd:
            assert sd2[k].shape == sd[k].shape and torch.equal(sd2[k], sd[k]), (tag, k)
    # g.pth into a freshly constructed mixing net AFTER its stack cache was built (advisor finding: stale cache)
    np.random.seed(0)
    g = inu.construct_invertible_mlp(n=4, n_layers=3, act_fct="leaky_relu", cond_thresh_ratio=0.0, n_iter_cond_thresh=50).to("cuda")
    before = g(x).clone()
    sd = torch.load(os.path.join(CKPT, "g.pth"), map_location="cpu")
    assert list(sd.keys()) == list(g.state_dict().keys())
    g.load_state_dict(sd, strict=True)
    y = g(x)
    assert not torch.allclose(before, y)
    PARITY.check("n3_checkpoints_g16", "g.pth", "forward", y.cpu().numpy(), z["g/y"])
    # the trainer's view of g is the same stack
    assert torch.equal(g.weight_stack().cpu(), torch.stack([sd[k] for k in sd]))


def test_n3_supervised_phase_goldens(golden):
    """G24: the SUPERVISED phase of main_mlp.py (the first of the default test_list = [True, False]): five injected steps of
    the reference's train_step with F.mse_loss(z1_rec, z1) (main_mlp.py:258-285, :274-276), run here through train_mlp's own
    step function (autograd_train_step: drop-in encoder / mixing net on the HIP kernels, flat-arena HIP Adam) -- per-step
    loss, step-0 reconstruction and gradients, parameters after five Adam updates."""
    from cl_ica_amd import invertible_network_utils as inu, train_mlp
    from cl_ica_amd.optim import Adam
    from test_gpu_configs import adam_trajectory_check, build_mlp, traj_tol
    from conftest import golden_view
    G = golden("g24_supervised.npz")
    for key, c in G.cases():
        n, B = int(c["meta"]["n"]), int(c["meta"]["B"])
        head = str(c["meta"]["head"]); head = None if head == "None" else head
        hidden = [int(h) for h in c["meta"]["hidden"]]; lr = float(c["meta"]["lr"]); steps = int(c["meta"]["steps"])
        stride = int(c["meta"]["stride"])
        f = build_mlp(n, hidden, head).to("cuda")
        g = inu.MixingMLP([c["in"][f"g{i}"] for i in range(3)], act_fct="leaky_relu").to("cuda")
        h = lambda z: f(g(z))   # noqa: E731
        opt = Adam(f.parameters(), lr=lr)
        fam, case = "n3_supervised_g24", f"{key} n={n} B={B} head={head}"
        for s in range(steps):
            z1, z2 = dev(c["in"][f"z1_{s}"]), dev(c["in"][f"z2_{s}"])
            if s == 0:
                with torch.no_grad():
                    PARITY.check(fam, case, "z1_rec0", h(z1).cpu().numpy(), c["out"]["z1_rec0"])
            tot = train_mlp.autograd_train_step(h, None, opt, z1, z2, supervised=True)
            tl, tn = traj_tol(s)
            PARITY.check(fam, f"{case} step{s}", "loss", tot.item(), c["out"]["loss"][s], tol=tl, note=tn)
            if s == 0:
                for name, prm in f.named_parameters():
                    ref = c["out"][f"grad0/{name}"]
                    PARITY.check(fam + "/grad", case, name, golden_view(prm.grad.cpu().numpy(), ref, stride).reshape(-1), ref.reshape(-1))
        masks = ({k[len("gmin/"):]: v for k, v in c["out"].items() if k.startswith("gmin/")},
                 {k[len("gmax/"):]: float(v) for k, v in c["out"].items() if k.startswith("gmax/")})
        adam_trajectory_check(fam + "/adam_params", key, f, c["out"], "param5", stride, lr, steps, masks=masks)


def test_n2_metrics_on_device(golden):
    """R^2 / MCC of the periodic evaluation (disentanglement_utils.py:63-221) with DEVICE tensors in, against the
    reference's sklearn + Munkres values (G11)."""
    from cl_ica_amd import disentanglement_utils as du
    z9 = golden("g11_metrics.npz").z
    for i in range(int(z9["n_cases"])):
        z, hz = dev(z9[f"c{i}/z"]), dev(z9[f"c{i}/hz"])
        (r2, none), (z2, pred) = du.linear_disentanglement(z, hz, mode="r2")
        assert none is None and pred.shape == z.shape and pred.is_cuda
        PARITY.check("n2_metrics_g11", f"c{i}", "r2", r2, float(z9[f"c{i}/r2"]))
        (mcc, corr), thz = du.permutation_disentanglement(z, hz, mode="pearson", solver="munkres", rescaling=True)
        PARITY.check("n2_metrics_g11", f"c{i}", "mcc", mcc, float(z9[f"c{i}/mcc"]))
        PARITY.check("n2_metrics_g11", f"c{i}", "corr_diag", np.abs(np.diag(corr)), np.abs(z9[f"c{i}/corr_diag"]))
        assert thz.shape == z.shape and thz.is_cuda


def test_n2_all_modes_and_solvers_on_device(golden):
    """Every mode (r2, adjusted_r2, pearson, spearman) x solver (munkres, naive) x rescaling / sign flips / train-test split of
    disentanglement_utils.py:63-221 with device tensors through clica_moments (csrc/moments.hip), against the reference's sklearn /
    scipy / Munkres values (G25, tests/golden/gen_goldens_r4.py)."""
    from cl_ica_amd import disentanglement_utils as du
    from test_host_logic import check_metric_modes

    def check(what, a, b, tol):
        PARITY.check("n2_metric_modes_g25", what.split("/")[0], what, a, b, tol=max(tol, 1e-5), floor=1.0,
                     note=None if tol <= 1e-5 else "rank statistic of fp32-computed values (see test_host_logic.check_metric_modes)")
    assert check_metric_modes(du, golden("g25_metrics_modes.npz").z, dev, check=check) >= 60


@pytest.mark.parametrize("M,da,db", [(4096, 10, 10), (1000, 4, 0), (63, 1, 1), (65, 40, 40), (12288, 64, 64), (517, 3, 7), (300, 100, 100), (257, 150, 0), (513, 70, 130)])
def test_moments_kernel_vs_fp64(M, da, db):
    """clica_moments: G = [A | B | 1]^T [A | B | 1] in fp64 against numpy fp64 on the same fp32 data (exact products, so only the
    summation order differs: 1e-12), on strided views, with and without B, batches that are not whole 64-row chunks, widths beyond one launch."""
    from cl_ica_amd import ops
    rng = np.random.default_rng(M + da)
    a = dev(rng.normal(size=(M, da + 3)) * 3 + 1)[:, 1:1 + da]
    b = dev(rng.uniform(size=(M, db + 2)))[:, :db] if db else None
    G = ops.moments(a, b).cpu().numpy()
    X = np.concatenate([a.cpu().numpy().astype(np.float64)] + ([b.cpu().numpy().astype(np.float64)] if db else []) + [np.ones((M, 1))], 1)
    ref = X.T @ X
    assert G.shape == ref.shape == (da + db + 1, da + db + 1)
    assert np.abs(G - ref).max() <= 1e-12 * np.abs(ref).max() and np.array_equal(G, G.T) and G[-1, -1] == M
    # (more than 129 columns -- n > 64 -- go through the same kernel over 64-column blocks: the last three cases)


def _synthetic_kitti(rng, n_seq=17, hw=64):
    lens = rng.integers(2, 40, size=n_seq)
    data = [rng.random((int(T), hw, hw)) < 0.1 for T in lens]                       # bool masks like the pickle's
    lat = [rng.normal(size=(int(T), 3)).astype(np.float32) for T in lens]
    return {"pedestrians": data, "pedestrians_latents": lat}


def test_kitti_pair_pipeline_matches_oracle():
    """N4, second half: KittiMasks.__getitem__ + custom_collate + return_data (kitti_masks/dataset.py:90-175) on the
    device -- batched index arithmetic + ONE gather launch -- against the oracle's restatement item by item: every start index of the
    synthetic data set with every time step 1..5 (sequence ends clamp), bit-exact images and labels, interleaving; the loader's epoch
    visits every index at most once, drops the ragged tail, draws time steps in 1..max_delta_t; the Solver trains from it."""
    import types
    from cl_ica_amd.kitti_masks import dataset as D
    rng = np.random.default_rng(5)
    raw = _synthetic_kitti(rng)
    ds = D.KittiMasks(data=raw, max_delta_t=5)
    cum = np.cumsum([len(s) - 1 for s in raw["pedestrians"]])
    assert len(ds) == int(cum[-1]) and ds.frames.dtype == torch.uint8
    idx = np.repeat(np.arange(len(ds)), 5); tt = np.tile(np.arange(1, 6), len(ds))
    img, lab = ds.batch(torch.as_tensor(idx), torch.as_tensor(tt))
    ref = O.kitti_collate([O.kitti_getitem(raw["pedestrians"], raw["pedestrians_latents"], cum, int(i), int(t)) for i, t in zip(idx, tt)])
    assert img.shape == (2 * len(idx), 1, 64, 64) and lab.shape == (2 * len(idx), 3) and img.dtype == torch.float32
    assert np.array_equal(img.cpu().numpy(), ref[0]) and np.array_equal(lab.cpu().numpy(), ref[1])       # bit-exact (byte data)
    # the host-style accessors and the reference's collate give the same batch
    np.random.seed(3)
    items = [ds[i] for i in (0, 5, len(ds) - 1)]
    ci, cl = D.custom_collate(items)
    assert ci.shape == (6, 1, 64, 64) and torch.equal(ci[0], torch.tensor(items[0][0])) and torch.equal(ci[1], torch.tensor(items[0][1]))
    assert set(np.unique(ci.numpy())) <= {0.0, 1.0}
    # loader semantics of return_data (:145-175)
    a = types.SimpleNamespace(dataset="KittiMasks", batch_size=64, num_workers=0, image_size=64, evaluate=False, kitti_max_delta_t=3, seed=11)
    loader = D.return_data(a, data=raw)
    assert loader.pairs == 32 and len(loader) == len(ds) // 32
    seen = []
    first_of_batch = None
    for images, labels in loader:
        assert images.shape == (64, 1, 64, 64) and labels.shape == (64, 3) and images.is_cuda
        seen.append(labels[::2].cpu().numpy())
        first_of_batch = images if first_of_batch is None else first_of_batch
    seen = np.concatenate(seen)
    all_first = np.concatenate([l[:-1] for l in raw["pedestrians_latents"]])
    keys = {tuple(np.round(r, 6)) for r in all_first}
    assert len({tuple(np.round(r, 6)) for r in seen}) == len(seen) == len(loader) * 32 and all(tuple(np.round(r, 6)) in keys for r in seen)
    ts = loader.dataset.sample_time_steps(20000).cpu().numpy()
    assert ts.min() == 1 and ts.max() == 3 and abs((ts == 2).mean() - 1 / 3) < 0.02
    e1 = next(iter(loader))[1]; e2 = next(iter(loader))[1]
    assert not torch.equal(e1, e2)                                                   # a fresh permutation every epoch
    # and the Solver consumes the batches (one iteration from the device loader)
    from cl_ica_amd.kitti_masks.solver import Solver
    sa = types.SimpleNamespace(cuda=True, ckpt_dir="/tmp", output_dir="/tmp", dataset="kitti", max_iter=1, z_dim=5, num_channel=1, lr=1e-4,
                               beta1=0.9, beta2=0.999, ckpt_name="last", log_step=10, save_step=10 ** 9, box_norm=True, p=1)
    S = Solver(sa, loader)
    S.net_mode(train=True)
    assert bool(torch.isfinite(S.train_iteration(first_of_batch)))


def test_autograd_loss_uses_forward_rowgrad_and_matches_row_pass():
    """Advisor finding: the flash-style row gradient of the forward sweep was never requested from losses.py.  Now it is
    whenever z1_rec needs a gradient; the result must equal the recomputing row pass of clica_lp_loss_bwd (rowgrad = NULL)."""
    import ctypes as C
    from cl_ica_amd import _lib
    from cl_ica_amd.losses import LpSimCLRLoss, SimCLRLoss, _PairLossFn
    torch.manual_seed(0)
    B, B3, n = 700, 900, 10
    z1 = torch.randn(B, n, device="cuda") * 0.7; z2 = z1 + 0.05 * torch.randn_like(z1); z3 = torch.randn(B3, n, device="cuda") * 0.7
    lib = _lib.load()
    for p in (1, 2, 3):
        a = z1.clone().requires_grad_(True); b = z2.clone().requires_grad_(True); c = z3.clone().requires_grad_(True)
        L = LpSimCLRLoss(p=p, tau=0.9, alpha=0.4, simclr_compatibility_mode=True)
        tot, per, _ = L(None, None, None, a, b, c)
        assert tot.grad_fn.rowgrad is not None            # the forward accumulated the row gradient
        tot.backward()
        d = L._desc(B, B3, n)
        fb, bb = C.c_size_t(), C.c_size_t()
        _lib.check(lib.clica_lp_loss_workspace_bytes(C.byref(d), C.byref(fb), C.byref(bb)), "ws")
        ws = torch.zeros(max(fb.value, bb.value), dtype=torch.uint8, device="cuda")
        o = torch.empty(3 * B + 3, device="cuda")
        dz = [torch.empty(B, n, device="cuda"), torch.empty(B, n, device="cuda"), torch.empty(B3, n, device="cuda")]
        _lib.check(lib.clica_lp_loss_fwd(C.byref(d), z1.data_ptr(), n, z2.data_ptr(), n, z3.data_ptr(), n, o[:B].data_ptr(),
                                         o[B:2 * B].data_ptr(), o[2 * B:3 * B].data_ptr(), o[3 * B:].data_ptr(), None, n,
                                         ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "fwd")
        _lib.check(lib.clica_lp_loss_bwd(C.byref(d), z1.data_ptr(), n, z2.data_ptr(), n, z3.data_ptr(), n, o[2 * B:3 * B].data_ptr(),
                                         None, n, None, None, None, None, dz[0].data_ptr(), n, dz[1].data_ptr(), n, dz[2].data_ptr(), n, 0,
                                         ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "bwd")
        torch.cuda.synchronize()
        for got, ref, nm in ((a.grad, dz[0], "dz1"), (b.grad, dz[1], "dz2"), (c.grad, dz[2], "dz3")):
            PARITY.check("rowgrad_vs_row_pass", f"p={p}", nm, got.cpu().numpy(), ref.cpu().numpy(), tol=3e-6, note="HIP vs HIP")
    # z1 without gradient: no row gradient is requested
    tot, _, _ = LpSimCLRLoss(p=2)(None, None, None, z1, z2.clone().requires_grad_(True), z3)
    assert tot.grad_fn.rowgrad is None


def test_flat_adam_matches_torch_adam():
    """cl_ica_amd.optim.Adam (one HIP launch over a flat arena) against torch.optim.Adam on the same gradients, and its
    state_dict in torch's layout."""
    from cl_ica_amd.optim import Adam
    torch.manual_seed(0)
    mk = lambda: torch.nn.Sequential(torch.nn.Linear(7, 13), torch.nn.Linear(13, 5)).cuda()   # noqa: E731
    a, b = mk(), mk()
    b.load_state_dict(a.state_dict())
    oa, ob = Adam(a.parameters(), lr=1e-2), torch.optim.Adam(b.parameters(), lr=1e-2)
    for s in range(6):
        x = torch.randn(32, 7, device="cuda")
        for m, o in ((a, oa), (b, ob)):
            o.zero_grad()
            (m(x) ** 2).mean().backward()
            o.step()
    for (k, p), q in zip(a.named_parameters(), b.parameters()):
        PARITY.check("flat_adam_vs_torch", "6 steps", k, p.detach().cpu().numpy(), q.detach().cpu().numpy(), tol=2e-6, note="vs torch.optim.Adam")
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sa["state"].keys() == sb["state"].keys() and int(sa["state"][0]["step"]) == 6
    for i in sa["state"]:
        assert torch.allclose(sa["state"][i]["exp_avg"], sb["state"][i]["exp_avg"], rtol=1e-5, atol=1e-8)
    oc = Adam(mk().parameters(), lr=1.0)
    oc.load_state_dict(sa)
    assert oc.param_groups[0]["lr"] == 1e-2 and int(oc.step_dev.item()) == 6 and torch.equal(oc.exp_avg, oa.exp_avg)


@pytest.mark.parametrize("opt_kind", ["torch", "flat"])
def test_dropin_fused_path_matches_per_layer_path(opt_kind, monkeypatch):
    """FusedMLP under autograd: the whole-encoder kernels (clica_mlp_fwd / clica_mlp_dgrad / clica_mlp_wgrad, taken for large
    batches) against the per-layer GEMM path on the same data, through two optimizer steps (the fragment-order weight cache
    must follow the parameter updates of torch.optim.Adam AND of the raw-pointer cl_ica_amd.optim.Adam), with the reference's
    two-calls-per-step structure and an input that needs a gradient."""
    from cl_ica_amd import encoders, losses, optim
    res = {}
    for fused in ("1", "0"):
        monkeypatch.setattr("cl_ica_amd.encoders.FUSED_MODE", fused)
        torch.manual_seed(0)
        f = encoders.get_mlp(10, 10, [100, 500, 500, 100]).cuda()
        opt = torch.optim.Adam(f.parameters(), lr=1e-3) if opt_kind == "torch" else optim.Adam(f.parameters(), lr=1e-3)
        L = losses.LpSimCLRLoss(p=2, tau=1.0, simclr_compatibility_mode=True)
        g = torch.Generator().manual_seed(1)
        outs = []
        for s in range(3):
            x1 = torch.rand(1000, 10, generator=g).cuda().requires_grad_(True)
            x2 = (x1.detach() + 0.05 * torch.randn(1000, 10, generator=g).cuda())
            opt.zero_grad()
            a, b = f(x1), f(x2)
            tot, _, _ = L(None, None, None, a, b, torch.roll(a, 1, 0))
            tot.backward()
            outs.append((tot.item(), x1.grad.clone(), [p.grad.clone() for p in f.parameters()]))
            opt.step()
        res[fused] = (outs, [p.detach().clone() for p in f.parameters()])
    for s in range(3):
        (la, dxa, ga), (lb, dxb, gb) = res["1"][0][s], res["0"][0][s]
        PARITY.check("dropin_fused_vs_per_layer", f"{opt_kind} step{s}", "loss", la, lb, tol=2e-6 * (10 ** s), note="HIP vs HIP")
        if s == 0:
            PARITY.check("dropin_fused_vs_per_layer", f"{opt_kind} step0", "dx", dxa.cpu().numpy(), dxb.cpu().numpy(), tol=3e-6, note="HIP vs HIP")
            for k, (u, v) in enumerate(zip(ga[:-1], gb[:-1])):     # last bias: exact gradient 0
                PARITY.check("dropin_fused_vs_per_layer", f"{opt_kind} step0", f"grad{k}", u.cpu().numpy(), v.cpu().numpy(), tol=3e-6, note="HIP vs HIP")
    assert res["1"][0][2][0] < res["1"][0][0][0]          # it trains: the packs followed the weights


@pytest.mark.parametrize("B,p", [(6144, 2), (1000, 1), (333, 3)])
def test_dropin_lazy_stacking_and_symmetric_loss_match_plain_path(B, p, monkeypatch):
    """the reference's train_step structure (main_mlp.py:258-285: two encoder calls, roll, LpSimCLRLoss, backward)
    on the drop-in modules.  Default path: the first f(.) is deferred, the second call stacks both batches into one launch per phase
    (cl_ica_amd/lazy.py), and the loss recognises z3_rec = roll(z1_rec) in the autograd graph and takes the one-sweep symmetric backward.
    Against the same step with both mechanisms off (CLICA_DROPIN_LAZY=0, losses.SYM_ENABLED = False: two half-size encoder passes, rolled copy,
    generic two-sweep backward) and against the fp64 oracle: loss, per-item losses, embeddings, every parameter gradient."""
    from cl_ica_amd import encoders, lazy, losses, optim
    n = 10
    res = {}
    g = torch.Generator().manual_seed(B)
    x1 = torch.rand(B, n, generator=g).cuda()
    x2 = (x1 + 0.05 * torch.randn(B, n, generator=g).cuda()).clamp(0, 1)
    for mode in ("fast", "plain"):
        monkeypatch.setenv("CLICA_DROPIN_LAZY", "1" if mode == "fast" else "0")
        monkeypatch.setattr(losses, "SYM_ENABLED", mode == "fast")
        f = build_mlp_n10().cuda()
        opt = optim.Adam(f.parameters(), lr=1e-3)
        L = losses.LpSimCLRLoss(p=p, tau=1.0, simclr_compatibility_mode=True)
        opt.zero_grad()
        a = f(x1)
        assert isinstance(a, lazy.LazyOut) == (mode == "fast") and tuple(a.shape) == (B, n) and a.device.type == "cuda"
        b = f(x2)
        assert not isinstance(b, lazy.LazyOut)
        z3 = torch.roll(a, 1, 0)
        assert losses._rolled_rows_of(z3, lazy.plain(a))
        tot, item, (pos, neg) = L(None, None, None, a, b, z3)
        before = dict(losses.PATHS)
        tot.backward()
        ran = {k: v - before.get(k, 0) for k, v in losses.PATHS.items() if v != before.get(k, 0)}
        # the backward the reference's train_step gets: ONE symmetric pair sweep (round 3 took the two-sweep fallback here without
        # anybody noticing: autograd handed the unused per-item output a tensor of zeros, which read as "a per-item upstream gradient")
        assert ran == ({"sym_one_sweep": 1} if mode == "fast" else {"generic": 1}), ran
        # .item() of the three scalars: one device copy, the same numbers Tensor.item returns
        assert (tot.item(), pos.item(), neg.item()) == (torch.Tensor.item(tot), torch.Tensor.item(pos), torch.Tensor.item(neg))
        # the whole-encoder kernels run in the engine's default arithmetic (f16x2) because the flat Adam owns the parameters
        fused_rows = 2 * B if mode == "fast" else B
        assert encoders.arith_state(f)["arith"] == ("f16x2" if (fused_rows + 47) // 48 >= 128 else "bf16x3")
        res[mode] = dict(loss=tot.item(), item=item.detach().cpu().numpy(), pos=pos.item(), neg=neg.item(), a=lazy.plain(a).detach().cpu().numpy(),
                         b=b.detach().cpu().numpy(), grads=[q.grad.detach().cpu().numpy().copy() for q in f.parameters()], f=f)
    fam, case = "dropin_lazy_sym", f"B={B} p={p}"
    lin = [m for m in res["fast"]["f"] if isinstance(m, torch.nn.Linear)]
    P = O.MLPParams([m.weight.detach().cpu().numpy().astype(np.float64) for m in lin], [m.bias.detach().cpu().numpy().astype(np.float64) for m in lin])
    y, cache = O.mlp_forward(P, np.concatenate([x1.cpu().numpy(), x2.cpu().numpy()]))
    ref = O.lp_simclr_loss(y[:B], y[B:], np.roll(y[:B], 1, 0), p=p, compat=True)
    for mode in ("fast", "plain"):
        r = res[mode]
        PARITY.check(fam, case, f"embeddings z1 [{mode}]", r["a"], y[:B]); PARITY.check(fam, case, f"embeddings z2 [{mode}]", r["b"], y[B:])
        PARITY.check(fam, case, f"loss [{mode}]", r["loss"], ref["loss_mean"])
        PARITY.check(fam, case, f"loss_i [{mode}]", r["item"], ref["loss_i"])
    # gradients: the two HIP paths against each other (p = 1 sign ties / LeakyReLU kinks make an end-to-end fp64 comparison a test of
    # those, see test_c3_engine_full_size_vs_oracle); the last bias has an exactly-zero gradient
    for k, (u, v) in enumerate(zip(res["fast"]["grads"][:-1], res["plain"]["grads"][:-1])):
        PARITY.check(fam, case, f"grad{k} fast vs plain", u, v, tol=1e-5 if p != 1 else 5e-5, note=None if p != 1 else "p = 1 sign ties (see p1_tie_analysis)")
    assert np.abs(res["fast"]["grads"][-1]).max() < 1e-6 * max(1.0, float(np.abs(res["fast"]["grads"][-2]).max()) * 1e3)


def build_mlp_n10():
    from test_gpu_configs import build_mlp
    return build_mlp(10, [100, 500, 500, 100], None, gain=1.8)


def test_dropin_lazy_input_mutation_is_loud_and_first_use_on_another_stream():
    """(a) an input written in place between the call and the first use of its deferred output raises (the output for the OLD
    values can no longer be computed) instead of silently giving the output for the new ones; (b) a first use on another stream runs
    the deferred launches on the CALL's stream and makes the using stream wait: same numbers as an eager call."""
    from cl_ica_amd import encoders, lazy
    torch.manual_seed(5)
    f = encoders.get_mlp(6, 6, [32, 64]).cuda()
    x = torch.rand(128, 6, device="cuda")
    a = f(x)
    assert isinstance(a, lazy.LazyOut)
    x.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified in place"):
        a.sum()
    x = torch.rand(128, 6, device="cuda")
    want = lazy.plain(f(x)).detach().clone()
    torch.cuda.synchronize()
    b = f(x)
    assert isinstance(b, lazy.LazyOut)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side), torch.no_grad():
        got = (b * 1.0)
    torch.cuda.synchronize()
    assert got.requires_grad is False and lazy.plain(b).requires_grad        # the call was made with grad mode on
    assert torch.equal(got, want)


def test_dropin_lazy_output_single_use_and_per_item_upstream():
    """A deferred output that is used before a second call runs on its own; a per-item upstream gradient takes the aliasing generic
    backward inside the symmetric node (clica_lp_loss_bwd with z3 = z1, column part accumulated) -- against the plain path."""
    from cl_ica_amd import encoders, lazy, losses
    torch.manual_seed(3)
    f = encoders.get_mlp(6, 6, [32, 64]).cuda()
    x1, x2 = torch.rand(200, 6, device="cuda"), torch.rand(200, 6, device="cuda")
    a = f(x1)
    assert isinstance(a, lazy.LazyOut)
    s = float(a.sum())                                    # any torch function materialises it
    assert a._value is not None and abs(s - float(f(x1).sum())) < 1e-4 * abs(s)
    L = losses.LpSimCLRLoss(p=2, tau=0.7, simclr_compatibility_mode=False)
    w = torch.rand(200, device="cuda")
    for q in f.parameters():
        q.grad = None
    a, b = f(x1), f(x2)
    tot, item, _ = L(None, None, None, a, b, torch.roll(a, 1, 0))
    (tot + (w * item).sum()).backward()
    outs = [[q.grad.clone() for q in f.parameters()]]
    # the same through the GENERIC node (autograd routes d loss / d z3 back through the roll)
    losses.SYM_ENABLED = False
    try:
        for q in f.parameters():
            q.grad = None
        a, b = f(x1), f(x2)
        tot, item, _ = L(None, None, None, a, b, torch.roll(a, 1, 0))
        (tot + (w * item).sum()).backward()
        ref = [q.grad.clone() for q in f.parameters()]
    finally:
        losses.SYM_ENABLED = True
    for k, (u, v) in enumerate(zip(outs[0][:-1], ref[:-1])):
        PARITY.check("dropin_lazy_sym", "per-item upstream", f"grad{k}", u.cpu().numpy(), v.cpu().numpy())


def test_dropin_stacked_outputs_are_ordinary_tensors():
    """The two results of a stacked call are outputs of ONE autograd node on one buffer: using only one of them, modifying one in
    place, and scalars whose tensor was written after the loss call must all behave like the plain path."""
    from cl_ica_amd import encoders, lazy, losses
    torch.manual_seed(5)
    f = encoders.get_mlp(10, 10, [100, 500, 100]).cuda()
    x1, x2 = torch.rand(6144, 10, device="cuda"), torch.rand(6144, 10, device="cuda")

    def grads(fn):
        for q in f.parameters():
            q.grad = None
        fn().backward()
        return [q.grad.clone() for q in f.parameters()]

    def only_second():
        a, b = f(x1), f(x2)
        assert isinstance(a, lazy.LazyOut)
        return (b ** 2).mean()                        # a is never used: its gradient arrives as None

    def plain_second():
        return (f(torch.cat([x2, x2]))[:6144] ** 2).mean()      # (>= 256 panels: not deferred)

    for k, (u, v) in enumerate(zip(grads(only_second), grads(plain_second))):
        PARITY.check("dropin_lazy_sym", "one of two outputs used", f"grad{k}", u.cpu().numpy(), v.cpu().numpy(), tol=2e-6, note="HIP vs HIP")

    def inplace_first():
        a, b = f(x1), f(x2)
        a = lazy.plain(a)
        a *= 2.0                                      # in place on one of the two outputs
        return (a * b).mean()

    def functional_first():
        y = f(torch.cat([x1, x2]))
        return (2.0 * y[:6144] * y[6144:]).mean()

    for k, (u, v) in enumerate(zip(grads(inplace_first), grads(functional_first))):
        PARITY.check("dropin_lazy_sym", "in-place on a stacked output", f"grad{k}", u.cpu().numpy(), v.cpu().numpy(), tol=2e-6, note="HIP vs HIP")
    L = losses.LpSimCLRLoss(p=2, tau=1.0, simclr_compatibility_mode=True)
    a, b = f(x1), f(x2)
    tot, _, (pos, neg) = L(None, None, None, a, b, torch.roll(a, 1, 0))
    v = torch.Tensor.item(pos)
    with torch.no_grad():
        pos.mul_(3.0)                                 # written after the call: the shared copy must not answer for it
    assert abs(pos.item() - 3.0 * v) <= 1e-6 * abs(v) and tot.item() == torch.Tensor.item(tot)


def test_dropin_autograd_grad_does_not_touch_the_arena():
    """with the flat optimizer installed, torch.autograd.grad(y, x) / jacobian (reference losses.py:279) through the encoder
    must not add dW / db into the parameters' .grad, and autograd.grad(loss, params) must return the gradients."""
    from cl_ica_amd import encoders, optim
    torch.manual_seed(0)
    f = encoders.get_mlp(10, 10, [100, 500, 500, 100]).cuda()
    opt = optim.Adam(f.parameters(), lr=1e-3)
    opt.zero_grad()
    x = torch.rand(6144, 10, device="cuda", requires_grad=True)
    y = f(x)
    (dx,) = torch.autograd.grad(y.sum(), x)
    assert dx.shape == x.shape and float(dx.abs().max()) > 0
    assert float(opt.grad_arena.abs().max()) == 0.0                  # nothing leaked into the arena
    y = f(x)
    gs = torch.autograd.grad((y ** 2).mean(), list(f.parameters()))
    assert all(g is not None and torch.isfinite(g).all() for g in gs) and float(opt.grad_arena.abs().max()) == 0.0
    y = f(x)
    (y ** 2).mean().backward()                                         # the plain backward accumulates in place
    for q, g in zip(f.parameters(), gs):
        PARITY.check("dropin_inplace_grads", "autograd.grad vs backward", "param grad", q.grad.cpu().numpy(), g.cpu().numpy(), tol=2e-6, note="HIP vs HIP")
    hits = []
    h = next(f.parameters()).register_hook(lambda g: hits.append(1))   # a tensor hook must fire: in-place accumulation steps aside
    opt.zero_grad(); y = f(x); (y ** 2).mean().backward(); h.remove()
    assert hits and float(next(f.parameters()).grad.abs().max()) > 0


def test_mixing_net_activations_goldens(golden):
    """Every hidden activation construct_invertible_mlp offers (--act-fct relu | leaky_relu | elu | smooth_leaky_relu | softplus,
    invertible_network_utils.py:51-66): the reference's weights loaded into MixingMLP, forward on the HIP kernel vs G17; the
    module list (state-dict layout) matches; the engine takes a non-piecewise-linear g through its separate mixing launch."""
    from cl_ica_amd import invertible_network_utils as inu, encoders
    from cl_ica_amd.engine import ContrastiveTrainer, SamplerSpec
    z = golden("g17_mixing_acts.npz").z
    for act in [str(a) for a in z["acts"]]:
        Ws = [z[f"{act}/W{l}"] for l in range(3)]
        g = inu.MixingMLP(Ws, act_fct=act).to("cuda")
        assert [type(m).__name__ for m in g] == [str(m) for m in z[f"{act}/modules"]]
        y = g(dev(z[f"{act}/x"]))
        PARITY.check("mixing_activations_g17", act, "forward", y.cpu().numpy(), z[f"{act}/y"])
        import contextlib, io
        np.random.seed(1)
        with contextlib.redirect_stdout(io.StringIO()):
            g2 = inu.construct_invertible_mlp(n=6, n_layers=3, act_fct=act, cond_thresh_ratio=0.0, n_iter_cond_thresh=50).to("cuda")
        assert g2.act_fct == act
        f = encoders.get_mlp(6, 6, [12, 24, 12])
        tr = ContrastiveTrainer(f, g2.weight_stack(), SamplerSpec(n=6), batch_size=256, p=2, lr=1e-3, g_slope=g2.slope,
                                g_act_kind=g2.act_kind, device="cuda")
        out = tr.step()
        assert torch.isfinite(out).all()
        assert torch.allclose(tr.x, g2(tr.z), rtol=1e-6, atol=1e-6)          # the engine's x = g(z) is the module's forward
    with pytest.raises(Exception):
        inu.construct_invertible_mlp(n=4, n_layers=2, act_fct="tanh")


# ---------------------------------------------------------------------------------------------- N4: latent lookup
@pytest.mark.parametrize("N,Q,n,k", [(60000, 700, 10, 2), (5000, 33, 3, 1), (4097, 257, 17, 4), (300, 64, 64, 2), (3, 5, 7, 4)])
def test_nn_search_vs_oracle(N, Q, n, k):
    """clica_nn_search (exact squared-L2 k-NN, the faiss.IndexFlatL2 lookup of threedident_dataset.py:104-105) against the
    fp64 oracle: same rows wherever the fp64 gap to the next candidate is resolvable in fp32, distances to 1e-5."""
    from cl_ica_amd import ops
    rng = np.random.default_rng(N + Q)
    tab = rng.uniform(-1, 1, size=(N, n)).astype(np.float32)
    qry = rng.uniform(-1, 1, size=(Q, n)).astype(np.float32)
    dist, idx = ops.nn_search(torch.tensor(tab, device="cuda"), torch.tensor(qry, device="cuda"), k)
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    D, I = O.flat_l2_search(tab, qry, min(k + 1, N))
    kk = min(k, N)
    assert (idx[:, kk:] == -1).all()                                    # fewer rows than k: padded like faiss
    scale = float(n)                                                    # |q - t|^2 <= 4 n; fp32 sum of n terms
    gap_ok = np.ones((Q, kk), bool)
    for c in range(kk):                                                 # column c is decided if its fp64 neighbours are not near-ties
        if c + 1 < D.shape[1]:
            gap_ok[:, c] &= (D[:, c + 1] - D[:, c]) > 1e-6 * scale
        if c > 0:
            gap_ok[:, c] &= (D[:, c] - D[:, c - 1]) > 1e-6 * scale
    assert gap_ok.mean() > 0.95
    assert (idx[:, :kk][gap_ok] == I[:, :kk][gap_ok]).all()
    PARITY.check("nn_search", f"N={N} Q={Q} n={n} k={k}", "dist", dist[:, :kk], D[:, :kk], floor=1e-3 * scale)
    # every returned row really is at the returned distance, and the columns ascend
    got = ((qry[:, None, :].astype(np.float64) - tab[idx[:, :kk]].astype(np.float64)) ** 2).sum(-1)
    assert np.abs(got - dist[:, :kk]).max() <= 1e-5 * max(got.max(), 1e-3 * scale)
    assert (np.diff(dist[:, :kk], axis=1) >= 0).all()


def test_nn_search_ties_and_errors():
    from cl_ica_amd import ops
    from cl_ica_amd._lib import ClicaError
    g = np.stack(np.meshgrid(np.arange(6), np.arange(5), np.arange(4), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    tab = np.concatenate([g, g])                                        # every row twice: the earlier copy wins
    d, i = ops.nn_search(torch.tensor(tab, device="cuda"), torch.tensor(g + 0.25, device="cuda"), 2)
    assert (i[:, 0].cpu().numpy() == np.arange(len(g))).all() and (i[:, 1].cpu().numpy() == np.arange(len(g)) + len(g)).all()
    assert torch.allclose(d, torch.full_like(d, 3 * 0.25 ** 2))
    with pytest.raises(ClicaError):
        ops.nn_search(torch.zeros(8, 65, device="cuda"), torch.zeros(2, 65, device="cuda"), 1)
    with pytest.raises(ClicaError):
        ops.nn_search(torch.zeros(8, 4, device="cuda"), torch.zeros(2, 4, device="cuda"), 5)
    with pytest.raises(ClicaError):
        ops.nn_search(torch.zeros(8, 4), torch.zeros(2, 4), 1)          # host tensors: no fallback


def test_threedident_latent_pairs_full_size():
    """ThreeDIdentDataset.__getitem__'s latent lookup (threedident_dataset.py:96-116) for a batch of 1024 pairs over a table
    of the dataset's size (250 000 x 10): properties at full size + the oracle on a sample of the batch."""
    from cl_ica_amd import latent_spaces, spaces
    from cl_ica_amd.datasets import IndexFlatL2, ThreeDIdentLatentPairs
    rng = np.random.default_rng(7)
    N, n, B = 250000, 10, 1024
    table = rng.uniform(-1, 1, size=(N, n)).astype(np.float32)
    space = spaces.NBoxSpace(n, -1.0, 1.0)
    ls = latent_spaces.LatentSpace(space, lambda sp, size, device="cuda": sp.uniform(size, device=device),
                                   lambda sp, z, size, device="cuda": sp.normal(z, 0.05, size, device=device))
    spaces.manual_seed(3)
    ds = ThreeDIdentLatentPairs(table, ls)
    assert len(ds) == N
    iz, izt, z, zt = ds.sample(B)
    assert iz.shape == (B,) and iz.dtype == torch.int64 and (iz != izt).all()
    assert torch.equal(z, ds.latents[iz]) and torch.equal(zt, ds.latents[izt])
    # rows of the table find themselves at distance 0 (encode -> lookup round trip at full size)
    pick = torch.tensor(rng.choice(N, 2048, replace=False), device="cuda")
    index = IndexFlatL2(n); index.add(table)
    assert index.ntotal == N
    D, I = index.search(ds.latents[pick], 2)
    assert torch.equal(I[:, 0], pick) and (D[:, 0] == 0).all() and (I[:, 1] != pick).all() and (D[:, 1] > 0).all()
    # the snapping rule against the oracle on a sample (fresh draws with a known pre-image)
    zq = torch.tensor(rng.uniform(-1, 1, size=(48, n)).astype(np.float32), device="cuda")
    ztq = (zq + 0.01 * torch.tensor(rng.normal(size=(48, n)).astype(np.float32), device="cuda")).clamp(-1, 1)
    a, b, _, _ = ds.snap(zq, ztq)
    oa, ob = O.threedident_snap(table, zq.cpu().numpy(), ztq.cpu().numpy())
    assert (a.cpu().numpy() == oa).all() and (b.cpu().numpy() == ob).all()
    assert (a == b).sum() == 0 and (torch.tensor(oa) == O.flat_l2_search(table, ztq.cpu().numpy(), 1)[1][:, 0]).any()   # the exclusion rule fired


def test_device_time_stamps_inside_a_graph():
    """clica_stamp (bench.py's in-graph timing): begin / end stamps around a known amount of work inside a captured graph give
    one completed interval per replay, in the ring order, of plausible length (the work is ~100 us of matmuls)."""
    from cl_ica_amd import ops
    dev = torch.device("cuda")
    slot = torch.zeros(1 + 2 * 4, dtype=torch.int64, device=dev)
    a = torch.randn(2048, 2048, device=dev)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        (a @ a).sum().item()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            ops.stamp(slot, 0)
            b = a @ a
            b = b @ a
            ops.stamp(slot, 1)
        for _ in range(6):          # six replays into a ring of four: the last four survive
            g.replay()
    torch.cuda.synchronize()
    iv = ops.stamp_intervals_us(slot)
    assert int(slot[0].item()) == 6 and len(iv) == 4
    assert all(20.0 < v < 20000.0 for v in iv), iv
    # the shader-clock probe (clica_clock_probe) on a side stream while the same graph replays: cycles / wall time inside a bracket is a
    # clock between idle and the 2.4 GHz peak
    # (HIP multiplexes streams onto a few hardware queues in creation order: in a long test session the probe's stream can land on the SAME
    #  queue as the replaying stream, the two then run one after the other and no sample falls into a bracket -- try a few fresh streams)
    ghz = []
    for _attempt in range(6):
        side = torch.cuda.Stream()
        probe = ops.clock_probe(3000, 10.0, side)
        with torch.cuda.stream(s):
            for _ in range(40):
                g.replay()
        torch.cuda.synchronize()
        smp = probe.cpu().numpy()
        assert (smp[:, 0] > 0).all() and (np.diff(smp[:, 0]) >= 1000).all()          # 3000 samples, >= 10 us apart
        ghz = [ops.clock_between(smp, b0, b1) for b0, b1 in ops.stamp_brackets(slot)]
        ghz = [x for x in ghz if x is not None]
        if len(ghz) >= 2:
            break
    assert len(ghz) >= 2 and all(0.3 < x < 2.6 for x in ghz), ghz


@pytest.mark.parametrize("flat_arith", ["bf16x3", "f16x2"])
def test_dropin_flat_adam_in_place_gradient_accumulation(flat_arith, monkeypatch):
    """The reference's train_step structure (two encoder calls per step, main_mlp.py:258-285) on the drop-in modules with
    cl_ica_amd.optim.Adam: the fused encoder backward adds dW / db straight into the optimizer's gradient arena (autograd gets
    None).  Three steps against the same loop with torch.optim.Adam (ordinary autograd accumulation): parameters agree.
    `bf16x3`: both sides in the same arithmetic (the flat side's f16x2 switched off) -- the accumulation path alone is under test;
    `f16x2`: the flat side in its default arithmetic against torch.optim.Adam's bf16x3 -- gradients differ at rounding level, which Adam
    turns into steps of a fraction of lr for the few elements whose gradient IS at rounding level (measured: 4e-4 of a layer's elements
    beyond 10 % of lr, the largest at 40 %): all but 1e-3 of the elements within 10 % of
    lr, none beyond the three steps' total travel."""
    from cl_ica_amd import encoders, losses, optim
    monkeypatch.setattr("cl_ica_amd.encoders.FUSED_MODE", "1")
    monkeypatch.setattr("cl_ica_amd.encoders.S16_ENABLED", flat_arith == "f16x2")
    n, B = 10, 1536
    loss = losses.LpSimCLRLoss(p=2, tau=1.0, simclr_compatibility_mode=True)
    outs = {}
    for kind in ("flat", "torch"):
        torch.manual_seed(3)
        f = encoders.get_mlp(n_in=n, n_out=n, layers=[n * 10, n * 50, n * 50, n * 10]).to("cuda")
        opt = optim.Adam(f.parameters(), lr=1e-3) if kind == "flat" else torch.optim.Adam(f.parameters(), lr=1e-3)
        g = torch.Generator(device="cuda").manual_seed(11)
        for _ in range(3):
            z1 = torch.rand(B, n, device="cuda", generator=g); z2 = (z1 + 0.05 * torch.randn(B, n, device="cuda", generator=g)).clamp(0, 1)
            opt.zero_grad()
            a, b = f(z1), f(z2)
            tot, _, _ = loss(z1, z2, torch.roll(z1, 1, 0), a, b, torch.roll(a, 1, 0))
            tot.backward()
            if kind == "flat":
                assert all(p.grad.data_ptr() == p._clica_grad_view.data_ptr() for p in f.parameters())
            opt.step()
        assert encoders.arith_state(f)["arith"] == (flat_arith if kind == "flat" else "bf16x3")
        outs[kind] = [p.detach().clone() for p in f.parameters()] + [tot.detach().clone()]
    # (two Adam implementations, three steps at lr = 1e-3: rounding-level gradient differences move an element by << lr)
    params = list(zip(outs["flat"][:-1], outs["torch"][:-1]))
    for i, (a, b) in enumerate(params):
        # 10 % of lr: an element whose gradient is at rounding level.  The LAST bias is all such elements: the loss sees only differences
        # of embeddings, so d loss / d b_last = sum_i d loss / d z_i is exactly zero and what reaches Adam is summation noise, which Adam
        # normalises to steps of order lr in whatever direction the noise points (measured 1e-5 ... 1.4e-4 between the two runs): bounded by
        # the three steps' total travel instead
        tol = 3e-3 if i == len(params) - 1 else 1e-4
        d = (a - b).abs()
        if flat_arith == "f16x2" and i != len(params) - 1:
            assert float((d > tol).float().mean()) <= 1e-3 and float(d.max()) <= 2.02 * 1e-3 * 3, (i, float(d.max()), float((d > tol).float().mean()))
        else:
            assert float(d.max()) <= tol, (i, float(d.max()))
    assert abs(float(outs["flat"][-1]) - float(outs["torch"][-1])) <= 1e-5 * abs(float(outs["torch"][-1]))


@pytest.mark.gpu
@pytest.mark.parametrize("opt_kind", ["flat", "torch_capturable"])
def test_captured_train_step_replays_the_reference_closure(opt_kind):
    """`cl_ica_amd.capture_train_step` records the reference's UNCHANGED train_step closure (main_mlp.py:258-285: two
    encoder calls, roll, loss, backward, optimizer.step, three `.item()` reads) into a HIP graph.  Two identical encoders are trained on
    the same batches, one through the closure itself (eager), one through the replaying callable: same returned floats, same parameters
    after every step (the same kernels run on the same inputs, so to fp32 rounding of nothing: bit-equal), and a batch of another shape
    goes through the closure itself."""
    import cl_ica_amd
    from cl_ica_amd import losses, optim
    n, B, steps = 10, 1536, 6
    g = torch.Generator().manual_seed(5)
    batches = []
    for _ in range(steps + 4):
        x1 = torch.rand(B, n, generator=g).cuda()
        batches.append((x1, (x1 + 0.05 * torch.randn(B, n, generator=g).cuda()).clamp(0, 1)))

    def make():
        torch.manual_seed(11)
        f = build_mlp_n10().cuda()
        opt = optim.Adam(f.parameters(), lr=1e-3) if opt_kind == "flat" else torch.optim.Adam(f.parameters(), lr=1e-3, capturable=True)
        L = losses.LpSimCLRLoss(p=2, tau=1.0, simclr_compatibility_mode=True)

        def train_step(data, loss, optimizer):
            z1, z2_con_z1 = data
            z3 = torch.roll(z1, 1, 0)
            optimizer.zero_grad()
            z1_rec = f(z1)
            z2_con_z1_rec = f(z2_con_z1)
            z3_rec = torch.roll(z1_rec, 1, 0)
            total_loss_value, _, losses_value = loss(z1, z2_con_z1, z3, z1_rec, z2_con_z1_rec, z3_rec)
            total_loss_value.backward()
            optimizer.step()
            return total_loss_value.item(), [v.item() for v in losses_value]
        return f, opt, L, train_step

    f_e, opt_e, L_e, step_e = make()
    f_c, opt_c, L_c, step_c = make()
    for q_e, q_c in zip(f_e.parameters(), f_c.parameters()):
        assert torch.equal(q_e, q_c)
    warm = 3
    replay = cl_ica_amd.capture_train_step(step_c, batches[0], L_c, opt_c, warmup=warm)
    assert replay.n_host_scalars == 3 and replay.n_early_scalars == 3      # all three are published from behind the loss forward
    # the warm-up calls were ordinary steps on batches[0]; the recording itself launched nothing.  Start both sides from the captured
    # side's state and walk in lockstep
    f_e.load_state_dict(f_c.state_dict())
    import copy
    opt_e.load_state_dict(copy.deepcopy(opt_c.state_dict()))      # (torch's load_state_dict keeps same-device tensors by reference)
    for k in range(steps):
        ref = step_e(batches[k + 2], L_e, opt_e)
        got = replay(batches[k + 2], L_c, opt_c)
        assert isinstance(got[0], float) and isinstance(got[1], list) and all(isinstance(v, float) for v in got[1])
        np.testing.assert_allclose(got[0], ref[0], rtol=2e-6, atol=0)
        np.testing.assert_allclose(got[1], ref[1], rtol=2e-6, atol=0)
        for q_e, q_c in zip(f_e.parameters(), f_c.parameters()):
            d = (q_e.detach() - q_c.detach()).abs().max().item()
            assert d <= 2e-6 * max(1.0, q_e.detach().abs().max().item()), (k, d)
    PARITY.check("dropin_captured", f"{opt_kind} B={B}", "loss after lockstep steps (replay vs eager closure)", got[0], ref[0])
    # another batch shape: the closure itself runs (and trains) -- the same step as the eager twin's
    x1 = torch.rand(333, n, generator=g).cuda()
    odd = (x1, (x1 + 0.05).clamp(0, 1))
    before = [q.detach().clone() for q in f_c.parameters()]
    out = replay(odd, L_c, opt_c)
    ref = step_e(odd, L_e, opt_e)
    assert isinstance(out[0], float) and any(not torch.equal(b, q.detach()) for b, q in zip(before, f_c.parameters()))
    # and the graph still replays afterwards, in lockstep with the twin
    out2 = replay(batches[0], L_c, opt_c)
    ref2 = step_e(batches[0], L_e, opt_e)
    for got_, ref_ in ((out, ref), (out2, ref2)):
        np.testing.assert_allclose(got_[0], ref_[0], rtol=2e-6, atol=0)
        np.testing.assert_allclose(got_[1], ref_[1], rtol=2e-6, atol=0)
    for q_e, q_c in zip(f_e.parameters(), f_c.parameters()):
        d = (q_e.detach() - q_c.detach()).abs().max().item()
        assert d <= 2e-6 * max(1.0, q_e.detach().abs().max().item()), ("after the fallback step", d)


@pytest.mark.gpu
def test_dropin_f16x2_arithmetic_under_the_flat_adam_and_its_guard(monkeypatch):
    """VERDICT r5 item 8 (first half): the drop-in encoder's whole-stack kernels in the engine's f16x2 arithmetic.  It needs the launch that
    applies the step to honour the arithmetic's guard, so it runs when `cl_ica_amd.optim.Adam` owns the parameters (torch.optim.Adam keeps
    bf16x3).  (a) first step from fresh parameters -- the scales are measured inside that step's forward / backward --: embeddings, loss
    and every weight gradient against the fp64 oracle at 1e-5, next to the same step in bf16x3; (b) five steps in each arithmetic give the
    same losses; (c) a batch 1 000 x larger than the scales know poisons the step ON THE DEVICE: the optimizer launch leaves parameters and
    moments bit-identical and counts it; the following steps on that data are applied once the scales have followed."""
    from cl_ica_amd import encoders, losses, optim
    n, B = 10, 6144
    g = torch.Generator().manual_seed(21)
    batches = []
    for _ in range(8):
        x1 = torch.rand(B, n, generator=g).cuda()
        batches.append((x1, (x1 + 0.05 * torch.randn(B, n, generator=g).cuda()).clamp(0, 1)))
    L = losses.LpSimCLRLoss(p=2, tau=1.0, simclr_compatibility_mode=True)

    def step(f, opt, data):
        x1, x2 = data
        opt.zero_grad()
        a = f(x1); b = f(x2)
        tot, _, _ = L(None, None, None, a, b, torch.roll(a, 1, 0))
        tot.backward()
        grads = [q.grad.detach().clone() for q in f.parameters()]
        opt.step()
        return tot.item(), a, b, grads

    runs = {}
    for arith in ("f16x2", "bf16x3"):
        monkeypatch.setattr(encoders, "S16_ENABLED", arith == "f16x2")
        torch.manual_seed(3)
        f = build_mlp_n10().cuda()
        opt = optim.Adam(f.parameters(), lr=1e-3)
        lin = [m for m in f if isinstance(m, torch.nn.Linear)]
        P = O.MLPParams([m.weight.detach().cpu().numpy().astype(np.float64) for m in lin], [m.bias.detach().cpu().numpy().astype(np.float64) for m in lin])
        lv, a, b, grads = step(f, opt, batches[0])
        st = encoders.arith_state(f)
        assert st["arith"] == arith, st
        x = np.concatenate([batches[0][0].cpu().numpy(), batches[0][1].cpu().numpy()]).astype(np.float64)
        y, cache = O.mlp_forward(P, x)
        ref = O.lp_simclr_loss(y[:B], y[B:], np.roll(y[:B], 1, 0), p=2, compat=True)
        fam, case = "dropin_f16x2", f"{arith} first step B={B}"
        from cl_ica_amd import lazy
        PARITY.check(fam, case, "embeddings z1", lazy.plain(a).detach().cpu().numpy(), y[:B])
        PARITY.check(fam, case, "embeddings z2", b.detach().cpu().numpy(), y[B:])
        PARITY.check(fam, case, "loss", lv, ref["loss_mean"])
        losses_seq = [lv]
        for k in range(1, 5):
            losses_seq.append(step(f, opt, batches[k])[0])
        runs[arith] = dict(f=f, opt=opt, grads=[q.cpu().numpy() for q in grads], losses=losses_seq, state=encoders.arith_state(f))
    # first-step weight gradients: the two arithmetics against each other (both are checked against fp64 in the engine's tests)
    for k, (u, v) in enumerate(zip(runs["f16x2"]["grads"][:-1], runs["bf16x3"]["grads"][:-1])):
        PARITY.check("dropin_f16x2", f"first step B={B}", f"grad{k} f16x2 vs bf16x3", u, v)
    np.testing.assert_allclose(runs["f16x2"]["losses"], runs["bf16x3"]["losses"], rtol=2e-5)
    st = runs["f16x2"]["state"]
    assert st["flags"] == 0 and st["skipped"] == 0 and not st["poisoned"], st
    assert all(1e-6 < sc < 1e12 and sc != 1.0 for sc in st["scales_d"][:3]), st          # the gradient scales were measured
    # (c) the guard
    monkeypatch.setattr(encoders, "S16_ENABLED", True)
    f, opt = runs["f16x2"]["f"], runs["f16x2"]["opt"]
    snap = [t.clone() for t in (opt.param_arena, opt.exp_avg, opt.exp_avg_sq)]
    t0 = int(opt.step_dev.item())
    big = (batches[5][0] * 1000.0, batches[5][1] * 1000.0)
    step(f, opt, big)
    torch.cuda.synchronize()
    st = encoders.arith_state(f)
    assert st["skipped"] == 1 and (st["flags"] & 2) and not (st["flags"] & 4), st
    assert int(opt.step_dev.item()) == t0
    for u, v in zip(snap, (opt.param_arena, opt.exp_avg, opt.exp_avg_sq)):
        assert torch.equal(u, v), "a withheld step must leave parameters and moments untouched"
    tries = 0
    while int(opt.step_dev.item()) == t0 and tries < 12:
        step(f, opt, big); tries += 1
    st = encoders.arith_state(f)
    assert int(opt.step_dev.item()) == t0 + 1 and st["skipped"] == tries and not (st["flags"] & 4), (tries, st)
    assert not torch.equal(snap[0], opt.param_arena)
    # torch.optim.Adam cannot be made to skip a step: the encoder stays on bf16x3 under it
    f2 = build_mlp_n10().cuda()
    o2 = torch.optim.Adam(f2.parameters(), lr=1e-3)
    step(f2, o2, batches[0])
    assert encoders.arith_state(f2)["arith"] == "bf16x3"
