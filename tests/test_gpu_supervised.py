"""The supervised phase of main_mlp.py (F.mse_loss(f(g(z1)), z1), :274-276) on the fused engine (SupervisedTrainer), in every
encoder arithmetic: G24 through the engine, the full benched size against the fp64 oracle, the output heads, the objective folded
into the backward chain against its stand-alone launch, graph replay, the f16x2 guard under replay, and the driver with both phases."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import PARITY, formula_weights, golden_view
from oracle import np_oracle as O
from test_gpu_configs import adam_trajectory_check, build_mlp, traj_tol

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.tensor(np.asarray(a, np.float32), device="cuda")


def _params64(f, head=None):
    lin = [m for m in f if isinstance(m, torch.nn.Linear)]
    hp = None
    if head is not None:
        h = f[-1]
        hp = (h.r if hasattr(h, "r") else h.max_abs_bound).detach().cpu().numpy().astype(np.float64).reshape(-1)
    return O.MLPParams([m.weight.detach().cpu().numpy().astype(np.float64) for m in lin],
                       [m.bias.detach().cpu().numpy().astype(np.float64) for m in lin], head=head, head_param=hp)


def _oracle_step(P, gW, z1, lr=0.0):
    shapes = [a.shape for l in range(len(P.W)) for a in (P.W[l], P.b[l])]
    if P.head in ("learnable_sphere", "learnable_box"):
        shapes.append(P.head_param.shape)
    state = dict(step=0, m=[np.zeros(s) for s in shapes], v=[np.zeros(s) for s in shapes])
    return O.supervised_train_step(P, [np.asarray(w, np.float64) for w in gW], z1, state, lr=lr, return_grads=True)


def _fold_expected(tr, arith):
    # the chain forms dY where it runs with its tail: whole-stack split path, no head
    return arith != "native_fp32" and tr.head is None and tr.split_wgrad


def test_g24_supervised_goldens_through_the_engine(golden, encoder_arith):
    """G24 (written by the reference's supervised train_step): five injected engine steps per case -- per-step loss, step-0
    gradients from the gradient arena, parameters after five Adam updates (G24's gmin / gmax masks): the families and tolerances
    of test_gpu_next_rows.py::test_n3_supervised_phase_goldens."""
    from cl_ica_amd.engine import SamplerSpec, SupervisedTrainer
    G = golden("g24_supervised.npz")
    for key, c in G.cases():
        n, B = int(c["meta"]["n"]), int(c["meta"]["B"])
        head = str(c["meta"]["head"]); head = None if head == "None" else head
        hidden = [int(h) for h in c["meta"]["hidden"]]; lr = float(c["meta"]["lr"]); steps = int(c["meta"]["steps"])
        stride = int(c["meta"]["stride"])
        f = build_mlp(n, hidden, head)
        gW = dev(np.stack([c["in"][f"g{i}"] for i in range(3)]))
        tr = SupervisedTrainer(f, gW, SamplerSpec(n=n), batch_size=B, lr=lr, device="cuda")
        fam, case = "supervised_engine_g24", f"{key} n={n} B={B} head={head}"
        for s in range(steps):
            out = tr.step_injected(dev(c["in"][f"z1_{s}"]))
            tl, tn = traj_tol(s)
            PARITY.check(fam, f"{case} step{s}", "loss", out[0].item(), c["out"]["loss"][s], tol=tl, note=tn)
            if s == 0:
                PARITY.check(fam, case, "z1_rec0", tr.y.cpu().numpy(), c["out"]["z1_rec0"])
                for name, prm in f.named_parameters():
                    ref = c["out"][f"grad0/{name}"]
                    got = golden_view(tr._gviews[id(prm)].cpu().numpy(), ref, stride)
                    PARITY.check(fam + "/grad", case, name, got.reshape(-1), ref.reshape(-1))
        assert tr.steps_done == steps
        assert (getattr(tr, "_mse_taken", 0) == steps) == _fold_expected(tr, encoder_arith), (key, getattr(tr, "_mse_taken", 0))
        masks = ({k[len("gmin/"):]: v for k, v in c["out"].items() if k.startswith("gmin/")},
                 {k[len("gmax/"):]: float(v) for k, v in c["out"].items() if k.startswith("gmax/")})
        adam_trajectory_check(fam + "/adam_params", key, f, c["out"], "param5", stride, lr, steps, masks=masks)


def test_supervised_engine_full_size_vs_oracle(encoder_arith):
    """The benched size: n = 10, hidden 100-500-500-500-500-100, B = 6144, formula weights; one injected step, each stage at 1e-5
    against the fp64 oracle on identical inputs (as test_gpu_configs.py::test_c2_engine_full_size_vs_oracle): embeddings, the loss and
    dY of the engine's embeddings, every dW / db from the engine's saved activations and dY.  Then the element-wise criterion on every
    gradient: fp64 truth and an fp32 torch run of the same layers from the engine's input x and dY."""
    from cl_ica_amd.engine import SamplerSpec, SupervisedTrainer
    n, B = 10, 6144
    hidden = [n * 10, n * 50, n * 50, n * 50, n * 50, n * 10]
    f = build_mlp(n, hidden, None, gain=2.2)
    rng = np.random.default_rng(31)
    gW = np.stack([formula_weights((n, n), 50 + i) * np.sqrt(n) for i in range(3)]).astype(np.float32)
    z1 = rng.uniform(size=(B, n)).astype(np.float32)
    tr = SupervisedTrainer(f, dev(gW), SamplerSpec(space="box", n=n), batch_size=B, lr=0.0, device="cuda")
    assert tr.fused_forward and tr.fused_backward and tr.x.shape[0] == B      # the encoder runs on the B rows of z1 only
    P = _params64(f)
    out = tr.step_injected(dev(z1)).cpu().numpy()
    fam, case = "supervised_engine_full_size", f"n={n} B={B}"
    xa = O.mixing_forward(list(gW), z1)
    y, _ = O.mlp_forward(P, xa)
    ye = tr.y.cpu().numpy().astype(np.float64)
    PARITY.check(fam, case, "mixing_net", tr.x.cpu().numpy(), xa)
    PARITY.check(fam, case, "embeddings", ye, y)
    diff = ye - z1.astype(np.float64)
    PARITY.check(fam, case, "loss", out[0], float((diff * diff).mean()))
    dye = tr.dy.cpu().numpy()
    PARITY.check(fam, case, "d_embeddings", dye, 2.0 * diff / diff.size)
    loss64, _ = _oracle_step(P, gW, z1)
    PARITY.check(fam, case, "loss_end_to_end", out[0], loss64)
    xe = tr.x.cpu().numpy().astype(np.float64)
    cache_e = dict(acts=[xe] + [tr.saved_activation(l).cpu().numpy().astype(np.float64) for l in range(len(tr.acts))])
    gr = O.mlp_backward(P, cache_e, dye.astype(np.float64))
    _, cache64 = O.mlp_forward(P, xe)
    truth = O.mlp_backward(P, cache64, dye.astype(np.float64))
    # the fp32 reference: the reference's own formulation in plain torch fp32 ops ON THE GPU (what main_mlp.py runs), from the same x and
    # dY.  (A CPU torch run is no fp32 yardstick at this size: its products accumulate the 6144-row sums far closer to fp64 -- 50 x
    # below the GPU's own fp32 error on dW1 / dW2 here, where the engine's error equals the GPU reference's.)
    ps = [q.detach().clone().requires_grad_(True) for q in build_mlp(n, hidden, None, gain=2.2).cuda().parameters()]
    h = torch.tensor(xe, dtype=torch.float32, device="cuda")
    for l in range(len(ps) // 2):
        h = h @ ps[2 * l].T + ps[2 * l + 1]
        if l < len(ps) // 2 - 1:
            h = F.leaky_relu(h, 0.01)
    h.backward(torch.tensor(dye, device="cuda"))
    lin = [m for m in f if isinstance(m, torch.nn.Linear)]
    for l, m in enumerate(lin):
        for kind, prm, ref, t64, r32 in (("dW", m.weight, gr["dW"][l], truth["dW"][l], ps[2 * l].grad),
                                         ("db", m.bias, gr["db"][l], truth["db"][l], ps[2 * l + 1].grad)):
            got = tr._gviews[id(prm)].cpu().numpy()
            PARITY.check(fam, case, f"{kind}{l}", got, ref)
            PARITY.check_elementwise(fam + "/grad", case, f"{kind}{l}", got, r32.cpu().numpy(), t64)
    assert (getattr(tr, "_mse_taken", 0) == 1) == _fold_expected(tr, encoder_arith)


@pytest.mark.parametrize("head", ["fixed_sphere", "learnable_sphere", "fixed_box"])
def test_supervised_engine_heads_vs_oracle(encoder_arith, head):
    """Output heads (--p 0 puts fixed_sphere on the supervised phase, --sphere-norm / --box-norm the learnable ones): the stand-alone
    objective launch between the head's forward and its backward; loss and every gradient (the head's parameter included) at 1e-5."""
    from cl_ica_amd.engine import SamplerSpec, SupervisedTrainer
    n, B, hidden = 4, 512, [40, 200, 200, 40]
    f = build_mlp(n, hidden, head, gain=1.6)
    rng = np.random.default_rng(7)
    gW = np.stack([formula_weights((n, n), 60 + i) * np.sqrt(n) for i in range(3)]).astype(np.float32)
    z1 = rng.uniform(size=(B, n)).astype(np.float32)
    tr = SupervisedTrainer(f, dev(gW), SamplerSpec(n=n), batch_size=B, lr=0.0, device="cuda")
    P = _params64(f, head)
    out = tr.step_injected(dev(z1)).cpu().numpy()
    loss, grads = _oracle_step(P, gW, z1)
    fam, case = "supervised_engine_heads", f"head={head} n={n} B={B}"
    PARITY.check(fam, case, "loss", out[0], loss)
    params = list(f.parameters())
    assert len(grads) == len(params)
    gmax = max(float(np.abs(g).max()) for g in grads)
    for k, prm in enumerate(params):
        PARITY.check(fam, case, f"grad{k}", tr._gviews[id(prm)].cpu().numpy().reshape(np.shape(grads[k])), grads[k], floor=1e-3 * gmax)
    assert getattr(tr, "_mse_taken", 0) == 0 and tr.steps_done == 1


def test_mse_folded_into_the_chain_equals_the_standalone_launch(encoder_arith, monkeypatch):
    """The same headless batch with the objective in the backward chain's prologue and with the stand-alone launch (test hook
    SupervisedTrainer.fold_mse): dY bit for bit, loss within 1e-6, gradients and parameters after the step within 1e-5 of each
    tensor's largest entry (test_gpu_mlp.py::test_wgrad_split_adam_equals_wgrad_then_adam)."""
    from cl_ica_amd import ops
    from cl_ica_amd.engine import SamplerSpec, SupervisedTrainer
    n, B, hidden = 10, 1024, [100, 500, 500, 100]
    rng = np.random.default_rng(3)
    gW = np.stack([formula_weights((n, n), 70 + i) * np.sqrt(n) for i in range(3)]).astype(np.float32)
    z1 = dev(rng.uniform(size=(B, n)))
    res = []
    for fold in (True, False):
        monkeypatch.setattr(SupervisedTrainer, "fold_mse", fold)
        f = build_mlp(n, hidden, None, gain=1.8)
        tr = SupervisedTrainer(f, dev(gW), SamplerSpec(n=n), batch_size=B, lr=1e-3, device="cuda")
        out = tr.step_injected(z1).clone()
        torch.cuda.synchronize()
        res.append((tr, out, tr.dy.clone(), tr.grad_arena.clone(), tr.param_arena.clone(), tr.steps_done))
        assert (getattr(tr, "_mse_taken", 0) == 1) == (fold and _fold_expected(tr, encoder_arith))
    (t1, l1, dy1, g1, p1, s1), (t2, l2, dy2, g2, p2, s2) = res
    assert s1 == s2 == 1
    assert torch.equal(dy1, dy2), float((dy1 - dy2).abs().max())
    assert abs(l1[0].item() - l2[0].item()) <= 1e-6 * abs(l2[0].item()), (l1[0].item(), l2[0].item())
    for prm1, prm2 in zip(t1.f.parameters(), t2.f.parameters()):
        a, b = t1._gviews[id(prm1)], t2._gviews[id(prm2)]
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()), float((a - b).abs().max())
        a, b = t1._views[id(prm1)], t2._views[id(prm2)]
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()), float((a - b).abs().max())
    PARITY.check("supervised_fold_vs_standalone", f"n={n} B={B}", "loss", l1[0].item(), l2[0].item())
    PARITY.check("supervised_fold_vs_standalone", f"n={n} B={B}", "gradients", g1.cpu().numpy(), g2.cpu().numpy())
    # the stand-alone kernel on strided rows against torch in fp64
    y = dev(rng.normal(size=(300, 17)))[:, 2:12]
    t = dev(rng.normal(size=(300, 13)))[:, 1:11]
    lo, dy = ops.mse_loss_fwd_bwd(y, t)
    d = (y.double() - t.double())
    assert abs(lo.item() - float((d * d).mean())) <= 1e-6 * float((d * d).mean())
    assert torch.equal(dy, (y - t) * np.float32(2.0 / y.numel()))
    lo2, dy2 = ops.mse_loss_fwd_bwd(y, t)           # the workspace's counter put itself back: the same bits again
    assert torch.equal(lo, lo2) and torch.equal(dy, dy2)


def test_supervised_graph_replay_equals_eager_and_trains():
    """Captured replays are the eager steps bit for bit (same snapshot, same seed, on-device sampling); 200 replays reduce the loss."""
    from cl_ica_amd.engine import SamplerSpec, SupervisedTrainer
    n, B, hidden = 10, 2048, [100, 500, 500, 100]
    gW = (torch.tensor(np.stack([formula_weights((n, n), 80 + i) * np.sqrt(n) for i in range(3)]).astype(np.float32))).cuda()
    res = []
    for graph in (False, True):
        f = build_mlp(n, hidden, None, gain=1.8)
        tr = SupervisedTrainer(f, gW, SamplerSpec(space="box", n=n, seed=4), batch_size=B, lr=1e-4, device="cuda")
        if graph:
            tr.capture(warmup=2)
            assert tr.steps_done == 0
        outs = [tr.step().clone() for _ in range(3)]
        torch.cuda.synchronize()
        res.append((torch.stack(outs), tr.param_arena.clone(), tr.exp_avg_sq.clone(), tr.steps_done))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    assert res[0][3] == res[1][3] == 3
    f = build_mlp(n, hidden, None, gain=1.8)
    tr = SupervisedTrainer(f, gW, SamplerSpec(space="box", n=n, seed=5), batch_size=B, lr=1e-3, device="cuda")
    tr.capture()
    first = tr.step().clone()
    for _ in range(199):
        last = tr.step()
    torch.cuda.synchronize()
    assert tr.steps_done == 200 and bool(torch.isfinite(tr.param_arena).all())
    assert last[0].item() < 0.9 * first[0].item(), (first[0].item(), last[0].item())


def test_supervised_f16x2_guard_withholds_the_step_and_redoes_it_inside_graph_replay():
    """test_gpu_engine.py's guard test on the supervised step: x = g(z) grown 1 000 x between replays -- the withheld replay leaves the
    parameter arena, the moments and steps_done alone, the following replays redo the SAME batch, and the applied step is the fp64
    oracle's (1e-5) and Adam(snapshot, gradient, t) bit for bit."""
    from cl_ica_amd import encoders, ops
    from cl_ica_amd.engine import SamplerSpec, SupervisedTrainer
    n, B = 10, 1024
    torch.manual_seed(7)
    f = encoders.get_mlp(n, n, [100, 500, 500, 100]).to("cuda")
    gW = (torch.randn(3, n, n, device="cuda") / n ** 0.5).contiguous()
    tr = SupervisedTrainer(f, gW, SamplerSpec(n=n, seed=3), batch_size=B, lr=1e-3, device="cuda", split_bf16=True, split_arith="f16")
    if tr.s16 is None or not tr.split_f16:
        pytest.skip("the f16x2 guard belongs to the f16x2 arithmetic")
    tr._watch_versions = False
    tr.capture()
    graph = tr.graph
    for _ in range(6):
        tr.step()
    torch.cuda.synchronize()
    g0 = tr.check_arith()
    steps0 = tr.steps_done
    assert g0["flags"] == 0 and g0["skipped"] == 0 and steps0 == 6, g0
    snap = [t.clone() for t in (tr.param_arena, tr.exp_avg, tr.exp_avg_sq)]
    tr.gW[-1].mul_(1000.0)
    tr.step(); torch.cuda.synchronize()
    g1 = tr.check_arith()
    assert g1["skipped"] == 1 and g1["new_skipped"] == 1 and (g1["flags"] & 2) and not (g1["flags"] & 4), g1
    assert tr.steps_done == steps0, "a withheld step must not advance the step / RNG counter"
    for a, b in zip(snap, (tr.param_arena, tr.exp_avg, tr.exp_avg_sq)):
        assert torch.equal(a, b), "a withheld step must leave parameters and moments untouched"
    z_withheld = tr.z[:B].clone()
    L = len(tr.linears)
    replays = 0
    while tr.steps_done == steps0 and replays < 2 * L + 6:
        tr.step(); torch.cuda.synchronize(); replays += 1
    g2 = tr.check_arith()
    assert tr.steps_done == steps0 + 1, (replays, g2)
    assert tr.graph is graph and not (g2["flags"] & 4) and g2["skipped"] == replays, (replays, g2)
    assert torch.equal(z_withheld, tr.z[:B]), "the redo must draw the batch of the withheld step"
    # the applied step against the oracle and against the optimizer kernel
    offs, o = [], 0
    for q in f.parameters():
        offs.append(o); o += (q.numel() + 3) // 4 * 4
    pa = snap[0].cpu().numpy().astype(np.float64)
    views = [pa[o:o + q.numel()].reshape(tuple(q.shape)) for o, q in zip(offs, f.parameters())]
    P = O.MLPParams([views[2 * l] for l in range(L)], [views[2 * l + 1] for l in range(L)])
    loss, grads = _oracle_step(P, tr.gW.cpu().numpy(), z_withheld.cpu().numpy().astype(np.float64))
    fam, case = "supervised_f16x2_guard_in_graph_replay", f"batch x 1000 between replays (applied after {replays} redo replays)"
    PARITY.check(fam, case, "loss", tr.loss_out[0].item(), loss)
    gmax = max(float(np.abs(g).max()) for g in grads)
    for k, q in enumerate(f.parameters()):
        PARITY.check(fam, case, f"grad{k}", tr._gviews[id(q)].cpu().numpy(), grads[k], floor=1e-3 * gmax)
    p2, m2, v2 = (t.clone() for t in snap[:3])
    cnt = torch.tensor([steps0], dtype=torch.int32, device="cuda")
    ops.adam_step(p2, tr.grad_arena, m2, v2, cnt, tr.lr, tr.betas[0], tr.betas[1], tr.eps)
    torch.cuda.synchronize()
    assert torch.equal(p2, tr.param_arena) and torch.equal(m2, tr.exp_avg) and torch.equal(v2, tr.exp_avg_sq)
    for _ in range(3):
        tr.step()
    torch.cuda.synchronize()
    g3 = tr.check_arith()
    assert tr.steps_done == steps0 + 4 and g3["new_skipped"] == 0 and not g3["poisoned"], g3


def test_train_mlp_both_phases_supervised_on_the_engine(tmp_path, capsys, encoder_arith):
    """The driver with the reference's default test_list = [True, False]: the supervised phase runs on SupervisedTrainer (the
    returned dict says so), every logged loss is finite, and both checkpoints load into get_mlp with the reference's keys."""
    from cl_ica_amd import encoders, train_mlp
    steps = 8
    r = train_mlp.main(["--n", "4", "--space-type", "box", "--p", "2", "--batch-size", "256", "--n-steps", str(steps),
                        "--more-unsupervised", "1", "--n-log-steps", "4", "--seed", "2", "--lr", "1e-3", "--num-eval-batches", "1",
                        "--save-dir", str(tmp_path)])
    se = r["supervised_engine"]
    assert se is not None and se["steps_applied"] == steps and se["graph"], se
    assert se["arith"] == {"native_fp32": "native_fp32", "split_bf16": "bf16x3", "split_f16": "f16x2"}[encoder_arith], se
    assert r["engine"] is not None and np.isfinite(se["last_loss"])
    assert len(r["losses"]) == steps and np.isfinite(r["losses"]).all()        # (the list restarts with the second phase, as in the reference)
    logged = [float(ln.split("Loss:")[1].split()[0]) for ln in capsys.readouterr().out.splitlines() if "\tLoss:" in ln or " Loss:" in ln]
    assert len(logged) >= 4 and np.isfinite(logged).all(), logged
    for name in ("sup_f.pth", "unsup_f.pth"):
        sd = torch.load(tmp_path / name)
        f = encoders.get_mlp(n_in=4, n_out=4, layers=[40, 200, 200, 200, 200, 40])
        missing = f.load_state_dict(sd, strict=True)
        assert not missing.missing_keys and not missing.unexpected_keys
        assert list(sd.keys()) == [f"{i}.{k}" for i in range(0, 13, 2) for k in ("weight", "bias")]
