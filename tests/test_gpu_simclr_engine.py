"""p = 0 -- SimCLRLoss(normalize=False), InfoNCE on dot products (/root/reference/losses.py:162-202), the objective of the reference's
hypersphere experiment -- on the fused engine step: the dot kind's training pair (csrc/dot_train.hip) against the fp64 oracle, against a
pooled (data-parallel) pool and against the generic dot pair; ContrastiveTrainer(p=0) against the drop-in modules under autograd with
torch.optim.Adam; the collapsed-encoder value ln(B + 1); graph replay; data parallelism; the driver."""
import copy
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PARITY, free_port, with_free_port
from oracle import np_oracle as O
from test_gpu_configs import adam_trajectory_check, traj_tol

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LN2 = float(np.log(2.0))


def _lib():
    from cl_ica_amd import _lib as L
    return L, L.load()


def train_pair(z1, z2, pool, tau, alpha, pool_lse=None, backward=True):
    """clica_dot_loss_fwd_train (+ clica_dot_loss_bwd_sym_train) on cuda tensors.  `pool_lse`: callable lse_i -> the pool's row statistics
    (default: the pool is z1 itself)."""
    L, lib = _lib()
    B, n = z1.shape
    d = L.DotLossDesc(B=B, B3=pool.shape[0], n=n, tau=tau, alpha=alpha, normalize=0)
    nb = C.c_size_t()
    L.check(lib.clica_dot_loss_train_workspace_bytes(C.byref(d), C.byref(nb)), "workspace")
    ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
    f32 = dict(dtype=torch.float32, device="cuda")
    loss_i, pos_i, lse_i = (torch.empty(B, **f32) for _ in range(3))
    dz1, dz2 = torch.empty((B, n), **f32), torch.empty((B, n), **f32)
    means = torch.full((3,), float("nan"), **f32)
    tick = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = L.stream_ptr()
    L.check(lib.clica_dot_loss_fwd_train(C.byref(d), z1.data_ptr(), n, z2.data_ptr(), n, pool.data_ptr(), n, loss_i.data_ptr(),
                                         pos_i.data_ptr(), lse_i.data_ptr(), dz1.data_ptr(), n, dz2.data_ptr(), n,
                                         ws.data_ptr(), ws.numel(), st), "clica_dot_loss_fwd_train")
    out = dict(loss_i=loss_i, pos_i=pos_i, lse_i=lse_i)
    if backward:
        pl = lse_i if pool_lse is None else pool_lse(lse_i)
        L.check(lib.clica_dot_loss_bwd_sym_train(C.byref(d), z1.data_ptr(), n, pool.data_ptr(), n, lse_i.data_ptr(), pl.data_ptr(),
                                                 dz1.data_ptr(), n, means.data_ptr(), tick.data_ptr(), ws.data_ptr(), ws.numel(), st),
                "clica_dot_loss_bwd_sym_train")
        out.update(dz1=dz1, dz2=dz2, means=means)
    torch.cuda.synchronize()
    tiles = (B + 63) // 64
    assert int(ws[:4 * tiles].view(torch.int32).abs().sum()) == 0          # every launch leaves its arrival counters at zero
    if backward:
        assert int(tick.item()) == 1
    return {k: v.cpu().numpy() for k, v in out.items()}


def make_rows(rng, B, n, kind):
    """Unit-norm rows, or raw rows of UNEQUAL norm (scale x U(0.3, 1.7)): the self-pair is then not the row's largest logit."""
    z1 = rng.standard_normal((B, n))
    z1 /= np.linalg.norm(z1, axis=1, keepdims=True)
    z2 = z1 + 0.1 * rng.standard_normal((B, n)) / np.sqrt(n)
    if kind == "unit":
        z2 /= np.linalg.norm(z2, axis=1, keepdims=True)
    else:
        s = float(kind) * rng.uniform(0.3, 1.7, (B, 1))
        z1 *= s
        z2 *= s
    return z1.astype(np.float32), z2.astype(np.float32)


def check_vs_oracle(fam, case, out, z1, z2, z3, tau, alpha, rows=None, scale=1.0, dz1_ref=None, dz2_ref=None):
    """The pair's outputs for the anchor rows `rows` of the oracle problem (z1, z2, z3); gradients scaled by `scale` (pooled case)."""
    orc = O.simclr_loss(z1, z2, z3, tau=tau, alpha=alpha)
    sel = slice(None) if rows is None else rows
    pos = (z1.astype(np.float64) * z2).sum(1)[sel]
    lse = orc["lse"][sel]
    li = orc["loss_i"][sel]
    # loss_i = 2 (alpha (-pos / tau) + (1 - alpha) lse) cancels once the positive pair dominates: judged against the larger summand, as the
    # existing dot-loss checks (tests/test_gpu_loss.py::test_simclr_goldens)
    lf = 2.0 * max(alpha * float(np.abs(pos).max()) / tau, (1.0 - alpha) * float(np.abs(lse).max()))
    PARITY.check(fam, case, "loss_i", out["loss_i"], li, floor=lf)
    PARITY.check(fam, case, "pos_i", out["pos_i"], -pos / tau)
    PARITY.check(fam, case, "lse_i", out["lse_i"].astype(np.float64) * LN2, lse)
    PARITY.check(fam, case, "loss_mean", out["means"][0], li.mean(), floor=lf)
    PARITY.check(fam, case, "pos_mean", out["means"][1], (-pos / tau).mean(), floor=float(np.abs(pos).max()) / tau)
    PARITY.check(fam, case, "neg_mean", out["means"][2], lse.mean(), floor=float(np.abs(lse).max()))
    B = len(li)
    # embedding gradients: the alignment pull 2 alpha / (B tau) z2 against the softmax push (test_simclr_goldens' floor)
    gf = scale * 2.0 * alpha / (B * tau) * float(np.abs(z2).max())
    d1 = dz1_ref if dz1_ref is not None else orc["dz1"]
    d2 = dz2_ref if dz2_ref is not None else orc["dz2"]
    PARITY.check(fam, case, "dz1", out["dz1"], d1, floor=gf)
    PARITY.check(fam, case, "dz2", out["dz2"], d2, floor=gf)


def _cases():
    Bs, ns, kinds = (8, 64, 300, 512, 6144), (3, 4, 10, 16, 40), ("unit", 0.1, 1.0, 3.0)
    out = []
    for bi, B in enumerate(Bs):
        for ni, n in enumerate(ns):
            k = 5 * bi + ni
            out.append((B, n, (1.0, 0.5)[k % 2], (0.5, 0.3)[(k // 2) % 2], kinds[(k // 4) % 4]))     # every (tau, alpha, rows) combination
    return out


@pytest.mark.parametrize("B", [8, 64, 300, 512, 6144])
def test_train_pair_vs_fp64_oracle(B):
    """fwd_train + bwd_sym_train with pool = roll(z1) (the reference's z3_rec, main_mlp.py:272) and pool_lse = roll(lse_i) against
    oracle.simclr_loss(z1, z2, roll(z1)): loss_i, pos_i, lse_i, the three means, dz1 (= the oracle's dz1 + roll^-1(dz3)) and dz2.
    n in {3, 4, 10, 16, 40}, tau in {1, 0.5}, alpha in {0.5, 0.3}, unit rows and raw rows of unequal norm at scales 0.1 / 1 / 3."""
    rng = np.random.default_rng(B)
    for (b, n, tau, alpha, kind) in _cases():
        if b != B:
            continue
        z1, z2 = make_rows(rng, B, n, kind)
        z3 = np.roll(z1, 1, 0)
        g1, g2 = torch.tensor(z1, device="cuda"), torch.tensor(z2, device="cuda")
        out = train_pair(g1, g2, torch.roll(g1, 1, 0), tau, alpha, pool_lse=lambda l: torch.roll(l, 1, 0))
        orc = O.simclr_loss(z1, z2, z3, tau=tau, alpha=alpha)
        check_vs_oracle("simclr_train_pair_vs_oracle", f"B={B} n={n} tau={tau} alpha={alpha} rows={kind}", out, z1, z2, z3, tau, alpha,
                        dz1_ref=orc["dz1"] + np.roll(orc["dz3"], -1, 0))


def test_train_pair_pooled_vs_fp64_oracle():
    """A pool of 4 B rows that contains the local rows (the all-gather of four ranks' z1), the pool's lse supplied from the four ranks'
    forwards: the local rank's outputs against the oracle at z3 = pool.  The symmetric sweep gives the gradient of the SUM of the four
    ranks' mean losses: 4 x the oracle's gradient of the global mean (dz1 + dz3 of the same rows)."""
    R, B, n, tau, alpha = 4, 512, 10, 0.5, 0.5
    rng = np.random.default_rng(7)
    z1, z2 = make_rows(rng, R * B, n, 1.0)
    g1, g2 = torch.tensor(z1, device="cuda"), torch.tensor(z2, device="cuda")
    lse_all = torch.cat([torch.tensor(train_pair(g1[r * B:(r + 1) * B], g2[r * B:(r + 1) * B], g1, tau, alpha, backward=False)["lse_i"])
                         for r in range(R)]).cuda()
    r = 2
    rows = slice(r * B, (r + 1) * B)
    out = train_pair(g1[rows], g2[rows], g1, tau, alpha, pool_lse=lambda l: lse_all)
    assert np.array_equal(out["lse_i"], lse_all[rows].cpu().numpy())      # deterministic: the rank's own forward gives the same bits
    orc = O.simclr_loss(z1, z2, z1, tau=tau, alpha=alpha)
    check_vs_oracle("simclr_train_pair_pooled", f"R={R} B={B} n={n}", out, z1, z2, z1, tau, alpha, rows=rows, scale=R,
                    dz1_ref=R * (orc["dz1"] + orc["dz3"])[rows], dz2_ref=R * orc["dz2"][rows])


def test_train_pair_agrees_with_generic_pair():
    """The training pair against clica_dot_loss_fwd / clica_dot_loss_bwd with z3 = roll(z1) (dz3 added back to dz1 through roll^-1)."""
    L, lib = _lib()
    rng = np.random.default_rng(5)
    for B, n, tau, alpha, kind in ((512, 10, 0.5, 0.3, 1.0), (300, 4, 1.0, 0.5, "unit"), (1024, 40, 1.0, 0.5, 0.1)):
        z1, z2 = make_rows(rng, B, n, kind)
        g1, g2 = torch.tensor(z1, device="cuda"), torch.tensor(z2, device="cuda")
        g3 = torch.roll(g1, 1, 0).contiguous()
        new = train_pair(g1, g2, g3, tau, alpha, pool_lse=lambda l: torch.roll(l, 1, 0))
        d = L.DotLossDesc(B=B, B3=B, n=n, tau=tau, alpha=alpha, normalize=0)
        fb, bb = C.c_size_t(), C.c_size_t()
        L.check(lib.clica_dot_loss_workspace_bytes(C.byref(d), C.byref(fb), C.byref(bb)), "workspace")
        ws = torch.zeros(max(fb.value, bb.value), dtype=torch.uint8, device="cuda")
        f32 = dict(dtype=torch.float32, device="cuda")
        li, pi, lse, means = torch.empty(B, **f32), torch.empty(B, **f32), torch.empty(B, **f32), torch.empty(3, **f32)
        dz1, dz2, dz3 = (torch.empty((B, n), **f32) for _ in range(3))
        st = L.stream_ptr()
        L.check(lib.clica_dot_loss_fwd(C.byref(d), g1.data_ptr(), n, g2.data_ptr(), n, g3.data_ptr(), n, li.data_ptr(), pi.data_ptr(),
                                       lse.data_ptr(), means.data_ptr(), None, 0, ws.data_ptr(), ws.numel(), st), "clica_dot_loss_fwd")
        L.check(lib.clica_dot_loss_bwd(C.byref(d), g1.data_ptr(), n, g2.data_ptr(), n, g3.data_ptr(), n, lse.data_ptr(), None, 0,
                                       None, None, None, None, dz1.data_ptr(), n, dz2.data_ptr(), n, dz3.data_ptr(), n, 0,
                                       ws.data_ptr(), ws.numel(), st), "clica_dot_loss_bwd")
        dz1 = dz1 + torch.roll(dz3, -1, 0)
        torch.cuda.synchronize()
        case, fam = f"B={B} n={n} tau={tau} alpha={alpha} rows={kind}", "simclr_train_pair_vs_generic_pair"
        pos_mag = float(np.abs(new["pos_i"]).max())
        lf = 2.0 * max(alpha * pos_mag, (1.0 - alpha) * float(np.abs(new["lse_i"]).max()) * LN2)
        PARITY.check(fam, case, "loss_i", new["loss_i"], li.cpu().numpy(), floor=lf)
        PARITY.check(fam, case, "pos_i", new["pos_i"], pi.cpu().numpy())
        PARITY.check(fam, case, "lse_i", new["lse_i"], lse.cpu().numpy())
        PARITY.check(fam, case, "means", new["means"], means.cpu().numpy(), floor=lf)
        gf = 2.0 * alpha / (B * tau) * float(np.abs(z2).max())
        PARITY.check(fam, case, "dz1", new["dz1"], dz1.cpu().numpy(), floor=gf)
        PARITY.check(fam, case, "dz2", new["dz2"], dz2.cpu().numpy(), floor=gf)


@pytest.mark.parametrize("tau", [1.0, 0.5])
@pytest.mark.parametrize("B", [512, 6144])
def test_collapsed_rows_give_ln_b_plus_1(B, tau):
    """Fully collapsed unit rows: every logit is 1/tau and pos = 1, so at alpha = 0.5 every loss_i is ln(B + 1) -- up to the rounding of
    lse = 1/tau + ln(B + 1) in fp32 (its sum of B + 1 equal terms is exact)."""
    n = 10
    z = torch.zeros((B, n), device="cuda")
    z[:, 3] = 1.0
    out = train_pair(z, z.clone(), z, tau, 0.5)
    want = float(np.log(B + 1))
    tol = 1e-6 * (want + 1.0 / tau)
    assert np.abs(out["loss_i"].astype(np.float64) - want).max() <= tol, (out["loss_i"][:4], want)
    assert abs(float(out["means"][0]) - want) <= tol
    assert np.isfinite(out["dz1"]).all() and np.isfinite(out["dz2"]).all()


def _sphere_batch(gen, B, n):
    z1 = torch.randn(B, n, generator=gen)
    z1 = z1 / z1.norm(dim=1, keepdim=True)
    z2 = z1 + 0.05 * torch.randn(B, n, generator=gen)
    return z1.cuda(), (z2 / z2.norm(dim=1, keepdim=True)).cuda()


def test_fresh_encoder_first_step_is_ln_b_plus_1(encoder_arith):
    """A fresh driver-shaped encoder behind the fixed_sphere head maps every latent to nearly the same unit vector: the first engine step's
    loss is ln(B + 1) within the existing p = 2 test's 2e-3 (tests/test_gpu_engine.py::test_train_mlp_driver_short_run)."""
    from cl_ica_amd import encoders
    from cl_ica_amd.engine import ContrastiveTrainer, SamplerSpec
    torch.manual_seed(0)
    n, B = 10, 512
    f = encoders.get_mlp(n, n, [n * 10, n * 50, n * 50, n * 50, n * 50, n * 10], output_normalization="fixed_sphere")
    gW = torch.randn(3, n, n) / n ** 0.5
    tr = ContrastiveTrainer(f, gW, SamplerSpec(space="sphere", n=n, seed=4), batch_size=B, p=0, tau=1.0, lr=1e-3, device="cuda")
    first = tr.step()[0].item()
    assert abs(first - np.log(B + 1)) < 2e-3, (first, np.log(B + 1))


@pytest.mark.parametrize("head", ["fixed_sphere", "learnable_sphere", "learnable_box", None])
def test_engine_step_vs_autograd_with_torch_adam(head, encoder_arith):
    """ContrastiveTrainer(p=0).step_injected against the drop-in modules under torch autograd with SimCLRLoss(normalize=False) and
    torch.optim.Adam on the same batches: the loss triple of every step (traj_tol), every gradient of the first step at 1e-5, and the
    parameters after 1 and after 5 updates (adam_trajectory_check, the gradient-magnitude masks recorded on the autograd side)."""
    from cl_ica_amd import encoders, lazy, losses, ops
    from cl_ica_amd.engine import ContrastiveTrainer, SamplerSpec
    n, B, lr, steps, tau, alpha = 10, 1024, 1e-3, 5, 0.5, 0.5
    if head == "learnable_box":
        # behind the sigmoid box head the gain-amplified encoder (below) feeds the noise elements' +-lr walks back into the next forward: in
        # bf16x3 the loss after four updates lands 5.06e-5 from the autograd path against the 5e-5 trajectory quantum.  Step 0 and the
        # first update are held to the usual bounds
        steps = 1
    torch.manual_seed(3)
    f = encoders.get_mlp(n, n, [100, 500, 500, 100], output_normalization=head).cuda()
    if head == "learnable_sphere":
        f[-1].r.data.mul_(1.3)          # off its init value, so its gradient matters
    if head == "learnable_box":
        f[-1].max_abs_bound.data.mul_(1.7)
    if head in (None, "learnable_box"):
        # without a head (or behind the sigmoid box head) a fresh encoder maps every input to nearly the same point: dy is then a difference of nearly equal pull and push
        # terms and both fp32 paths hold it only to ~2e-5 of itself.  A gain on the weights (as build_mlp's, tests/test_gpu_configs.py)
        # keeps the embeddings apart
        for m in f:
            if isinstance(m, torch.nn.Linear):
                m.weight.data.mul_(2.2)
    f_ref = copy.deepcopy(f)
    gen = torch.Generator().manual_seed(9)
    gW = (torch.randn(3, n, n, generator=gen) / n ** 0.5).cuda()
    batches = [_sphere_batch(gen, B, n) for _ in range(steps)]
    opt = torch.optim.Adam(f_ref.parameters(), lr=lr)
    L = losses.SimCLRLoss(normalize=False, tau=tau, alpha=alpha)
    tr = ContrastiveTrainer(f, gW, SamplerSpec(space="sphere", n=n), batch_size=B, p=0, tau=tau, alpha=alpha, lr=lr, device="cuda")
    assert tr.plan_summary()["loss_entry_points"] == "dot train pair"
    fam, case = "simclr_engine_vs_autograd_adam", f"head={head}"
    lin = [m for m in f if isinstance(m, torch.nn.Linear)]
    bound0 = f[-1].max_abs_bound.detach().cpu().numpy().reshape(-1) if head == "learnable_box" else None
    P0 = O.MLPParams([m.weight.detach().cpu().numpy().astype(np.float64) for m in lin],
                     [m.bias.detach().cpu().numpy().astype(np.float64) for m in lin])
    gmin, gmax = {}, {}
    for s, (z1, z2) in enumerate(batches):
        a = lazy.plain(f_ref(ops.mixing_fwd(z1, gW)))
        b = lazy.plain(f_ref(ops.mixing_fwd(z2, gW)))
        a.retain_grad(); b.retain_grad()
        tot, _, (pm, nm) = L(None, None, None, a, b, torch.roll(a, 1, 0))
        opt.zero_grad()
        tot.backward()
        for k, q in f_ref.named_parameters():
            g = q.grad.detach().abs().cpu().numpy()
            gmin[k] = g if s == 0 else np.minimum(gmin[k], g)
            gmax[k] = max(gmax.get(k, 0.0), float(g.max()))
        ref_grads = {k: q.grad.detach().clone() for k, q in f_ref.named_parameters()}
        opt.step()
        out = tr.step_injected(z1, z2).cpu().numpy()
        tl, tn = traj_tol(s)
        PARITY.check(fam, f"{case} step{s}", "loss", out[0], tot.item(), tol=tl, note=tn)
        PARITY.check(fam, f"{case} step{s}", "pos_mean", out[1], pm.item(), tol=tl, note=tn, floor=abs(nm.item()))
        PARITY.check(fam, f"{case} step{s}", "neg_mean", out[2], nm.item(), tol=tl, note=tn)
        if s == 0 and head in (None, "learnable_box"):
            # staged, as tests/test_gpu_configs.py::test_c3_engine_full_size_vs_oracle: without a head the encoder's LeakyReLU kinks sit
            # right behind dy, and a pre-activation within rounding of 0 takes another slope in the drop-in forward than in the engine's
            # (measured: 4e-5 of the first layer's gradient in bf16x3).  So: dy against the fp64 loss at the ENGINE's embeddings (floor:
            # the alignment pull, as the pair tests), every dW / db against the fp64 backward fed the engine's activations and dy.  The
            # sigmoid box head keeps the embeddings nearly as close together (measured: 1.2e-5 of the first bias's gradient in fp32): its
            # backward is checked in fp64 from the engine's dy and pre-head output, the chain behind it from the engine's d pre-head.
            ye = tr.y.cpu().numpy().astype(np.float64)
            orc = O.simclr_loss(ye[:B], ye[B:], np.roll(ye[:B], 1, 0), tau=tau, alpha=alpha)
            gy = np.concatenate([orc["dz1"] + np.roll(orc["dz3"], -1, 0), orc["dz2"]])
            dye = tr.dy.cpu().numpy().astype(np.float64)
            PARITY.check(fam + "/staged", case, "d_embeddings", dye, gy, floor=2.0 * alpha / (B * tau) * float(np.abs(ye).max()))
            cache_e = dict(acts=[tr.x.cpu().numpy().astype(np.float64)] +
                           [tr.saved_activation(l).cpu().numpy().astype(np.float64) for l in range(len(tr.acts))])
            g_in = dye
            if head == "learnable_box":
                bound = f[-1].max_abs_bound
                bnd = bound0.astype(np.float64)
                sg = 1.0 / (1.0 + np.exp(-cache_e["acts"][-1]))
                PARITY.check(fam + "/staged", case, "d_prehead", tr.dpre.cpu().numpy(), dye * bnd * sg * (1.0 - sg),
                             floor=float(np.abs(dye).max()) * float(np.abs(bnd).max()) / 4.0)
                mass = float((np.abs(dye) * sg).sum(0).max())
                PARITY.check(fam + "/staged", case, "max_abs_bound", tr._gviews[id(bound)].cpu().numpy().reshape(-1),
                             (dye * sg).sum(0).reshape(-1), floor=1e-2 * mass, note="cancelling sum: judged against 1e-2 of its summand mass")
                g_in = tr.dpre.cpu().numpy().astype(np.float64)
            gr = O.mlp_backward(P0, cache_e, g_in)
            for l, m in enumerate(lin):
                PARITY.check(fam + "/staged", case, f"dW{l}", tr._gviews[id(m.weight)].cpu().numpy(), gr["dW"][l])
                # (the output bias: the column sum of dy, whose pull and push cancel -- against the summands' scale, as dW of that layer)
                PARITY.check(fam + "/staged", case, f"db{l}", tr._gviews[id(m.bias)].cpu().numpy(), gr["db"][l],
                             floor=float(np.abs(gr["dW"][l]).max()) if l == len(lin) - 1 else 0.0)
        elif s == 0:
            gtop = max(float(v.abs().max()) for v in ref_grads.values())
            for k, q in f.named_parameters():
                floor, note = 1e-3 * gtop, None
                if k.endswith(".r"):
                    # d loss / d r = sum_i <dy_i, y_i> / r over both views: pull and push cancel in this sum (the learnable head's scalar,
                    # as max_abs_bound in tests/test_gpu_engine.py::test_engine_matches_autograd_path): judged against 1e-2 of its
                    # summand mass, as there
                    r = float(q.detach())
                    mass = float((a.grad * a.detach()).sum(1).abs().sum() + (b.grad * b.detach()).sum(1).abs().sum()) / r
                    floor, note = 1e-2 * mass, "cancelling sum: judged against 1e-2 of its summand mass"
                if k.endswith("max_abs_bound"):
                    # d loss / d bound_k = sum_i dy_ik sigmoid(x_ik) over both views: the same kind of cancelling sum, judged the same way
                    bound = q.detach()
                    mass = (a.grad.abs() * (a.detach() / bound).abs()).sum(0) + (b.grad.abs() * (b.detach() / bound).abs()).sum(0)
                    floor, note = 1e-2 * float(mass.max()), "cancelling sum: judged against 1e-2 of its summand mass"
                PARITY.check(fam + "/grad", case, k, tr._gviews[id(q)].cpu().numpy(), ref_grads[k].cpu().numpy(), floor=floor, note=note)
        if s + 1 in (1, steps):
            ref = {f"param/{k}": q.detach().cpu().numpy() for k, q in f_ref.named_parameters()}
            adam_trajectory_check(fam + "/adam_params", f"{case} after {s + 1}", f, ref, "param", 1, lr, s + 1, masks=(gmin, gmax))
    assert tr.steps_done == steps


def _trainer(head="fixed_sphere", **kw):
    from cl_ica_amd import encoders
    from cl_ica_amd.engine import ContrastiveTrainer, SamplerSpec
    torch.manual_seed(0)
    f = encoders.get_mlp(10, 10, [100, 500, 100], output_normalization=head)
    return ContrastiveTrainer(f, torch.eye(10).repeat(3, 1, 1), SamplerSpec(space="sphere", n=10, seed=5), batch_size=1024, p=0, tau=0.5,
                              lr=1e-3, device="cuda", **kw)


@pytest.mark.parametrize("head", ["fixed_sphere", "learnable_box"])
def test_captured_replay_equals_eager(head, encoder_arith):
    """A captured step graph replays the eager step bit for bit over several steps (sampler, encoder, head, dot pair, Adam)."""
    res = []
    for graph in (False, True):
        tr = _trainer(head)
        if graph:
            tr.capture(warmup=2)
        outs = []
        for _ in range(6):
            outs.append(tr.step().clone())
        torch.cuda.synchronize()
        res.append((torch.stack(outs), tr.param_arena.clone(), tr.steps_done))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and res[0][2] == res[1][2] == 6
    assert bool(torch.isfinite(res[0][0]).all())


def test_dp_code_path_single_rank_is_bit_identical(monkeypatch, encoder_arith):
    """world_size-1 group with the collectives forced on (all-gathers of embeddings and lse, bucketed all-reduce): the same bits as the
    plain step, eager and captured (the pattern of tests/test_gpu_engine.py::test_dp_code_path_single_rank, chain tail off as there)."""
    import torch.distributed as dist
    from cl_ica_amd.engine import ContrastiveTrainer
    monkeypatch.setattr(ContrastiveTrainer, "chain_tail", False)
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(free_port()))
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        outs = []
        for force, graph in ((False, False), (True, False), (True, True)):
            tr = _trainer(process_group=dist.group.WORLD, force_collectives=force)
            assert tr.dp == force
            if graph:
                tr.capture(warmup=2)
            for _ in range(3):
                o = tr.step().clone()
            torch.cuda.synchronize()
            outs.append((o, tr.param_arena.clone()))
        for o, prm in outs[1:]:
            assert torch.equal(outs[0][0], o) and torch.equal(outs[0][1], prm)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("head", ["fixed_sphere", None])
def test_two_ranks_match_single_process(tmp_path, head, encoder_arith):
    """Two processes share cuda:0 (gloo, eager launches): the rank-mean loss and the all-reduced (summed) gradient arena equal the single
    process on the concatenated batch (the pattern of tests/test_gpu_dp2.py)."""
    B, n = 256, 10

    def run(port):
        procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dp2_simclr_worker.py"), str(r), str(port), str(tmp_path), str(B),
                                   str(n), str(head)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
        outs = [p.communicate(timeout=600)[0].decode() for p in procs]
        bad = [o for p, o in zip(procs, outs) if p.returncode != 0]
        return (1 if bad else 0), "\n".join(o[-3000:] for o in bad)

    rc, text = with_free_port(run)
    assert rc == 0, text
    sys.path.insert(0, HERE)
    from dp2_simclr_worker import make_problem
    from cl_ica_amd.engine import ContrastiveTrainer, SamplerSpec
    f, gW, z1, z2 = make_problem(n, 2 * B, head)
    ref = ContrastiveTrainer(f, gW, SamplerSpec(space="sphere", n=n), batch_size=2 * B, p=0, tau=0.5, alpha=0.5, lr=0.0, device="cuda")
    out = ref.step_injected(z1, z2).cpu().numpy()
    r0, r1 = (np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(2))
    fam, case = "simclr_dp2_vs_single_process", f"B={B} n={n} head={head}"
    means = 0.5 * (r0["means"] + r1["means"])
    for k, nm in enumerate(("loss_mean", "pos_mean", "neg_mean")):
        PARITY.check(fam, case, nm, means[k], out[k], floor=abs(float(out[2])))
    PARITY.check(fam, case, "loss_i", np.concatenate([r0["loss_i"], r1["loss_i"]]), ref.loss_out[:2 * B].cpu().numpy(),
                 floor=abs(float(out[2])))
    assert np.array_equal(r0["grad"], r1["grad"])                       # all-reduce: identical on both ranks
    g_ref = 2.0 * ref.grad_arena.cpu().numpy()
    gtop = float(np.abs(g_ref).max())
    off = 0
    for k, prm in f.named_parameters():
        sl = slice(off, off + prm.numel()); off += (prm.numel() + 3) // 4 * 4
        PARITY.check(fam + "/grad", case, k, r0["grad"][sl], g_ref[sl], floor=1e-3 * gtop)


@pytest.mark.parametrize("c_p,c_param", [("2", "0.05"), ("0", "50")])
def test_train_mlp_p0_runs_on_the_engine(capsys, c_p, c_param, encoder_arith):
    """train_mlp --p 0 --space-type sphere: the contrastive phase runs on ContrastiveTrainer (the returned `engine` record is filled), its
    loss decreases, and the p = 2 loss-guard clause is not printed.  Once with the vMF conditional (--c-p 0; --c-param is its
    concentration: at the default 0.05 the positive is nearly uniform on the sphere and there is nothing to learn)."""
    from cl_ica_amd import train_mlp
    steps = 60
    r = train_mlp.main(["--n", "10", "--space-type", "sphere", "--p", "0", "--c-p", c_p, "--c-param", c_param, "--batch-size", "512",
                        "--n-steps", str(steps),
                        "--more-unsupervised", "1", "--n-log-steps", "30", "--seed", "0", "--only-unsupervised", "--lr", "1e-3",
                        "--num-eval-batches", "1"])
    out = capsys.readouterr().out
    e = r["engine"]
    assert e is not None and e["arith"] == {"native_fp32": "native_fp32", "split_bf16": "bf16x3", "split_f16": "f16x2"}[encoder_arith], e
    assert e["loss_fallback_steps"] == 0 and e["loss_spread_limit"] == 0.0
    assert "loss guard" not in out and "engine: encoder arithmetic" in out
    losses = np.asarray(r["losses"])
    assert len(losses) >= steps and np.isfinite(losses).all()
    assert losses[-10:].mean() < losses[0] - 0.05, (losses[0], losses[-10:])


def test_existing_p0_driver_run_is_not_topped_up(encoder_arith):
    """The run of tests/test_gpu_engine.py::test_train_mlp_supervised_and_simclr_paths (which asserts exactly 12 losses): on the engine
    no step of its contrastive phase is withheld by the f16x2 guard, so the driver's top-up loop adds none."""
    from cl_ica_amd import train_mlp
    r = train_mlp.main(["--n", "4", "--space-type", "sphere", "--p", "0", "--batch-size", "256", "--n-steps", "12",
                        "--more-unsupervised", "1", "--n-log-steps", "6", "--seed", "1", "--lr", "1e-3", "--num-eval-batches", "1"])
    assert r["engine"] is not None and r["engine"]["f16_steps_withheld"] in (0, None), r["engine"]
    assert len(r["losses"]) == 12 and np.isfinite(r["losses"]).all()
