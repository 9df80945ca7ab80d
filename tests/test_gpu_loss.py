"""HIP loss kernels (through the C ABI / ctypes) against the reference goldens and the oracle."""
import os
import numpy as np
import pytest
import torch

from conftest import PARITY, rel_err
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-5   # north_star: loss value and embedding gradients within 1e-5 relative fp32
SAT_CAP = 3e-5   # hard ceiling of the saturated-row allowance (saturation_allowance)


def dev(a):
    return torch.tensor(np.asarray(a, np.float32), device="cuda")


def grad_scale(z1, z2, p, tau, alpha):
    d = np.abs(np.asarray(z1, np.float64) - np.asarray(z2, np.float64))
    return 2 * alpha / (d.shape[0] * tau) * float((p * np.maximum(d, 1e-12) ** (p - 1)).max())


def run_hip(loss_obj, z1, z2, z3, roll=False):
    a = dev(z1).requires_grad_(True)
    b = dev(z2).requires_grad_(True)
    if roll:
        c = torch.roll(a, 1, 0)
    else:
        c = dev(z3).requires_grad_(True)
    mean, per, (pm, nm) = loss_obj(None, None, None, a, b, c)
    mean.backward()
    out = dict(loss_mean=mean.item(), loss_i=per.detach().cpu().numpy(), pos_mean=pm.item(), neg_mean=nm.item(),
               dz1=a.grad.cpu().numpy(), dz2=b.grad.cpu().numpy())
    if not roll:
        out["dz3"] = c.grad.cpu().numpy()
    return out


def summand_floors(ref_or_orc, alpha, tau, gscale):
    """Scales of the UN-CANCELLED summands.  loss_i = 2 (alpha pos_i / tau + (1 - alpha) lse_i) is a sum of two terms of
    opposite sign once the positive pair dominates the softmax (lse_i -> -pos_i / tau); the embedding gradients are a
    difference of the alignment pull (scale `gscale` = 2 alpha / (B tau) max p |d|^(p-1), grad_scale()) and the softmax
    push.  A backward-stable fp32 evaluation is accurate relative to the larger summand, not to the cancelled result, so
    these are the floors of the relative error's denominator (they are NOT multipliers: without cancellation max|ref| is
    the larger of the two and the floor is inert)."""
    if "lse" in ref_or_orc:       # oracle dict: per-row values available (means of signed rows can cancel as well)
        pm = float(np.abs(ref_or_orc["pos"]).max()) / tau
        nm = float(np.abs(ref_or_orc["lse"]).max())
    else:
        pm = abs(float(np.asarray(ref_or_orc["pos_mean"]))) if "pos_mean" in ref_or_orc else 0.0
        nm = abs(float(np.asarray(ref_or_orc["neg_mean"]))) if "neg_mean" in ref_or_orc else 0.0
    return 2.0 * max(alpha * pm, (1.0 - alpha) * nm), gscale


def compare(family, case, out, ref, grads, sat_tol=None, note=None, loss_floor=0.0, grad_floor=0.0, means_floor=(0.0, 0.0)):
    """Norm-wise relative error of every output against the reference golden, bound 1e-5 (north_star).
    `sat_tol` (with `note`) is the documented allowance of a saturated case -- see saturation_allowance()."""
    tol = TOL if sat_tol is None else sat_tol
    PARITY.check(family, case, "loss_mean", out["loss_mean"], float(ref["loss_mean"]), tol=tol, note=note, floor=loss_floor)
    PARITY.check(family, case, "loss_i", out["loss_i"], ref["loss_i"], tol=tol, note=note, floor=loss_floor)
    if "pos_mean" in ref:
        # means over rows of signed per-row values: relative to the largest row (the mean itself can cancel)
        PARITY.check(family, case, "pos_mean", out["pos_mean"], float(ref["pos_mean"]), tol=tol, note=note, floor=means_floor[0])
        PARITY.check(family, case, "neg_mean", out["neg_mean"], float(ref["neg_mean"]), tol=tol, note=note, floor=means_floor[1])
    for g in grads:
        PARITY.check(family, case, g, out[g], ref[g], tol=tol, note=note, floor=0.0 if g == "dz3" else grad_floor)


def saturation_allowance(z1, z2, z3, p, tau, alpha, compat, pw, ref, loss_floor=0.0, grad_floor=0.0):
    """Case-specific allowance for SATURATED softmax cases only (the scale-3 / p = 3 goldens).  With logits of magnitude
    |lse| ~ 10^2 the fp32 REFERENCE golden itself is only accurate to eps32 * |lse| relative to the summands; its own
    distance `dev` from the fp64 oracle is measured here with the same denominators the comparison uses.  Returns
    (tol, note): tol = 1e-5 unless dev > 2.5e-6, in which case tol = 1e-5 + 2 dev (the HIP result may sit on the other side
    of the fp64 truth) -- CAPPED at SAT_CAP = 3e-5 whatever the formula gives (an allowance that scales with the
    golden's own error must not be able to hide a regression; the largest error ever measured under it is 2.9e-5).
    Why these few rows cannot be held to 1e-5 at all: one ulp of a logit of magnitude 300 is 3e-5, and a softmax weight
    inherits the logit's ABSOLUTE error as a relative error, so two correct fp32 evaluations of the same row -- this one and
    the reference's, whose torch.norm accumulates in fp64 but then rounds to fp32 and takes ** p and / tau in fp32 -- differ
    by that much unless they share pow / exp bit for bit."""
    orc = O.lp_simclr_loss(z1, z2, z3, p=p, tau=tau, alpha=alpha, compat=compat, pow=pw)
    dev_ref = 0.0
    for k in ("loss_i", "dz1", "dz2", "dz3"):
        if k in ref and k in orc:
            fl = loss_floor if k == "loss_i" else (0.0 if k == "dz3" else grad_floor)
            den = max(float(np.abs(orc[k]).max()), fl, 1e-30)
            dev_ref = max(dev_ref, float(np.abs(np.asarray(ref[k], np.float64) - orc[k]).max()) / den)
    # (b) logits of magnitude |x| carry an fp32 evaluation error of ~eps32 |x| (the distance is a sum of n rounded
    # terms), which is a RELATIVE error on every softmax weight.  The CPU reference accumulates torch.norm in fp64
    # (at::acc_type<float, /*cuda*/false> = double) and so stays below that; any all-fp32 evaluation -- the reference's own
    # CUDA path included -- does not.  Only counted when the rows are saturated (|lse| > 20).
    lse_mag = float(np.abs(orc["lse"] + (0.0 if compat else np.log(np.asarray(z3).shape[0]))).max())
    logit_tol = 8.0 * float(np.finfo(np.float32).eps) * lse_mag if lse_mag > 20.0 else 0.0
    if dev_ref <= 2.5e-6 and logit_tol == 0.0:
        return None, None
    return min(SAT_CAP, TOL + max(2.0 * dev_ref if dev_ref > 2.5e-6 else 0.0, logit_tol)), \
        "saturated golden (|lse| > 20): tol = min(3e-5, 1e-5 + max(2 x fp32 reference's own deviation from the fp64 oracle, 8 eps32 max|lse|))"


@pytest.mark.parametrize("name", ["g1_lp_loss.npz", "g2_rect.npz", "g3_misc.npz", "g19_wide_lp.npz", "g22_lp_loss_large.npz"])
def test_lp_goldens(golden, name):
    from cl_ica_amd.losses import LpSimCLRLoss
    G = golden(name)
    for key, c in G.cases():
        m = c["meta"]
        p = float(m["p"]); p = int(p) if p == int(p) else p
        L = LpSimCLRLoss(p=p, tau=float(m["tau"]), alpha=float(m["alpha"]),
                         simclr_compatibility_mode=bool(m["compat"]), pow=bool(m["pow"]))
        out = run_hip(L, c["in"]["z1"], c["in"]["z2"], c["in"]["z3"])
        orc = O.lp_simclr_loss(c["in"]["z1"], c["in"]["z2"], c["in"]["z3"], p=float(m["p"]), tau=float(m["tau"]),
                               alpha=float(m["alpha"]), compat=bool(m["compat"]), pow=bool(m["pow"]), grad=False)
        lf, gf = summand_floors(orc, float(m["alpha"]), float(m["tau"]),
                                grad_scale(c["in"]["z1"], c["in"]["z2"], float(m["p"]), float(m["tau"]), float(m["alpha"])))
        mf = (float(np.abs(orc["pos"]).max()) / float(m["tau"]), float(np.abs(orc["lse"]).max()))
        sat_tol, note = saturation_allowance(c["in"]["z1"], c["in"]["z2"], c["in"]["z3"], float(m["p"]), float(m["tau"]),
                                             float(m["alpha"]), bool(m["compat"]), bool(m["pow"]), c["out"], lf, gf)
        case = (f"{key} p={float(m['p']):g} tau={float(m['tau']):g} compat={int(m['compat'])} "
                f"shape={c['in']['z1'].shape}x{c['in']['z3'].shape[0]}")
        compare(f"lp_goldens/{name[:-4]}", case, out, c["out"], ("dz1", "dz2", "dz3"), sat_tol, note, lf, gf, mf)
        # element-wise: against the fp64 oracle the HIP result may be at most 4 x as far off as the reference's own
        # fp32 golden is, element by element (p99.9) -- loss rows and all three gradients
        orc_g = O.lp_simclr_loss(c["in"]["z1"], c["in"]["z2"], c["in"]["z3"], p=float(m["p"]), tau=float(m["tau"]),
                                 alpha=float(m["alpha"]), compat=bool(m["compat"]), pow=bool(m["pow"]))
        # (saturated goldens -- |lse| > 20, see saturation_allowance: a logit's fp32 ulp is a RELATIVE error of every softmax weight, and the
        #  reference's fp64-accumulated norm escapes it -- get the same widening as the norm-wise check: factor 4 x sat_tol / 1e-5 <= 12)
        fac, fnote = (4.0, None) if sat_tol is None else (4.0 * sat_tol / TOL, "saturated golden: factor 4 x (norm-wise allowance / 1e-5)")
        for k in ("loss_i", "dz1", "dz2", "dz3"):
            PARITY.check_elementwise(f"lp_goldens/{name[:-4]}", case, k, out[k], c["out"][k], orc_g[k], factor=fac, note=fnote,
                                     scale_floor=lf if k == "loss_i" else (0.0 if k == "dz3" else gf))


def test_lp_roll_goldens(golden):
    """z3 = roll(z1) inside the autograd graph (main_mlp.py:272): exact-zero distances every row."""
    from cl_ica_amd.losses import LpSimCLRLoss
    for key, c in golden("g1r_lp_roll.npz").cases():
        m = c["meta"]
        L = LpSimCLRLoss(p=int(m["p"]), tau=float(m["tau"]), simclr_compatibility_mode=True)
        out = run_hip(L, c["in"]["z1"], c["in"]["z2"], None, roll=True)
        z1 = c["in"]["z1"]
        assert not np.isnan(out["dz1"]).any()
        orc = O.lp_simclr_loss(z1, c["in"]["z2"], np.roll(z1, 1, 0), p=float(m["p"]), tau=float(m["tau"]), compat=True, grad=False)
        lf, gf = summand_floors(orc, 0.5, float(m["tau"]), grad_scale(z1, c["in"]["z2"], float(m["p"]), float(m["tau"]), 0.5))
        mf = (float(np.abs(orc["pos"]).max()) / float(m["tau"]), float(np.abs(orc["lse"]).max()))
        sat_tol, note = saturation_allowance(z1, c["in"]["z2"], np.roll(z1, 1, 0), float(m["p"]), float(m["tau"]), 0.5, True, True,
                                             {"loss_i": c["out"]["loss_i"], "dz2": c["out"]["dz2"]}, lf, gf)
        compare("lp_roll_goldens", f"{key} p={int(m['p'])} shape={z1.shape}", out, c["out"], ("dz1", "dz2"), sat_tol, note, lf, gf, mf)


def test_lp_roll_fractional_p_vs_oracle():
    """p < 1 with z3 = roll(z1) in the graph: the reference's p < 1 branch transposes the pair matrix (losses.py:433-442), so
    row k of the negatives belongs to z3[k] = z1[k-1] while pos[k] is z1[k] vs z2[k] -- the roll shortcut (pool := z1) is NOT valid there
    and must not be taken.  Checked against the fp64 oracle fed the really rolled z3, compat on and off."""
    from cl_ica_amd import losses
    from cl_ica_amd.losses import LpSimCLRLoss
    rng = np.random.default_rng(5)
    z1 = rng.normal(size=(48, 6)).astype(np.float32)
    z2 = (z1 + 0.1 * rng.normal(size=z1.shape)).astype(np.float32)
    for compat in (True, False):
        losses.PATHS.clear()
        out = run_hip(LpSimCLRLoss(p=0.5, tau=0.7, simclr_compatibility_mode=compat), z1, z2, None, roll=True)
        assert not any(k.startswith("sym") for k in losses.PATHS), dict(losses.PATHS)
        orc = O.lp_simclr_loss(z1, z2, np.roll(z1, 1, 0), p=0.5, tau=0.7, compat=compat)
        ref = dict(loss_mean=orc["loss_mean"], loss_i=orc["loss_i"], dz1=orc["dz1"] + np.roll(orc["dz3"], -1, 0), dz2=orc["dz2"])
        fam, case = "lp_roll_fractional_p", f"p=0.5 compat={int(compat)}"
        PARITY.check(fam, case, "loss_mean", out["loss_mean"], float(ref["loss_mean"]))
        PARITY.check(fam, case, "loss_i", out["loss_i"], ref["loss_i"])
        PARITY.check(fam, case, "dz2", out["dz2"], ref["dz2"])
        # d |d + 1e-12|^0.5 / dd is 5e5 at the exact-zero pairs the roll guarantees; those terms enter dz1 through z1 and (rolled back)
        # through z3 with opposite signs, so dz1 is a cancelled sum of 1e4-sized summands (the fp32 reference itself sits 6e-3 of max|dz1|
        # from the fp64 oracle on this case): accurate relative to the summands -- the floor, as everywhere (summand_floors)
        PARITY.check(fam, case, "dz1", out["dz1"], ref["dz1"], floor=float(np.abs(orc["dz1"]).max()))
        # and NOT the value the shortcut would give (pool := z1 pairs pos[k] with the wrong row): the two differ by 5e-5 of the loss
        wrong = O.lp_simclr_loss(z1, z2, z1, p=0.5, tau=0.7, compat=compat, grad=False)
        if compat:
            assert abs(out["loss_mean"] - orc["loss_mean"]) < 0.1 * abs(wrong["loss_mean"] - orc["loss_mean"])


def test_rolled_rows_placeholder_equals_torch_roll():
    """`losses.RolledRows(z1, 1)` (the KITTI-masks solver's negatives, never materialised) gives bit for bit what ``torch.roll(z1, 1, 0)``
    gives through the same module: p = 1 / 2 on the one-sweep path, p = 0.5 by materialising the roll (the shortcut is invalid there)."""
    import torch
    from cl_ica_amd import losses
    from cl_ica_amd.losses import LpSimCLRLoss
    rng = np.random.default_rng(11)
    base = torch.tensor(rng.normal(size=(64, 5)).astype(np.float32), device="cuda")
    for p_, compat in ((1, True), (2, False), (0.5, True)):
        res = []
        for mode in ("placeholder", "roll"):
            mu = base.clone().requires_grad_(True)
            first, second = mu[::2], mu[1::2]
            losses.PATHS.clear()
            neg = losses.RolledRows(first, 1) if mode == "placeholder" else torch.roll(first, 1, 0)
            total, per_item, _ = LpSimCLRLoss(p=p_, tau=1.0, simclr_compatibility_mode=compat)(None, None, None, first, second, neg)
            total.backward()
            took_sym = any(k.startswith("sym") for k in losses.PATHS)
            assert took_sym == (p_ >= 1), (p_, mode, dict(losses.PATHS))
            res.append((float(total), per_item.detach().cpu().numpy(), mu.grad.detach().cpu().numpy()))
        assert res[0][0] == res[1][0], (p_, res[0][0], res[1][0])
        assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2]), p_


@pytest.fixture
def dot_path(request):
    """SimCLRLoss contraction path: "mfma" (default from n = 96: fp32 MFMA GEMMs over a materialised logit matrix) or "valu" (pair sweep)."""
    from cl_ica_amd import _lib
    assert _lib.load().clica_set_tuning(b"dot_mfma", 1 if request.param == "mfma" else 0) == 0
    yield request.param
    assert _lib.load().clica_set_tuning(b"dot_mfma", 1) == 0


@pytest.mark.parametrize("dot_path", ["mfma", "valu"], indirect=True)
@pytest.mark.parametrize("name", ["g5_simclr.npz", "g19_wide_simclr.npz"])
def test_simclr_goldens(golden, name, dot_path):
    from cl_ica_amd.losses import SimCLRLoss
    if dot_path == "valu" and name.startswith("g5"):
        pytest.skip("n < 96 takes the pair sweep in both settings")
    for key, c in golden(name).cases():
        m = c["meta"]
        L = SimCLRLoss(normalize=bool(m["normalize"]), tau=float(m["tau"]), alpha=float(m["alpha"]))
        out = run_hip(L, c["in"]["z1"], c["in"]["z2"], c["in"]["z3"])
        # un-cancelled size of the embedding gradients: the alignment pull (2 alpha / (B tau)) z2 (times d u / d z ~ 1 / |z| when
        # normalised); with a dominant positive (n = 512: <z1, z2> / tau ~ 10) the softmax push cancels it to 1/400th
        z1 = np.asarray(c["in"]["z1"], np.float64)
        mag = 1.0 / np.linalg.norm(z1, axis=1).min() if bool(m["normalize"]) else float(np.abs(c["in"]["z2"]).max())
        gf = 2 * float(m["alpha"]) / (z1.shape[0] * float(m["tau"])) * mag
        # loss_i = 2 (alpha (-pos / tau) + (1 - alpha) lse) cancels the same way: relative to the larger summand
        orc = O.simclr_loss(c["in"]["z1"], c["in"]["z2"], c["in"]["z3"], normalize=bool(m["normalize"]), tau=float(m["tau"]),
                            alpha=float(m["alpha"]), grad=False)
        pos_mag = float(np.abs(orc["lse"] - orc["loss_i"] / 2.0).max())       # ~ alpha |pos| / tau + alpha |lse|: size of the summands
        lf = 2.0 * max(pos_mag, (1.0 - float(m["alpha"])) * float(np.abs(orc["lse"]).max()))
        compare(f"simclr_goldens/{name[:-4]}" + ("/valu" if dot_path == "valu" else ""), f"{key} norm={int(m['normalize'])} tau={float(m['tau']):g} n={z1.shape[1]}", out,
                c["out"], ("dz1", "dz2", "dz3"), loss_floor=lf, grad_floor=gf, means_floor=(float(np.abs(orc["lse"]).max()),) * 2)


def test_strided_views(golden):
    """mu[::2] / mu[1::2] (kitti_masks/solver.py:64-65) and z[:, :k] (main_3dident.py:429-438)."""
    from cl_ica_amd.losses import LpSimCLRLoss
    G = golden("g10_strided.npz")
    c = G.case("kitti")
    mu = dev(c["in"]["mu"]).requires_grad_(True)
    a, b = mu[::2], mu[1::2]
    tot, per, (pm, nm) = LpSimCLRLoss(p=1, tau=1.0, simclr_compatibility_mode=True)(None, None, None, a, b, torch.roll(a, 1, 0))
    tot.backward()
    PARITY.check("strided_views", "kitti mu[::2]", "loss_mean", tot.item(), float(c["out"]["loss_mean"]))
    PARITY.check("strided_views", "kitti mu[::2]", "loss_i", per.detach().cpu().numpy(), c["out"]["loss_i"])
    PARITY.check("strided_views", "kitti mu[::2]", "dmu", mu.grad.cpu().numpy(), c["out"]["dmu"])
    c = G.case("ident")
    za = dev(c["in"]["z"]).requires_grad_(True); zb = dev(c["in"]["z2"]).requires_grad_(True)
    tot, per, _ = LpSimCLRLoss(p=2, tau=1.0, simclr_compatibility_mode=True)(
        None, None, None, za[:, :3], zb[:, :3], torch.roll(za, 1, 0)[:, :3])
    tot.backward()
    PARITY.check("strided_views", "ident z[:, :3]", "loss_i", per.detach().cpu().numpy(), c["out"]["loss_i"])
    PARITY.check("strided_views", "ident z[:, :3]", "dz", za.grad.cpu().numpy(), c["out"]["dz"])
    PARITY.check("strided_views", "ident z[:, :3]", "dz2", zb.grad.cpu().numpy(), c["out"]["dz2"])


def test_analytic_kats():
    from cl_ica_amd.losses import LpSimCLRLoss
    for B in (8, 512, 6144):
        z = torch.zeros(B, 10, device="cuda")
        v = LpSimCLRLoss(p=2, simclr_compatibility_mode=True)(None, None, None, z, z, z)[0].item()
        assert abs(v - np.log(B + 1)) < 1e-5 * np.log(B + 1)
        v = LpSimCLRLoss(p=2)(None, None, None, z, z, z)[0].item()
        assert abs(v) < 1e-5


@pytest.mark.parametrize("B,B3,n,p", [(6144, 6144, 10, 2), (6144, 6144, 10, 1), (1000, 3001, 7, 3), (6144, 12288, 40, 1),
                                       (300, 5000, 33, 2), (257, 63, 1, 2), (2048, 2048, 64, 1.5), (1, 1, 3, 2), (1, 777, 5, 1),
                                       (5, 2, 2, 3)])
def test_full_size_vs_oracle(B, B3, n, p):
    """BASELINE sizes and ragged shapes vs the fp64 oracle; all four upstream gradients exercised."""
    from cl_ica_amd.losses import LpSimCLRLoss
    rng = np.random.default_rng(B + n)
    z1 = rng.normal(size=(B, n)).astype(np.float32) * 0.7
    z2 = (z1 + 0.05 * rng.normal(size=(B, n))).astype(np.float32)
    z3 = rng.normal(size=(B3, n)).astype(np.float32) * 0.7
    gi = (rng.normal(size=B) / B).astype(np.float32)
    for compat in (True, False):
        a = dev(z1).requires_grad_(True); b = dev(z2).requires_grad_(True); c = dev(z3).requires_grad_(True)
        mean, per, (pm, nm) = LpSimCLRLoss(p=p, tau=0.8, alpha=0.4, simclr_compatibility_mode=compat)(None, None, None, a, b, c)
        (1.3 * mean + (per * dev(gi)).sum() + 0.4 * pm - 0.2 * nm).backward()
        orc = O.lp_simclr_loss(z1, z2, z3, p=p, tau=0.8, alpha=0.4, compat=compat, g_mean=1.3, g_item=gi, g_pos=0.4, g_neg=-0.2)
        fam, case = "full_size_vs_fp64_oracle", f"B={B} B3={B3} n={n} p={p} compat={int(compat)}"
        lf, gf = summand_floors(orc, 0.4, 0.8, grad_scale(z1, z2, p, 0.8, 0.4) * 2.5)       # 2.5: the upstream weights used above
        PARITY.check(fam, case, "loss_mean", mean.item(), orc["loss_mean"], floor=lf)
        PARITY.check(fam, case, "loss_i", per.detach().cpu().numpy(), orc["loss_i"], floor=lf)
        PARITY.check(fam, case, "pos_mean", pm.item(), orc["pos_mean"], floor=float(np.abs(orc["pos"]).max()) / 0.8)
        PARITY.check(fam, case, "neg_mean", nm.item(), orc["neg_mean"], floor=float(np.abs(orc["lse"]).max()))
        for got, name in ((a.grad, "dz1"), (b.grad, "dz2"), (c.grad, "dz3")):
            PARITY.check(fam, case, name, got.cpu().numpy(), orc[name], floor=0.0 if name == "dz3" else gf)


def test_permutation_invariance_and_roll_identity():
    """Size-independent properties at BASELINE size: the LSE is invariant to the order of z3 rows, so
    z3 = roll(z1) and z3 = z1 give the same loss (what the fused train step relies on)."""
    from cl_ica_amd.losses import LpSimCLRLoss
    torch.manual_seed(0)
    a = torch.randn(6144, 10, device="cuda"); b = a + 0.05 * torch.randn_like(a)
    L = LpSimCLRLoss(p=2, tau=1.0, simclr_compatibility_mode=True)
    v1 = L(None, None, None, a, b, torch.roll(a, 1, 0))
    v2 = L(None, None, None, a, b, a)
    perm = torch.randperm(6144, device="cuda")
    v3 = L(None, None, None, a, b, a[perm])
    assert abs(v1[0].item() - v2[0].item()) < 1e-6 * abs(v1[0].item())
    assert abs(v1[0].item() - v3[0].item()) < 1e-6 * abs(v1[0].item())
    assert torch.allclose(v1[1], v3[1], rtol=1e-5, atol=1e-6)


def test_error_paths():
    from cl_ica_amd.losses import LpSimCLRLoss
    from cl_ica_amd._lib import ClicaError
    z = torch.zeros(4, 3)
    with pytest.raises(ClicaError):
        LpSimCLRLoss(p=2)(None, None, None, z, z, z)          # CPU tensors: no fallback
    zc = torch.zeros(4, 513, device="cuda")
    with pytest.raises(ClicaError):
        LpSimCLRLoss(p=2)(None, None, None, zc, zc, zc)       # n > 512 (register kernels to 64, wide-row kernels to 512)
    with pytest.raises(ClicaError):
        LpSimCLRLoss(p=0.5)(None, None, None, zc[:, :3], zc[:, :3], torch.zeros(5, 3, device="cuda"))


def test_rowgrad_forward_equals_row_pass():
    """The flash-style row gradient accumulated in the forward sweep equals the backward's recomputing
    row pass (C ABI called directly both ways, all exponent kinds + dot)."""
    import ctypes as C
    from cl_ica_amd import _lib
    lib = _lib.load()
    torch.manual_seed(3)
    B, B3, n = 1500, 2100, 10
    z1 = torch.randn(B, n, device="cuda") * 0.6; z2 = z1 + 0.05 * torch.randn_like(z1); z3 = torch.randn(B3, n, device="cuda") * 0.6
    for p, pw in ((1, 1), (2, 1), (3, 1), (1.5, 1), (2, 0)):
        d = _lib.LpLossDesc(B=B, B3=B3, n=n, p=float(p), tau=0.9, alpha=0.4, compat=1, pow=pw)
        fb, bb = C.c_size_t(), C.c_size_t()
        _lib.check(lib.clica_lp_loss_workspace_bytes(C.byref(d), C.byref(fb), C.byref(bb)), "ws")
        ws = torch.zeros(max(fb.value, bb.value), dtype=torch.uint8, device="cuda")
        outs = []
        for use_rg in (False, True):
            o = torch.empty(3 * B + 3, device="cuda"); rg = torch.empty(B, n, device="cuda")
            dz = [torch.empty(B, n, device="cuda"), torch.empty(B, n, device="cuda"), torch.empty(B3, n, device="cuda")]
            rgp = rg.data_ptr() if use_rg else None
            _lib.check(lib.clica_lp_loss_fwd(C.byref(d), z1.data_ptr(), n, z2.data_ptr(), n, z3.data_ptr(), n, o[:B].data_ptr(),
                                             o[B:2 * B].data_ptr(), o[2 * B:3 * B].data_ptr(), o[3 * B:].data_ptr(), rgp, n,
                                             ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "fwd")
            _lib.check(lib.clica_lp_loss_bwd(C.byref(d), z1.data_ptr(), n, z2.data_ptr(), n, z3.data_ptr(), n, o[2 * B:3 * B].data_ptr(),
                                             rgp, n, None, None, None, None, dz[0].data_ptr(), n, dz[1].data_ptr(), n, dz[2].data_ptr(), n, 0,
                                             ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "bwd")
            torch.cuda.synchronize()
            outs.append((o.clone(), [t.clone() for t in dz]))
        assert torch.allclose(outs[0][0], outs[1][0], rtol=2e-6, atol=1e-6), p
        for a, b in zip(outs[0][1], outs[1][1]):
            assert (a - b).abs().max().item() < 2e-6 * max(a.abs().max().item(), 1e-6) + 1e-9, p


@pytest.mark.parametrize("gname", ["g12_align_uniform.npz", "g18_align_uniform_frac.npz"])
def test_uniformity_alignment_vs_golden(golden, gname):
    """UniformityLoss / AlignmentLoss (reference losses.py:205-241) on the all-pairs kernel, against G12 (p = 1, 2, 3) and
    G18 (fractional exponents 0.5, 0.75, 1.5: plain sum |d|^p, no eps branch)."""
    from cl_ica_amd.losses import AlignmentLoss, UniformityLoss
    G = golden(gname)
    for i in range(G.n_cases):
        u = G.case(f"u{i:03d}"); p = float(u["meta"]["p"])
        z1 = dev(u["in"]["z1"]).requires_grad_(True); z3 = dev(u["in"]["z3"]).requires_grad_(True)
        tot, per, extra = UniformityLoss(p)(z1, z3)
        tot.backward()
        assert extra[0] is tot
        PARITY.check("uniformity_goldens", f"u{i:03d} p={p:g}", "loss_mean", tot.item(), float(u["out"]["loss_mean"]))
        PARITY.check("uniformity_goldens", f"u{i:03d} p={p:g}", "loss_i", per.detach().cpu().numpy(), u["out"]["loss_i"])
        for name, t in (("dz1", z1), ("dz3", z3)):
            PARITY.check("uniformity_goldens", f"u{i:03d} p={p:g}", name, t.grad.cpu().numpy(), u["out"][name])
        a = G.case(f"a{i:03d}")
        z1 = dev(a["in"]["z1"]).requires_grad_(True); z2 = dev(a["in"]["z2"]).requires_grad_(True)
        tot, per, _ = AlignmentLoss(p)(z1, z2)
        tot.backward()
        PARITY.check("alignment_goldens", f"a{i:03d} p={p:g}", "loss_mean", tot.item(), float(a["out"]["loss_mean"]))
        PARITY.check("alignment_goldens", f"a{i:03d} p={p:g}", "loss_i", per.detach().cpu().numpy(), a["out"]["loss_i"])
        PARITY.check("alignment_goldens", f"a{i:03d} p={p:g}", "dz1", z1.grad.cpu().numpy(), a["out"]["dz1"])
        PARITY.check("alignment_goldens", f"a{i:03d} p={p:g}", "dz2", z2.grad.cpu().numpy(), a["out"]["dz2"])


def test_alignment_uniformity_loss_is_the_convex_combination(golden):
    """AlignmentUniformityLoss (reference losses.py:242-250: weights [1 - alpha, alpha]; the reference's own CombinedCLLoss cannot be
    called with the pair losses and raises) = (1 - alpha) x AlignmentLoss + alpha x UniformityLoss, value and all three gradients, against
    the reference's goldens of the two parts (G12) combined in fp64."""
    from cl_ica_amd.losses import AlignmentUniformityLoss
    G = golden("g12_align_uniform.npz")
    u, a = G.case("u000"), G.case("a000")
    p = float(u["meta"]["p"])
    for alpha in (0.5, 0.2):
        L = AlignmentUniformityLoss(alpha=alpha, p=p)
        # inputs: the uniformity golden's (z1, z3) with the alignment golden's z2 where its shape fits (else zeros); expectations: the fp64
        # oracle of the two parts, which tests/test_oracle_golden.py pins to the reference's G12 outputs
        z1 = dev(u["in"]["z1"]).requires_grad_(True); z3 = dev(u["in"]["z3"]).requires_grad_(True)
        z2 = dev(a["in"]["z2"][:z1.shape[0]] if a["in"]["z2"].shape[0] >= z1.shape[0] and a["in"]["z2"].shape[1] == z1.shape[1]
                 else np.zeros(tuple(z1.shape), np.float32)).requires_grad_(True)
        tot, per, (al, un) = L(None, None, None, z1, z2, z3)
        tot.backward()
        orc_u = O.uniformity_loss(u["in"]["z1"], u["in"]["z3"], p=p)
        orc_a = O.alignment_loss(u["in"]["z1"], z2.detach().cpu().numpy(), p=p)
        case = f"alpha={alpha} p={p:g}"
        PARITY.check("alignment_uniformity", case, "uniformity part", un.item(), orc_u["loss_mean"])
        PARITY.check("alignment_uniformity", case, "alignment part", al.item(), orc_a["loss_mean"])
        PARITY.check("alignment_uniformity", case, "loss", tot.item(), (1 - alpha) * orc_a["loss_mean"] + alpha * orc_u["loss_mean"])
        PARITY.check("alignment_uniformity", case, "dz1", z1.grad.cpu().numpy(), (1 - alpha) * orc_a["dz1"] + alpha * orc_u["dz1"])
        PARITY.check("alignment_uniformity", case, "dz2", z2.grad.cpu().numpy(), (1 - alpha) * orc_a["dz2"])
        PARITY.check("alignment_uniformity", case, "dz3", z3.grad.cpu().numpy(), alpha * orc_u["dz3"])
        if per is not None:
            PARITY.check("alignment_uniformity", case, "per_item", per.detach().cpu().numpy(), (1 - alpha) * orc_a["loss_i"] + alpha * orc_u["loss_i"])


def test_lp_loss_seeded_sweep_vs_oracle():
    """Forty seeded random shapes / parameters around the kernels' internal boundaries (owner tiles of 64, LDS tiles of 128
    rows, on-chip partitions of 16 rows, the planner's split lengths, the 64-coordinate switch to the wide-row kernels)
    against the fp64 oracle: loss_i and all three embedding gradients at 1e-5 of the un-cancelled summands."""
    from cl_ica_amd.losses import LpSimCLRLoss
    rng = np.random.default_rng(2024)
    edges_b = [1, 2, 31, 32, 33, 63, 64, 65, 127, 129, 200, 511, 640]
    edges_b3 = [1, 15, 16, 17, 127, 128, 129, 255, 257, 1000, 1023, 1025, 1537]
    dims = [1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 16, 17, 24, 33, 40, 41, 64, 65, 70, 129]
    for case in range(40):
        B, B3, n = int(rng.choice(edges_b)), int(rng.choice(edges_b3)), int(rng.choice(dims))
        p = float(rng.choice([1.0, 2.0, 3.0, 1.5, 2.5]))
        tau, alpha = float(rng.choice([0.5, 1.0, 2.0])), float(rng.choice([0.5, 0.3, 0.8]))
        compat, pw = bool(rng.integers(2)), bool(rng.integers(2))
        scale = 0.7 / np.sqrt(n)                       # summed distances stay O(1): unsaturated rows
        z1 = (rng.normal(size=(B, n)) * scale).astype(np.float32)
        z2 = (z1 + 0.1 * scale * rng.normal(size=(B, n))).astype(np.float32)
        z3 = (rng.normal(size=(B3, n)) * scale).astype(np.float32)
        L = LpSimCLRLoss(p=int(p) if p == int(p) else p, tau=tau, alpha=alpha, simclr_compatibility_mode=compat, pow=pw)
        out = run_hip(L, z1, z2, z3)
        orc = O.lp_simclr_loss(z1, z2, z3, p=p, tau=tau, alpha=alpha, compat=compat, pow=pw)
        lf, gf = summand_floors(orc, alpha, tau, grad_scale(z1, z2, p, tau, alpha))
        if not pw:        # pow=False: d|x|/dx of the root at a near-zero positive pair is O(1) whatever p is
            gf = max(gf, 2 * alpha / (B * tau))
        case_id = f"#{case} B={B} B3={B3} n={n} p={p:g} tau={tau:g} alpha={alpha:g} compat={int(compat)} pow={int(pw)}"
        PARITY.check("lp_sweep_vs_oracle", case_id, "loss_i", out["loss_i"], orc["loss_i"], floor=lf)
        PARITY.check("lp_sweep_vs_oracle", case_id, "loss_mean", out["loss_mean"], float(orc["loss_mean"]), floor=lf)
        for g in ("dz1", "dz2", "dz3"):
            PARITY.check("lp_sweep_vs_oracle", case_id, g, out[g], orc[g], floor=gf if g != "dz3" else float(np.abs(orc["dz3"]).max()))


def test_other_losses_seeded_sweep_vs_oracle():
    """Seeded random shapes for the remaining loss kinds against the fp64 oracle: SimCLRLoss with and without row
    normalisation (incl. rows wider than 64), LpSimCLRLoss in its p < 1 eps branch (B3 = B), UniformityLoss / AlignmentLoss
    with fractional and integer exponents."""
    from cl_ica_amd.losses import AlignmentLoss, LpSimCLRLoss, SimCLRLoss, UniformityLoss
    rng = np.random.default_rng(31)
    shapes_b = [1, 2, 33, 64, 65, 130, 400]
    shapes_b3 = [1, 16, 17, 129, 300, 1025]
    dims = [2, 3, 10, 13, 40, 64, 65, 128]
    for case in range(16):                                           # dot-product InfoNCE
        B, B3, n = int(rng.choice(shapes_b)), int(rng.choice(shapes_b3)), int(rng.choice(dims))
        normalize = bool(rng.integers(2)); tau = float(rng.choice([0.2, 0.5, 1.0])); alpha = float(rng.choice([0.5, 0.3]))
        sc = 1.0 if normalize else 1.0 / np.sqrt(n)
        z1 = (rng.normal(size=(B, n)) * sc).astype(np.float32); z2 = (z1 + 0.2 * sc * rng.normal(size=(B, n))).astype(np.float32)
        z3 = (rng.normal(size=(B3, n)) * sc).astype(np.float32)
        out = run_hip(SimCLRLoss(normalize=normalize, tau=tau, alpha=alpha), z1, z2, z3)
        orc = O.simclr_loss(z1, z2, z3, normalize=normalize, tau=tau, alpha=alpha)
        mag = 1.0 / np.linalg.norm(z1.astype(np.float64), axis=1).min() if normalize else float(np.abs(z2).max())
        gf = 2 * alpha / (B * tau) * mag
        lf = 2.0 * max(float(np.abs(orc["lse"] - orc["loss_i"] / 2.0).max()), (1.0 - alpha) * float(np.abs(orc["lse"]).max()))
        cid = f"dot #{case} B={B} B3={B3} n={n} norm={int(normalize)} tau={tau:g}"
        PARITY.check("other_losses_sweep", cid, "loss_i", out["loss_i"], orc["loss_i"], floor=lf)
        for g in ("dz1", "dz2", "dz3"):
            PARITY.check("other_losses_sweep", cid, g, out[g], orc[g], floor=gf if g != "dz3" else float(np.abs(orc["dz3"]).max()))
    for case in range(8):                                            # p < 1: eps inside the abs, transposed pair orientation
        B, n = int(rng.choice([2, 33, 64, 130])), int(rng.choice([2, 5, 10, 17]))
        p = float(rng.choice([0.5, 0.75])); tau = float(rng.choice([0.5, 1.0]))
        z1 = rng.normal(size=(B, n)).astype(np.float32) * 0.5; z2 = (z1 + 0.05 * rng.normal(size=(B, n))).astype(np.float32)
        z3 = rng.normal(size=(B, n)).astype(np.float32) * 0.5
        out = run_hip(LpSimCLRLoss(p=p, tau=tau, simclr_compatibility_mode=True), z1, z2, z3)
        orc = O.lp_simclr_loss(z1, z2, z3, p=p, tau=tau, alpha=0.5, compat=True, pow=True)
        lf, gf = summand_floors(orc, 0.5, tau, grad_scale(z1, z2, p, tau, 0.5))
        cid = f"frac #{case} B={B} n={n} p={p:g} tau={tau:g}"
        PARITY.check("other_losses_sweep", cid, "loss_i", out["loss_i"], orc["loss_i"], floor=lf)
        for g in ("dz1", "dz2", "dz3"):
            # pull and push cancel when the positive dominates the softmax (n = 17, p = 0.5: the fp32 reference returns loss 0
            # and dz2 = 0 exactly there, the fp64 oracle 1e-8 and 3e-7): relative to the pull's scale, as everywhere else
            PARITY.check("other_losses_sweep", cid, g, out[g], orc[g], floor=gf if g != "dz3" else max(float(np.abs(orc["dz3"]).max()), 1e-3 * gf))
    for case in range(8):                                            # uniformity / alignment
        B, B3, n = int(rng.choice(shapes_b[1:])), int(rng.choice(shapes_b3[1:])), int(rng.choice(dims[:6]))
        p = float(rng.choice([0.5, 1.0, 1.5, 2.0, 3.0]))
        z1 = (rng.normal(size=(B, n)) / np.sqrt(n)).astype(np.float32); z3 = (rng.normal(size=(B3, n)) / np.sqrt(n)).astype(np.float32)
        z2 = (z1 + 0.1 * rng.normal(size=(B, n)) / np.sqrt(n)).astype(np.float32)
        a = dev(z1).requires_grad_(True); c = dev(z3).requires_grad_(True)
        u, ui, _ = UniformityLoss(p)(a, c); u.backward()
        ou = O.uniformity_loss(z1, z3, p)
        cid = f"unif #{case} B={B} B3={B3} n={n} p={p:g}"
        comp = max(float(np.abs(ou["loss_i"]).max()) + np.log(B3), 1.0)
        PARITY.check("other_losses_sweep", cid, "loss_i", ui.detach().cpu().numpy(), ou["loss_i"], floor=comp)
        wscale = float(np.abs(O._dpowabs(z1[None].astype(np.float64) - z3[:, None].astype(np.float64), p)).max()) / B3
        PARITY.check("other_losses_sweep", cid, "dz1", a.grad.cpu().numpy(), ou["dz1"], floor=wscale)
        PARITY.check("other_losses_sweep", cid, "dz3", c.grad.cpu().numpy(), ou["dz3"], floor=wscale)
        a = dev(z1).requires_grad_(True); b = dev(z2).requires_grad_(True)
        al, ali, _ = AlignmentLoss(p)(a, b); al.backward()
        oa = O.alignment_loss(z1, z2, p)
        PARITY.check("other_losses_sweep", "align" + cid[4:], "loss_i", ali.detach().cpu().numpy(), oa["loss_i"])
        PARITY.check("other_losses_sweep", "align" + cid[4:], "dz1", a.grad.cpu().numpy(), oa["dz1"], floor=1e-3 * float(np.abs(oa["dz1"]).max()))


@pytest.mark.parametrize("normalize", [False, True])
def test_simclr_mfma_matches_pair_sweep(normalize):
    """SimCLRLoss (losses.py:162-202) at n = 192, B = 1000, B3 = 2501 (ragged chunk, B3 % 4 != 0): the MFMA path (logit matrix +
    three fp32-MFMA GEMMs) against the pair sweep and the fp64 oracle, with gradients flowing into every output."""
    import os
    from cl_ica_amd import _lib
    from cl_ica_amd.losses import SimCLRLoss
    rng = np.random.default_rng(5)
    B, B3, n = 1000, 2501, 192
    z1 = rng.standard_normal((B, n)).astype(np.float32) * 0.3
    z2 = (z1 + 0.1 * rng.standard_normal((B, n))).astype(np.float32)
    z3 = rng.standard_normal((B3, n)).astype(np.float32) * 0.3
    gi = rng.standard_normal(B).astype(np.float32)
    res = {}
    for path in ("1", "0"):
        assert _lib.load().clica_set_tuning(b"dot_mfma", int(path)) == 0
        a, b, c = (dev(x).requires_grad_(True) for x in (z1, z2, z3))
        tot, per, (pm, nm) = SimCLRLoss(normalize=normalize, tau=0.7, alpha=0.4)(None, None, None, a, b, c)
        (tot + (per * dev(gi)).sum() * 1e-3 + 0.5 * pm - 0.25 * nm).backward()
        res[path] = [t.detach().cpu().numpy().astype(np.float64) for t in (tot, per, pm, nm, a.grad, b.grad, c.grad)]
    assert _lib.load().clica_set_tuning(b"dot_mfma", 1) == 0
    orc = O.simclr_loss(z1, z2, z3, normalize=normalize, tau=0.7, alpha=0.4, grad=False)
    for name, x, y in zip(("loss", "loss_i", "pos", "neg", "dz1", "dz2", "dz3"), res["1"], res["0"]):
        PARITY.check("simclr_mfma_vs_sweep", f"norm={int(normalize)}", name, x, y)
    for path in ("1", "0"):
        PARITY.check("simclr_mfma_vs_sweep", f"norm={int(normalize)} path={path} vs fp64 oracle", "loss_i", res[path][1], orc["loss_i"])


@pytest.fixture
def matrix_cores_every_pool():
    """Round 6: by default the matrix-core sweeps run only against a pool of >= 4 x the local rows (include/clica.h); the tests that
    characterise them at a local pool (B3 = B) switch them on for every pool and restore the default policy afterwards."""
    from cl_ica_amd import _lib
    _lib.check(_lib.load().clica_lp_loss_set_matrix_cores(2), "every pool")
    yield
    _lib.check(_lib.load().clica_lp_loss_set_matrix_cores(-1), "default policy")


def _train_pair(z1, z2, pool, pool_lse, n, p, tau, alpha, compat=1, pow=1):
    """clica_lp_loss_fwd_train + clica_lp_loss_bwd_sym_train on device tensors; returns (out [3B+3], dz [2B, n], path).
    The matrix-core sweeps build their planes on the grid the PREVIOUS call measured (csrc/lp_mfma.h), so a fresh workspace gets one
    un-checked forward call first; `path` is 1 only if the checked forward then really ran on the matrix cores (no fallback counted)."""
    import ctypes as C
    from cl_ica_amd import _lib
    lib = _lib.load()
    B, B3 = z1.shape[0], pool.shape[0]
    d = _lib.LpLossDesc(B=B, B3=B3, n=n, p=float(p), tau=tau, alpha=alpha, compat=compat, pow=pow)
    nb, path = C.c_size_t(), C.c_int32()
    _lib.check(lib.clica_lp_loss_train_workspace_bytes(C.byref(d), C.byref(nb)), "ws")
    _lib.check(lib.clica_lp_loss_train_path(C.byref(d), C.byref(path)), "path")
    ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
    o = torch.empty(3 * B + 3, device="cuda"); dz = torch.full((2 * B, n), float("nan"), device="cuda")
    st = _lib.stream_ptr()

    def fwd():
        _lib.check(lib.clica_lp_loss_fwd_train(C.byref(d), z1.data_ptr(), z1.stride(0), z2.data_ptr(), z2.stride(0), pool.data_ptr(), pool.stride(0),
                                               o[:B].data_ptr(), o[B:2 * B].data_ptr(), o[2 * B:3 * B].data_ptr(),
                                               dz[:B].data_ptr(), n, dz[B:].data_ptr(), n, ws.data_ptr(), ws.numel(), st), "fwd_train")

    def fallbacks():
        v = (C.c_float * 4)()
        _lib.check(lib.clica_lp_loss_train_guard(C.byref(d), ws.data_ptr(), ws.numel(), v, st), "guard")
        return int(v[3]), float(v[1]), float(v[2])

    fwd()                                  # measures the grid (and falls back itself: there was none)
    before = fallbacks()[0]
    dz.fill_(float("nan"))
    fwd()
    after, m_step, limit = fallbacks()
    if path.value == 1 and m_step <= limit and after != before:
        path.value = -1                    # should have run on the matrix cores and did not
    elif path.value == 1 and m_step > limit:
        path.value = 2                     # beyond the guard's limit: the difference sweeps, by design
    lse = o[2 * B:3 * B] if pool_lse is None else pool_lse
    if pool_lse is not None and pool_lse.numel() == 0:
        return o, dz, path.value          # forward only
    _lib.check(lib.clica_lp_loss_bwd_sym_train(C.byref(d), z1.data_ptr(), z1.stride(0), pool.data_ptr(), pool.stride(0), o[2 * B:3 * B].data_ptr(),
                                               lse.data_ptr(), dz[:B].data_ptr(), n, o[3 * B:].data_ptr(), None, ws.data_ptr(), ws.numel(), st),
               "bwd_sym_train")
    torch.cuda.synchronize()
    return o, dz, path.value


@pytest.mark.gpu
@pytest.mark.parametrize("B,n,tau,space", [(6144, 10, 1.0, "box"), (1000, 3, 0.3, "box"), (333, 9, 1.0, "sphere"), (97, 1, 0.5, "box"),
                                           (2048, 10, 0.1, "box"), (4096, 7, 1.0, "far")])
def test_p2_train_sweeps_on_matrix_cores_vs_oracle(B, n, tau, space, matrix_cores_every_pool):
    """The p = 2 training sweeps on the bf16 matrix cores (csrc/lp_mfma.hip) against the fp64 oracle, single rank (pool = z1): loss
    statistics and the complete gradient, at the bench size and at ragged sizes / other widths / temperatures.  'far': the cloud sits
    1000 units from the coordinate origin (the kernel shifts rows by an origin inside the data: the expansion must not see the offset)."""
    rng = np.random.default_rng(B + n)
    alpha = 0.5
    if space == "sphere":
        z = rng.normal(size=(B, n)); z /= np.linalg.norm(z, axis=1, keepdims=True)
        zt = z + 0.05 * rng.normal(size=(B, n)); zt /= np.linalg.norm(zt, axis=1, keepdims=True)
    else:
        z = rng.random((B, n)); zt = np.clip(z + 0.05 * rng.normal(size=(B, n)), 0, 1)
        if space == "far":
            z += 1000.0; zt += 1000.0
    z, zt = z.astype(np.float32), zt.astype(np.float32)
    o, dz, path = _train_pair(dev(z), dev(zt), dev(z), None, n, 2, tau, alpha)
    assert path == 1, "the p = 2 training sweeps must take the matrix-core path (switched on for every pool by the fixture)"
    # the engine's single-rank call passes ONE buffer as anchors and pool: then the forward's finalize writes the pool's feature planes
    # itself (no plane launch in the backward call) -- same builder, so the same bits as the two-buffer call above
    zd = dev(z)
    o1, dz1b, _ = _train_pair(zd, dev(zt), zd, None, n, 2, tau, alpha)
    assert torch.equal(o1, o) and torch.equal(dz1b, dz)
    orc = O.lp_simclr_loss(z, zt, z, p=2, tau=tau, alpha=alpha, compat=True, grad=False)
    fam, case = "p2_train_matrix_cores", f"B={B} n={n} tau={tau} {space}"
    oc = o.cpu().numpy()
    LN2 = np.log(2.0)
    PARITY.check(fam, case, "loss_i", oc[:B], orc["loss_i"])
    PARITY.check(fam, case, "lse_i", oc[2 * B:3 * B].astype(np.float64) * LN2, orc["lse"])
    lse_nat = orc["lse"]
    g1, g2 = O.lp_symmetric_row_grads(z, zt, z, lse_nat, lse_nat, 2, tau, alpha, local_rows=B)
    PARITY.check(fam, case, "dz1", dz[:B].cpu().numpy(), g1)
    PARITY.check(fam, case, "dz2", dz[B:].cpu().numpy(), g2)
    assert abs(oc[3 * B] - oc[:B].astype(np.float64).mean()) < 2e-6 * abs(oc[3 * B])


@pytest.mark.gpu
def _spread_of(z, tau):
    """M as the library measures it: log2(e)/tau max_i |z_i - origin|^2, origin = mean of the pool's first 64 rows."""
    z = np.asarray(z, np.float64)
    return 1.4426950408889634 / tau * float(((z - z[:64].mean(0)) ** 2).sum(1).max())


def _guard_state(d, ws):
    import ctypes as C
    from cl_ica_amd import _lib
    v = (C.c_float * 4)()
    _lib.check(_lib.load().clica_lp_loss_train_guard(C.byref(d), ws.data_ptr(), ws.numel(), v, _lib.stream_ptr()), "guard")
    return dict(max_spread=float(v[0]), last_spread=float(v[1]), limit=float(v[2]), fallback_steps=int(v[3]))


@pytest.mark.gpu
def test_p2_train_sweeps_on_matrix_cores_spread_limit(matrix_cores_every_pool):
    """The guard of the matrix-core sweeps (include/clica.h).  The expansion's terms are of size M = log2(e)/tau max_i |z_i - origin|^2; the
    logit's large part is exact, so the LOSS holds 1e-5 at every spread, but the gradient's second product accumulates terms of size
    sqrt(M) in fp32 and its error grows ~ sqrt(M).  Box clouds of growing edge at tau = 1 against the fp64 oracle:
    (A) with the DEFAULT limit every spread -- far beyond what the reference's training reaches -- holds 1e-5 in loss and gradient, because
        calls beyond the limit fall back to the coordinate-difference sweeps on the device (counted by the guard);
    (B) with the guard LIFTED (limit = 1e30) the raw error of the matrix-core sweeps is logged per spread: the curve the default limit was
        chosen from (asserted at 1e-5 up to the limit, logged at 1e-4 beyond it -- a path the default never takes)."""
    import ctypes as C
    from cl_ica_amd import _lib
    lib = _lib.load()
    B, n, tau, alpha = 2048, 10, 1.0, 0.5
    rng = np.random.default_rng(5)
    base = rng.random((B, n)); noise = 0.05 * rng.normal(size=(B, n))
    # (three points right below / at / above the limit -- M ~ 700, 755, 780 -- so that the 1e-5 claim is ASSERTED where the
    #  limit sits and not interpolated between 631 and 1 304; inside the limit the raw gradient error must stay <= 8e-6)
    edges = (1.0, 2.0, 4.0, 6.0, 8.0, 11.0, 13.0, 16.0, 16.85, 17.5, 17.8, 23.0, 32.0, 64.0)
    refs = {}
    for edge in edges:
        z = (edge * base).astype(np.float32); zt = (edge * base + noise).astype(np.float32)
        orc = O.lp_simclr_loss(z, zt, z, p=2, tau=tau, alpha=alpha, compat=True, grad=False)
        g1, _ = O.lp_symmetric_row_grads(z, zt, z, orc["lse"], orc["lse"], 2, tau, alpha, local_rows=B)
        refs[edge] = (z, zt, orc["loss_i"], g1, _spread_of(z, tau))
    d = _lib.LpLossDesc(B=B, B3=B, n=n, p=2.0, tau=tau, alpha=alpha, compat=1, pow=1)
    nb = C.c_size_t(); _lib.check(lib.clica_lp_loss_train_workspace_bytes(C.byref(d), C.byref(nb)), "ws")

    def run(z, zt, ws):
        zd, ztd = dev(z), dev(zt)
        o = torch.empty(3 * B + 3, device="cuda"); dz = torch.empty(2 * B, n, device="cuda")
        st = _lib.stream_ptr()
        # (the planes are built on the grid the previous call measured: one un-checked forward on THIS cloud first)
        _lib.check(lib.clica_lp_loss_fwd_train(C.byref(d), zd.data_ptr(), n, ztd.data_ptr(), n, zd.data_ptr(), n, o[:B].data_ptr(), o[B:2 * B].data_ptr(),
                                               o[2 * B:3 * B].data_ptr(), dz[:B].data_ptr(), n, dz[B:].data_ptr(), n, ws.data_ptr(), ws.numel(), st), "fwd_train (grid)")
        run.before = _guard_state(d, ws)["fallback_steps"]
        _lib.check(lib.clica_lp_loss_fwd_train(C.byref(d), zd.data_ptr(), n, ztd.data_ptr(), n, zd.data_ptr(), n, o[:B].data_ptr(), o[B:2 * B].data_ptr(),
                                               o[2 * B:3 * B].data_ptr(), dz[:B].data_ptr(), n, dz[B:].data_ptr(), n, ws.data_ptr(), ws.numel(), st), "fwd_train")
        _lib.check(lib.clica_lp_loss_bwd_sym_train(C.byref(d), zd.data_ptr(), n, zd.data_ptr(), n, o[2 * B:3 * B].data_ptr(), o[2 * B:3 * B].data_ptr(),
                                                   dz[:B].data_ptr(), n, o[3 * B:].data_ptr(), None, ws.data_ptr(), ws.numel(), st), "bwd_sym_train")
        torch.cuda.synchronize()
        return o.cpu().numpy(), dz.cpu().numpy()

    # (A) the default guard
    _lib.check(lib.clica_lp_loss_set_spread_limit(0.0), "default limit")
    ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
    limit = _guard_state(d, ws)["limit"]
    expected_fallbacks = 0
    for edge in edges:
        z, zt, li, g1, M = refs[edge]
        o, dz = run(z, zt, ws)
        st = _guard_state(d, ws)
        assert abs(st["last_spread"] - M) < 2e-3 * M, (st, M)
        expected_fallbacks += int(st["last_spread"] > limit)
        assert st["fallback_steps"] - run.before == int(st["last_spread"] > limit), (edge, st, run.before)      # the checked call fell back iff M > limit
        path = "difference sweeps (guard)" if st["last_spread"] > limit else "matrix cores"
        PARITY.check("p2_train_guarded", f"box edge {edge} (M = {M:.0f}, {path})", "loss_i", o[:B], li)
        PARITY.check("p2_train_guarded", f"box edge {edge} (M = {M:.0f}, {path})", "dz1", dz[:B], g1)
    assert 0 < expected_fallbacks < len(edges), "the sweep of edges must cross the limit"
    assert abs(_guard_state(d, ws)["max_spread"] - max(r[4] for r in refs.values())) < 2e-3 * max(r[4] for r in refs.values())
    # (A2) a cloud that GROWS between two calls: the planes of the second call sit on the grid the smaller cloud left behind.  Up to 2 x
    #      beyond that grid the expansion stays exact (rows on the doubled grid step), so the call stays on the matrix cores and holds
    #      1e-5; beyond 2 x it falls back.  (The reference's training moves the cloud's extent by per cents per step.)
    ws3 = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
    z6, zt6, li6, g6, M6 = refs[6.0]

    def one_call(z, zt, ws, bwd):
        zd, ztd = dev(z), dev(zt)
        o = torch.empty(3 * B + 3, device="cuda"); dz = torch.empty(2 * B, n, device="cuda")
        st = _lib.stream_ptr()
        _lib.check(lib.clica_lp_loss_fwd_train(C.byref(d), zd.data_ptr(), n, ztd.data_ptr(), n, zd.data_ptr(), n, o[:B].data_ptr(), o[B:2 * B].data_ptr(),
                                               o[2 * B:3 * B].data_ptr(), dz[:B].data_ptr(), n, dz[B:].data_ptr(), n, ws.data_ptr(), ws.numel(), st), "fwd_train")
        if bwd:
            _lib.check(lib.clica_lp_loss_bwd_sym_train(C.byref(d), zd.data_ptr(), n, zd.data_ptr(), n, o[2 * B:3 * B].data_ptr(), o[2 * B:3 * B].data_ptr(),
                                                       dz[:B].data_ptr(), n, o[3 * B:].data_ptr(), None, ws.data_ptr(), ws.numel(), st), "bwd_sym_train")
        torch.cuda.synchronize()
        return o.cpu().numpy(), dz.cpu().numpy()

    centre = z6.mean(axis=0, keepdims=True)
    # (the grid step leaves max |x'| / D in [124, 248): growth <= 2 x always stays below 512, growth > 4.2 x never does)
    for shrink, stays in ((1.0 / 1.7, True), (1.0 / 4.5, False)):
        zs = (centre + shrink * (z6 - centre)).astype(np.float32); zts = (centre + shrink * (zt6 - centre)).astype(np.float32)
        one_call(zs, zts, ws3, False); one_call(zs, zts, ws3, False)              # the grid of the SMALL cloud is in force and measured
        before = _guard_state(d, ws3)["fallback_steps"]
        o, dz = one_call(z6, zt6, ws3, True)                                      # the cloud grew by 1 / shrink since the last call
        fell = _guard_state(d, ws3)["fallback_steps"] - before
        assert fell == (0 if stays else 1), (shrink, fell)
        case = f"box edge 6 right after the same cloud at edge {6 * shrink:.2f} ({'matrix cores, rows beyond the grid' if stays else 'difference sweeps'})"
        PARITY.check("p2_train_guarded", case, "loss_i", o[:B], li6)
        PARITY.check("p2_train_guarded", case, "dz1", dz[:B], g6)
    # (B) the guard lifted: the raw error curve of the matrix-core sweeps
    _lib.check(lib.clica_lp_loss_set_spread_limit(1e30), "lift")
    try:
        ws2 = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
        curve = {}
        for edge in edges:
            z, zt, li, g1, M = refs[edge]
            o, dz = run(z, zt, ws2)
            assert _guard_state(d, ws2)["fallback_steps"] == run.before, "guard lifted: the checked call must run on the matrix cores"
            curve[round(M)] = (rel_err(o[:B], li), rel_err(dz[:B], g1))
            inside = M <= limit
            fam = "p2_train_matrix_cores" if inside else "p2_train_matrix_cores_guard_lifted_characterisation"
            note = None if inside else "guard lifted (limit 1e30): a spread the default path hands to the difference sweeps; logged to document the limit"
            PARITY.check(fam, f"box edge {edge} (M = {M:.0f})", "loss_i", o[:B], li)
            PARITY.check(fam, f"box edge {edge} (M = {M:.0f})", "dz1", dz[:B], g1, tol=1e-5 if inside else 1e-4, note=note)
            if inside:
                assert curve[round(M)][1] <= 8e-6, f"matrix-core gradient error {curve[round(M)][1]:.2e} at M = {M:.0f} inside the limit {limit:.0f}: lower the limit"
        print("matrix-core sweep error by spread M (loss_i, dz1), guard lifted:", curve, "limit", limit)
        import json, os
        out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
        os.makedirs(out, exist_ok=True)
        json.dump({"what": "raw error of the p = 2 matrix-core loss sweeps against the fp64 oracle by spread M (guard lifted), box clouds, B = 2048, n = 10, tau = 1",
                   "limit_in_force": limit, "M": list(curve), "loss_i_rel_err": [v[0] for v in curve.values()],
                   "dz1_rel_err": [v[1] for v in curve.values()]}, open(os.path.join(out, "r6_loss_spread_curve.json"), "w"), indent=1)
    finally:
        _lib.check(lib.clica_lp_loss_set_spread_limit(0.0), "restore")
    # the older diagnostic entry point still answers (largest M a workspace has seen)
    got = C.c_float()
    _lib.check(lib.clica_lp_loss_train_spread(C.byref(d), ws.data_ptr(), ws.numel(), C.byref(got), _lib.stream_ptr()), "spread")
    assert abs(got.value - _guard_state(d, ws)["max_spread"]) < 1e-6 * got.value


@pytest.mark.gpu
def test_p2_train_default_policy_local_pool_runs_the_difference_sweeps():
    """The default policy (round 6): a single-rank step (pool = the local rows) runs the coordinate-difference sweeps, a pool of >= 4 x the
    local rows the matrix cores; 2 forces them for every pool, 0 removes them.  And the difference sweeps at the local pool hold the oracle
    with the margin that motivated the policy (<= 4e-6 on loss and gradient at the bench size, inside the reference's spread)."""
    import ctypes as C
    from cl_ica_amd import _lib
    lib, path = _lib.load(), C.c_int32()
    _lib.check(lib.clica_lp_loss_set_matrix_cores(-1), "default")

    def path_of(B, B3):
        d = _lib.LpLossDesc(B=B, B3=B3, n=10, p=2.0, tau=1.0, alpha=0.5, compat=1, pow=1)
        _lib.check(lib.clica_lp_loss_train_path(C.byref(d), C.byref(path)), "path")
        return path.value
    if os.environ.get("CLICA_LP_MFMA") in (None, "1"):
        assert path_of(6144, 6144) == 0 and path_of(6144, 3 * 6144) == 0 and path_of(6144, 4 * 6144) == 1 and path_of(6144, 49152) == 1
    try:
        _lib.check(lib.clica_lp_loss_set_matrix_cores(2), "every pool"); assert path_of(6144, 6144) == 1
        _lib.check(lib.clica_lp_loss_set_matrix_cores(0), "never"); assert path_of(6144, 49152) == 0
    finally:
        _lib.check(lib.clica_lp_loss_set_matrix_cores(-1), "default")
    rng = np.random.default_rng(77)
    B, n, tau, alpha = 6144, 10, 1.0, 0.5
    z = (12.0 * rng.random((B, n))).astype(np.float32)              # M ~ 350-400: the spread of the reference's own training
    zt = (z + 0.05 * rng.normal(size=(B, n))).astype(np.float32)
    o, dz, pth = _train_pair(dev(z), dev(zt), dev(z), None, n, 2, tau, alpha)
    assert pth == 0
    orc = O.lp_simclr_loss(z, zt, z, p=2, tau=tau, alpha=alpha, compat=True, grad=False)
    g1, g2 = O.lp_symmetric_row_grads(z, zt, z, orc["lse"], orc["lse"], 2, tau, alpha, local_rows=B)
    case = f"B={B} n={n} box edge 12 (M = {_spread_of(z, tau):.0f}), difference sweeps by the default policy"
    PARITY.check("p2_train_default_policy", case, "loss_i", o[:B].cpu().numpy(), orc["loss_i"], tol=4e-6, note="margin asserted: 2.5 x inside the contract")
    PARITY.check("p2_train_default_policy", case, "dz1", dz[:B].cpu().numpy(), g1, tol=4e-6, note="margin asserted: 2.5 x inside the contract")
    PARITY.check("p2_train_default_policy", case, "dz2", dz[B:].cpu().numpy(), g2, tol=4e-6, note="margin asserted: 2.5 x inside the contract")


@pytest.mark.gpu
def test_p2_train_sweeps_on_matrix_cores_pool_49152():
    """The 8-rank shape of BASELINE config 2: B = 6144 local rows against the gathered pool of 49 152 rows, n = 10, p = 2; 96 sampled
    rows exactly against the fp64 oracle (forward statistics of rows from every 'rank', gradients of local rows)."""
    rng = np.random.default_rng(21)
    B, R, n, tau, alpha = 6144, 8, 10, 1.0, 0.5
    Bg = B * R
    z_all = rng.random((Bg, n)).astype(np.float32)
    zt_all = np.clip(z_all + 0.05 * rng.normal(size=(Bg, n)), 0, 1).astype(np.float32)
    pool, pool2 = dev(z_all), dev(zt_all)
    lse_all = torch.empty(Bg, device="cuda")
    empty = torch.empty(0, device="cuda")
    for r in range(R):
        sl = slice(r * B, (r + 1) * B)
        o_r, _, path = _train_pair(pool[sl], pool2[sl], pool, empty, n, 2, tau, alpha)
        assert path == 1
        lse_all[sl] = o_r[2 * B:3 * B]
    o, dz, _ = _train_pair(pool[:B], pool2[:B], pool, lse_all, n, 2, tau, alpha)
    S = np.sort(rng.choice(B, size=96, replace=False))
    S2 = np.sort(rng.choice(Bg, size=64, replace=False))
    fam, case = "p2_train_matrix_cores", f"B={B} B3={Bg} n={n} (sampled rows)"
    LN2 = np.log(2.0)
    orc = O.lp_simclr_loss(z_all[S], zt_all[S], z_all, p=2, tau=tau, alpha=alpha, compat=True, grad=False)
    orc2 = O.lp_simclr_loss(z_all[S2], zt_all[S2], z_all, p=2, tau=tau, alpha=alpha, compat=True, grad=False)
    oc = o.cpu().numpy()
    lse_nat = lse_all.cpu().numpy().astype(np.float64) * LN2
    PARITY.check(fam, case, "loss_i", oc[:B][S], orc["loss_i"])
    PARITY.check(fam, case, "lse_pool", lse_nat[S2], orc2["lse"])
    g1, g2 = O.lp_symmetric_row_grads(z_all[S], zt_all[S], z_all, lse_nat[S], lse_nat, 2, tau, alpha, local_rows=B)
    PARITY.check(fam, case, "dz1", dz[:B].cpu().numpy()[S], g1)
    PARITY.check(fam, case, "dz2", dz[B:].cpu().numpy()[S], g2)


@pytest.mark.gpu
@pytest.mark.parametrize("B,B3,n", [(1500, 2100, 10), (64, 64, 4), (6144, 6144, 10), (1000, 333, 14)])
def test_forward_in_one_launch_equals_the_three_launch_form(B, B3, n, request):
    """clica_lp_loss_fwd as ONE launch (lp_finalize.h: the last workgroup of an owner tile finishes its rows, the last finisher of the launch
    the three means) == sweep + fwd_finalize_k + means_k (clica_set_tuning("lp_fused_finalize", 0)), bit for bit: loss_i, pos_i, lse_i and
    the means, for the specialised exponents, both `pow` forms, logsumexp and logmeanexp, ragged tiles, a pool smaller / larger than the
    batch; called repeatedly on ONE zero-filled workspace shared with the backward call in between (the arrival counters live in the
    workspace's header: every launch must leave them zero and the backward must keep clear of them)."""
    import ctypes as C
    from cl_ica_amd import _lib
    lib = _lib.load()
    request.addfinalizer(lambda: _lib.check(lib.clica_set_tuning(b"lp_fused_finalize", 1), "clica_set_tuning"))
    torch.manual_seed(3)
    z1 = torch.randn(B, n, device="cuda") * 0.6; z2 = z1 + 0.05 * torch.randn_like(z1); z3 = torch.randn(B3, n, device="cuda") * 0.6
    for p, pw, compat in ((1, 1, 1), (2, 1, 1), (3, 1, 0), (2, 0, 1), (1, 0, 0)):
        d = _lib.LpLossDesc(B=B, B3=B3, n=n, p=float(p), tau=0.9, alpha=0.4, compat=compat, pow=pw)
        fb, bb = C.c_size_t(), C.c_size_t()
        _lib.check(lib.clica_lp_loss_workspace_bytes(C.byref(d), C.byref(fb), C.byref(bb)), "ws")
        ws = torch.zeros(max(fb.value, bb.value), dtype=torch.uint8, device="cuda")
        dz = [torch.empty(B, n, device="cuda"), torch.empty(B, n, device="cuda"), torch.empty(B3, n, device="cuda")]
        outs = {}
        for fused in (1, 0, 1):
            _lib.check(lib.clica_set_tuning(b"lp_fused_finalize", fused), "clica_set_tuning")
            for rep in range(3):
                o = torch.full((3 * B + 3,), float("nan"), device="cuda")
                _lib.check(lib.clica_lp_loss_fwd(C.byref(d), z1.data_ptr(), n, z2.data_ptr(), n, z3.data_ptr(), n, o[:B].data_ptr(),
                                                 o[B:2 * B].data_ptr(), o[2 * B:3 * B].data_ptr(), o[3 * B:].data_ptr(), None, n,
                                                 ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "fwd")
                _lib.check(lib.clica_lp_loss_bwd(C.byref(d), z1.data_ptr(), n, z2.data_ptr(), n, z3.data_ptr(), n, o[2 * B:3 * B].data_ptr(),
                                                 None, n, None, None, None, None, dz[0].data_ptr(), n, dz[1].data_ptr(), n, dz[2].data_ptr(), n, 0,
                                                 ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "bwd")
                torch.cuda.synchronize()
                assert torch.isfinite(o).all(), (p, pw, compat, fused, rep)
                outs.setdefault(fused, []).append((o.clone(), dz[0].clone()))
        ref_o, ref_dz = outs[0][0]
        for fused, runs in outs.items():
            for o, g in runs:
                assert torch.equal(o, ref_o) and torch.equal(g, ref_dz), (p, pw, compat, fused, float((o - ref_o).abs().max()))
        assert int(ws[64:4096].view(torch.int32).abs().max()) == 0, "the arrival counters must be zero between launches"
