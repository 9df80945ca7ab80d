"""The step pieces called one by one OUTSIDE a step -- sample, pack, forward, loss_forward_backward, backward_chain, weight_grads,
optimizer_step, as bench.py's roofline leg calls them -- against step() on an identically seeded trainer.  Outside a step nothing is
folded: the loss's reduction launch runs, the chain has no tail, Adam is its own launch; step() folds what its plan allows."""
import pytest
import torch

from conftest import PARITY
from test_gpu_configs import ADAM_MASK_THETA

pytestmark = pytest.mark.gpu

N, B, STEPS, LR = 10, 200, 3, 1e-4        # 400 (200) encoder rows: 48-row panels and 64-row loss tiles, each with a ragged last one


def _build(cls, **kw):
    from cl_ica_amd import encoders
    from cl_ica_amd.engine import SamplerSpec
    torch.manual_seed(0)
    f = encoders.get_mlp(N, N, [100, 500, 500, 100])
    gW = torch.randn(3, N, N) / N ** 0.5
    tr = cls(f, gW, SamplerSpec(space="box", n=N, seed=5), batch_size=B, lr=LR, device="cuda", **kw)
    tr.calibrate_scales()       # (f16x2: step() would do it by itself, the bare pieces would not)
    return tr


def _pieces_vs_step(cls, result, arith, zero_grad_bias=False, **kw):
    """STEPS steps in both forms; PARITY-checks means, moments and parameters and asserts the counter.  Parameters by the suite's rule for
    Adam trajectories (test_gpu_configs.adam_trajectory_check): Adam divides by sqrt(v), so an element whose gradient lies within the two
    forms' summation-order difference moves by up to lr per step either way and says nothing; elements whose |gradient| stayed above
    ADAM_MASK_THETA of their tensor's largest at every step are held to the plain 1e-5 of max |param|, the rest to 2 lr STEPS.
    `zero_grad_bias` (as adam_trajectory_check's `skip`): the Lp loss sees differences of embeddings only, so the last layer's bias has
    an exactly-zero true gradient and every element of it walks by +-lr per step in both forms.
    The forms are NOT bit-identical in the split arithmetics (the chain's tail sums the n-wide layers' gradients over 48-row partials, the
    tiny-dimension launch in another order); measured on the commit that added this test, before and after the engine's refactoring
    alike: contrastive f16x2 -- means 3.4e-13, exp_avg 4.9e-7, exp_avg_sq 6.8e-7 of their largest, strict parameters <= 7.5e-9 absolute
    (7.4e-8 of max |param|), the last bias 1.0e-5 absolute = 0.1 lr; supervised f16x2 -- means 8.7e-8, exp_avg 2.4e-7, exp_avg_sq 4.6e-7,
    strict parameters <= 7.5e-9 absolute; native fp32 -- bit-identical in both trainers, which is asserted."""
    fam, case = "engine_pieces_vs_step", f"{cls.__name__} B={B}"
    whole, parts = _build(cls, **kw), _build(cls, **kw)
    means, gmin, gmax = [[], []], {}, {}
    for _ in range(STEPS):
        means[0].append(result(whole.step()).clone())
        for name, prm in whole.f.named_parameters():
            a = whole._gviews[id(prm)].abs()
            gmin[name] = a.clone() if name not in gmin else torch.minimum(gmin[name], a)
            gmax[name] = max(gmax.get(name, 0.0), float(a.max()))
        parts._packed_current = False
        parts.sample(); parts.pack(); parts.forward(); parts.loss_forward_backward()
        g = parts.dy
        parts.backward_chain(g); parts.weight_grads(g); parts.optimizer_step()
        means[1].append(result(parts.loss_out).clone())
    torch.cuda.synchronize()
    assert whole.steps_done == parts.steps_done == STEPS and torch.equal(whole.step_dev, parts.step_dev)
    got = dict(means=torch.stack(means[1]), exp_avg=parts.exp_avg, exp_avg_sq=parts.exp_avg_sq, param_arena=parts.param_arena)
    ref = dict(means=torch.stack(means[0]), exp_avg=whole.exp_avg, exp_avg_sq=whole.exp_avg_sq, param_arena=whole.param_arena)
    for k in got:
        print(f"pieces vs step [{case} {arith}] {k}: max |diff| {float((got[k] - ref[k]).abs().max()):.3e} "
              f"of max |ref| {float(ref[k].abs().max()):.3e}, equal {torch.equal(got[k], ref[k])}")
    if arith == "native_fp32":      # nothing folds in either form: the same launches
        assert all(torch.equal(got[k], ref[k]) for k in got)
    for k in ("means", "exp_avg", "exp_avg_sq"):
        PARITY.check(fam, case, k, got[k].cpu().numpy(), ref[k].cpu().numpy())
    for (name, pw), pp in zip(whole.f.named_parameters(), parts.f.parameters()):
        w, q = pw.detach(), pp.detach()
        strict = gmin[name] > ADAM_MASK_THETA * gmax[name]
        if zero_grad_bias and name == f"{2 * (len(whole.linears) - 1)}.bias":
            strict = torch.zeros_like(strict)
        worst = float((q - w).abs().max())
        print(f"    {name}: {int(strict.sum())}/{strict.numel()} strict, max |diff| strict "
              f"{float((q - w)[strict].abs().max()) if strict.any() else 0.0:.3e} / all {worst:.3e}, max |param| {float(w.abs().max()):.3e}")
        if strict.any():
            PARITY.check(fam, case, f"param {name} [|grad| > {100 * ADAM_MASK_THETA:g} % of max at every step]",
                         q[strict].cpu().numpy(), w[strict].cpu().numpy(), floor=float(w.abs().max()))
        assert worst <= 2 * STEPS * LR * 1.01, (name, worst)


def test_contrastive_pieces_outside_a_step_equal_the_step(encoder_arith):
    from cl_ica_amd.engine import ContrastiveTrainer
    _pieces_vs_step(ContrastiveTrainer, lambda o: o[-3:], encoder_arith, zero_grad_bias=True, p=2)


def test_supervised_pieces_outside_a_step_equal_the_step(encoder_arith):
    """(`z2` unused: the supervised step runs on the B rows of z1)"""
    from cl_ica_amd.engine import SupervisedTrainer
    _pieces_vs_step(SupervisedTrainer, lambda o: o, encoder_arith)
