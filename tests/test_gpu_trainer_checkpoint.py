"""Checkpoint and resume of the fused trainers on the GPU: K = 3 steps, state_dict(), torch.save / torch.load(weights_only=True), a NEW
trainer, load_state_dict(), 3 more steps -- against 6 uninterrupted steps, bit for bit (parameters, both moments, the step / RNG counter,
every step's result, the last batch), on every path of the engine: the three encoder arithmetics eager and captured, the heads and
objectives, the per-layer path, the matrix-core loss sweeps (whose workspace carries a grid and a guard from call to call), the one-rank
collectives form, the driver.  Every case first holds two uninterrupted runs against each other (the precondition: the step is
deterministic) and asserts the path it names through plan_summary() / arith_state().  The portable domain (another arithmetic on the
loading side) restores parameters, moments and counter exactly and continues within the arithmetics' tolerance."""
import os
import shutil

import pytest
import torch

from conftest import PARITY

pytestmark = pytest.mark.gpu

K = 3
ARITH = {"f16": dict(split_arith="f16"), "bf16": dict(split_arith="bf16"), "native": dict(split_bf16=False)}
ARITH_NAME = {"f16": "f16x2", "bf16": "bf16x3", "native": "native_fp32"}
WHOLE = dict(n=10, hidden=(100, 500, 500, 100), B=1024)          # tests/test_gpu_engine.py: _guard_trainer
SMALL = dict(n=4, hidden=(40, 200, 40), B=256)


def _make(n, hidden, B, p=2, head=None, supervised=False, init_seed=7, lr=1e-3, **kw):
    """A trainer of the given configuration.  `init_seed` only decides the encoder's initial weights (a resumed trainer is built on
    OTHER ones: everything it continues from must come out of the checkpoint); mixing weights and sampler seed are the run's."""
    from cl_ica_amd import encoders
    from cl_ica_amd.engine import ContrastiveTrainer, SamplerSpec, SupervisedTrainer
    torch.manual_seed(init_seed)
    f = encoders.get_mlp(n, n, list(hidden), output_normalization=head).to("cuda")
    gW = (torch.randn(3, n, n, generator=torch.Generator().manual_seed(11)) / n ** 0.5).to("cuda").contiguous()
    space = "sphere" if p == 0 else "box"
    spec = SamplerSpec(space=space, n=n, seed=3, conditional="vmf" if p == 0 else "normal", c_param=10.0 if p == 0 else 0.05)
    if supervised:
        return SupervisedTrainer(f, gW, spec, batch_size=B, lr=lr, device="cuda", **kw)
    return ContrastiveTrainer(f, gW, spec, batch_size=B, p=p, lr=lr, device="cuda", **kw)


def _steps(tr, k):
    return [tr.step().clone() for _ in range(k)]


def _final(tr):
    torch.cuda.synchronize()
    return [t.clone() for t in (tr.param_arena, tr.exp_avg, tr.exp_avg_sq, tr.step_dev, tr.z)]


def _same(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"{what}: item {i} differs (max |d| = {float((x.float() - y.float()).abs().max()):.3e})"


def _through_a_file(sd, tmp_path):
    path = os.path.join(str(tmp_path), "trainer.pth")
    torch.save(sd, path)
    return torch.load(path, map_location="cpu", weights_only=True)


def _resume_equals_uninterrupted(make, tmp_path, mode, expect, between=None):
    """The core check.  `mode`: "eager"; "captured" (the loading trainer is captured first, then loads: the graph must stay);
    "load_then_capture" (saved from a captured trainer, loaded into a fresh one, captured afterwards).  `expect(tr)` asserts the path.
    Returns (saving trainer, its state at the checkpoint as a loaded dict, loading trainer)."""
    cap = mode != "eager"
    a = make()
    expect(a)
    if cap:
        a.capture()
    outs_a = _steps(a, K)
    sd = a.state_dict()                                  # between steps: must not disturb the run it is taken from
    extra = between(a) if between is not None else None
    outs_a += _steps(a, K)
    fin_a = _final(a)
    assert a.steps_done == 2 * K and sd["step"] == K
    b = make()                                           # the precondition: two uninterrupted runs agree bit for bit
    if cap:
        b.capture()
    outs_b = _steps(b, 2 * K)
    _same(outs_a, outs_b, "precondition: step results of two uninterrupted runs")
    _same(fin_a, _final(b), "precondition: final state of two uninterrupted runs")
    del b
    sd = _through_a_file(sd, tmp_path)
    c = make(init_seed=8)
    expect(c)
    if mode == "captured":
        c.capture()
    graph = c.graph
    ptrs = [t.data_ptr() for t in (c.param_arena, c.exp_avg, c.exp_avg_sq, c.step_dev, c.loss_ws)]
    assert c.load_state_dict(sd) == "exact"
    assert ptrs == [t.data_ptr() for t in (c.param_arena, c.exp_avg, c.exp_avg_sq, c.step_dev, c.loss_ws)] and c.graph is graph
    assert c.steps_done == K
    if mode == "load_then_capture":
        c.capture()
    outs_c = _steps(c, K)
    _same(outs_a[K:], outs_c, "step results after the resume")
    _same(fin_a, _final(c), "final state after the resume")
    assert c.plan_summary()["graph_captured"] == cap
    if extra is not None:
        extra(c, sd)
    return a, sd, c


def _expect(path, arith, cls=None):
    def check(tr):
        ps = tr.plan_summary()
        assert ps["encoder_path"] == path, ps
        assert tr.arith_state()["arith"].startswith(ARITH_NAME[arith]), tr.arith_state()
        assert (tr.s16 is not None) == (arith == "f16")
        if cls is not None:
            assert type(tr).__name__ == cls
    return check


@pytest.mark.parametrize("mode", ["eager", "captured"])
@pytest.mark.parametrize("arith", ["f16", "bf16", "native"])
def test_whole_stack_resume_is_bit_identical(arith, mode, tmp_path):
    def between(a):
        g = a.check_arith() if arith == "f16" else None

        def after(c, sd):
            assert (sd["arith"]["split16"] is not None) == (arith == "f16") and sd["arith"]["arith"] == ARITH_NAME[arith]
            if arith == "f16":
                gc = c.check_arith()
                # the guard's counters round-trip as numbers (0 withheld steps here), and a load is not a "new" withheld step
                assert (gc["skipped"], gc["new_skipped"], gc["flags"]) == (g["skipped"], 0, g["flags"]) == (0, 0, 0), (g, gc)
                assert gc["updates"] == g["updates"] + K
        return after
    _resume_equals_uninterrupted(lambda **kw: _make(**WHOLE, **ARITH[arith], **kw), tmp_path, mode, _expect("whole-stack", arith), between)


def test_load_into_a_captured_trainer_that_has_stepped_past_the_checkpoint(tmp_path):
    tr = _make(**WHOLE, split_arith="f16")
    _expect("whole-stack", "f16")(tr)
    tr.capture()
    graph = tr.graph
    _steps(tr, K)
    sd = _through_a_file(tr.state_dict(), tmp_path)
    outs = _steps(tr, K)
    fin = _final(tr)
    _steps(tr, 2)                                        # ... and past it
    ptrs = [t.data_ptr() for t in (tr.param_arena, tr.exp_avg, tr.exp_avg_sq, tr.step_dev, tr.loss_ws, tr.s16.buf)]
    assert tr.load_state_dict(sd) == "exact"
    assert tr.graph is graph and tr.steps_done == K
    assert ptrs == [t.data_ptr() for t in (tr.param_arena, tr.exp_avg, tr.exp_avg_sq, tr.step_dev, tr.loss_ws, tr.s16.buf)]
    _same(outs, _steps(tr, K), "step results after going back to the checkpoint")
    _same(fin, _final(tr), "final state after going back to the checkpoint")
    assert tr.graph is graph


def test_save_from_captured_load_into_fresh_then_capture(tmp_path):
    _resume_equals_uninterrupted(lambda **kw: _make(**WHOLE, split_arith="f16", **kw), tmp_path, "load_then_capture", _expect("whole-stack", "f16"))


@pytest.mark.parametrize("case", ["p1", "p0_fixed_sphere", "p2_learnable_box", "supervised"])
def test_heads_and_objectives_resume_is_bit_identical(case, tmp_path):
    cfg = {"p1": dict(p=1), "p0_fixed_sphere": dict(p=0, head="fixed_sphere"), "p2_learnable_box": dict(p=2, head="learnable_box"),
           "supervised": dict(supervised=True)}[case]

    def expect(tr):
        _expect("whole-stack", "f16", "SupervisedTrainer" if case == "supervised" else "ContrastiveTrainer")(tr)
        if case == "p0_fixed_sphere":
            assert tr.dot and tr.plan_summary()["loss_entry_points"] == "dot train pair" and tr.head is not None
        if case == "p1":
            assert tr.plan_summary()["loss_entry_points"] == "train pair" and tr.p == 1.0
        if case == "p2_learnable_box":      # the head's parameter rides in the arena: saved and restored with it
            assert tr.head_learnable and len(list(tr.f.parameters())) == 2 * len(tr.linears) + 1
        if case == "supervised":
            assert tr.plan_summary()["objective"] == "mse"
    a, sd, c = _resume_equals_uninterrupted(lambda **kw: _make(**SMALL, **cfg, **kw), tmp_path, "captured", expect)
    assert sd["kind"] == ("supervised" if case == "supervised" else "contrastive")
    if case == "p2_learnable_box":
        assert len(sd["optimizer"]["state"]) == 2 * len(a.linears) + 1


def test_per_layer_path_resume_is_bit_identical(tmp_path):
    def expect(tr):
        _expect("per-layer", "f16")(tr)
        assert tr.split_f16_wide and 2 in tr.chain, tr.chain      # the 640 x 640 layer runs on the split chain kernels
    _resume_equals_uninterrupted(lambda **kw: _make(n=4, hidden=(40, 640, 640, 40), B=256, split_arith="f16", **kw), tmp_path, "eager", expect)


def test_matrix_core_loss_state_resumes(tmp_path):
    """The p = 2 matrix-core sweeps build a call's planes on the grid the PREVIOUS call measured and keep a guard in their workspace: a
    trainer that resumed without that state would send its first call to the difference sweeps (as every first call on a fresh
    workspace) and continue on other bits."""
    from cl_ica_amd import _lib
    _lib.check(_lib.load().clica_lp_loss_set_matrix_cores(2), "matrix cores for every pool")
    try:
        def expect(tr):
            _expect("whole-stack", "f16")(tr)
            assert tr.loss_guard()["limit"] > 0

        def between(a):
            g = a.loss_guard()
            assert g["fallback_steps"] >= 1 and 0 < g["last_spread"] <= g["limit"], g      # the first call fell back, the run is on the matrix cores

            def after(c, sd):
                assert sd["arith"]["loss"] is not None and bool(sd["arith"]["loss"].any())
                gc, ga = c.loss_guard(), a.loss_guard()
                assert gc == ga and gc["fallback_steps"] >= g["fallback_steps"], (g, ga, gc)      # the counters went on from the saved ones
            return after
        for mode in ("eager", "captured"):
            _resume_equals_uninterrupted(lambda **kw: _make(**WHOLE, split_arith="f16", **kw), tmp_path, mode, expect, between)
    finally:
        _lib.check(_lib.load().clica_lp_loss_set_matrix_cores(-1), "default policy")


def test_guard_state_right_after_the_load_equals_the_saved_one(tmp_path):
    """loss_guard() / check_arith() of a fresh trainer right after the load are the saving trainer's at the checkpoint (matrix-core
    loss sweeps on: both blobs carry something)."""
    from cl_ica_amd import _lib
    _lib.check(_lib.load().clica_lp_loss_set_matrix_cores(2), "matrix cores for every pool")
    try:
        a = _make(**WHOLE, split_arith="f16")
        _steps(a, K)
        lg, ag, st = a.loss_guard(), a.check_arith(), a.arith_state()
        sd = _through_a_file(a.state_dict(), tmp_path)
        c = _make(**WHOLE, split_arith="f16", init_seed=8)
        assert c.loss_guard()["fallback_steps"] == 0
        assert c.load_state_dict(sd) == "exact"
        assert c.loss_guard() == lg and lg["fallback_steps"] >= 1
        gc = c.check_arith()
        assert {k: gc[k] for k in ("flags", "skipped", "updates", "poisoned")} == {k: ag[k] for k in ("flags", "skipped", "updates", "poisoned")}
        assert c.arith_state() == st and c._s16_calibrated
    finally:
        _lib.check(_lib.load().clica_lp_loss_set_matrix_cores(-1), "default policy")


def test_one_rank_collectives_form_resumes(tmp_path):
    """A one-rank process group with the collectives forced on (the data-parallel code path on one GPU): here the importing state holds
    a verdict slot of its own (dp_poison != NULL), which must stay this trainer's.  More than one rank cannot be run on one GPU."""
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29517")
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        def expect(tr):
            _expect("whole-stack", "f16")(tr)
            assert tr.dp and tr.buckets is not None and tr.plan_summary()["collectives_per_step"]
            assert tr.s16._dp_slot.data_ptr() == tr._guard_slot.data_ptr()
        mk = lambda **kw: _make(n=10, hidden=(100, 500, 100), B=1024, split_arith="f16", process_group=dist.group.WORLD, force_collectives=True, **kw)
        a, sd, c = _resume_equals_uninterrupted(mk, tmp_path, "eager", expect)
        assert a._guard_slot.data_ptr() != c._guard_slot.data_ptr()
        g = c.check_arith()
        assert g["skipped"] == 0 and g["flags"] == 0 and not g["poisoned"], g
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("src,dst", [("f16", "bf16"), ("bf16", "f16")])
def test_portable_domain(src, dst, tmp_path):
    """Another arithmetic on the loading side: parameters, moments and counter exactly, the blobs ignored, scales calibrated anew (with
    the counter put back: the next step draws the saved run's next batch and advances the counter by exactly one).  Each arithmetic
    holds the project's 1e-5 against fp64, so the two next-step losses on the same batch agree within twice that."""
    a = _make(**WHOLE, **ARITH[src])
    _steps(a, K)
    saved = _final(a)
    sd = _through_a_file(a.state_dict(), tmp_path)
    loss_a = a.step().clone()
    z_a = a.z.clone()
    for captured in (False, True):
        c = _make(**WHOLE, **ARITH[dst], init_seed=8)
        _expect("whole-stack", dst)(c)
        if captured:
            c.capture()
        assert c.load_state_dict(sd) == "portable"
        torch.cuda.synchronize()
        _same(saved[:4], [c.param_arena, c.exp_avg, c.exp_avg_sq, c.step_dev], "state right after a portable load")
        assert c.steps_done == K
        loss_c = c.step().clone()
        assert c.steps_done == K + 1
        assert torch.equal(c.z, z_a), "the batch after the resume is the saved run's next batch"
        st, g = c.arith_state(), c.check_arith()
        assert st["arith"] == ARITH_NAME[dst] and st.get("flags", 0) == 0 and g["flags"] == 0 and g["skipped"] == 0 and not g["poisoned"], (st, g)
        PARITY.check("trainer_checkpoint_portable", f"{src} -> {dst}, {'captured' if captured else 'eager'}", "loss of the step after the load",
                     loss_c[0].item(), loss_a[0].item(), tol=2e-5, note="two arithmetics, each within 1e-5 of fp64, on the same batch")


def test_skipped_count_round_trips_where_it_is_not_zero(tmp_path):
    """The guard's count of withheld steps where it is 1: raised as tests/test_gpu_engine.py raises it (the mixing net's last layer x 1000
    under the captured graph), saved, and read back from a fresh trainer as a number -- not as a new event."""
    a = _make(**WHOLE, split_arith="f16")
    a._watch_versions = False
    a.capture()
    _steps(a, K)
    a.gW[-1].mul_(1000.0)
    a.step(); torch.cuda.synchronize()
    ga = a.check_arith()
    assert ga["skipped"] == 1 and a.steps_done == K, ga
    sd = _through_a_file(a.state_dict(), tmp_path)
    c = _make(**WHOLE, split_arith="f16", init_seed=8)
    with pytest.raises(ValueError, match="`g_weights`"):
        c.load_state_dict(sd)
    c.gW.copy_(a.gW)
    assert c.load_state_dict(sd) == "exact"
    gc = c.check_arith()
    assert gc["skipped"] == 1 and gc["new_skipped"] == 0 and gc["flags"] == ga["flags"] and gc["poisoned"] == ga["poisoned"], (ga, gc)
    assert c.steps_done == K


def test_driver_resume_reproduces_the_straight_run(tmp_path, monkeypatch):
    """train_mlp: 12 steps straight with --checkpoint-every 6, against --resume-from the file written behind step 6."""
    from cl_ica_amd import train_mlp
    base = ["--n", "4", "--batch-size", "256", "--n-steps", "12", "--more-unsupervised", "1", "--n-log-steps", "6", "--seed", "1",
            "--only-unsupervised", "--num-eval-batches", "1"]
    d1, d2 = os.path.join(str(tmp_path), "straight"), os.path.join(str(tmp_path), "resumed")
    write = train_mlp.write_checkpoint

    def keep_each(path, payload):       # the driver overwrites one file per phase: keep what it wrote behind every checkpointed step
        write(path, payload)
        shutil.copy(path, "%s.step%d" % (path, payload["driver"]["global_step"] - 1))
    monkeypatch.setattr(train_mlp, "write_checkpoint", keep_each)
    r1 = train_mlp.main(base + ["--checkpoint-every", "6", "--save-dir", d1])
    monkeypatch.setattr(train_mlp, "write_checkpoint", write)
    assert sorted(os.listdir(d1)) == ["g.pth", "unsup_f.pth", "unsup_trainer.pth", "unsup_trainer.pth.step12", "unsup_trainer.pth.step6"]
    mid = torch.load(os.path.join(d1, "unsup_trainer.pth.step6"), map_location="cpu", weights_only=True)
    end = torch.load(os.path.join(d1, "unsup_trainer.pth"), map_location="cpu", weights_only=True)
    assert (mid["step"], mid["driver"]["global_step"], mid["driver"]["phase"], mid["driver"]["phase_done"], len(mid["driver"]["losses"])) == (6, 7, "unsup", False, 6)
    assert (end["step"], end["driver"]["phase_done"], end["driver"]["losses"]) == (12, True, r1["losses"])
    f1 = torch.load(os.path.join(d1, "unsup_f.pth"), map_location="cpu")
    assert list(end["f"]) == list(f1) and all(torch.equal(end["f"][k], f1[k]) for k in f1)      # unsup_f.pth is a sub-dict of the checkpoint
    r2 = train_mlp.main(base + ["--resume-from", os.path.join(d1, "unsup_trainer.pth.step6"), "--save-dir", d2])
    assert len(r1["losses"]) == 12 and r2["losses"] == r1["losses"]
    f2 = torch.load(os.path.join(d2, "unsup_f.pth"), map_location="cpu")
    assert list(f1) == list(f2) and all(torch.equal(f1[k], f2[k]) for k in f1)
    assert (r1["linear"], r1["perm"]) == (r2["linear"], r2["perm"])      # the evaluation sampler's counter was carried over too
    with pytest.raises(SystemExit):
        train_mlp.main(base[:-5] + ["--seed", "2", "--only-unsupervised", "--num-eval-batches", "1", "--resume-from", os.path.join(d1, "unsup_trainer.pth")])
