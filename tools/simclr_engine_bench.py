#!/usr/bin/env python3
"""Steps/s of the p = 0 contrastive phase (SimCLRLoss(normalize=False), the reference's hypersphere experiment) at the driver's shapes:
`train_mlp --p 0 --space-type sphere` builds a fixed_sphere head and unit-sphere latents.  The captured ContrastiveTrainer(p=0) in each
encoder arithmetic (native fp32, bf16x3, f16x2), f16x2 once more with the vMF conditional (--c-p 0), against today's autograd path
(train_mlp.autograd_train_step over the drop-in modules + the flat-arena Adam, latents sampled every step as the driver does).  One
process; the legs alternate window by window (5 windows after warm-up, median reported); the shader clock over each leg's windows comes
from the one-wave probe bench.py uses (clica_clock_probe).  Prints one JSON line.

    python tools/simclr_engine_bench.py [--batch-size 6144 --n 10 --steps 200 --windows 5]
    python tools/simclr_engine_bench.py --leg f16x2 --steps 50          # one leg only (a kernel-trace run: rocprofv3 --kernel-trace --stats -- ...)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cl_ica_amd import encoders, invertible_network_utils, losses, ops, train_mlp  # noqa: E402
from cl_ica_amd.engine import ContrastiveTrainer  # noqa: E402
from cl_ica_amd.optim import Adam as FlatAdam  # noqa: E402

LEGS = ("native_fp32", "bf16x3", "f16x2", "f16x2_vmf", "autograd")


def make_leg(name, args, g):
    n = args.n
    flags = ["--n", str(n), "--batch-size", str(args.batch_size), "--p", "0", "--space-type", "sphere", "--tau", str(args.tau)]
    if name == "f16x2_vmf":
        flags += ["--c-p", "0"]
    targs = train_mlp.parse_args(flags)
    spec = train_mlp.sampler_spec(targs, 0)
    torch.manual_seed(1)
    f = encoders.get_mlp(n_in=n, n_out=n, layers=[n * 10, n * 50, n * 50, n * 50, n * 50, n * 10], output_normalization="fixed_sphere").cuda()
    if name == "autograd":
        latent_space = train_mlp.build_latent_space(targs, spec)
        loss = losses.SimCLRLoss(normalize=False, tau=args.tau)
        opt = FlatAdam(f.parameters(), lr=args.lr)
        h = lambda z: f(g(z))   # noqa: E731

        def step():
            z1 = latent_space.sample_marginal(size=args.batch_size)
            z2 = latent_space.sample_conditional(z1, size=args.batch_size)
            return train_mlp.autograd_train_step(h, loss, opt, z1, z2, False)
        return step, None
    kw = dict(native_fp32=dict(split_bf16=False), bf16x3=dict(split_bf16=True, split_arith="bf16"),
              f16x2=dict(split_bf16=True, split_arith="f16"), f16x2_vmf=dict(split_bf16=True, split_arith="f16"))[name]
    tr = ContrastiveTrainer(f, g.weight_stack(), spec, batch_size=args.batch_size, p=0, tau=args.tau, lr=args.lr, g_slope=g.slope,
                            g_act_kind=g.act_kind, device="cuda", **kw)
    tr.capture()
    return tr.step, tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=6144)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--tau", type=float, default=1.0)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--steps", type=int, default=200, help="steps per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--leg", choices=LEGS, default=None, help="run this leg only, no clock probe (kernel-trace runs)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "simclr_engine_bench.py needs the MI355X"
    np.random.seed(0)
    g = invertible_network_utils.construct_invertible_mlp(n=args.n, n_layers=3, act_fct="leaky_relu", cond_thresh_ratio=0.0,
                                                          n_iter_cond_thresh=25000).cuda()
    names = (args.leg,) if args.leg else LEGS
    legs = {nm: make_leg(nm, args, g) for nm in names}
    for nm in names:
        for _ in range(args.warmup):
            legs[nm][0]()
    torch.cuda.synchronize()
    probe = None
    if not args.leg:
        probe_stream = torch.cuda.Stream()
        probe = ops.clock_probe(100000, 100.0, probe_stream)          # 10 s of samples, 100 us apart
    slots = {nm: torch.zeros(1 + 2 * args.windows, dtype=torch.int64, device="cuda") for nm in names}
    times = {nm: [] for nm in names}
    last = {}
    for _ in range(args.windows):
        for nm in names:
            step = legs[nm][0]
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ops.stamp(slots[nm], 0)
            s.record()
            for _ in range(args.steps):
                out = step()
            e.record()
            ops.stamp(slots[nm], 1)
            e.synchronize()
            times[nm].append(s.elapsed_time(e) / 1e3 / args.steps)
            last[nm] = out
    torch.cuda.synchronize()
    res = dict(metric="simclr_p0_steps_per_s", batch_size=args.batch_size, n=args.n, tau=args.tau, head="fixed_sphere", space="sphere",
               steps_per_window=args.steps, windows=args.windows,
               timing="median of the windows' time per step, legs alternating window by window in one process")
    smp = probe.cpu().numpy() if probe is not None else None
    for nm in names:
        med = float(np.median(times[nm]))
        r = dict(steps_per_s=round(1.0 / med, 1), us_per_step=round(med * 1e6, 2), loss=float(last[nm].reshape(-1)[0]))
        if smp is not None:
            ghz = [ops.clock_between(smp, b0, b1) for b0, b1 in ops.stamp_brackets(slots[nm])]
            ghz = [v for v in ghz if v is not None]
            r["shader_clock_ghz"] = round(float(np.median(ghz)), 3) if ghz else None
        tr = legs[nm][1]
        if tr is not None:
            ga = tr.check_arith()
            r.update(arith=tr.arith_state()["arith"], loss_entry_points=tr.plan_summary()["loss_entry_points"], steps_withheld=ga["skipped"])
        res[nm] = r
    if "autograd" in res and "f16x2" in res:
        res["speedup_f16x2_vs_autograd"] = round(res["f16x2"]["steps_per_s"] / res["autograd"]["steps_per_s"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
