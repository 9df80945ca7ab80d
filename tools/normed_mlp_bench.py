#!/usr/bin/env python3
"""Time per training forward + backward (through autograd) of get_mlp(10, 10, [100, 500, 500, 500, 500, 100], layer_normalization=mode)
at B = 6144 for mode = "bn" and "gn": the fused norm + LeakyReLU kernels (encoders.NORM_MODE = "hip", csrc/norm.hip) against torch's
own normalisation modules with the stand-alone activation kernel behind them (NORM_MODE = "torch").  One process; the legs alternate
window by window (5 windows of 200 iterations after warm-up, median reported, and the spread max - min of every leg's windows); the
shader clock over each leg's windows comes from the one-wave probe bench.py uses (clica_clock_probe).  Prints one JSON line.

    python tools/normed_mlp_bench.py [--batch-size 6144 --steps 200 --windows 5]
    python tools/normed_mlp_bench.py --leg bn:hip --steps 50        # one leg only (a kernel-trace run: rocprofv3 --kernel-trace --stats -- ...)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cl_ica_amd import encoders, ops  # noqa: E402

LEGS = ("bn:hip", "bn:torch", "gn:hip", "gn:torch")


def make_leg(name, args):
    mode, norm_mode = name.split(":")
    torch.manual_seed(1)
    n = args.n
    f = encoders.get_mlp(n_in=n, n_out=n, layers=[n * 10, n * 50, n * 50, n * 50, n * 50, n * 10], layer_normalization=mode).cuda().train()
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(args.batch_size, n, generator=gen).cuda()
    gy = torch.randn(args.batch_size, n, generator=gen).cuda()

    def step():
        encoders.NORM_MODE = norm_mode
        for p in f.parameters():
            p.grad = None
        y = f(x)
        y.backward(gy)
        return y
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=6144)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--steps", type=int, default=200, help="iterations per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--leg", choices=LEGS, default=None, help="run this leg only, no clock probe (kernel-trace runs)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "normed_mlp_bench.py needs the MI355X"
    names = (args.leg,) if args.leg else LEGS
    legs = {nm: make_leg(nm, args) for nm in names}
    for nm in names:
        for _ in range(args.warmup):
            legs[nm]()
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
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ops.stamp(slots[nm], 0)
            s.record()
            for _ in range(args.steps):
                out = legs[nm]()
            e.record()
            ops.stamp(slots[nm], 1)
            e.synchronize()
            times[nm].append(s.elapsed_time(e) / 1e3 / args.steps)
            last[nm] = out
    torch.cuda.synchronize()
    res = dict(metric="normed_mlp_fwd_bwd_us", batch_size=args.batch_size, n=args.n, steps_per_window=args.steps, windows=args.windows,
               timing="median of the windows' time per iteration, legs alternating window by window in one process; spread = max - min "
                      "of a leg's windows")
    smp = probe.cpu().numpy() if probe is not None else None
    for nm in names:
        t = np.asarray(times[nm]) * 1e6
        r = dict(us_per_iter=round(float(np.median(t)), 2), windows_us=[round(float(v), 2) for v in t],
                 spread_us=round(float(t.max() - t.min()), 2), y_abs_mean=float(last[nm].detach().abs().mean()))
        if smp is not None:
            ghz = [ops.clock_between(smp, b0, b1) for b0, b1 in ops.stamp_brackets(slots[nm])]
            ghz = [v for v in ghz if v is not None]
            r["shader_clock_ghz"] = round(float(np.median(ghz)), 3) if ghz else None
        res[nm] = r
    for mode in ("bn", "gn"):
        if f"{mode}:hip" in res and f"{mode}:torch" in res:
            d = res[f"{mode}:hip"]["us_per_iter"] - res[f"{mode}:torch"]["us_per_iter"]
            res[f"{mode}_hip_minus_torch_us"] = round(d, 2)
            res[f"{mode}_within_torch_spread"] = bool(d <= res[f"{mode}:torch"]["spread_us"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
