#!/usr/bin/env python3
"""Memory-format A/B of bench.py's c4 step (3DIdent train_step, ResNet-18 on (1024, 3, 64, 64) x 2 views) in ONE process (GPU box):

    (a) nchw        contiguous model and inputs: bench.py's own leg, the baseline
    (b) nhwc-torch  channels_last model and inputs, CLICA_RESNET_NHWC=torch: torch's / MIOpen's own BatchNorm, ReLU, add
    (c) nhwc-hip    channels_last model and inputs, CLICA_RESNET_NHWC=hip: the units of csrc/bn2d_nhwc.hip
    (d) nhwc-hip-stem  as (c) with CLICA_RESNET_NHWC_STEM=hip: the stem's bn1 + relu + maxpool as the fused unit of csrc/bn2d_nhwc.hip
    (e) nhwc-torch-bf16     as (b) with the encoder passes under torch.autocast(bfloat16): what bf16 mixed precision was before BF16_MODE
    (f) nhwc-hip-stem-bf16  as (d) under the same autocast with CLICA_RESNET_BF16=hip: the bf16 instances of csrc/bn2d_nhwc.hip
    (g) <leg>-clocked       the leg's step as threedident.clocked_iteration: the batch is drawn under a device clock, snapped to a
                            synthetic grid of 4096 latents and gathered from a 4096 x 64 x 64 x 3 uint8 table in the model's format
                            inside every iteration (legs a - f step on two fixed tensors and draw nothing), launched from Python
    (h) <leg>-graph         the same iteration recorded once and replayed as ONE HIP graph (threedident.capture_iteration)

  python tools/c4_layout_ab.py                      a throw-away run of every leg (MIOpen's find step), then two rounds alternating the
                                                    legs; each figure the median of three 20-step windows after 6 warm-up steps
  python tools/c4_layout_ab.py --legs nchw,nhwc-hip,nhwc-hip-stem       the same with these legs only
  python tools/c4_layout_ab.py --leg nhwc-hip       one leg alone, 6 + 30 steps: the program for `rocprofv3 --kernel-trace --stats -- ...`
  python tools/c4_layout_ab.py --units              the fused unit alone per ResNet-18 (M, C) at N = 1024, NHWC against NCHW, event-timed
                                                    calls (forward = statistics + apply, backward = sums + backward apply) and TB/s;
                                                    then the stem with its max-pool, fused, in both layouts; then the channels-last
                                                    units, stem and average pool on bf16 activations (layout "nhwc-bf16")
  python tools/c4_layout_ab.py --summarise T.csv    buckets and per-(kernel, grid) rows of a rocprofv3 *_kernel_trace.csv (no GPU)
Every mode prints JSON lines; --out FILE also appends them there."""
import argparse
import csv
import json
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# leg -> (memory format, NHWC_MODE, NHWC_STEM_MODE)
LEGS = {"nchw": ("contiguous", "torch", "torch"), "nhwc-torch": ("channels_last", "torch", "torch"),
        "nhwc-hip": ("channels_last", "hip", "torch"), "nhwc-hip-stem": ("channels_last", "hip", "hip"),
        "nhwc-torch-bf16": ("channels_last", "torch", "torch"), "nhwc-hip-stem-bf16": ("channels_last", "hip", "hip")}
# leg -> (BF16_MODE, train_step's amp); every other leg: ("torch", None)
BF16_LEGS = {"nhwc-torch-bf16": ("torch", "bf16"), "nhwc-hip-stem-bf16": ("hip", "bf16")}
# the legs whose iteration draws its own batch: eager under the device clock, and the captured graph of that
BATCH_LEGS = {leg + sfx: (leg, sfx[1:]) for leg in ("nchw", "nhwc-hip-stem", "nhwc-hip-stem-bf16") for sfx in ("-clocked", "-graph")}
ALL_LEGS = list(LEGS) + list(BATCH_LEGS)
TABLE_IMAGES = 4096
# ResNet-18's units at N = 1024 on 64 x 64 images: (name, N, C, H, W, units with / without a residual per view)
UNIT_SHAPES = [("stem", 1024, 64, 32, 32), ("layer 1", 1024, 64, 16, 16), ("layer 2", 1024, 128, 8, 8), ("layer 3", 1024, 256, 4, 4),
               ("layer 4", 1024, 512, 2, 2)]


def emit(out, obj):
    line = json.dumps(obj)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def make_leg(leg):
    """bench.py's c4 step (conv_config_leg) with the model and the inputs in the leg's memory format."""
    import torch
    from cl_ica_amd import resnet, threedident as T
    from cl_ica_amd.optim import Adam
    leg, batches = BATCH_LEGS.get(leg, (leg, None))
    fmt_name, nhwc_mode, stem_mode = LEGS[leg]
    bf16_mode, amp = BF16_LEGS.get(leg, ("torch", None))
    fmt = getattr(torch, fmt_name + "_format" if fmt_name == "contiguous" else fmt_name)
    dev = torch.device("cuda")
    torch.manual_seed(0)
    a = types.SimpleNamespace(position_only=True, rotation_and_color_only=False, rotation_only=False, color_only=False,
                              non_periodic_rotation_and_color=False, box_constraint="fix", sphere_constraint=None,
                              unsupervised_loss="l2", identity_solution=False, encoder="rn18")
    f = T.setup_f(a, 3, 0).to(dev).to(memory_format=fmt)
    f.train()
    if amp is not None and bf16_mode == "torch":
        # torch's modules hand the head bf16 logits, which the HIP head (fp32 only) refuses: this leg widens them behind the backbone
        f[0].register_forward_hook(lambda mod, inp, out: out.float())
    loss = T.make_unsupervised_loss(a, 3)
    opt = Adam(f.parameters(), lr=1e-4)
    if batches is not None:
        return make_batch_leg(batches, f, loss, opt, amp, (nhwc_mode, stem_mode, bf16_mode))
    x1 = torch.randn(1024, 3, 64, 64, device=dev)
    x2 = (x1 + 0.1 * torch.randn_like(x1)).contiguous(memory_format=fmt)
    x1 = x1.contiguous(memory_format=fmt)

    def step():
        resnet.NHWC_MODE, resnet.NHWC_STEM_MODE, resnet.BF16_MODE = nhwc_mode, stem_mode, bf16_mode      # (read at call time)
        if amp is None:
            return T.train_step(((None, None), (x1, x2)), loss, opt, f, sync=False)[0]
        return T.train_step(((None, None), (x1, x2)), loss, opt, f, sync=False, amp=amp)[0]
    return step


def make_batch_leg(how, f, loss, opt, amp, modes):
    """The leg's step with the batch inside: `how` = "clocked" (eager) or "graph" (one replay)."""
    import tempfile
    import numpy as np
    import torch
    from cl_ica_amd import latent_spaces, resnet, spaces, threedident as T
    from cl_ica_amd.datasets import ThreeDIdentDataset
    rng = np.random.default_rng(0)
    ls = latent_spaces.LatentSpace(spaces.NBoxSpace(3), lambda s, size, device="cuda": s.uniform(size, device=device),
                                   lambda s, z, size, device="cuda": s.normal(z, 0.1, size, device=device))
    with tempfile.TemporaryDirectory() as root:
        np.save(os.path.join(root, "raw_latents.npy"), rng.uniform(-1, 1, size=(TABLE_IMAGES, 3)).astype(np.float32))
        images = torch.randint(0, 256, (TABLE_IMAGES, 64, 64, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
        ds = ThreeDIdentDataset(root, ls, images=images, normalize=([0.3292, 0.3278, 0.3215], [0.0778, 0.0776, 0.0771]))
    clock = spaces.DeviceClock(0, "cuda")

    def set_modes():
        resnet.NHWC_MODE, resnet.NHWC_STEM_MODE, resnet.BF16_MODE = modes

    if how == "clocked":
        def step():
            set_modes()
            return T.clocked_iteration(ds, loss, opt, f, 1024, clock, amp=amp)[0][0]
        return step
    set_modes()
    first = []
    captured = T.capture_iteration(ds, loss, opt, f, 1024, amp=amp, warmup=2, clock=clock, on_warmup=lambda r: first.append(r[0].clone()))

    def step():                                       # every call is one replay: the two eager warm-up iterations ran above
        return captured()[0]
    step.captured, step.first_loss = captured, first[0]
    return step


def run_leg(leg, steps, warmup, windows):
    import torch
    step = make_leg(leg)
    first = getattr(step, "first_loss", None)         # (a -graph leg ran its first iteration while it was being recorded)
    for _ in range(warmup):
        last = step()
        first = last if first is None else first
    torch.cuda.synchronize()
    ws = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            last = step()
        e1.record()
        torch.cuda.synchronize()
        ws.append(e0.elapsed_time(e1) * 1e-3)
    el = statistics.median(ws)
    res = {"leg": leg, "steps_per_s": round(steps / el, 2), "ms_per_step": round(1e3 * el / steps, 2), "final_loss": round(float(last.item()), 5),
           "windows_s": [round(w, 4) for w in ws]}
    if (leg in BF16_LEGS or leg in BATCH_LEGS) and first is not None:
        res["first_loss"] = round(float(first.item()), 5)
    del step
    torch.cuda.empty_cache()
    return res


def units(out, reps=20):
    """The unit alone at ResNet-18's shapes.  E = N C H W x 4 bytes; algorithmic bytes: forward E (statistics) + 2 E (apply), + E with a
    residual; backward 3 E (sums) + 4 E (backward apply), + E with dr."""
    import torch
    from cl_ica_amd import ops
    dev = torch.device("cuda")
    for name, N, C, H, W in UNIT_SHAPES:
        E = N * C * H * W * 4
        w = torch.ones(C, device=dev); b = torch.zeros(C, device=dev)
        for layout in ("nchw", "nhwc"):
            fmt = torch.channels_last if layout == "nhwc" else torch.contiguous_format
            x, r, dy = (torch.randn(N, C, H, W, device=dev).contiguous(memory_format=fmt) for _ in range(3))
            fwd = ops.batchnorm2d_act_fwd_nhwc if layout == "nhwc" else ops.batchnorm2d_act_fwd
            bwd = ops.batchnorm2d_act_bwd_nhwc if layout == "nhwc" else ops.batchnorm2d_act_bwd
            ev = ops.batchnorm2d_act_eval_nhwc if layout == "nhwc" else ops.batchnorm2d_act_eval
            for res in (False, True):
                rr = r if res else None
                y, m, i = fwd(x, w, b, None, None, 1e-5, 0.1, 0.0, residual=rr)
                calls = {"forward (statistics + apply)": (lambda: fwd(x, w, b, None, None, 1e-5, 0.1, 0.0, residual=rr), (4 if res else 3) * E),
                         "backward (sums + backward apply)": (lambda: bwd(x, y, dy, w, m, i, 0.0, need_dr=res), (8 if res else 7) * E),
                         "inference apply": (lambda: ev(x, w, b, m, i.reciprocal().square(), 1e-5, 0.0, residual=rr), (3 if res else 2) * E)}
                for what, (call, nbytes) in calls.items():
                    for _ in range(3):
                        call()
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps):
                        call()
                    e1.record()
                    torch.cuda.synchronize()
                    us = e0.elapsed_time(e1) * 1e3 / reps
                    emit(out, {"unit": name, "M": N * H * W, "C": C, "E_MB": round(E / 1e6, 1), "layout": layout, "residual": res, "call": what,
                               "us_per_call": round(us, 1), "TB_per_s": round(nbytes / us / 1e6, 2)})
            del x, r, dy, y
            torch.cuda.empty_cache()


def stem_units(out, reps=20):
    """The fused stem unit (bn1 + relu + max-pool 3/2/1) alone at ResNet-18's stem shape, both layouts.  E = N C H W x 4 bytes of x,
    E / 4 of P and dP; algorithmic bytes: forward x read twice (statistics, pool) + P = 2.25 E; backward x and dP read twice (sums,
    backward apply) + dx = 3.5 E."""
    import torch
    from cl_ica_amd import ops
    dev = torch.device("cuda")
    name, N, C, H, W = UNIT_SHAPES[0]
    E = N * C * H * W * 4
    w = torch.ones(C, device=dev); b = torch.zeros(C, device=dev)
    for layout in ("nchw", "nhwc"):
        fmt = torch.channels_last if layout == "nhwc" else torch.contiguous_format
        sfx = "_nhwc" if layout == "nhwc" else ""
        fwd, bwd, ev = (getattr(ops, "batchnorm2d_act_maxpool_" + k + sfx) for k in ("fwd", "bwd", "eval"))
        x = torch.randn(N, C, H, W, device=dev).contiguous(memory_format=fmt)
        p, m, i = fwd(x, w, b, None, None, 1e-5, 0.1, 0.0)
        dp = torch.randn(*p.shape, device=dev).contiguous(memory_format=fmt)
        calls = {"forward (statistics + pool)": (lambda: fwd(x, w, b, None, None, 1e-5, 0.1, 0.0), 2.25 * E),
                 "backward (sums + backward apply)": (lambda: bwd(x, dp, w, b, m, i, 0.0), 3.5 * E),
                 "inference pool": (lambda: ev(x, w, b, m, i.reciprocal().square(), 1e-5, 0.0), 1.25 * E)}
        for what, (call, nbytes) in calls.items():
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / reps
            emit(out, {"unit": "stem + max-pool", "M": N * H * W, "C": C, "E_MB": round(E / 1e6, 1), "layout": layout, "call": what,
                       "us_per_call": round(us, 1), "TB_per_s": round(nbytes / us / 1e6, 2)})
        del x, p, dp
        torch.cuda.empty_cache()


def _timed(call, reps):
    import torch
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def bf16_units(out, reps=20):
    """The channels-last units, the fused stem and the average pool on bf16 activations, at the shapes and with the calls of units()
    and stem_units(): E is now N C H W x 2 bytes, the byte counts are the same multiples of it (the average pool: E in, E out)."""
    import torch
    from cl_ica_amd import ops
    dev, bf = torch.device("cuda"), torch.bfloat16
    nhwc = lambda t: t.contiguous(memory_format=torch.channels_last)
    for name, N, C, H, W in UNIT_SHAPES:
        E = N * C * H * W * 2
        w = torch.ones(C, device=dev); b = torch.zeros(C, device=dev)
        x, r, dy = (nhwc(torch.randn(N, C, H, W, device=dev).to(bf)) for _ in range(3))
        fwd, bwd, ev = ops.batchnorm2d_act_fwd_nhwc, ops.batchnorm2d_act_bwd_nhwc, ops.batchnorm2d_act_eval_nhwc
        for res in (False, True):
            rr = r if res else None
            y, m, i = fwd(x, w, b, None, None, 1e-5, 0.1, 0.0, residual=rr)
            calls = {"forward (statistics + apply)": (lambda: fwd(x, w, b, None, None, 1e-5, 0.1, 0.0, residual=rr), (4 if res else 3) * E),
                     "backward (sums + backward apply)": (lambda: bwd(x, y, dy, w, m, i, 0.0, need_dr=res), (8 if res else 7) * E),
                     "inference apply": (lambda: ev(x, w, b, m, i.reciprocal().square(), 1e-5, 0.0, residual=rr), (3 if res else 2) * E)}
            for what, (call, nbytes) in calls.items():
                us = _timed(call, reps)
                emit(out, {"unit": name, "M": N * H * W, "C": C, "E_MB": round(E / 1e6, 1), "layout": "nhwc-bf16", "residual": res,
                           "call": what, "us_per_call": round(us, 1), "TB_per_s": round(nbytes / us / 1e6, 2)})
        del x, r, dy, y
        torch.cuda.empty_cache()
    name, N, C, H, W = UNIT_SHAPES[0]
    E = N * C * H * W * 2
    w = torch.ones(C, device=dev); b = torch.zeros(C, device=dev)
    x = nhwc(torch.randn(N, C, H, W, device=dev).to(bf))
    fwd, bwd, ev = ops.batchnorm2d_act_maxpool_fwd_nhwc, ops.batchnorm2d_act_maxpool_bwd_nhwc, ops.batchnorm2d_act_maxpool_eval_nhwc
    p, m, i = fwd(x, w, b, None, None, 1e-5, 0.1, 0.0)
    dp = nhwc(torch.randn(*p.shape, device=dev).to(bf))
    calls = {"forward (statistics + pool)": (lambda: fwd(x, w, b, None, None, 1e-5, 0.1, 0.0), 2.25 * E),
             "backward (sums + backward apply)": (lambda: bwd(x, dp, w, b, m, i, 0.0), 3.5 * E),
             "inference pool": (lambda: ev(x, w, b, m, i.reciprocal().square(), 1e-5, 0.0), 1.25 * E)}
    for what, (call, nbytes) in calls.items():
        us = _timed(call, reps)
        emit(out, {"unit": "stem + max-pool", "M": N * H * W, "C": C, "E_MB": round(E / 1e6, 1), "layout": "nhwc-bf16", "call": what,
                   "us_per_call": round(us, 1), "TB_per_s": round(nbytes / us / 1e6, 2)})
    del x, p, dp
    torch.cuda.empty_cache()
    name, N, C, H, W = UNIT_SHAPES[-1]                        # the average pool sits behind layer 4
    for dtype, tag in ((torch.float32, "nhwc"), (bf, "nhwc-bf16")):
        x = nhwc(torch.randn(N, C, H, W, device=dev).to(dtype))
        E = x.numel() * x.element_size()
        g = torch.randn(N, C, device=dev)
        calls = {"average pool forward": (lambda: ops.avgpool2d_global_fwd_nhwc(x), E + N * C * 4),
                 "average pool backward": (lambda: ops.avgpool2d_global_bwd_nhwc(g, H, W, dtype), E + N * C * 4)}
        for what, (call, nbytes) in calls.items():
            us = _timed(call, reps)
            emit(out, {"unit": "average pool", "M": N * H * W, "C": C, "E_MB": round(E / 1e6, 1), "layout": tag, "call": what,
                       "us_per_call": round(us, 1), "TB_per_s": round(nbytes / us / 1e6, 2)})
        del x
    torch.cuda.empty_cache()


def bucket_of(name):
    n = name
    if "clica::bn2d::nhwc::avgpool" in n or "clica::bn2d::nhwc::pool_" in n or "clica::avgpool" in n or "clica::bn2d::pool_" in n:
        return "clica pool kernels"
    if "clica::bn2d::nhwc" in n:
        return "clica::bn2d::nhwc::* units"
    if "clica::bn2d" in n:
        return "clica::bn2d::* (NCHW)"
    if "clica::" in n:
        return "other HIP library kernels (head, loss, Adam)"
    low = n.lower()
    if "transpose" in low or "subtensorop" in low:
        return "MIOpen layout transposes / SubTensorOp"
    if "max_pool" in low or "maxpool" in low:
        return "ATen max-pool (stem, unfused in NHWC)"
    if "batch_norm" in low or "batchnorm" in low or "bn_fwd" in low or "bn_bwd" in low or "bnfwd" in low or "bnbwd" in low:
        return "MIOpen / ATen BatchNorm"
    if "at::native" in n or "at::" in n:
        return "ATen element-wise / reductions / copies"
    return "MIOpen / rocBLAS convolution kernels"


def summarise(path, out, top=45):
    rows = list(csv.DictReader(open(path)))
    name_key = "Kernel_Name" if "Kernel_Name" in rows[0] else "Name"
    gx = [k for k in ("Grid_Size_X", "Grid_Size") if k in rows[0]]
    gy = "Grid_Size_Y" if "Grid_Size_Y" in rows[0] else None
    wx = "Workgroup_Size_X" if "Workgroup_Size_X" in rows[0] else ("Workgroup_Size" if "Workgroup_Size" in rows[0] else None)
    buckets, groups = {}, {}
    total = 0.0
    for r in rows:
        d = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3      # us
        total += d
        full = r[name_key]
        b = buckets.setdefault(bucket_of(full), [0.0, 0])
        b[0] += d; b[1] += 1
        short = full.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0][:96]
        grid = (int(r[gx[0]]) // max(int(r[wx]), 1) if gx and wx else 0, int(r[gy]) if gy else 0)
        groups.setdefault((short, grid), []).append(d)
    emit(out, {"trace": path, "kernel_ms": round(total / 1e3, 1), "launches": len(rows)})
    for k, (t, n) in sorted(buckets.items(), key=lambda kv: -kv[1][0]):
        emit(out, {"bucket": k, "share_pct": round(100 * t / total, 1), "ms": round(t / 1e3, 1), "launches": n})
    listed = sorted(groups.items(), key=lambda kv: -sum(kv[1]))[:top]
    for (short, grid), ds in listed:
        ds = sorted(ds)
        # one (kernel, grid) may serve two tensor sizes (the C = 64 units of the stem and of layer 1): split at the widest gap over 2 x
        cut = max(range(1, len(ds)), key=lambda i: ds[i] / max(ds[i - 1], 1e-9), default=None)
        parts = [ds[:cut], ds[cut:]] if cut and ds[cut] > 2.0 * ds[cut - 1] else [ds]
        for p in parts:
            emit(out, {"kernel": short, "grid_workgroups": list(grid), "calls": len(p), "mean_us": round(statistics.fmean(p), 1),
                       "min_us": round(p[0], 1), "max_us": round(p[-1], 1), "total_ms": round(sum(p) / 1e3, 2)})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", choices=sorted(ALL_LEGS), help="run this leg alone (for a profiler)")
    ap.add_argument("--legs", default=None, help="comma-separated legs of the alternating run (default: all)")
    ap.add_argument("--units", action="store_true")
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV")
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.out)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("c4_layout_ab.py measures on the GPU: none here")
    if args.units:
        units(args.out)
        stem_units(args.out)
        return bf16_units(args.out)
    if args.leg:
        return emit(args.out, dict(run_leg(args.leg, args.steps or 30, args.warmup, 1), run="alone"))
    legs = args.legs.split(",") if args.legs else list(LEGS)      # (the batch legs run when named)
    if any(leg not in ALL_LEGS for leg in legs):
        raise SystemExit(f"--legs {args.legs!r}: legs are {sorted(ALL_LEGS)}")
    for leg in legs:                                   # MIOpen's find step of every leg, outside every window
        emit(args.out, dict(run_leg(leg, 4, 2, 1), run="throw-away"))
    for rnd in range(1, args.rounds + 1):
        for leg in legs:
            emit(args.out, dict(run_leg(leg, args.steps or 20, args.warmup, 3), run=f"round {rnd}"))


if __name__ == "__main__":
    main()
