#!/usr/bin/env python3
"""Feeding A/B of the captured KITTI-masks step at config 5's shapes (1024 pairs of 64 x 64, z_dim 5, p = 1, box_norm) in ONE process
(GPU box), on a synthetic frame table (400 sequences of 2 .. 40 masks):

    (a) loader+copy   DevicePairLoader batch (randperm slice, randint, searchsorted, ..., gather launch), copy into the static x,
                      Solver.capture replay: how a captured step was fed before the stream sampler
    (b) stream        Solver.capture_stream replay: the draw and the gather are one launch inside the graph

  python tools/c5_stream_ab.py                 a throw-away round, then --rounds (2) rounds alternating the legs; each figure the median
                                               of --windows (5) wall-clock windows of --steps (200) steps (synchronised at both ends)
  python tools/c5_stream_ab.py --kernels       clica_kitti_sample_pairs against clica_kitti_gather_pairs alone, event-timed: both move
                                               2 B H W bytes in and 8 B H W bytes out (the sampler walks its stream, the gather repeats
                                               the pairs of the sampler's last draw)
Every mode prints JSON lines; --out FILE also appends them there; --md FILE writes the summary table of a full run."""
import argparse
import json
import os
import statistics
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAIRS, Z_DIM = 1024, 5


def emit(out, obj):
    line = json.dumps(obj)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def synthetic_table(n_seq=400, hw=64, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    lens = rng.integers(2, 40, size=n_seq)
    return {"pedestrians": [rng.random((int(T), hw, hw)) < 0.1 for T in lens],
            "pedestrians_latents": [rng.normal(size=(int(T), 3)).astype(np.float32) for T in lens]}


def solver():
    import torch
    from cl_ica_amd.kitti_masks.solver import Solver
    torch.manual_seed(0)
    a = types.SimpleNamespace(cuda=True, ckpt_dir="/tmp", output_dir="/tmp", dataset="kitti", max_iter=1, z_dim=Z_DIM, num_channel=1,
                              lr=1e-4, beta1=0.9, beta2=0.999, ckpt_name="last", log_step=1000, save_step=10 ** 9, box_norm=True, p=1)
    S = Solver(a, None)
    S.net_mode(train=True)
    return S


def make_legs(ds):
    """leg name -> step(): one training iteration, data included."""
    import itertools
    import torch
    from cl_ica_amd.kitti_masks import dataset as D
    loader = D.DevicePairLoader(ds, PAIRS, seed=1)
    batches = (images for _ in itertools.count() for images, _labels in loader)
    Sa = solver()
    x = next(batches).clone()
    replay_a, _loss_a = Sa.capture(x)

    def step_a():
        x.copy_(next(batches))
        replay_a()

    Sb = solver()
    replay_b, _loss_b = Sb.capture_stream(D.StreamPairSampler(ds, PAIRS, seed=1))
    torch.cuda.synchronize()
    return {"loader+copy": step_a, "stream": replay_b}


def window(step, steps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def run_leg(name, step, steps, warmup, windows):
    for _ in range(warmup):
        step()
    ws = [window(step, steps) for _ in range(windows)]
    el = statistics.median(ws)
    return {"leg": name, "steps_per_s": round(steps / el, 1), "us_per_step": round(1e6 * el / steps, 1), "windows_s": [round(w, 4) for w in ws]}


def kernels(ds, out, reps=50, windows=7):
    """The two launches alone, event-timed: median and spread over `windows` windows of `reps` launches."""
    import torch
    from cl_ica_amd import _lib
    from cl_ica_amd.kitti_masks import dataset as D
    lib = _lib.load()
    s = D.StreamPairSampler(ds, PAIRS, seed=1)
    images, labels = s.draw()
    _index, _t, first, second = s.last_draw()
    elems = ds.frames[0].numel()

    def sample():
        s._launch(images, labels)

    def gather():
        _lib.check(lib.clica_kitti_gather_pairs(ds.frames.data_ptr(), elems, ds.frames.shape[0], first.data_ptr(), second.data_ptr(), PAIRS,
                                                images.data_ptr(), ds.frame_latents.data_ptr(), 3, labels.data_ptr(), _lib.stream_ptr()), "gather")

    res = {}
    for rnd in range(2):                                        # alternated; the first pass is thrown away
        for name, call in (("clica_kitti_sample_pairs", sample), ("clica_kitti_gather_pairs", gather)):
            for _ in range(5):
                call()
            us = []
            for _ in range(windows):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(reps):
                    call()
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / reps)
            if rnd:
                nbytes = 10 * PAIRS * elems
                res[name] = {"kernel": name, "windows": windows, "launches_per_window": reps, "us_per_launch": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
                             "TB_per_s": round(nbytes / statistics.median(us) / 1e6, 2)}
                emit(out, res[name])
    return res


def write_md(path, legs, kern, args):
    a, b = legs["loader+copy"], legs["stream"]
    spread = lambda rs: max(r["steps_per_s"] for r in rs) - min(r["steps_per_s"] for r in rs)      # noqa: E731
    mid = lambda rs: round(statistics.median(r["steps_per_s"] for r in rs), 1)                      # noqa: E731
    ks, kg = kern["clica_kitti_sample_pairs"], kern["clica_kitti_gather_pairs"]
    lines = ["# Captured KITTI-masks step: feeding A/B at config 5's shapes", "",
             f"`tools/c5_stream_ab.py`, one process, {PAIRS} pairs of 64 x 64, z_dim {Z_DIM}, p = 1, synthetic frame table; a throw-away round, then "
             f"{args.rounds} rounds alternating the legs, each figure the median of {args.windows} wall-clock windows of {args.steps} steps.", "",
             "| leg | steps/s per round | median | round-to-round spread |", "|---|---|---|---|"]
    for name, rs in (("(a) DevicePairLoader batch + copy into x + `Solver.capture` replay", a), ("(b) `Solver.capture_stream` replay", b)):
        lines.append(f"| {name} | {', '.join(str(r['steps_per_s']) for r in rs)} | {mid(rs)} | {round(spread(rs), 1)} |")
    lines += ["", f"(b) - (a) = {round(mid(b) - mid(a), 1)} steps/s ({round(100 * (mid(b) / mid(a) - 1), 1)} %); "
                  f"the larger of the two spreads is {round(max(spread(a), spread(b)), 1)} steps/s.", "",
              f"The two launches alone, event-timed (median of {ks['windows']} windows of {ks['launches_per_window']} launches, min .. max of "
              "the windows), both 2 B H W bytes in and 8 B H W bytes out:", "", "| launch | us | min .. max | TB/s |", "|---|---|---|---|"]
    for k in (ks, kg):
        lines.append(f"| `{k['kernel']}` | {k['us_per_launch']} | {k['min_us']} .. {k['max_us']} | {k['TB_per_s']} |")
    lines += ["", "(Everything above this line is written by `--md`; a 'Reading' section below it, where there is one, is written by hand.)"]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("c5_stream_ab.py measures on the GPU: none here")
    from cl_ica_amd.kitti_masks import dataset as D
    ds = D.KittiMasks(data=synthetic_table(), max_delta_t=5)
    if args.kernels:
        return kernels(ds, args.out)
    legs = make_legs(ds)
    for name, step in legs.items():
        emit(args.out, dict(run_leg(name, step, 50, args.warmup, 1), run="throw-away"))
    results = {name: [] for name in legs}
    for rnd in range(1, args.rounds + 1):
        for name, step in legs.items():
            results[name].append(run_leg(name, step, args.steps, args.warmup, args.windows))
            emit(args.out, dict(results[name][-1], run=f"round {rnd}"))
    kern = kernels(ds, args.out)
    if args.md:
        write_md(args.md, results, kern, args)


if __name__ == "__main__":
    main()
