#!/usr/bin/env python3
"""clica_image_gather_norm (csrc/image_table.hip) at the 3DIdent batch: ONE launch gathers 2 x 1024 images (both views of a pair batch)
from a uint8 table of at least 2 GB in HBM, seeded random rows, ToTensor + Normalize -> float32 [2048, 3, H, W]; at 224 x 224 x 3
(308 MB read, 1.23 GB written) and at 64 x 64 x 3.  Legs, alternating window by window in one process, timed by device events after
warm-up, median of the windows (every leg replays a captured graph of 10 launches):
    gather        the kernel as shipped (non-temporal stores)
    gather_plain  the same kernel with plain stores (clica_set_tuning("image_nt_stores", 0)): the streaming-store A/B, same bits
    copy        the yardstick: out2.copy_(out) of the output tensor -- 2.0 output sizes of bytes moved against the kernel's 1.25
and clica_image_channel_stats over the whole table (one line: time, GB/s over the table's bytes).  Prints one JSON line (--out: also
writes it to a file).  Numbers are written down, not gated on.

    python tools/image_gather_bench.py [--pairs 1024 --windows 5 --table-gb 2.0 --out profiles/image_gather_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cl_ica_amd import _lib, ops  # noqa: E402

INNER = 10
MEAN, STD = [0.3292, 0.3278, 0.3215], [0.0778, 0.0776, 0.0771]          # main_3dident.py:791-793


def set_nt(on):
    _lib.check(_lib.load().clica_set_tuning(b"image_nt_stores", int(on)), "clica_set_tuning")


def bench_shape(H, W, args):
    C = 3
    img_bytes = H * W * C
    N = int(np.ceil(args.table_gb * 2 ** 30 / img_bytes))
    gen = torch.Generator(device="cuda").manual_seed(1)
    table = torch.empty((N, H, W, C), dtype=torch.uint8, device="cuda")
    rows = max(1, (256 << 20) // img_bytes)
    for r0 in range(0, N, rows):
        table[r0:r0 + rows] = torch.randint(0, 256, (min(rows, N - r0), H, W, C), dtype=torch.uint8, device="cuda", generator=gen)
    n = 2 * args.pairs
    index = torch.randint(0, N, (n,), device="cuda", generator=gen)
    out = torch.empty((n, C, H, W), dtype=torch.float32, device="cuda")
    out2 = torch.empty_like(out)

    def gather():
        ops.image_gather_norm(table, index, MEAN, STD, out=out)

    def copy():
        out2.copy_(out)

    set_nt(0); gather(); set_nt(1); torch.cuda.synchronize()
    ref = out.clone()
    gather(); torch.cuda.synchronize()
    same_bits = bool(torch.equal(out.view(torch.int32), ref.view(torch.int32)))
    del ref
    out_bytes, in_bytes = out.numel() * 4, n * img_bytes
    # every leg is a captured graph of INNER launches (the host's launch cost stays out of the 64 x 64 numbers); the store flavour is
    # chosen when the launch is recorded
    legs = {}
    for name, fn, nt in (("gather", gather, 1), ("gather_plain", gather, 0), ("copy", copy, 1)):
        set_nt(nt)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(INNER):
                fn()
        set_nt(1)
        legs[name] = g
    replays = max(2, int(args.window_ms * 1e-3 * 3e12 / out_bytes) // INNER)          # per window, sized for ~window_ms at 3 TB/s
    steps = replays * INNER
    for g in legs.values():
        for _ in range(max(1, replays // 4)):
            g.replay()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.windows):
        for k, g in legs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(replays):
                g.replay()
            e.record()
            e.synchronize()
            times[k].append(s.elapsed_time(e) * 1e3 / steps)
    res = dict(shape=[H, W, C], table_images=N, table_bytes=N * img_bytes, batch_images=n, bytes_read=in_bytes, bytes_written=out_bytes,
               launches_per_window=steps, plain_same_bits=same_bits)
    for k in legs:
        t = np.asarray(times[k])
        moved = 2 * out_bytes if k == "copy" else in_bytes + out_bytes
        res[k] = dict(us=round(float(np.median(t)), 2), windows_us=[round(float(v), 2) for v in t],
                      gb_per_s=round(moved / float(np.median(t)) / 1e3, 1))
    res["gather_over_copy"] = round(res["gather"]["us"] / res["copy"]["us"], 3)
    res["nt_over_plain"] = round(res["gather"]["us"] / res["gather_plain"]["us"], 3)
    # channel statistics over the whole table
    ops.image_channel_sums(table); torch.cuda.synchronize()
    ts = []
    for _ in range(args.windows):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); ops.image_channel_sums(table); e.record(); e.synchronize()
        ts.append(s.elapsed_time(e) * 1e3)
    res["channel_stats"] = dict(us=round(float(np.median(ts)), 1), gb_per_s=round(N * img_bytes / float(np.median(ts)) / 1e3, 1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=60.0, help="target length of one timed window")
    ap.add_argument("--table-gb", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "image_gather_bench.py needs the MI355X"
    res = dict(metric="image_gather_norm_us", timing="median of the windows' time per launch (device events), legs alternating window by "
                      "window in one process after warm-up; GB/s by algorithmic bytes (kernel: bytes read + written; copy: 2 x output bytes)",
               device=torch.cuda.get_device_name(0), pairs=args.pairs, windows=args.windows,
               shapes=[bench_shape(224, 224, args), bench_shape(64, 64, args)])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
