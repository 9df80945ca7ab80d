#!/usr/bin/env python3
"""Phase timing inside the two Lp loss sweeps of the headline step (-DCLICA_LP_TRACE build of csrc/lp_loss_pk.hip, p = 2): where a
workgroup of fwd_partial_fin_k / bwd_pairs_k spends its cycles -- prologue, per tile (loads issued / pair loop / barrier), merge, arrival,
finisher.  Stamps are taken by thread 0 of every workgroup; medians over the workgroups are printed.
    make -C cl_ica_amd/csrc lptrace && python tools/lp_trace.py [library ...]
Every library named (default: cl_ica_amd/lib/libclica_hip_lptrace.so) is traced in a child process of its own under a time limit; the
first child that fails ends the run."""
import ctypes, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = os.path.join(ROOT, "cl_ica_amd/lib/libclica_hip_lptrace.so")
LIMIT_S = 180
MAXWG, MAXT, HEAD = 1024, 8, 8          # csrc/lp_kernels.h: LPT_MAXWG, LPT_MAXT, the slots in front of the per-tile stamps
NS = HEAD + 4 * MAXT


def worker():
    import numpy as np, torch
    sys.path.insert(0, ROOT)
    from cl_ica_amd import _lib, encoders
    from cl_ica_amd.engine import ContrastiveTrainer, SamplerSpec
    lib = _lib.load()
    lib.clica_debug_lp_trace.argtypes = [ctypes.c_void_p]
    n, B = 10, 6144
    torch.manual_seed(0)
    f = encoders.get_mlp(n, n, [n * 10, n * 50, n * 50, n * 50, n * 50, n * 10]).to("cuda")
    gW = torch.randn(3, n, n, device="cuda") / n ** 0.5
    tr = ContrastiveTrainer(f, gW, SamplerSpec(n=n), batch_size=B, p=2, lr=1e-4, device="cuda", split_bf16=True)
    for _ in range(30):
        tr.step()
    torch.cuda.synchronize()
    buf = torch.zeros(2 * MAXWG * NS, dtype=torch.int64, device="cuda")
    tr._packed_current = False
    tr.sample(); tr.pack(); tr.forward(); torch.cuda.synchronize()
    assert lib.clica_debug_lp_trace(buf.data_ptr()) == 0
    tr.loss_forward_backward(); torch.cuda.synchronize()
    lib.clica_debug_lp_trace(None)
    t = buf.cpu().numpy().reshape(2, MAXWG, NS).astype(np.float64)
    med = lambda a: int(np.median(a)) if a.size else -1
    for kind, name in ((0, "forward  fwd_partial_fin_k"), (1, "backward bwd_pairs_k")):
        w = t[kind][t[kind][:, 0] > 0]
        if not len(w):
            print(f"== {name}: no stamps (kernel not run from the traced translation unit)")
            continue
        t0 = w[:, 0:1]
        tiles = int((w[:, HEAD + 1::4] > 0).sum(1).max())
        print(f"== {name}: {len(w)} workgroups, {tiles} tiles each; cycles from the workgroup's entry, median over the workgroups")
        print(f"  owner loads issued {med(w[:, 1] - t0[:, 0])}   first tile staged, barrier passed {med(w[:, 2] - t0[:, 0])}")
        for k in range(tiles):
            s = w[:, HEAD + 4 * k:HEAD + 4 * k + 4]
            ok = s[:, 1] > 0
            s = s[ok]
            print(f"  tile {k}: loads issued at {med(s[:, 0] - t0[ok, 0])} (+{med(s[:, 1] - s[:, 0])} to enter the pair loop)   pair loop {med(s[:, 2] - s[:, 1])}"
                  f"   store + barrier {med(s[:, 3] - s[:, 2])}")
        last = w[:, HEAD + 4 * (tiles - 1) + 3]
        print(f"  merge done {med(w[:, 3] - t0[:, 0])} (+{med(w[:, 3] - last)} behind the last barrier)")
        if kind == 0:
            print(f"  arrival {med(w[:, 4] - t0[:, 0])} (+{med(w[:, 4] - w[:, 3])})")
            fin = w[w[:, 5] > 0]
            print(f"  finisher ({len(fin)} workgroups): +{med(fin[:, 5] - fin[:, 4])} behind their arrival")
        print(f"  workgroup total {med(w[:, 6] - t0[:, 0])}      (stamps of different workgroups are not compared: the counters of the XCDs are not aligned)")


def main():
    libs = sys.argv[1:] or [DEFAULT]
    for path in libs:
        print(f"#### {path}", flush=True)
        env = dict(os.environ, CLICA_LIB=os.path.abspath(path))
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"], env=env, timeout=LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit(f"lp_trace: {path} ran into the {LIMIT_S} s limit; nothing more is started")
        if rc != 0:
            raise SystemExit(f"lp_trace: {path} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    worker() if sys.argv[1:2] == ["--worker"] else main()
