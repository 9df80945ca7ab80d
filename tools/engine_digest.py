#!/usr/bin/env python3
"""What the fused trainers compute and launch, as one JSON line per configuration: SHA-256 of parameters, moments, step counter, dy and every
step's result after 3 eager steps and after 3 replays of a captured step, the ordered names of the library calls of the eager run, and
plan_summary().  Two commits whose outputs are byte-identical run the same launches on the same bits (a refactor of engine.py: run this
at both).  The call names are what _lib.check reports under CLICA_DEBUG_SYNC=1; clica_mlp_chain_tail_supported -- a host-side question to
the library's planner that launches nothing -- is left out of the list, so that WHEN a trainer asks it does not count.
    python tools/engine_digest.py OUT.jsonl          # the digest
    python tools/engine_digest.py --eager            # prints steps/s of 300 eager steps at B = 6144 behind 50 warm-up steps (one event pair)
    python tools/engine_digest.py --eager --hidden 100,640,640,100      # ... with these hidden widths (here: the per-layer path)"""
import hashlib, json, os, sys
os.environ["CLICA_DEBUG_SYNC"] = "1" if "--eager" not in sys.argv else "0"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                  # noqa: E402
import torch.distributed as dist                              # noqa: E402
from cl_ica_amd import encoders                               # noqa: E402
from cl_ica_amd.engine import ContrastiveTrainer, SamplerSpec, SupervisedTrainer      # noqa: E402

N, B = 10, 200       # 400 encoder rows: eight 48-row panels + a ragged one, three 64-row loss tiles + a ragged one


class Calls:
    """Stands in for sys.stderr while a run is recorded: keeps the names _lib.check reports."""
    def __init__(self):
        self.names = []

    def write(self, text):
        self.names += [ln[8:] for ln in text.splitlines() if ln.startswith("[clica] ") and ln[8:] != "clica_mlp_chain_tail_supported"]

    def flush(self):
        pass


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def build(cls=ContrastiveTrainer, hidden=(100, 500, 500, 100), head=None, space="box", arith="f16", split=True, hooks=(), **kw):
    torch.manual_seed(0)
    f = encoders.get_mlp(N, N, list(hidden), output_normalization=head)
    gW = torch.randn(3, N, N) / N ** 0.5
    return cls(f, gW, SamplerSpec(space=space, n=N, seed=5), batch_size=B, lr=1e-3, device="cuda", split_bf16=split, split_arith=arith, **kw)


def hooked(fn):
    """Run fn(name, **cfg) with cfg["hooks"] -- (class, attribute, value): the trainers' test hooks are class attributes -- set from
    before the trainers are constructed until the run is over, as the tests do."""
    def wrapped(name, **cfg):
        hooks = cfg.get("hooks", ())
        saved = [(c, k, k in c.__dict__, c.__dict__.get(k)) for c, k, _ in hooks]
        for c, k, v in hooks:
            setattr(c, k, v)
        try:
            return fn(name, **cfg)
        finally:
            for c, k, own, old in saved:
                setattr(c, k, old) if own else delattr(c, k)
    return wrapped


def state(tr, results):
    torch.cuda.synchronize()
    d = {k: sha(getattr(tr, k)) for k in ("param_arena", "exp_avg", "exp_avg_sq", "step_dev", "dy")}
    d["results"] = [sha(r) for r in results]
    return d


@hooked
def run(name, **cfg):
    tr = build(**cfg)
    rec, err = Calls(), sys.stderr
    sys.stderr = rec
    try:
        results = [tr.step().clone() for _ in range(3)]
    finally:
        sys.stderr = err
    row = dict(config=name, eager=state(tr, results), calls=rec.names, plan=tr.plan_summary())
    tr = build(**cfg)
    tr.capture(warmup=2)
    row["replay"] = state(tr, [tr.step().clone() for _ in range(3)])
    return row


def checkpoint_round_trip(name, **cfg):
    a = build(**cfg)
    ra = [a.step().clone() for _ in range(4)]
    b = build(**cfg)
    rb = [b.step().clone() for _ in range(2)]
    sd = b.state_dict()
    c = build(**cfg)
    domain = c.load_state_dict(sd)
    rb += [c.step().clone() for _ in range(2)]
    sa, sc = state(a, ra), state(c, rb)
    return dict(config=name, domain=domain, uninterrupted=sa, resumed=sc, identical=sa == sc)


def configs():
    C, S = ContrastiveTrainer, SupervisedTrainer
    yield "p2/f16x2", dict(p=2)
    yield "p2/bf16x3", dict(p=2, arith="bf16")
    yield "p2/native_fp32", dict(p=2, split=False)
    yield "p1/f16x2", dict(p=1)
    yield "p0/fixed_sphere", dict(p=0, tau=0.5, head="fixed_sphere", space="sphere")
    yield "p2/learnable_box", dict(p=2, head="learnable_box")
    yield "p2/fold_dy_reduce=False", dict(p=2, hooks=((C, "fold_dy_reduce", False),))
    yield "p2/chain_tail=False", dict(p=2, hooks=((C, "chain_tail", False),))
    yield "supervised/fold_mse=True", dict(cls=S, hooks=((S, "fold_mse", True),))
    yield "supervised/fold_mse=False", dict(cls=S, hooks=((S, "fold_mse", False),))
    yield "supervised/learnable_box", dict(cls=S, head="learnable_box")
    yield "per-layer/f16x2", dict(p=2, hidden=(100, 640, 640, 100))
    yield "per-layer/bf16x3", dict(p=2, hidden=(100, 640, 640, 100), arith="bf16")
    yield "dry_ranks=2", dict(p=2, process_group=dist.group.WORLD, force_collectives=True, dry_ranks=2)
    # the encoder paths the rows above do not reach (EncoderPlan): split forward and chain with fp32 grouped weight gradients; the plain
    # per-layer path; split weight gradients with an empty chain; a narrow encoder kept off the whole-stack kernels; the per-layer body
    # without the side stream.  (A single-Linear encoder -- fused_forward without fused_backward -- is not here: get_mlp refuses it.)
    yield "two-layer/f16x2", dict(hidden=(100,))
    yield "per-layer/native_fp32", dict(hidden=(100, 640, 640, 100), split=False)
    yield "per-layer/no-chain", dict(hidden=(100, 600, 100))
    yield "per-layer/forced", dict(hidden=(100, 500, 500, 100), fused_forward=False)
    yield "per-layer/f16x2/one-stream", dict(hidden=(100, 640, 640, 100), overlap_backward=False)


def eager_rate():
    hidden = [100, 500, 500, 500, 500, 100]
    if "--hidden" in sys.argv:           # e.g. --hidden 100,640,640,100: the same loop on the per-layer path
        hidden = [int(w) for w in sys.argv[sys.argv.index("--hidden") + 1].split(",")]
    torch.manual_seed(0)
    f = encoders.get_mlp(N, N, hidden)
    tr = ContrastiveTrainer(f, torch.randn(3, N, N) / N ** 0.5, SamplerSpec(n=N, seed=5), batch_size=6144, p=2, lr=1e-4, device="cuda")
    for _ in range(50):
        tr.step()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(300):
        tr.step()
    ev[1].record()
    torch.cuda.synchronize()
    print(json.dumps(dict(eager_steps_per_s=300.0 / (ev[0].elapsed_time(ev[1]) * 1e-3))))


def main():
    if "--eager" in sys.argv:
        return eager_rate()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29531")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        with open(sys.argv[1], "w") as out:
            for name, cfg in configs():
                out.write(json.dumps(run(name, **cfg), sort_keys=True) + "\n"); out.flush()
            out.write(json.dumps(checkpoint_round_trip("checkpoint/p2/f16x2", p=2), sort_keys=True) + "\n")
            out.write(json.dumps(checkpoint_round_trip("checkpoint/supervised", cls=SupervisedTrainer), sort_keys=True) + "\n")
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
