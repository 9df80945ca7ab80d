"""bench.py end to end on the GPU (short runs): the contract JSON line of a plain run, and with --full its roofline / kernels / loss legs and the
native-fp32 leg."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_emits_contract_line():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "20", "--warmup", "3", "--full", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "kernels", "loss_kernel", "native_fp32"):
        assert k in line, k
    assert line["n_gpus"] == 1 and line["steps"] == 20 and line["value"] > 100
    assert line["metric"] == "training steps/sec (B=6144, n=10 MLP)" and "f16x2 split" in line["dtype"]
    rf = line["roofline"]      # headline mode: ALGORITHMIC flops against the dense fp16 / bf16 peak; the issued piece products (x 3) beside it
    assert rf["bound"] == "mfma" and 0 < rf["frac"] < 1 and rf["peak"] == 2500.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert abs(rf["frac_issued"] - 3 * rf["frac"]) < 2e-3 and abs(rf["achieved_issued"] - 3 * rf["achieved"]) < 0.05
    # `achieved` must follow from the line's own numbers: algorithmic GFLOP per launch / the launch's measured duration
    assert abs(rf["achieved"] - rf["algorithmic_gflop_per_launch"] / rf["avg_launch_us"] * 1e3) < 0.02 * rf["achieved"]
    fe = rf["fp32_equivalent"]
    # (the fp32-EQUIVALENT rate may exceed the fp32 matrix peak: the three fp16 products of one fp32 product cost 0.19 of its matrix time)
    assert fe["peak"] == 157.3 and 0 < fe["frac"] < 5.0 and abs(fe["achieved"] - rf["achieved"]) < 0.05 * rf["achieved"]
    b3 = line["split_bf16x3"]      # the rounds 3-4 arithmetic on the same box in the same call
    assert b3["value"] > 100 and abs(b3["final_loss"]) < 20
    dr = line["dry_ranks_8"]       # rank 0 of an 8-rank job planned, captured with its RCCL collectives and run on this GPU
    assert "error" not in dr, dr
    assert dr["value"] > 100 and dr["negatives_pool"] == 8 * 6144 and dr["collective_bytes_per_step"] > 0 and dr["plan"]["planned_ranks"] == 8
    nat = line["native_fp32"]
    assert nat["value"] > 100 and nat["dtype"] == "f32" and nat["roofline"]["peak"] == 157.3 and 0 < nat["roofline"]["frac"] < 1
    assert abs(line["final_loss"]) < 20 and abs(nat["final_loss"]) < 20


def test_bench_plain_run_measures_the_headline_alone():
    """Without --full the run sets up, warms up, times its steps and prints the contract line, nothing else: no side leg in the line, and
    at most 30 s of the process's wall time outside its --warmup and --steps steps (import, set-up, capture, settle steps, exit)."""
    import time
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "50", "--warmup", "5"],
                       capture_output=True, text=True, timeout=300)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "final_loss"):
        assert k in line, k
    assert line["metric"] == "training steps/sec (B=6144, n=10 MLP)" and line["unit"] == "steps/s" and line["higher_is_better"] is True
    assert line["steps"] == 50 and line["warmup"] == 5 and line["value"] > 100 and "f16x2 split" in line["dtype"]
    for k in ("roofline", "kernels", "loss_kernel", "loss_kernel_pool_49152", "cpu_baseline", "speedup_vs_cpu", "dropin", "native_fp32",
              "split_bf16x3", "dry_ranks_8", "secondary", "ranks"):
        assert k not in line, k
    outside = wall - (50 + 5) * line["ms_per_step"] * 1e-3
    assert outside < 30.0, outside


def test_bench_gpus_2_starts_its_own_ranks_and_falls_back_to_eager():
    """`python bench.py --gpus 2 ...` exactly as the driver types it for N = 1 (no torchrun, no WORLD_SIZE): bench.py starts the two
    ranks itself.  On this one-GPU box both ranks share cuda:0 and the collectives run over gloo (RCCL refuses two ranks on one
    device), and the capture is made to fail on every rank, so the run also covers `capture_or_eager`'s agreement on eager launches
    (VERDICT r5 item 3).  The product collectives, the barrier-bracketed windows, the max over ranks, the `ranks` object and the
    single JSON line from rank 0 are the real ones; the numbers mean nothing."""
    env = dict(os.environ, CLICA_DIST_BACKEND="gloo", CLICA_BENCH_INJECT_CAPTURE_FAILURE="all", PYTHONFAULTHANDLER="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2", "--windows", "2", "--full"],
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "eager launches" in r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and line["steps"] == 5 and line["scaling"] == "weak" and line["value"] > 0
    assert line["config"]["launch"] == "eager" and line["config"]["negatives_pool"] == 2 * 6144 and line["config"]["parallelism"] == "dp2"
    assert [e["rank"] for e in line["ranks"]] == [0, 1] and all(e["world_size_seen"] == 2 for e in line["ranks"])
    assert sum(1 for l in r.stdout.splitlines() if l.startswith("{")) == 1        # only rank 0 prints
    assert abs(line["final_loss"]) < 20


def test_bench_dump_outputs_are_the_last_timed_step(tmp_path):
    """`--dump-outputs DIR`: after exactly `--steps` timed steps the last step's results (loss vector, parameters and gradients of the
    encoder) land in DIR as float32 .npy files, at most 64 MB.  Two runs with the same arguments except the split into windows run the
    same steps on the same inputs: a different step count would change the batch, and with it the gradients by far more than the
    bound below."""
    import numpy as np
    runs = []
    for windows in ("1", "3"):
        d = tmp_path / f"w{windows}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "12", "--warmup", "3", "--windows", windows,
                            "--no-cpu-baseline", "--no-roofline", "--no-dropin", "--no-native-leg", "--no-dry-leg", "--no-secondary",
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["steps"] == 12 and line["timed_steps_total"] == 12 and line["windows"] == int(windows)
        assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] - 1e3) < 1e-6 * line["value"] * line["ms_per_step"]
        files = sorted(p.name for p in d.iterdir())
        out = {f[:-4]: np.load(d / f) for f in files}
        assert sum((d / f).stat().st_size for f in files) <= 64 << 20
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in out.values())
        assert out["loss"].tolist() == [line["final_loss"], line["final_pos"], line["final_neg"]]
        n_lin = 7      # get_mlp(10, 10, [100, 500, 500, 500, 500, 100]): seven Linear layers, weight + bias each
        assert sum(1 for k in out if k.startswith("param.")) == sum(1 for k in out if k.startswith("grad.")) == 2 * n_lin
        assert out["param.0.weight"].shape == out["grad.0.weight"].shape == (100, 10)
        runs.append(out)
    a, b = runs
    assert sorted(a) == sorted(b)
    for k in a:
        den = max(float(np.abs(a[k]).max()), 1e-30)
        assert float(np.abs(a[k] - b[k]).max()) / den < 1e-3, k
