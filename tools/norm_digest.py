#!/usr/bin/env python3
"""What the batch-normalisation family computes (csrc/norm.hip, bn2d.hip, pool2d.hip through the ops wrappers), as one JSON line per
case -- an entry point at a shape, over its input classes, residual settings and slopes --: the case's name and a SHA-256 per output --
y / p, save_mean, save_invstd, the running statistics after the call, dx, dr, dgamma, dbeta, GroupNorm's mean and rstd, as the entry
point has them -- over the bytes of that output in every run of the case.  Two libraries whose outputs are byte-identical
compute the same bits (a refactor of the kernels: run this on both, CLICA_LIB picks the library).
Cases: the sweeps of tests/norm_oracle.py, tests/bn2d_oracle.py and tests/pool2d_oracle.py with their inference and unaligned lists,
every slope, inputs seeded as the oracles seed them; and the five BatchNorm2d shapes of ResNet-18 on 64 x 64 images (BASELINE config 4)
at N = 1024, where a channel has 4 .. 32 split partials, training forward and backward, the first also through the stem unit.
    python tools/norm_digest.py OUT.jsonl"""
import hashlib, json, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np                                            # noqa: E402
import torch                                                  # noqa: E402
import norm_oracle as O                                       # noqa: E402
import bn2d_oracle as B                                       # noqa: E402
import pool2d_oracle as Q                                     # noqa: E402
from bn_family_util import dev, off_by_4_bytes                # noqa: E402
from cl_ica_amd import ops                                    # noqa: E402

WORKLOAD = [(1024, 64, 32, 32), (1024, 64, 16, 16), (1024, 128, 8, 8), (1024, 256, 4, 4), (1024, 512, 2, 2)]


def eval_stats(c):
    """Running statistics of the size of the data's own, as the inference tests make them."""
    return dev((c["x"].mean(0) + c["running_mean"]).astype(np.float32)), dev((c["x"].var(0) * c["running_var"]).astype(np.float32))


def norm_cases():
    for kind, shapes in (("bn", O.BN_SHAPES), ("gn", O.GN_SHAPES)):
        for M, C in shapes:
            for cls in range(len(O.CLASSES)):
                c = O.make_case(kind, M, C, cls)
                x, gamma, beta, dy = dev(c["x"]), dev(c["gamma"]), dev(c["beta"]), dev(c["dy"])
                for slope in O.SLOPES:
                    name = f"{kind} {M}x{C} cls{cls} slope{slope}"
                    if kind == "bn":
                        rm, rv = dev(c["running_mean"]), dev(c["running_var"])
                        y, a, b = ops.batchnorm_lrelu_fwd(x, gamma, beta, rm, rv, O.EPS, O.MOMENTUM, slope)
                        dx, dg, db = ops.batchnorm_lrelu_bwd(x, y, dy, gamma, a, b, slope)
                        yield name, dict(y=y, save_mean=a, save_invstd=b, running_mean=rm, running_var=rv, dx=dx, dgamma=dg, dbeta=db)
                    else:
                        y, mean, rstd = ops.groupnorm_lrelu_fwd(x, gamma, beta, O.EPS, slope)
                        dx, dg, db = ops.groupnorm_lrelu_bwd(x, y, dy, gamma, mean, rstd, slope)
                        yield name, dict(y=y, mean=mean, rstd=rstd, dx=dx, dgamma=dg, dbeta=db)
    for M, C in O.BN_EVAL_SHAPES:
        for cls in range(len(O.CLASSES)):
            c = O.make_case("bn", M, C, cls)
            rm, rv = eval_stats(c)
            for slope in O.SLOPES:
                yield f"bn eval {M}x{C} cls{cls} slope{slope}", dict(y=ops.batchnorm_lrelu_eval(dev(c["x"]), dev(c["gamma"]), dev(c["beta"]), rm, rv, O.EPS, slope))


def bn2d_step(x, r, dy, gamma, beta, rm, rv, slope):
    """Training forward, then the backward with and without the residual's gradient."""
    y, a, b = ops.batchnorm2d_act_fwd(x, gamma, beta, rm, rv, B.EPS, B.MOMENTUM, slope, residual=r)
    out = dict(y=y, save_mean=a, save_invstd=b, running_mean=rm, running_var=rv)
    for need_dr in (False, True):
        dx, dr, dg, db = ops.batchnorm2d_act_bwd(x, y, dy, gamma, a, b, slope, need_dr=need_dr)
        out.update({f"dx/need_dr={need_dr}": dx, f"dr/need_dr={need_dr}": dr, f"dgamma/need_dr={need_dr}": dg, f"dbeta/need_dr={need_dr}": db})
    return out


def bn2d_cases():
    maps = lambda c, shape: [None if c[k] is None else dev(B.to_nchw(c[k], *shape)) for k in ("x", "r", "dy")]
    for shape, cls, residual in B.sweep():
        c = B.make_case(*shape, cls, residual)
        x, r, dy = maps(c, shape)
        gamma, beta = dev(c["gamma"]), dev(c["beta"])
        for slope in B.SLOPES:
            yield (f"bn2d {shape} cls{cls} res{int(residual)} slope{slope}",
                   bn2d_step(x, r, dy, gamma, beta, dev(c["running_mean"]), dev(c["running_var"]), slope))
    for shape in B.EVAL_SHAPES:
        for cls in range(len(B.CLASSES)):
            for residual in (False, True):
                c = B.make_case(*shape, cls, residual)
                x, r, _ = maps(c, shape)
                rm, rv = eval_stats(c)
                for slope in B.SLOPES:
                    yield (f"bn2d eval {shape} cls{cls} res{int(residual)} slope{slope}",
                           dict(y=ops.batchnorm2d_act_eval(x, dev(c["gamma"]), dev(c["beta"]), rm, rv, B.EPS, slope, residual=r)))
    for shape in B.UNALIGNED_SHAPES:
        c = B.make_case(*shape, 1, True)
        x, r, dy = maps(c, shape)
        gamma, beta = dev(c["gamma"]), dev(c["beta"])
        for slope in B.SLOPES:
            for tag, (xu, ru, dyu) in (("x", (off_by_4_bytes(x), r, dy)), ("x,r,dy", (off_by_4_bytes(x), off_by_4_bytes(r), off_by_4_bytes(dy)))):
                out = bn2d_step(xu, ru, dyu, gamma, beta, dev(c["running_mean"]), dev(c["running_var"]), slope)
                out["eval"] = ops.batchnorm2d_act_eval(xu, gamma, beta, dev(c["running_mean"]), dev(c["running_var"]), B.EPS, slope, residual=ru)
                yield f"bn2d unaligned({tag}) {shape} slope{slope}", out


def pool_step(x, dp, gamma, beta, rm, rv, slope):
    p, a, b = ops.batchnorm2d_act_maxpool_fwd(x, gamma, beta, rm, rv, Q.EPS, Q.MOMENTUM, slope)
    dx, dg, db = ops.batchnorm2d_act_maxpool_bwd(x, dp, gamma, beta, a, b, slope)
    return dict(p=p, save_mean=a, save_invstd=b, running_mean=rm, running_var=rv, dx=dx, dgamma=dg, dbeta=db)


def pool_cases():
    for shape, cls in Q.sweep():
        c = Q.make_case(*shape, cls)
        x, dp, gamma, beta = dev(B.to_nchw(c["x"], *shape)), dev(c["dp"]), dev(c["gamma"]), dev(c["beta"])
        for slope in Q.SLOPES:
            yield f"pool {shape} cls{cls} slope{slope}", pool_step(x, dp, gamma, beta, dev(c["running_mean"]), dev(c["running_var"]), slope)
    for shape in Q.EVAL_SHAPES:
        for cls in range(len(Q.CLASSES)):
            c = Q.make_case(*shape, cls)
            rm, rv = eval_stats(c)
            for slope in Q.SLOPES:
                yield (f"pool eval {shape} cls{cls} slope{slope}",
                       dict(p=ops.batchnorm2d_act_maxpool_eval(dev(B.to_nchw(c["x"], *shape)), dev(c["gamma"]), dev(c["beta"]), rm, rv, Q.EPS, slope)))
    for shape in Q.UNALIGNED_SHAPES:
        c = Q.make_case(*shape, 1)
        x, dp, gamma, beta = dev(B.to_nchw(c["x"], *shape)), dev(c["dp"]), dev(c["gamma"]), dev(c["beta"])
        for slope in Q.SLOPES:
            for tag, (xu, dpu) in (("x", (off_by_4_bytes(x), dp)), ("x,dp", (off_by_4_bytes(x), off_by_4_bytes(dp)))):
                out = pool_step(xu, dpu, gamma, beta, dev(c["running_mean"]), dev(c["running_var"]), slope)
                out["eval"] = ops.batchnorm2d_act_maxpool_eval(xu, gamma, beta, dev(c["running_mean"]), dev(c["running_var"]), Q.EPS, slope)
                yield f"pool unaligned({tag}) {shape} slope{slope}", out


def workload_cases():
    for i, shape in enumerate(WORKLOAD):
        cls, residual = i % len(B.CLASSES), i > 0           # (the stem unit has no shortcut)
        c = B.make_case(*shape, cls, residual, attempt=0)
        x, r, dy = [None if c[k] is None else dev(B.to_nchw(c[k], *shape)) for k in ("x", "r", "dy")]
        yield (f"workload bn2d {shape} cls{cls} res{int(residual)} slope0.0",
               bn2d_step(x, r, dy, dev(c["gamma"]), dev(c["beta"]), dev(c["running_mean"]), dev(c["running_var"]), 0.0))
        del c, x, r, dy
    shape = WORKLOAD[0]
    c = Q.make_case(*shape, 0, attempt=0)
    yield (f"workload pool {shape} cls0 slope0.0",
           pool_step(dev(B.to_nchw(c["x"], *shape)), dev(c["dp"]), dev(c["gamma"]), dev(c["beta"]), dev(c["running_mean"]), dev(c["running_var"]), 0.0))


def main():
    """One line per group: the runs that differ only in input class, residual and slope, in the order the generators give them.  An
    output's digest covers that output of every run of the group, each preceded by the run's name."""
    group, digests, runs = None, {}, 0
    with open(sys.argv[1], "w") as out:
        def close():
            if group is not None:
                out.write(json.dumps(dict(case=group, runs=runs, sha256={k: h.hexdigest() for k, h in digests.items()}), sort_keys=True) + "\n")
                out.flush()
        for cases in (norm_cases, bn2d_cases, pool_cases, workload_cases):
            for name, tensors in cases():
                torch.cuda.synchronize()
                g = re.sub(r" (cls\d+|res\d|slope[\d.]+)|(?<=unaligned)\([^)]*\)", "", name)
                if g != group:
                    close()
                    group, digests, runs = g, {}, 0
                runs += 1
                for k, t in tensors.items():
                    k = k.split("/")[0]                     # (the backward with and without dr: one digest per output)
                    if t is not None:
                        h = digests.setdefault(k, hashlib.sha256())
                        h.update(name.encode())
                        h.update(t.detach().contiguous().cpu().numpy().tobytes())
        close()


if __name__ == "__main__":
    main()
