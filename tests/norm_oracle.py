"""NumPy fp64 oracle of BatchNorm1d (training and inference) and GroupNorm(1, C), each fused with the LeakyReLU behind it:
forward, backward and running statistics; the input generator of the norm tests; the near-kink helper.

    y = lrelu(z, slope),  z = gamma xhat + beta          slope = 1: no activation, slope = 0: ReLU
    batch norm:  xhat = (x - mean_c) invstd_c,  invstd = 1 / sqrt(var_c + eps)  (biased variance over the M rows)
    group norm:  xhat = (x - mean_r) rstd_r,    rstd = 1 / sqrt(var_r + eps)    (biased variance over the C columns)

Shared by tests/test_norm_host.py (CPU) and tests/test_gpu_norm.py."""
import zlib

import numpy as np

EPS = 1e-5
MOMENTUM = 0.1
SLOPES = (0.01, 1.0, 0.0)
CLASSES = ((0.0, 1.0), (3.0, 0.5))          # (offset, std) of x
BN_SHAPES = [(2, 65), (3, 1), (3, 7), (63, 24), (64, 64), (65, 257), (257, 500), (4099, 40), (1000, 2000)]
GN_SHAPES = [(1, 65), (3, 7), (2, 3), (63, 24), (64, 64), (65, 257), (257, 500), (4099, 40), (1000, 2000), (5, 2049)]
BN_EVAL_SHAPES = [(3, 7), (65, 257), (4099, 40)]
KINK_REL = 2e-6          # |z| <= KINK_REL max|z|: an fp32 evaluation may put the element on the other side of the kink
MAX_LEFT_OUT = 0.05      # of a case's columns (batch norm) or rows (group norm)
# Conditioning of a case.  Any fp32 evaluation subtracts a mean that is rounded to fp32: an absolute error of up to 2^-24 |mean|, that is
# 6e-8 kappa of a standard deviation with kappa = max|x| / std over the column (batch norm) or row (group norm).  The two input classes
# have kappa around 1 and 7; with a handful of rows or columns the SAMPLE deviation can come out tiny by chance (two rows that nearly
# coincide) and kappa in the thousands, where no fp32 evaluation -- torch's included -- is a yardstick at 1e-5.  Cases are drawn with
# kappa <= MAX_KAPPA: 6e-8 x 80 = 4.8e-6, half of the bound (for 65 columns of two rows that takes a few hundred draws).
MAX_KAPPA = 80.0

# Seeds are derived from the case; a case whose first seed leaves out more than MAX_LEFT_OUT of its columns / rows, or is conditioned
# worse than MAX_KAPPA, takes the next attempt that is not (found once by `python tests/norm_oracle.py`, from the inputs and the fp64
# oracle alone; both properties are asserted by tests/test_norm_host.py).
SEED_ATTEMPT = {('bn', 2, 65, 0): 1, ('bn', 2, 65, 1): 1093}


def lrelu(z, slope):
    return np.where(z > 0, z, slope * z)


def gate(z, slope):
    return np.where(z > 0, 1.0, slope)


# ------------------------------------------------------------------------------------------------ batch norm
def bn_forward(x, gamma, beta, slope, eps=EPS, running_mean=None, running_var=None, momentum=MOMENTUM):
    x, gamma, beta = (np.asarray(a, np.float64) for a in (x, gamma, beta))
    M = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    invstd = 1.0 / np.sqrt(var + eps)
    xhat = (x - mean) * invstd
    z = gamma * xhat + beta
    out = dict(y=lrelu(z, slope), z=z, xhat=xhat, mean=mean, invstd=invstd)
    if running_mean is not None:
        out["running_mean"] = (1.0 - momentum) * np.asarray(running_mean, np.float64) + momentum * mean
        out["running_var"] = (1.0 - momentum) * np.asarray(running_var, np.float64) + momentum * var * (M / (M - 1.0))
    return out


def bn_backward(fw, gamma, dy, slope):
    gamma, dy = np.asarray(gamma, np.float64), np.asarray(dy, np.float64)
    dz = dy * gate(fw["z"], slope)
    xhat = fw["xhat"]
    dbeta = dz.sum(0)
    dgamma = (dz * xhat).sum(0)
    dx = gamma * fw["invstd"] * (dz - dz.mean(0) - xhat * (dz * xhat).mean(0))
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta)


def bn_eval(x, gamma, beta, running_mean, running_var, slope, eps=EPS):
    x, gamma, beta, rm, rv = (np.asarray(a, np.float64) for a in (x, gamma, beta, running_mean, running_var))
    z = gamma * (x - rm) / np.sqrt(rv + eps) + beta
    return dict(y=lrelu(z, slope), z=z)


# ------------------------------------------------------------------------------------------------ group norm, one group
def gn_forward(x, gamma, beta, slope, eps=EPS):
    x, gamma, beta = (np.asarray(a, np.float64) for a in (x, gamma, beta))
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (x - mean[:, None]) * rstd[:, None]
    z = gamma * xhat + beta
    return dict(y=lrelu(z, slope), z=z, xhat=xhat, mean=mean, rstd=rstd)


def gn_backward(fw, gamma, dy, slope):
    gamma, dy = np.asarray(gamma, np.float64), np.asarray(dy, np.float64)
    dz = dy * gate(fw["z"], slope)
    xhat = fw["xhat"]
    g = dz * gamma
    dx = fw["rstd"][:, None] * (g - g.mean(1, keepdims=True) - xhat * (g * xhat).mean(1, keepdims=True))
    return dict(dx=dx, dgamma=(dz * xhat).sum(0), dbeta=dz.sum(0))


# ------------------------------------------------------------------------------------------------ inputs
def make_case(kind, M, C, cls, attempt=None):
    """Seeded fp32 inputs of one case: x ~ off + std N(0, 1) (batch norm: times per-column scales logspace(-1, 1, C)),
    gamma = 1 + 0.5 N, beta = 0.3 N, dy ~ N, and non-trivial running statistics to start from.
    `attempt` overrides the case's recorded seed attempt (0: the first, unselected draw)."""
    off, std = CLASSES[cls]
    seed = zlib.crc32(f"{kind}:{M}:{C}:{cls}".encode()) + 7919 * (SEED_ATTEMPT.get((kind, M, C, cls), 0) if attempt is None else attempt)
    rng = np.random.default_rng(seed)
    x = off + std * rng.normal(size=(M, C))
    if kind == "bn":
        x = x * np.logspace(-1.0, 1.0, C)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(x=f32(x), gamma=f32(1.0 + 0.5 * rng.normal(size=C)), beta=f32(0.3 * rng.normal(size=C)), dy=f32(rng.normal(size=(M, C))),
                running_mean=f32(0.1 * rng.normal(size=C)), running_var=f32(1.0 + 0.5 * rng.uniform(size=C)))


def sweep(kind):
    """(M, C, cls, slope) of every case of the sweep."""
    for (M, C) in (BN_SHAPES if kind == "bn" else GN_SHAPES):
        for cls in range(len(CLASSES)):
            for slope in SLOPES:
                yield M, C, cls, slope


def left_out(kind, z, slope):
    """The near-kink helper.  An element with |z| <= KINK_REL max|z| may take the other LeakyReLU slope in an fp32 evaluation, which
    changes dx, dgamma, dbeta of its whole column (batch norm) resp. dx of its whole row (group norm).  Returns (cols, rows): boolean
    masks of the columns and rows to leave out of those comparisons (batch norm: rows all False; group norm: `cols` marks the columns whose
    dgamma / dbeta hold such an element).  slope = 1 has no kink."""
    z = np.asarray(z, np.float64)
    near = (np.abs(z) <= KINK_REL * np.abs(z).max()) if slope != 1.0 else np.zeros(z.shape, bool)
    if kind == "bn":
        return near.any(0), np.zeros(z.shape[0], bool)
    return near.any(0), near.any(1)


def left_out_fraction(kind, z, slope):
    cols, rows = left_out(kind, z, slope)
    return float(cols.mean()) if kind == "bn" else float(rows.mean())


def kappa(kind, x):
    """max|x| / std per column (batch norm) or row (group norm), the worst of the case."""
    x = np.asarray(x, np.float64)
    ax = 0 if kind == "bn" else 1
    with np.errstate(divide="ignore"):
        return float(np.max(np.abs(x).max(ax) / x.std(ax)))


def reference(kind, M, C, cls, slope):
    """(inputs, forward, backward) of one case from the oracle."""
    c = make_case(kind, M, C, cls)
    if kind == "bn":
        fw = bn_forward(c["x"], c["gamma"], c["beta"], slope, running_mean=c["running_mean"], running_var=c["running_var"])
        return c, fw, bn_backward(fw, c["gamma"], c["dy"], slope)
    fw = gn_forward(c["x"], c["gamma"], c["beta"], slope)
    return c, fw, gn_backward(fw, c["gamma"], c["dy"], slope)


def norm_err(got, ref, floor=0.0):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if not ref.size:
        return 0.0
    return float(np.max(np.abs(got - ref))) / max(float(np.max(np.abs(ref))), floor, 1e-300)


# ------------------------------------------------------------------------------------------------ a small normalised MLP
def mlp_train_pass(kind, Ws, bs, gammas, betas, x, c, slope=0.01, running=None):
    """get_mlp(layer_normalization=kind) in training mode on one batch: Linear, norm + LeakyReLU, ..., Linear, objective sum(y c).
    Returns (y, dx, grads in named_parameters() order, running statistics per norm layer after the pass)."""
    L = len(Ws)
    h = np.asarray(x, np.float64)
    ins, fws = [], []
    new_running = []
    for l in range(L):
        ins.append(h)
        h = h @ np.asarray(Ws[l], np.float64).T + np.asarray(bs[l], np.float64)
        if l < L - 1:
            if kind == "bn":
                rm, rv = running[l] if running is not None else (None, None)
                fw = bn_forward(h, gammas[l], betas[l], slope, running_mean=rm, running_var=rv)
                if running is not None:
                    new_running.append((fw["running_mean"], fw["running_var"]))
            else:
                fw = gn_forward(h, gammas[l], betas[l], slope)
            fws.append(fw)
            h = fw["y"]
    y = h
    g = np.asarray(c, np.float64)
    grads = [None] * L
    for l in reversed(range(L)):
        if l < L - 1:
            bw = (bn_backward if kind == "bn" else gn_backward)(fws[l], gammas[l], g, slope)
            g = bw["dx"]
            norm_grads = [bw["dgamma"], bw["dbeta"]]
        else:
            norm_grads = []
        grads[l] = [g.T @ ins[l], g.sum(0)] + norm_grads
        g = g @ np.asarray(Ws[l], np.float64)
    return y, g, [a for layer in grads for a in layer], new_running


def mlp_eval(kind, Ws, bs, gammas, betas, x, slope=0.01, running=None):
    L = len(Ws)
    h = np.asarray(x, np.float64)
    for l in range(L):
        h = h @ np.asarray(Ws[l], np.float64).T + np.asarray(bs[l], np.float64)
        if l < L - 1:
            h = (bn_eval(h, gammas[l], betas[l], running[l][0], running[l][1], slope) if kind == "bn" else
                 gn_forward(h, gammas[l], betas[l], slope))["y"]
    return h


if __name__ == "__main__":      # seed search: prints the SEED_ATTEMPT entries the sweep needs
    found = {}
    SEED_ATTEMPT.clear()
    for kind in ("bn", "gn"):
        for (M, C) in (BN_SHAPES if kind == "bn" else GN_SHAPES):
            for cls in range(len(CLASSES)):
                for attempt in range(20000):
                    SEED_ATTEMPT[(kind, M, C, cls)] = attempt
                    _, fw, _ = reference(kind, M, C, cls, 0.01)
                    if left_out_fraction(kind, fw["z"], 0.01) <= MAX_LEFT_OUT and kappa(kind, make_case(kind, M, C, cls)["x"]) <= MAX_KAPPA:
                        break
                else:
                    raise SystemExit(f"no seed for {(kind, M, C, cls)}")
                if attempt:
                    found[(kind, M, C, cls)] = attempt
    print("SEED_ATTEMPT =", found)
