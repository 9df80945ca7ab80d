"""The flat SGD update (csrc/sgd.hip, include/clica.h "SGD") twice over in NumPy, plus the seeded inputs the host and the GPU tests share.

    gr = g s  (negated for maximize) ;  gr += wd p  (wd != 0)
    momentum != 0:  buf = gr  (t == 0)  |  momentum buf + (1 - dampening) gr ;   d = gr + momentum buf  (nesterov)  |  buf
    momentum == 0:  d = gr
    p' = p - lr d

`sgd_update` is the fp64 restatement; with `abi=True` the scalars are the fp32 values the C ABI receives (and 1 - dampening the fp32
difference the library forms), with `abi=False` they are the Python doubles torch.optim.SGD computes with.  `sgd_fp32_emulation` is the
documented operation sequence, one NumPy float32 operation per line: the kernel's exact expectation.

Distance of one emulated update from the fp64 update OF THE SAME fp32 STATE, counted from the roundings (u = EPS32 / 2 per rounding,
G = |g s| + |wd p| the terms gr is the sum of):
    gr      one rounding of g s, one of wd p, one of their sum                       <= 2 u G
    buf     t == 0: buf = gr                                                          <= 2 u G
            t  > 0: a, b, a + b round once each and b carries gr's error              <= 4 u Bm,  Bm = |momentum buf| + |1 - dampening| G
    d       plain: gr; momentum: buf; nesterov: c = momentum buf' rounds, gr + c rounds, and both operands carry their errors
                                                                                      <= 6 u D,   D = G | Bm | G + |momentum| Bm
    p'      lr d rounds once (u lr |d| <= u lr D), the subtraction rounds to half an ulp of the result
                                                                                      <= ulp(p') / 2 + 7 u lr D
so  |buf_emu - buf_64| <= SGD_BUF_LIMIT EPS32 Bm  and  |p_emu - p_64| <= ulp(|p'|) / 2 + SGD_P_LIMIT EPS32 lr D, with a relative 1e-6 on top
for the second-order terms and 2^-147 for products that land in the denormal range.
"""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
SGD_BUF_LIMIT, SGD_P_LIMIT = 2.0, 3.5
SGD_TINY = 2.0 ** -147

# name -> options.  The scalars are NOT fp32 numbers on purpose (0.9, 1e-2, 0.1): the ABI rounds them
SGD_OPTION_SETS = {
    "plain": dict(lr=0.1),
    "momentum": dict(lr=0.1, momentum=0.9),
    "dampening": dict(lr=0.1, momentum=0.9, dampening=0.5),
    "nesterov": dict(lr=0.1, momentum=0.9, nesterov=True),
    "momentum_wd": dict(lr=0.1, momentum=0.9, weight_decay=1e-2),
    "wd_maximize": dict(lr=0.1, weight_decay=1e-2, maximize=True),
    "grad_scale": dict(lr=0.1, momentum=0.9, grad_scale=0.5),
}
_DEFAULTS = dict(lr=0.1, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False, grad_scale=1.0)


def options(name_or_dict):
    o = dict(_DEFAULTS)
    o.update(SGD_OPTION_SETS[name_or_dict] if isinstance(name_or_dict, str) else name_or_dict)
    return o


def f32(x):
    return float(np.float32(x))


def scalars(o, abi):
    """(lr, momentum, 1 - dampening, weight_decay, grad_scale) as doubles: the ABI's fp32 values or the Python values."""
    o = options(o)
    if abi:
        return f32(o["lr"]), f32(o["momentum"]), float(np.float32(1) - np.float32(o["dampening"])), f32(o["weight_decay"]), f32(o["grad_scale"])
    return float(o["lr"]), float(o["momentum"]), 1.0 - float(o["dampening"]), float(o["weight_decay"]), float(o["grad_scale"])


def sgd_update(p, g, buf, t, o, abi=True):
    """Update number t (0-based: t updates were applied before) in fp64.  Returns (p', buf', D, Bm): D and Bm are the term sizes the
    error bounds are stated in (Bm is None without a momentum)."""
    o = options(o)
    lr, mom, omd, wd, s = scalars(o, abi)
    p = np.asarray(p, np.float64); g = np.asarray(g, np.float64)
    gr = g * s
    if o["maximize"]:
        gr = -gr
    G = np.abs(gr)
    if wd != 0:
        gr = gr + wd * p
        G = G + np.abs(wd * p)
    if mom == 0:
        return p - lr * gr, None, G, None
    if t == 0:
        buf_new, Bm = gr, G
    else:
        buf = np.asarray(buf, np.float64)
        buf_new = mom * buf + omd * gr
        Bm = np.abs(mom * buf) + abs(omd) * G
    if o["nesterov"]:
        d, D = gr + mom * buf_new, G + abs(mom) * Bm
    else:
        d, D = buf_new, Bm
    return p - lr * d, buf_new, D, Bm


def sgd_fp32_emulation(p, g, buf, t, o):
    """The operation sequence of include/clica.h, one float32 operation per line.  Returns (p', buf') in fp32 (buf' None without momentum)."""
    F = np.float32
    o = options(o)
    lr, mom, damp, wd, s = F(o["lr"]), F(o["momentum"]), F(o["dampening"]), F(o["weight_decay"]), F(o["grad_scale"])
    omd = F(1) - damp
    with np.errstate(all="ignore"):
        p = np.asarray(p, F); g = np.asarray(g, F)
        gr = g * s
        if o["maximize"]:
            gr = -gr
        if wd != 0:
            wp = wd * p
            gr = gr + wp
        buf_new = None
        if mom != 0:
            if t == 0:
                buf_new = gr.copy()
            else:
                a = mom * np.asarray(buf, F)
                b = omd * gr
                buf_new = a + b
            if o["nesterov"]:
                c = mom * buf_new
                d = gr + c
            else:
                d = buf_new
        else:
            d = gr
        u = lr * d
        p_new = p - u
    assert p_new.dtype == F and d.dtype == F and (buf_new is None or buf_new.dtype == F)
    return p_new, buf_new


def sgd_errors(got_p, got_buf, p, g, buf, t, o):
    """The two figures of one update from the fp32 state (p, g, buf), worst element each: the distance of got_p from the fp64 p' beyond
    half an ulp of got_p, in units of EPS32 lr D, and the distance of got_buf from the fp64 buf' in units of EPS32 Bm."""
    lr = scalars(o, True)[0]
    p_ref, buf_ref, D, Bm = sgd_update(p, g, buf, t, o, abi=True)
    got_p64 = np.asarray(got_p, np.float64)
    half_ulp = 0.5 * np.spacing(np.abs(np.asarray(got_p, np.float32))).astype(np.float64)
    over = np.abs(got_p64 - p_ref) - half_ulp - SGD_TINY
    with np.errstate(all="ignore"):
        ep = np.where(over > 0, over / (EPS32 * lr * D * (1 + 1e-6)), 0.0)
        ep = np.where((over > 0) & (D == 0), np.inf, ep)
        eb = 0.0
        if buf_ref is not None:
            overb = np.abs(np.asarray(got_buf, np.float64) - buf_ref) - SGD_TINY
            eb = np.where(overb > 0, overb / (EPS32 * Bm * (1 + 1e-6)), 0.0)
            eb = np.where((overb > 0) & (Bm == 0), np.inf, eb)
            eb = float(eb.max())
    return dict(p=float(ep.max()), buf=eb)


def sgd_inputs(count=4099, steps=6, seed=7):
    """(p0, [g_0 .. g_{steps-1}]) in fp32: N(0, 1) parameters and injected N(0, 1) gradients, with a few exact zeros in both."""
    rng = np.random.default_rng([seed, count])
    p0 = rng.normal(size=count).astype(np.float32)
    grads = [rng.normal(size=count).astype(np.float32) for _ in range(steps)]
    k = min(3, count)
    p0[:k] = 0.0
    for g in grads:
        g[count - k:] = 0.0
    return p0, grads


def emulate_steps(p0, grads, o, buf=None, t0=0):
    """The emulation over consecutive updates from t0.  Returns the list of (p, buf) after each update."""
    out, p = [], np.asarray(p0, np.float32)
    for k, g in enumerate(grads):
        p, buf = sgd_fp32_emulation(p, g, buf, t0 + k, o)
        out.append((p, buf))
    return out


def torch_trajectory(p0, grads, o, dtype):
    """torch.optim.SGD on the CPU in `dtype`: (p, momentum_buffer or None) after the last step, as float64 arrays.  grad_scale is
    applied to the injected gradient (the ABI's own argument; torch has none)."""
    import torch
    o = options(o)
    prm = torch.nn.Parameter(torch.tensor(np.asarray(p0, np.float64), dtype=dtype))
    opt = torch.optim.SGD([prm], lr=o["lr"], momentum=o["momentum"], dampening=o["dampening"], weight_decay=o["weight_decay"],
                          nesterov=o["nesterov"], maximize=o["maximize"])
    for g in grads:
        prm.grad = torch.tensor(np.asarray(g, np.float64) * o["grad_scale"], dtype=dtype)
        opt.step()
    b = opt.state[prm].get("momentum_buffer") if prm in opt.state else None
    return prm.detach().double().numpy(), None if b is None else b.detach().double().numpy()
