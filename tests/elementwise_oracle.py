"""NumPy fp64 restatements of the small stand-alone kernels: Adam (csrc/adam.hip, adam_math.h), the output heads and the stand-alone
LeakyReLU (csrc/heads.hip) and the mixing net with its four hidden activations (csrc/mixing.hip), plus the seeded inputs the host and
the GPU tests share.

    Adam      m' = b1 m + (1 - b1) g s ;  v' = b2 v + (1 - b2) (g s)^2 ;  p' = p - (lr / (1 - b1^t)) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)
              with lr, b1, b2, eps and s = grad_scale AS THE C ABI RECEIVES THEM (fp32 values), the complements taken from those values
    Rescale   y = r x / |x|               dx = r (dy - u <dy, u>) / |x|, u = x / |x| ;  dr = sum_i <dy_i, u_i>        (layers.py:63-66)
    Softclip  y = sigmoid(x) bound        dx = dy bound s (1 - s) ;  dbound_k = sum_i dy_ik s_ik                      (layers.py:87-91)
    LeakyReLU y = x > 0 ? x : a x         dx = y > 0 ? dy : a dy  (the gate is recovered from the saved output)
    Mixing    x = W_L phi(... phi(W_1 z)), phi by kind (invertible_network_utils.py:44-66):
              0 LeakyReLU(a), 1 ELU(alpha = a), 2 SmoothLeakyReLU a v + (1 - a) log(1 + e^v), 3 Softplus(beta = a, threshold 20)
Every function takes logical (M, n) arrays -- strided views of a padded buffer are fine; `padded` / `logical` build and read such buffers.
"""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)      # 2^-23


def f32(x):
    """A Python / NumPy scalar as the C ABI's `float` argument holds it."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------------------------ Adam
def adam_consts(t, lr, b1, b2):
    """(lr / (1 - b1^t), 1 / sqrt(1 - b2^t)) in fp64 from the fp32 scalars."""
    lr, b1, b2 = f32(lr), f32(b1), f32(b2)
    t = float(t)
    return lr / (1.0 - b1 ** t), 1.0 / np.sqrt(1.0 - b2 ** t)


def adam_delta(m_new, v_new, t, lr, b1, b2, eps):
    """The parameter step p - p' in fp64, given the NEW moments."""
    step_size, inv_bc2_sqrt = adam_consts(t, lr, b1, b2)
    m_new = np.asarray(m_new, np.float64); v_new = np.asarray(v_new, np.float64)
    return step_size * m_new / (np.sqrt(v_new) * inv_bc2_sqrt + f32(eps))


def adam_update(p, g, m, v, t, lr, b1, b2, eps, grad_scale):
    """One update number t (1-based) from an arbitrary state.  Returns (m', v', p', summands) with
    summands = |b1 m| + |(1 - b1) g s|: the size of the two terms m' is the sum of."""
    b1_, b2_, s = f32(b1), f32(b2), f32(grad_scale)
    p = np.asarray(p, np.float64); g = np.asarray(g, np.float64); m = np.asarray(m, np.float64); v = np.asarray(v, np.float64)
    gr = g * s
    m_new = b1_ * m + (1.0 - b1_) * gr
    v_new = b2_ * v + (1.0 - b2_) * gr * gr
    p_new = p - adam_delta(m_new, v_new, t, lr, b1, b2, eps)
    return m_new, v_new, p_new, np.abs(b1_ * m) + np.abs((1.0 - b1_) * gr)


# (b1, b2, eps, grad_scale, lr): torch's defaults, the engine's 1 / B gradient scale, a coarse set, no first moment, slow moments at lr 1
ADAM_COMBOS = [(0.9, 0.999, 1e-8, 1.0, 1e-3), (0.9, 0.999, 1e-8, 1.0 / 6144.0, 1e-4), (0.5, 0.9, 1e-3, 3.0, 1e-2), (0.0, 0.99, 1e-8, 1.0, 1e-3),
               (0.99, 0.9999, 1e-12, 1.0, 1.0)]
ADAM_TS = [1, 2, 3, 10, 100, 1000, 10 ** 4, 10 ** 5, 2 * 10 ** 6]
ADAM_M_LIMIT, ADAM_V_LIMIT, ADAM_P_LIMIT = 2.0, 3.0, 4.0      # in units of EPS32: the number of roundings of each formula plus one
ADAM_V_TINY = 1e-37                                           # below it v' is held absolutely (the fp32 denormal range starts at 1.18e-38)


def adam_state(combo, t, count):
    """Seeded (p, g, m, v) in fp32: gradients = normal draws times 10^U(-15, 15) with 100 exact zeros, m and v within 10^+-2 of |g| and g^2
    (or, where g = 0, of a scale of their own) with 50 exact zeros, which sit where g = 0 as well."""
    rng = np.random.default_rng([11, combo, t])
    scale = 10.0 ** rng.uniform(-15, 15, size=count)
    g = rng.normal(size=count) * scale
    g[:100] = 0.0
    base = np.where(g == 0.0, scale, np.abs(g))
    m = np.where(rng.random(count) < 0.5, -1.0, 1.0) * base * 10.0 ** rng.uniform(-2, 2, size=count)
    v = base * base * 10.0 ** rng.uniform(-2, 2, size=count)
    m[50:100] = 0.0; v[50:100] = 0.0
    p = rng.normal(size=count)
    return p.astype(np.float32), g.astype(np.float32), m.astype(np.float32), v.astype(np.float32)


def adam_errors(got_m, got_v, got_p, p, g, m, v, t, combo):
    """The three figures of one update in units of EPS32 (worst element each), and the number of g = m = v = 0 elements whose parameter
    changed.  The p figure is taken against the fp64 step formed from the GOT moments, after half an ulp of the got parameter."""
    b1, b2, eps, gs, lr = combo
    m_ref, v_ref, _, summ = adam_update(p, g, m, v, t, lr, b1, b2, eps, gs)
    got_m64 = np.asarray(got_m, np.float64); got_v64 = np.asarray(got_v, np.float64); got_p64 = np.asarray(got_p, np.float64)
    with np.errstate(all="ignore"):
        em = np.abs(got_m64 - m_ref) / (EPS32 * summ)
        em = np.where(summ > 0, em, np.where(got_m64 == m_ref, 0.0, np.inf))
        big = v_ref >= ADAM_V_TINY
        ev = np.where(big, np.abs(got_v64 - v_ref) / (EPS32 * np.where(big, v_ref, 1.0)), 0.0)
        ev_tiny = np.where(big, 0.0, np.abs(got_v64 - v_ref))
        delta = adam_delta(got_m, got_v, t, lr, b1, b2, eps)
        over = np.abs(got_p64 - (np.asarray(p, np.float64) - delta)) - 0.5 * np.spacing(np.abs(np.asarray(got_p, np.float32))).astype(np.float64)
        ep = np.where(over > 0, over / (EPS32 * np.abs(delta)), 0.0)
        ep = np.where((over > 0) & (delta == 0), np.inf, ep)
    zero = (np.asarray(g) == 0) & (np.asarray(m) == 0) & (np.asarray(v) == 0)
    moved = int((np.asarray(got_p, np.float32).view(np.uint32)[zero] != np.asarray(p, np.float32).view(np.uint32)[zero]).sum())
    return dict(m=float(em.max()), v=float(ev.max()), v_tiny=float(ev_tiny.max()), p=float(ep.max()), n_zero=int(zero.sum()), moved=moved)


def adam_fp32_emulation(p, g, m, v, t, lr, b1, b2, eps, grad_scale):
    """adam_math.h::update operation by operation in NumPy fp32 (consts_of in fp64, rounded once); fmaf = fp64 product-sum rounded once to
    fp32 (the product of two fp32 numbers is exact in fp64).  Returns (m', v', p') in fp32."""
    F = np.float32
    lr, b1, b2, eps, s = F(lr), F(b1), F(b2), F(eps), F(grad_scale)
    step_size, inv_bc2_sqrt = adam_consts(t, lr, b1, b2)
    step_size, inv_bc2_sqrt = F(step_size), F(inv_bc2_sqrt)

    def fma(a, b, c):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)

    with np.errstate(all="ignore"):
        p = np.asarray(p, F); g = np.asarray(g, F); m = np.asarray(m, F); v = np.asarray(v, F)
        gr = g * s
        m_new = fma(b1, m, (F(1) - b1) * gr)
        v_new = fma(b2, v, ((F(1) - b2) * gr) * gr)
        denom = fma(np.sqrt(v_new), inv_bc2_sqrt, eps)
        p_new = p - (step_size * m_new) / denom
    assert m_new.dtype == v_new.dtype == p_new.dtype == F
    return m_new, v_new, p_new


def adam_trajectory_grads(count=4099, steps=200, seed=5):
    """The gradients of the 200-step trajectory: a per-element scale 10^U(-6, 2) times a normal draw that changes every step."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-6, 2, size=count)
    p0 = rng.normal(size=count).astype(np.float32)
    return p0, [(rng.normal(size=count) * scale).astype(np.float32) for _ in range(steps)]


def adam_trajectory_torch(p0, grads, dtype, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam on the CPU in `dtype`: (p, exp_avg, exp_avg_sq) after the last step, as float64 arrays."""
    import torch
    prm = torch.nn.Parameter(torch.tensor(np.asarray(p0, np.float64), dtype=dtype))
    opt = torch.optim.Adam([prm], lr=lr, betas=betas, eps=eps)
    for g in grads:
        prm.grad = torch.tensor(np.asarray(g, np.float64), dtype=dtype)
        opt.step()
    st = opt.state[prm]
    return tuple(x.detach().double().numpy() for x in (prm, st["exp_avg"], st["exp_avg_sq"]))


def beta2_complement_gap(b2):
    """|fl32(1 - b2) - (1 - fl32(b2))| / (1 - b2): how far the (1 - beta2) of an ABI that takes fp32 betas is from the one torch.optim.Adam
    multiplies a float32 state by.  1.29e-5 at 0.999, 0 where b2 is an fp32 number."""
    return abs(f32(1.0 - b2) - (1.0 - f32(b2))) / (1.0 - b2)


# ------------------------------------------------------------------------------------------------------------------ buffers
def padded(a, ld, extra_rows=0, fill=-0.0):
    """An fp32 buffer [M + extra_rows, ld] pre-filled with `fill` (default -0.0: a kernel that writes +0.0 or anything else into the
    padding changes its bits) holding the (M, n) array `a` in its leading columns."""
    a = np.asarray(a, np.float32)
    M, n = a.shape
    assert ld >= n
    buf = np.full((M + extra_rows, ld), fill, np.float32)
    buf[:M, :n] = a
    return buf


def padding_bits(buf, M, n):
    """The bits of everything in `buf` outside its leading (M, n) block."""
    buf = np.asarray(buf, np.float32)
    mask = np.ones(buf.shape, bool)
    mask[:M, :n] = False
    return buf.view(np.uint32)[mask]


# ------------------------------------------------------------------------------------------------------------------ heads
def rescale_fwd(x, r):
    """(y, inv_norm): y = r x / |x|, inv_norm = 1 / |x| per row."""
    x = np.asarray(x, np.float64)
    inv = 1.0 / np.sqrt((x * x).sum(-1))
    return x * inv[:, None] * float(r), inv


def rescale_bwd(x, r, dy):
    """(dx, dr, dx_floor, dr_floor).  dx_floor = max r |dy_ik| / |x_i|: the size of the terms dx is a difference of;
    dr_floor = sum_i |<dy_i, u_i>|."""
    x = np.asarray(x, np.float64); dy = np.asarray(dy, np.float64)
    inv = 1.0 / np.sqrt((x * x).sum(-1, keepdims=True))
    u = x * inv
    dot = (dy * u).sum(-1, keepdims=True)
    dx = float(r) * (dy - u * dot) * inv
    return dx, float(dot.sum()), float((abs(float(r)) * np.abs(dy) * inv).max()), float(np.abs(dot).sum())


def sigmoid(x):
    x = np.asarray(x, np.float64)
    return np.exp(-np.logaddexp(0.0, -x))


def softclip_fwd(x, bound):
    return sigmoid(x) * np.asarray(bound, np.float64)[None, :]


def softclip_bwd(x, bound, dy):
    """(dx, dbound, dbound_floor) with dbound_floor_k = sum_i |dy_ik s_ik|."""
    dy = np.asarray(dy, np.float64)
    s = sigmoid(x)
    return dy * np.asarray(bound, np.float64)[None, :] * s * (1.0 - s), (dy * s).sum(0), np.abs(dy * s).sum(0)


def leaky_fwd(x, slope):
    x = np.asarray(x, np.float64)
    return np.where(x > 0, x, float(slope) * x)


def leaky_bwd(y, dy, slope):
    dy = np.asarray(dy, np.float64)
    return np.where(np.asarray(y) > 0, dy, float(slope) * dy)


# ------------------------------------------------------------------------------------------------------------------ mixing net
MIX_KINDS = {"leaky_relu": 0, "elu": 1, "smooth_leaky_relu": 2, "softplus": 3}


def mix_act(v, kind, a):
    v = np.asarray(v, np.float64); a = float(a)
    with np.errstate(over="ignore"):
        if kind == 0:
            return np.where(v > 0, v, a * v)
        if kind == 1:
            return np.where(v > 0, v, a * np.expm1(np.minimum(v, 0.0)))
        if kind == 2:
            return a * v + (1.0 - a) * np.logaddexp(0.0, v)
        if kind == 3:
            return np.where(a * v > 20.0, v, np.logaddexp(0.0, a * v) / a)
    raise ValueError(f"activation kind {kind}")


def mixing_forward(Ws, z, act_kind, a, pre=None):
    """x = W_L phi(... phi(W_1 z)) in fp64; `pre` (a list) receives the pre-activations of the hidden layers."""
    x = np.asarray(z, np.float64)
    for l, W in enumerate(Ws):
        x = x @ np.asarray(W, np.float64).T
        if l < len(Ws) - 1:
            if pre is not None:
                pre.append(x)
            x = mix_act(x, act_kind, a)
    return x


def mixing_weights(z, n_layers, act_kind, a, target, seed):
    """[L, n, n] fp32: orthogonal matrices times a gain per layer, chosen on the rows `z` so that the largest pre-activation of every
    hidden layer (and the largest output) is `target` in absolute value."""
    rng = np.random.default_rng(seed)
    x = np.asarray(z, np.float64)
    n = x.shape[1]
    Ws = []
    for l in range(n_layers):
        q, rr = np.linalg.qr(rng.normal(size=(n, n)))
        q = q * np.sign(np.diag(rr))[None, :]
        top = float(np.abs(x @ q.T).max())
        W = (q * (target / top if top > 0 else 1.0)).astype(np.float32)
        Ws.append(W)
        x = x @ W.astype(np.float64).T
        if l < n_layers - 1:
            x = mix_act(x, act_kind, a)
    return np.stack(Ws)


def mixing_lds_bytes(n, n_layers):
    rows = min(max(256 // n, 1), 64)
    return 4 * (n_layers * n * n + 2 * rows * n), rows
