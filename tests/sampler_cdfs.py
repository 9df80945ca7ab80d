"""fp64 reference distributions of the latent samplers (cl_ica_amd/spaces.py, csrc/sampler.hip), written from the mathematics.

Every sampler kind has a one-dimensional statistic whose CDF is known in closed form or by one-dimensional quadrature:

    box uniform on [a, b)                       F(x) = (x - a) / (b - a)
    normal / Laplace / generalized normal       G(x) below; truncated to the box [a, b]: F(x) = (G(x) - G(a)) / (G(b) - G(a))
        normal(m, s)         G = (1 + erf((x - m) / (s sqrt 2))) / 2
        Laplace(m, s)        density exp(-|x - m| / s) / (2 s)   (the scale of torch.distributions.Laplace: variance 2 s^2)
        gen. normal(m, s, p) density prop. to exp(-(|x - m| / s)^p):  P(|x - m| / s <= t) = gammainc(1 / p, t^p), symmetric sign
                             (p = 1 is the Laplace, p = 2 is Normal(m, s / sqrt 2))
    sphere S^(n-1), angle theta to a pole       density prop. to sin^(n-2) theta                           (uniform)
                                                density prop. to exp(kappa (cos theta - 1)) sin^(n-2) theta  (von Mises-Fisher)
                                                projected normal normalize(mu + sigma eps): see `projected_normal_angle`

Angle distributions are tabulated over theta (smooth for every n >= 2, also where the density of w = cos theta is singular at +-1) on a
uniform grid over the part of [0, pi] that carries all but e^-50 of the mass, and interpolated linearly: `AngleTable`.  Everything is torch
float64 and runs on whichever device the argument lives on.

`ks_stat` is the exact one-sample Kolmogorov-Smirnov statistic; `BOUND` the bound on sqrt(N) D every comparison uses:
Dvoretzky-Kiefer-Wolfowitz / Massart, P(sqrt(N) D > lambda) <= 2 exp(-2 lambda^2) for every N, 2.7e-6 at lambda = 2.6.
"""
import math

import numpy as np
import torch

F64 = torch.float64
BOUND = 2.6


def _t(x, like=None):
    if torch.is_tensor(x):
        return x.to(F64)
    return torch.as_tensor(x, dtype=F64, device=None if like is None else like.device)


# ------------------------------------------------------------------------------------------------ box / R^n kinds
def g_normal(z):
    return 0.5 * (1.0 + torch.special.erf(z / math.sqrt(2.0)))


def g_laplace(z):
    h = 0.5 * torch.exp(-z.abs())
    return torch.where(z < 0, h, 1.0 - h)


def g_gennorm(z, p):
    a = torch.full_like(z, 1.0 / p)
    return 0.5 + 0.5 * torch.sign(z) * torch.special.gammainc(a, z.abs() ** p)


class LocationScale:
    """cdf of m + s e, e ~ unit normal / Laplace / generalized normal(p); truncated to [lo, hi] when a box is given.
    m and s are numbers: draws with per-coordinate scales are standardised before they are pooled."""

    def __init__(self, kind, m=0.0, s=1.0, p=None, box=None):
        assert kind in ("normal", "laplace", "gennorm") and (kind != "gennorm" or p)
        self.kind, self.m, self.s, self.p, self.box = kind, m, s, p, box

    def _g(self, x):
        z = (x - _t(self.m, x)) / _t(self.s, x)
        return g_normal(z) if self.kind == "normal" else g_laplace(z) if self.kind == "laplace" else g_gennorm(z, float(self.p))

    def cdf(self, x):
        x = _t(x)
        if self.box is None:
            return self._g(x)
        lo, hi = (torch.full_like(x, float(v)) for v in self.box)
        ga, gb = self._g(lo), self._g(hi)
        return ((self._g(x.clamp(lo, hi)) - ga) / (gb - ga)).clamp(0.0, 1.0)

    def two_sided_quantile(self, q):
        """t with P(|x - m| / s > t) = q (untruncated)."""
        if self.kind == "laplace":
            return -math.log(q)
        lo, hi = 0.0, 64.0
        for _ in range(200):      # bisection in fp64: the tail functions are monotone
            mid = 0.5 * (lo + hi)
            z = torch.tensor([mid], dtype=F64)
            if self.kind == "normal":
                tail = float(torch.special.erfc(z / math.sqrt(2.0)))
            else:
                tail = float(torch.special.gammaincc(torch.full_like(z, 1.0 / self.p), z ** self.p))
            lo, hi = (mid, hi) if tail > q else (lo, mid)
        return 0.5 * (lo + hi)


class BoxUniform:
    def __init__(self, lo, hi):
        self.lo, self.hi = float(lo), float(hi)

    def cdf(self, x):
        return ((_t(x) - self.lo) / (self.hi - self.lo)).clamp(0.0, 1.0)


# ------------------------------------------------------------------------------------------------ angle distributions
class AngleTable:
    """CDF of an angle theta in [0, pi] with unnormalised log density `logdens(theta)` (a float64 tensor function), by the cumulative
    trapezoid rule on `grid` + 1 uniform nodes over the window that holds all mass above e^-50 of the peak, linearly interpolated.
    Both errors are O(h^2): halving the grid bounds them (tests/test_sampler_cdfs_host.py)."""

    def __init__(self, logdens, grid=1 << 16, device="cpu"):
        coarse = torch.linspace(0.0, math.pi, 4097, dtype=F64, device=device)
        lc = logdens(coarse)
        lc = torch.where(torch.isfinite(lc), lc, torch.full_like(lc, -1e300))
        keep = torch.nonzero(lc > lc.max() - 50.0).flatten()
        step = math.pi / 4096
        self.lo = max(0.0, float(coarse[keep[0]]) - step)
        self.hi = min(math.pi, float(coarse[keep[-1]]) + step)
        th = torch.linspace(self.lo, self.hi, grid + 1, dtype=F64, device=device)
        ld = logdens(th)
        ld = torch.where(torch.isfinite(ld), ld, torch.full_like(ld, -1e300))
        d = torch.exp(ld - ld.max())
        c = torch.cumsum(0.5 * (d[1:] + d[:-1]), 0)
        self.F = torch.cat([torch.zeros(1, dtype=F64, device=device), c]) / c[-1]
        self.grid, self.h = grid, (self.hi - self.lo) / grid

    def cdf_angle(self, theta):
        """P(angle <= theta)."""
        theta = _t(theta)
        F = self.F.to(theta.device)
        u = ((theta - self.lo) / self.h).clamp(0.0, float(self.grid))
        i = u.floor().clamp(max=self.grid - 1).to(torch.int64)
        f = u - i.to(F64)
        return F[i] * (1.0 - f) + F[i + 1] * f

    def cdf(self, w):
        """P(cos(angle) <= w)."""
        return 1.0 - self.cdf_angle(torch.acos(_t(w).clamp(-1.0, 1.0)))


def _logsin(theta, k):
    return k * torch.log(torch.sin(theta).clamp_min(1e-300)) if k else torch.zeros_like(theta)


def vmf_logdens(n, kappa):
    """theta = angle(x, mu), x ~ vMF(mu, kappa) on S^(n-1); kappa = 0 is the uniform distribution (any coordinate's marginal).
    The peak value kappa is subtracted first so that kappa = 1e4 stays in range."""
    return lambda th: kappa * (torch.cos(th) - 1.0) + _logsin(th, n - 2)


def vmf_angle(n, kappa, grid=1 << 16, device="cpu"):
    return AngleTable(vmf_logdens(n, kappa), grid, device)


def sphere_uniform_angle(n, grid=1 << 16, device="cpu"):
    return AngleTable(vmf_logdens(n, 0.0), grid, device)


def projected_normal_logdens(n, sigma, nodes=256):
    """theta = angle(mu + sigma eps, mu), |mu| = 1, eps ~ N(0, I_n).  With a = 1 + sigma g along mu and the orthogonal radius
    r = sigma chi_{n-1}, in polar coordinates (a, r) = rho (cos theta, sin theta) the density of theta is
        sin^(n-2) theta  int_0^inf rho^(n-1) exp(-(rho^2 - 2 rho cos theta + 1) / (2 sigma^2)) d rho
    up to a constant: an analytic integrand, Gauss-Legendre over rho in [0, 1 + sigma (sqrt n + 12)] (the trapezoid rule would
    carry the end-point term of rho^(n-1) at rho = 0 for small n)."""
    top = 1.0 + sigma * (math.sqrt(n) + 12.0)
    xs, ws = np.polynomial.legendre.leggauss(nodes)

    def f(th):
        rho = torch.as_tensor(0.5 * top * (xs + 1.0), dtype=F64, device=th.device)
        lw = torch.log(torch.as_tensor(0.5 * top * ws, dtype=F64, device=th.device))
        e = (n - 1) * torch.log(rho)[None, :] - (rho[None, :] ** 2 - 2.0 * rho[None, :] * torch.cos(th)[:, None] + 1.0) / (2.0 * sigma * sigma)
        return torch.logsumexp(e + lw[None, :], 1) + _logsin(th, n - 2)

    def chunked(th):
        return torch.cat([f(c) for c in th.split(4096)])
    return chunked


def projected_normal_angle(n, sigma, grid=1 << 15, device="cpu"):
    return AngleTable(projected_normal_logdens(n, sigma), grid, device)


def projected_normal_cdf_w(t, n, sigma, nodes=1 << 17):
    """P(w <= t), w = <normalize(mu + sigma eps), mu>, by the other route: condition on g (a = 1 + sigma g), r^2 = sigma^2 chi^2_{n-1}:
        t > 0:  E_g[ 1{a <= 0} + 1{a > 0} Q((n-1)/2, a^2 (1 - t^2) / (2 sigma^2 t^2)) ]
        t < 0:  E_g[ 1{a < 0} P((n-1)/2, a^2 (1 - t^2) / (2 sigma^2 t^2)) ]
    trapezoid rule over g in [-10, 10].  Used to cross-check the table at a few t (not near t = 0, where the integrand turns into a step)."""
    g = torch.linspace(-10.0, 10.0, nodes + 1, dtype=F64)
    wgt = torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi) * (20.0 / nodes)
    wgt[0] *= 0.5; wgt[-1] *= 0.5
    a = 1.0 + sigma * g
    x = a * a * (1.0 - t * t) / (2.0 * sigma * sigma * t * t)
    k = torch.full_like(x, 0.5 * (n - 1))
    if t > 0:
        v = torch.where(a <= 0, torch.ones_like(x), torch.special.gammaincc(k, x))
    else:
        v = torch.where(a < 0, torch.special.gammainc(k, x), torch.zeros_like(x))
    return float((wgt * v).sum())


def angle_between(x, mu):
    """Angle between unit vectors in float64 from the chord, theta = 2 asin(|x - mu| / 2): accurate where 1 - <x, mu> drowns in the
    rounding of float32 coordinates (a concentrated conditional: theta^2 / 2 below 6e-8 is an atom at w = 1 otherwise)."""
    d = (x.to(F64) - mu.to(F64)).norm(dim=-1)
    return 2.0 * torch.asin((0.5 * d).clamp(max=1.0))


class Empirical:
    """CDF of a reference SAMPLE (fp64 simulation); compare with the two-sample size N N2 / (N + N2)."""

    def __init__(self, sample):
        self.s = torch.sort(_t(sample).flatten()).values

    def cdf(self, x):
        x = _t(x)
        return torch.searchsorted(self.s.to(x.device), x.contiguous(), right=True).to(F64) / self.s.numel()


def projected_laplace_sim(mu, scale, size, seed=0, chunk=1 << 20):
    """w = <normalize(mu + scale e), mu>, e ~ iid unit Laplace: numpy float64 simulation (the Laplace noise is not rotation invariant,
    the distribution depends on mu's direction)."""
    rng = np.random.default_rng(seed)
    mu = np.asarray(mu, np.float64)
    out = np.empty(size, np.float64)
    for lo in range(0, size, chunk):
        m = min(chunk, size - lo)
        v = mu[None, :] + scale * rng.laplace(size=(m, mu.size))
        out[lo:lo + m] = (v @ mu) / np.linalg.norm(v, axis=1)
    return out


# ------------------------------------------------------------------------------------------------ statistics
def ks_stat(sample, cdf):
    """Exact one-sample statistic D = max(max_i(i / N - F(x_(i))), max_i(F(x_(i)) - (i - 1) / N)); `sample` a tensor on either device."""
    x = torch.sort(_t(sample).flatten()).values
    N = x.numel()
    F = cdf(x)
    i = torch.arange(1, N + 1, dtype=F64, device=x.device)
    return float(torch.maximum((i / N - F).max(), (F - (i - 1.0) / N).max()))


def ks_scaled(sample, cdf, n_ref=None):
    """sqrt(N_eff) D; N_eff = N N2 / (N + N2) against a reference sample of size n_ref."""
    N = sample.numel()
    Ne = N if n_ref is None else N * n_ref / (N + n_ref)
    return math.sqrt(Ne) * ks_stat(sample, cdf)


def corr(a, b):
    a = _t(a).flatten(); b = _t(b).flatten()
    a = a - a.mean(); b = b - b.mean()
    return float((a * b).sum() / torch.sqrt((a * a).sum() * (b * b).sum()))
