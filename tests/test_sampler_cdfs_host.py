"""tests/sampler_cdfs.py is right: every reference CDF against the same construction drawn in numpy float64 by an independent route
(Generator.gamma for the generalized normal, truncation by discarding, accept-reject on the angle's own density for vMF -- not Wood's
algorithm), inside the bound the GPU tests use (sqrt(N) D < 2.6, Dvoretzky-Kiefer-Wolfowitz: 2.7e-6 per comparison).  The quadrature
tables are shown to be exact to 1e-6 (thresholds are >= 2.5e-3) by halving their grids.  No GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

import sampler_cdfs as S

N = 1 << 20
PS = (0.5, 1.0, 2.0, 3.0, 8.0)


def _check(name, sample, cdf, n_ref=None):
    v = S.ks_scaled(torch.as_tensor(np.asarray(sample, np.float64)), cdf, n_ref)
    print(f"{name}: sqrt(N) D = {v:.3f}")
    assert v < S.BOUND, (name, v)
    return v


def _noise(rng, kind, p, size):
    if kind == "normal":
        return rng.standard_normal(size)
    if kind == "laplace":
        return rng.laplace(size=size)
    return rng.gamma(1.0 / p, size=size) ** (1.0 / p) * rng.choice([-1.0, 1.0], size=size)


KINDS = [("normal", None), ("laplace", None)] + [("gennorm", p) for p in PS]


def test_ks_stat_is_the_exact_statistic():
    x = torch.tensor([0.1, 0.4, 0.35, 0.8], dtype=torch.float64)
    # sorted 0.1 0.35 0.4 0.8 against F(x) = x: i/N - F = .15 .15 .35 .2 ; F - (i-1)/N = .1 .1 -.1 .05
    assert abs(S.ks_stat(x, lambda t: t) - 0.35) < 1e-15
    assert abs(S.ks_stat(x.to(torch.float32), lambda t: t) - 0.35) < 1e-7
    # a 1 % error in a normal's scale is at the bound for N = 2^20 (the sensitivity the GPU tests quote)
    rng = np.random.default_rng(0)
    v = S.ks_scaled(torch.as_tensor(1.01 * rng.standard_normal(N)), S.LocationScale("normal").cdf)
    print(f"normal x 1.01: sqrt(N) D = {v:.3f}")
    assert v > 2.0
    e = S.Empirical(torch.tensor([1.0, 2.0, 3.0, 4.0]))
    assert e.cdf(torch.tensor([0.5, 1.0, 2.5, 4.0, 5.0])).tolist() == [0.0, 0.25, 0.5, 1.0, 1.0]


def test_box_uniform():
    rng = np.random.default_rng(1)
    for lo, hi in ((0.0, 1.0), (-1.0, 1.0)):
        _check(f"box uniform [{lo}, {hi})", lo + (hi - lo) * rng.random(N), S.BoxUniform(lo, hi).cdf)


@pytest.mark.parametrize("kind,p", KINDS)
def test_location_scale_untruncated(kind, p):
    rng = np.random.default_rng(2)
    for s in (1e-3, 2.0):
        _check(f"real {kind} p={p} s={s}", 0.25 + s * _noise(rng, kind, p, N), S.LocationScale(kind, 0.25, s, p).cdf)
    # per-coordinate scales: each column against its own scale, and the standardised columns pooled against the unit CDF
    sv = np.array([0.03, 3.0])
    x = sv[None, :] * _noise(rng, kind, p, (N // 2, 2))
    for k in range(2):
        _check(f"real {kind} p={p} scale vector, column {k}", x[:, k], S.LocationScale(kind, 0.0, sv[k], p).cdf)
    _check(f"real {kind} p={p} scale vector, standardised", x / sv[None, :], S.LocationScale(kind, p=p).cdf)


@pytest.mark.parametrize("kind,p", KINDS)
def test_location_scale_truncated_by_discarding(kind, p):
    rng = np.random.default_rng(3)
    lo, hi = 0.0, 1.0
    for m in (0.5, 0.02, lo, hi):
        for s in (0.05, 1.0, 5.0):
            x = np.empty(0)
            while x.size < N // 4:
                c = m + s * _noise(rng, kind, p, N)
                x = np.concatenate([x, c[(c >= lo) & (c <= hi)]])
            _check(f"box {kind} p={p} m={m} s={s}", x[:N // 4], S.LocationScale(kind, m, s, p, box=(lo, hi)).cdf)


def test_gennorm_identities_and_laplace_scale():
    x = torch.linspace(-6.0, 6.0, 4001, dtype=torch.float64)
    assert float((S.LocationScale("gennorm", 0.3, 0.7, 1.0).cdf(x) - S.LocationScale("laplace", 0.3, 0.7).cdf(x)).abs().max()) < 1e-14
    assert float((S.LocationScale("gennorm", 0.3, 0.7, 2.0).cdf(x) - S.LocationScale("normal", 0.3, 0.7 / math.sqrt(2.0)).cdf(x)).abs().max()) < 1e-14
    # Laplace(m, s) has variance 2 s^2 (the convention of the recorded reference statistics: scale 0.7 -> variance 0.98)
    d = S.LocationScale("laplace", 0.0, 0.7)
    xs = torch.linspace(-30.0, 30.0, 600001, dtype=torch.float64)
    pdf = torch.diff(d.cdf(xs)); mid = 0.5 * (xs[1:] + xs[:-1])
    assert abs(float((pdf * mid * mid).sum()) - 2 * 0.49) < 1e-6
    for kind, p, q, want in (("normal", None, 1e-4, 3.8905919), ("laplace", None, 1e-5, 11.5129255)):
        assert abs(S.LocationScale(kind, p=p).two_sided_quantile(q) - want) < 1e-6
    t = S.LocationScale("gennorm", p=3.0).two_sided_quantile(1e-4)
    assert abs(float(torch.special.gammaincc(torch.tensor([1 / 3], dtype=torch.float64), torch.tensor([t ** 3], dtype=torch.float64))) - 1e-4) < 1e-12


def test_recorded_laplace_statistics_use_this_scale(golden):
    """The reference's 1e5 R^n Laplace draws at lbd = 0.7 (tests/golden/g9_samplers.npz): their quantiles sit on Laplace(0, 0.7)'s CDF."""
    z9 = golden("g9_samplers.npz").z
    qs = torch.tensor(z9["quantiles"], dtype=torch.float64)
    F = S.LocationScale("laplace", 0.0, 0.7).cdf(torch.tensor(z9["real_laplace/q"], dtype=torch.float64))     # (quantile, coordinate)
    assert float((F - qs[:, None]).abs().max()) < 0.006       # 1e5 draws: 2.6 / sqrt(1e5) = 0.008
    assert abs(float(np.mean(z9["real_laplace/var"])) - 2 * 0.49) < 0.03


def _reject_angle(rng, logdens, size):
    """accept-reject on theta against a uniform proposal over the window where the density exceeds e^-40 of its peak"""
    th = np.linspace(0.0, math.pi, 8193)
    ld = logdens(th)
    top = ld.max()
    keep = np.nonzero(ld > top - 40.0)[0]
    lo, hi = th[max(keep[0] - 1, 0)], th[min(keep[-1] + 1, th.size - 1)]
    fine = np.linspace(lo, hi, 200001)
    top = logdens(fine).max() + 1e-9
    out = np.empty(0)
    while out.size < size:
        c = lo + (hi - lo) * rng.random(4 * size)
        out = np.concatenate([out, c[np.log(rng.random(c.size)) < logdens(c) - top]])
    return out[:size]


@pytest.mark.parametrize("n", (2, 3, 4, 10, 40))
def test_vmf_and_sphere_uniform_angle(n):
    rng = np.random.default_rng(4 + n)
    M = N // 4
    for kappa in (0.0, 0.01, 1.0, 10.0, 100.0, 1e3, 1e4):
        with np.errstate(divide="ignore"):
            ld = lambda t: kappa * (np.cos(t) - 1.0) + ((n - 2) * np.log(np.sin(t)) if n > 2 else 0.0 * t)
            th = _reject_angle(rng, ld, M)
        tab = S.vmf_angle(n, kappa)
        _check(f"vmf n={n} kappa={kappa:g} angle", th, tab.cdf_angle)
        _check(f"vmf n={n} kappa={kappa:g} cos", np.cos(th), tab.cdf)
    # the uniform marginal by its construction: a coordinate of a normalised Gaussian vector
    v = rng.standard_normal((M, n))
    _check(f"sphere uniform n={n} coordinate", v[:, 0] / np.linalg.norm(v, axis=1), S.sphere_uniform_angle(n).cdf)


@pytest.mark.parametrize("n", (2, 3, 4, 10, 40))
def test_projected_normal(n):
    rng = np.random.default_rng(20 + n)
    M = N // 4
    mu = np.linspace(1.0, 2.0, n) * np.where(np.arange(n) % 2, -1.0, 1.0); mu /= np.linalg.norm(mu)
    for sigma in (0.05, 1.0):
        v = mu[None, :] + sigma * rng.standard_normal((M, n))
        x = v / np.linalg.norm(v, axis=1, keepdims=True)
        tab = S.projected_normal_angle(n, sigma)
        _check(f"sphere normal n={n} sigma={sigma} angle", S.angle_between(torch.as_tensor(x), torch.as_tensor(mu)), tab.cdf_angle)
        # the polar-coordinate table against the conditional-on-g formula, where that one is a smooth integrand
        ts = [math.cos(a) for a in np.linspace(tab.lo, tab.hi, 13)[1:-1] if abs(math.cos(a)) > 0.05]
        for t in ts:
            a = float(tab.cdf(torch.tensor([t], dtype=torch.float64)))
            b = S.projected_normal_cdf_w(t, n, sigma)
            assert abs(a - b) < 1e-6, (n, sigma, t, a, b)


def test_projected_laplace_simulations_agree():
    mu = np.array([2.0, -1.0, 0.5]); mu /= np.linalg.norm(mu)
    ref = S.Empirical(torch.as_tensor(S.projected_laplace_sim(mu, 0.05, 1 << 22, seed=1)))
    _check("sphere laplace n=3 (two simulations)", S.projected_laplace_sim(mu, 0.05, N // 4, seed=2), ref.cdf, n_ref=1 << 22)


def test_tables_are_exact_to_1e_6_by_halving():
    """Trapezoid and linear interpolation errors are both O(h^2): a table differs from the one on half the grid by three times its own
    error.  Evaluated off the nodes of both."""
    worst = 0.0
    cases = [(lambda g, n=n, k=k: S.vmf_angle(n, k, grid=g), 1 << 16, f"vmf n={n} kappa={k:g}")
             for n in (2, 3, 4, 10, 40) for k in (0.0, 0.01, 1.0, 10.0, 100.0, 1e3, 1e4)]
    cases += [(lambda g, n=n, s=s: S.projected_normal_angle(n, s, grid=g), 1 << 15, f"projected normal n={n} sigma={s}")
              for n in (2, 3, 4, 10, 40) for s in (0.05, 1.0)]
    gen = torch.Generator().manual_seed(0)
    for make, grid, name in cases:
        fine, half = make(grid), make(grid // 2)
        th = fine.lo + (fine.hi - fine.lo) * torch.rand(20000, dtype=torch.float64, generator=gen)
        d = float((fine.cdf_angle(th) - half.cdf_angle(th)).abs().max())
        worst = max(worst, d)
        assert d <= 1e-6, (name, d)
        assert abs(fine.lo - half.lo) < 1e-12 and float(fine.cdf_angle(torch.tensor([fine.lo, fine.hi]))[1]) == 1.0
    print(f"largest |table(G) - table(G/2)| = {worst:.2e}")


def test_angle_between_resolves_what_the_dot_product_cannot():
    th = torch.tensor([1e-5, 3e-4, 1e-2, 1.0, 3.0], dtype=torch.float64)
    mu = torch.tensor([0.6, 0.8], dtype=torch.float64)
    x = torch.stack([mu[0] * torch.cos(th) - mu[1] * torch.sin(th), mu[1] * torch.cos(th) + mu[0] * torch.sin(th)], 1)
    assert float((S.angle_between(x, mu) - th).abs().max()) < 1e-12
    got = S.angle_between(x.to(torch.float32), mu.to(torch.float32))
    assert float(((got - th).abs() / th).max()) < 0.02     # float32 coordinates: 6e-8 absolute on a chord of 1e-5


def test_vmf_in_one_dimension_is_refused():
    """S^0 has no tangent direction and Wood's Beta(0, 0) draw is undefined: the C ABI refuses n = 1 with a message (on the host, before
    any launch: the dummy addresses never reach a kernel)."""
    from cl_ica_amd import _lib
    lib = _lib.load()
    P = 1 << 20
    d = _lib.SamplerDesc(space=2, dist=4, n=1, box_min=0.0, box_max=1.0, scale=10.0, shape_p=2.0, seed=0, stream_id=0)
    assert lib.clica_sample(ctypes.byref(d), P, 1, P, 1, 16, None, None) == -1
    assert b"vMF" in lib.clica_last_error() and b"n >= 2" in lib.clica_last_error()
    d.n, d.scale = 3, float("nan")
    assert lib.clica_sample(ctypes.byref(d), P, 3, P, 3, 16, None, None) == -1 and b"kappa > 0" in lib.clica_last_error()
    d.scale, d.space = 10.0, 0
    assert lib.clica_sample(ctypes.byref(d), P, 3, P, 3, 16, None, None) == -1 and b"sphere" in lib.clica_last_error()
