"""The on-device latent samplers (csrc/sampler.hip, csrc/sampler_dev.h) against their exact distributions (tests/sampler_cdfs.py,
verified on the host by tests/test_sampler_cdfs_host.py), every kind, at the dimensions, scales and concentrations where each
hand-written part can go wrong: Marsaglia-Tsang gamma on both sides of shape 1, Wood's vMF rejection from n = 2 to 40 and kappa = 0.01 to
1e4, per-element truncation down to 4 % acceptance, the Philox counter layout, the 24-bit uniforms' tails.

One bound for every comparison: sqrt(N) D < 2.6 with D the exact one-sample Kolmogorov-Smirnov statistic of N = 2^20 draws (2^18 rows
for n >= 40).  Dvoretzky-Kiefer-Wolfowitz / Massart: P(sqrt(N) D > 2.6) <= 2 exp(-2 * 2.6^2) = 2.7e-6 for a correct sampler at every N; with
the ~500 comparisons below the file fails by chance with probability about 1e-3 -- once, not per run: seeds are fixed and Philox is counter
based, a run is deterministic.  Against a reference that is itself a sample of size N2, N N2 / (N + N2) takes the place of N.
For orientation: a 1 % error in a normal's scale gives sqrt(N) D = 2.6 at N = 2^20, 0.3 % when ten columns are pooled.

Angles to the mean are measured from the chord in float64 (sampler_cdfs.angle_between): <x, mu> of float32 coordinates cannot
resolve 1 - w below 6e-8, which is a visible atom for a concentrated conditional in low dimension.
`pytest -rA` shows every statistic."""
import math
import zlib

import numpy as np
import pytest
import torch

import sampler_cdfs as S

pytestmark = pytest.mark.gpu
N = 1 << 20
DEV = "cuda"
PS = (0.5, 1.0, 2.0, 3.0, 8.0)
KINDS = [("normal", None), ("laplace", None)] + [("gennorm", p) for p in PS]
DIMS = (2, 3, 4, 10, 40)
F64 = torch.float64


def rows(n):
    return N if n < 40 else N // 4


def seed_of(name):
    return zlib.crc32(name.encode())


def ks(name, sample, cdf, n_ref=None):
    v = S.ks_scaled(sample, cdf, n_ref)
    print(f"{name}: sqrt(N) D = {v:.3f}  (N = {sample.numel()})")
    assert math.isfinite(v) and v < S.BOUND, (name, v)
    return v


def ks_columns(name, x, cdf, pooled=True):
    """first and last coordinate separately; all coordinates pooled where they are i.i.d."""
    ks(f"{name} [first]", x[:, 0], cdf)
    if x.shape[1] > 1:
        ks(f"{name} [last]", x[:, -1], cdf)
        if pooled:
            ks(f"{name} [pooled]", x, cdf)


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def draw(name, space, dist, n, size, **kw):
    from cl_ica_amd import ops
    kw.setdefault("seed", seed_of(name))
    kw.setdefault("stream_id", 4)
    out = ops.sample(space, dist, n, size, DEV, **kw)
    assert bool(torch.isfinite(out).all()), name
    return out


def unit_mean(n):
    mu = torch.linspace(1.0, 2.0, n) * torch.where(torch.arange(n) % 2 == 1, -1.0, 1.0)      # no axis vector, mixed signs
    return (mu / mu.norm()).to(DEV)


# ------------------------------------------------------------------------------------------------ box
@pytest.mark.parametrize("n", (1, 10))
def test_box_uniform(n):
    for lo, hi in ((0.0, 1.0), (-1.0, 1.0)):
        name = f"box uniform [{lo}, {hi}) n={n}"
        z = draw(name, "box", "uniform", n, N, box=(lo, hi))
        assert float(z.min()) >= lo and float(z.max()) < hi
        ks_columns(name, z, S.BoxUniform(lo, hi).cdf)


@pytest.mark.parametrize("kind,p", KINDS)
def test_box_truncated(kind, p):
    """Means in the middle, near an edge and exactly on either edge; scales from 1/20 of the box to 5 boxes wide (acceptance down to
    4 %: the register loop's 4096 tries must still leave every value inside)."""
    n = 10
    for lo, hi in ((0.0, 1.0),):
        for m in (0.5, 0.02, lo, hi):
            for s in (0.05, 1.0, 5.0 * (hi - lo)):
                name = f"box {kind} p={p} m={m} s={s}"
                mean = torch.full((n,), m, device=DEV)
                z = draw(name, "box", kind, n, N, mean=mean, scale=s, shape_p=p or 2.0, box=(lo, hi))
                assert float(z.min()) >= lo and float(z.max()) <= hi, name
                ks_columns(name, z, S.LocationScale(kind, f32(m), f32(s), p, box=(lo, hi)).cdf)
                if p == 1.0:
                    ks(f"{name} [pooled, against Laplace]", z, S.LocationScale("laplace", f32(m), f32(s), box=(lo, hi)).cdf)
                if p == 2.0:
                    ks(f"{name} [pooled, against Normal(m, s / sqrt 2)]", z, S.LocationScale("normal", f32(m), f32(s) / math.sqrt(2.0), box=(lo, hi)).cdf)


def test_box_other_box_and_one_dimension():
    """box (-1, 1) (spaces.NBoxSpace's default) and n = 1, one kind each: the box bounds and n enter the element index only."""
    for kind, p, n, m, s in (("normal", None, 1, -0.98, 0.1), ("laplace", None, 10, 1.0, 2.0), ("gennorm", 3.0, 1, 0.0, 10.0)):
        name = f"box(-1, 1) {kind} p={p} n={n} m={m} s={s}"
        z = draw(name, "box", kind, n, N, mean=torch.full((n,), m, device=DEV), scale=s, shape_p=p or 2.0, box=(-1.0, 1.0))
        assert float(z.min()) >= -1.0 and float(z.max()) <= 1.0
        ks_columns(name, z, S.LocationScale(kind, f32(m), f32(s), p, box=(-1.0, 1.0)).cdf)


# ------------------------------------------------------------------------------------------------ R^n
@pytest.mark.parametrize("kind,p", KINDS)
def test_real(kind, p):
    n = 10
    for s in (1e-3, 2.0):
        name = f"real {kind} p={p} s={s}"
        z = draw(name, "real", kind, n, N, mean=torch.full((n,), 0.25, device=DEV), scale=s, shape_p=p or 2.0)
        ks_columns(name, z, S.LocationScale(kind, f32(0.25), f32(s), p).cdf)
    # per-coordinate scales a factor 100 apart: (n,) and (size, n)
    unit = S.LocationScale(kind, p=p).cdf
    sv = torch.where(torch.arange(n) % 2 == 0, 0.03, 3.0).to(DEV)
    name = f"real {kind} p={p} scale (n,)"
    z = draw(name, "real", kind, n, N, mean=torch.zeros(n, device=DEV), scale=1.0, shape_p=p or 2.0, scale_vec=sv)
    ks(f"{name} [first, s=0.03]", z[:, 0], S.LocationScale(kind, 0.0, f32(0.03), p).cdf)
    ks(f"{name} [last, s=3]", z[:, -1], S.LocationScale(kind, 0.0, 3.0, p).cdf)
    ks(f"{name} [standardised, pooled]", z.to(F64) / sv.to(F64), unit)
    name = f"real {kind} p={p} scale (size, n)"
    sv2 = torch.where((torch.arange(N, device=DEV)[:, None] + torch.arange(n, device=DEV)[None, :]) % 2 == 0, 0.03, 3.0)
    z = draw(name, "real", kind, n, N, mean=torch.zeros(n, device=DEV), scale=1.0, shape_p=p or 2.0, scale_vec=sv2)
    u = z.to(F64) / sv2.to(F64)
    ks_columns(f"{name} [standardised]", u, unit)
    ks(f"{name} [first, rows with s=0.03]", z[0::2, 0], S.LocationScale(kind, 0.0, f32(0.03), p).cdf)


@pytest.mark.parametrize("kind,p,vmax", [("normal", None, 5.77), ("laplace", None, 16.64), ("gennorm", 3.0, None)])
def test_tails(kind, p, vmax):
    """Where KS is blind: the draws beyond the analytic two-sided 1e-4 and 1e-5 quantiles among N n pooled values, within 5 binomial
    standard deviations (two-sided normal tail 5.7e-7), and the largest |value| / scale 24-bit uniforms can produce: sqrt(2 * 24 ln 2) = 5.768
    for Box-Muller, 24 ln 2 = 16.636 for the inverse-CDF Laplace behind its 0.99999994 clamp."""
    n = 10
    name = f"tails {kind} p={p}"
    z = draw(name, "real", kind, n, N, mean=torch.zeros(n, device=DEV), scale=1.0, shape_p=p or 2.0).abs().to(F64)
    d = S.LocationScale(kind, p=p)
    for q in (1e-4, 1e-5):
        t = d.two_sided_quantile(q)
        got, want = int((z > t).sum()), N * n * q
        sd = math.sqrt(N * n * q * (1.0 - q))
        print(f"{name}: |x| > {t:.4f} (q = {q:g}): {got} draws, expected {want:.1f} +- {sd:.1f} ({(got - want) / sd:+.2f} sd)")
        assert abs(got - want) < 5.0 * sd, (name, q, got, want, sd)
    top = float(z.max())
    print(f"{name}: largest |x| / scale = {top:.4f}" + (f" (24-bit limit {vmax})" if vmax else ""))
    if vmax:
        assert top <= vmax, (name, top)


# ------------------------------------------------------------------------------------------------ sphere
def unit_norm(x, name):
    err = float((x.to(F64).norm(dim=-1) - 1.0).abs().max())
    assert err < 1e-5, (name, err)


@pytest.mark.parametrize("n", DIMS)
def test_sphere_uniform(n):
    name = f"sphere uniform n={n}"
    x = draw(name, "sphere", "uniform", n, rows(n))
    unit_norm(x, name)
    ks_columns(name, x, S.sphere_uniform_angle(n, device=DEV).cdf, pooled=False)


@pytest.mark.parametrize("n", DIMS)
def test_sphere_normal(n):
    mu = unit_mean(n)
    for sigma in (0.05, 1.0):
        name = f"sphere normal n={n} sigma={sigma}"
        x = draw(name, "sphere", "normal", n, rows(n), mean=mu, scale=sigma)
        unit_norm(x, name)
        ks(f"{name} [angle to the mean]", S.angle_between(x, mu), S.projected_normal_angle(n, f32(sigma), device=DEV).cdf_angle)


def test_sphere_laplace_against_a_simulation():
    """Laplace noise is not rotation invariant: the reference is a numpy float64 simulation of 2^24 draws at the same mean."""
    n, scale, N2 = 3, 0.05, 1 << 24
    mu = unit_mean(n)
    ref = S.Empirical(torch.as_tensor(S.projected_laplace_sim(mu.cpu().numpy().astype(np.float64), f32(scale), N2, seed=7)))
    name = f"sphere laplace n={n} scale={scale}"
    x = draw(name, "sphere", "laplace", n, N, mean=mu, scale=scale)
    unit_norm(x, name)
    w = (x.to(F64) * mu.to(F64)).sum(-1)
    ks(f"{name} [<x, mu> against 2^24 simulated]", w.cpu(), ref.cdf, n_ref=N2)


def tangent_coordinate(x, mu):
    """x without its component along mu, normalised: one fixed coordinate of that direction in the tangent space at mu (float64).
    Returns it with the length of the tangent part before normalising."""
    x, mu = x.to(F64), mu.to(F64).expand_as(x)
    mu = mu / mu.norm(dim=-1, keepdim=True)
    t = x - (x * mu).sum(-1, keepdim=True) * mu
    tn = t.norm(dim=-1, keepdim=True)
    t = t / tn
    v = torch.zeros(x.shape[1], dtype=F64, device=x.device); v[0], v[-1] = 0.6, -0.8
    e = v - (v * mu).sum(-1, keepdim=True) * mu
    e = e / e.norm(dim=-1, keepdim=True)
    return (t * e).sum(-1), tn[:, 0]


@pytest.mark.parametrize("rowmean", (False, True), ids=("one_mean", "mean_per_row"))
@pytest.mark.parametrize("n", DIMS)
def test_vmf(n, rowmean):
    """Wood's rejection for w = <x, mu> and the uniform tangent direction: the angle to the mean against the vMF angle density, the
    tangent part's fixed coordinate against the uniform marginal on S^(n-2) (a fair sign for n = 2), unit norm."""
    M = rows(n)
    mu = draw(f"vmf means n={n}", "sphere", "uniform", n, M) if rowmean else unit_mean(n)
    tangent = S.sphere_uniform_angle(n - 1, device=DEV).cdf if n > 2 else None
    for kappa in (0.01, 1.0, 10.0, 100.0, 1e3, 1e4):
        name = f"vmf n={n} kappa={kappa:g} {'mean per row' if rowmean else 'one mean'}"
        x = draw(name, "sphere", "vmf", n, M, mean=mu, scale=kappa)
        unit_norm(x, name)
        ks(f"{name} [angle to the mean]", S.angle_between(x, mu), S.vmf_angle(n, kappa, device=DEV).cdf_angle)
        c, tn = tangent_coordinate(x, mu)
        if n > 2:
            ks(f"{name} [tangent coordinate]", c, tangent)
        else:
            # (x == +-mu to float32 resolution has no tangent direction: about 1e-6 of the draws at kappa = 1e4, counted as "not +")
            c = torch.where(tn > 1e-6, c, torch.zeros_like(c))
            v = math.sqrt(M) * abs(float((c > 0).to(F64).mean()) - 0.5)
            print(f"{name} [tangent sign]: sqrt(N) |P(+) - 1/2| = {v:.3f}  ({int((c == 0).sum())} draws without a tangent part)")
            assert float(c[c != 0].abs().min()) > 0.999 and v < S.BOUND, (name, v)


def test_through_spaces():
    """One draw per space through cl_ica_amd.spaces: the Python scale / mean plumbing in front of the same kernels."""
    from cl_ica_amd import spaces
    spaces.manual_seed(11)
    n = 10
    z = spaces.NBoxSpace(n, 0.0, 1.0).laplace(torch.full((N, n), 0.02, device=DEV), 0.05, N, device=DEV)
    ks_columns("spaces box laplace m=0.02 s=0.05", z, S.LocationScale("laplace", f32(0.02), f32(0.05), box=(0.0, 1.0)).cdf)
    std = torch.where(torch.arange(n) % 2 == 0, 0.03, 3.0)                     # a host tensor, moved like the reference does
    z = spaces.NRealSpace(n).normal(torch.zeros(n, device=DEV), std, N, device=DEV)
    ks("spaces real normal std tensor [standardised, pooled]", z.to(F64) / std.to(DEV).to(F64), S.LocationScale("normal").cdf)
    z = spaces.NRealSpace(n).generalized_normal(torch.zeros(n, device=DEV), 0.7, p=3, size=N, device=DEV)
    ks_columns("spaces real gennorm p=3 s=0.7", z, S.LocationScale("gennorm", 0.0, f32(0.7), 3.0).cdf)
    mu = unit_mean(4)
    x = spaces.NSphereSpace(4).von_mises_fisher(mu, 50.0, N, device=DEV)
    ks("spaces vmf n=4 kappa=50 [angle to the mean]", S.angle_between(x, mu), S.vmf_angle(4, 50.0, device=DEV).cdf_angle)


# ------------------------------------------------------------------------------------------------ counters
def independent(name, a, b):
    a, b = a.flatten(), b.flatten()
    r = S.corr(a, b)
    lim = 5.0 / math.sqrt(a.numel())
    print(f"{name}: correlation {r:+.5f} over {a.numel()} pairs (limit {lim:.5f})")
    assert not torch.equal(a, b), name
    assert abs(r) < lim, (name, r)


def test_counters_give_independent_draws():
    """Philox counter = (element or row index, draw block, step, stream id), key = the 64-bit seed: changing any one of them gives
    independent numbers -- for the element-wise kernel (R^n normal) and the row-wise one (sphere uniform)."""
    n, seed = 2, 0x1234ABCD
    step = lambda v: torch.full((1,), v, dtype=torch.int32, device=DEV)
    for what, kw in (("element-wise", dict(space="real", dist="normal", mean=torch.zeros(n, device=DEV))),
                     ("row-wise", dict(space="sphere", dist="uniform"))):
        def d(seed=seed, stream_id=4, s=7):
            return draw(what, kw["space"], kw["dist"], n, N, mean=kw.get("mean"), seed=seed, stream_id=stream_id, step_dev=step(s))
        base = d()
        independent(f"{what}: seed against seed + 1", base[:, 0], d(seed=seed + 1)[:, 0])
        independent(f"{what}: seed against seed + 2^32", base[:, 0], d(seed=seed + (1 << 32))[:, 0])
        independent(f"{what}: stream 4 against 5", base[:, 0], d(stream_id=5)[:, 0])
        independent(f"{what}: step 7 against 8", base[:, 0], d(s=8)[:, 0])
        independent(f"{what}: row i against row i + 1", base[:-1, 0], base[1:, 0])
        independent(f"{what}: coordinate 0 against 1", base[:, 0], base[:, 1])


def test_pair_noise_is_independent_of_the_marginal():
    from cl_ica_amd import ops
    n = 2
    for cond in ("normal", "laplace"):
        z, zt = torch.empty(N, n, device=DEV), torch.empty(N, n, device=DEV)
        ops.sample_pair("real", "normal", cond, n, N, z, zt, marginal_mean=torch.zeros(N, n, device=DEV), m_scale=1.0, c_scale=0.05,
                        seed=99, stream_id=4, step_dev=torch.full((1,), 3, dtype=torch.int32, device=DEV))
        independent(f"sample_pair real normal / {cond}: z against z~ - z", z[:, 0], (zt - z)[:, 0])
        ks(f"sample_pair real normal / {cond}: z~ - z [pooled]", (zt.to(F64) - z.to(F64)), S.LocationScale(cond, 0.0, f32(0.05)).cdf)


def test_row_wise_and_element_wise_kernels_do_not_share_numbers():
    """The sphere kernel counts rows and the box kernel counts elements: at the same seed, stream and step the noise of sphere row i must be
    independent of the box draw's element i (the same first counter word) as well as of the box draw's row i."""
    n, kw = 4, dict(seed=5, stream_id=4, step_dev=torch.full((1,), 2, dtype=torch.int32, device=DEV))
    sph = draw("sphere", "sphere", "uniform", n, N, **kw)
    box = (draw("box", "box", "normal", n, N, mean=torch.full((n,), 0.5, device=DEV), scale=0.05, box=(0.0, 1.0), **kw) - 0.5) / 0.05
    independent("sphere row i, coordinate 0 against box row i, coordinate 0", sph[:, 0], box[:, 0])
    independent("sphere row i, coordinate 0 against box element i", sph[:, 0], box.flatten()[:N])
    independent("sphere row i, coordinate 1 against box element i", sph[:, 1], box.flatten()[:N])


KINDS_EXACT = (("element-wise", "box", "normal", dict(scale=0.05, box=(0.0, 1.0))), ("row-wise", "sphere", "vmf", dict(scale=20.0)))


def test_a_draw_depends_on_its_counters_only():
    """Prefix: the first M rows of a 2 M row draw are the M row draw.  Stride: a draw into a column slice of a wider tensor equals the
    contiguous one and leaves the other columns alone.  Seed: the same (seed, stream, step) twice is bit-identical.  Graph replay and the
    training step's merged front launch rest on all three."""
    from cl_ica_amd import ops
    M, n = 1000, 10
    step = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    for what, space, dist, kw in KINDS_EXACT:
        mean2 = ops.sample("sphere" if space == "sphere" else "box", "uniform", n, 2 * M, DEV, seed=1, stream_id=0)
        args = dict(seed=77, stream_id=4, step_dev=step, **kw)
        a = ops.sample(space, dist, n, M, DEV, mean=mean2[:M], **args)
        b = ops.sample(space, dist, n, 2 * M, DEV, mean=mean2, **args)
        assert torch.equal(a, b[:M]) and not torch.equal(a, b[M:]), what
        wide = torch.full((M, 16), -7.0, device=DEV)
        ops.sample(space, dist, n, M, DEV, mean=mean2[:M], out=wide[:, 3:3 + n], **args)
        assert torch.equal(wide[:, 3:3 + n], a), what
        assert bool((wide[:, :3] == -7.0).all()) and bool((wide[:, 3 + n:] == -7.0).all()), what
        assert torch.equal(ops.sample(space, dist, n, M, DEV, mean=mean2[:M], **args), a), what
