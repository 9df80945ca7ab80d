"""tests/sgd_oracle.py without a GPU: the fp64 restatement against torch.optim.SGD in float64, and the NumPy float32 emulation of the
documented operation sequence (include/clica.h "SGD") held to the bound derived from its roundings (sgd_oracle's docstring) -- so what
tests/test_gpu_sgd.py compares the kernel with, bit for bit, is itself tied to torch's update and never to the code under test."""
import numpy as np
import pytest
import torch

import sgd_oracle as S
from test_elementwise_host import close

COUNT, STEPS = 4099, 6
NAMES = list(S.SGD_OPTION_SETS)


@pytest.fixture(scope="module")
def inputs():
    p0, grads = S.sgd_inputs(COUNT, STEPS)
    p0.setflags(write=False)
    for g in grads:
        g.setflags(write=False)
    return p0, grads


@pytest.mark.parametrize("name", NAMES)
def test_fp64_restatement_against_torch_float64(inputs, name):
    """Six steps of torch.optim.SGD on float64 parameters; both sides compute with the Python scalars (abi=False)."""
    p0, grads = inputs
    p, buf = p0.astype(np.float64), None
    for t, g in enumerate(grads):
        p, buf, D, Bm = S.sgd_update(p, g, buf, t, name, abi=False)
        assert (D >= 0).all() and (Bm is None) == (S.options(name)["momentum"] == 0)
    pt, bt = S.torch_trajectory(p0, grads, name, torch.float64)
    close(p, pt)
    assert (buf is None) == (bt is None)
    if buf is not None:
        close(buf, bt)


@pytest.mark.parametrize("name", NAMES)
def test_fp32_emulation_stays_inside_the_derived_bound(inputs, name):
    """Every one of the six updates, from the emulation's own fp32 state: p' within ulp(p') / 2 + 3.5 EPS32 lr D of the fp64 update of
    that state, buf' within 2 EPS32 Bm.  The distance to the fp64 TRAJECTORY after six steps is printed (about one ulp of max(|p|, 1))."""
    p0, grads = inputs
    p, buf, worst = p0, None, dict(p=0.0, buf=0.0)
    p64, buf64 = p0.astype(np.float64), None
    for t, g in enumerate(grads):
        p_new, buf_new = S.sgd_fp32_emulation(p, g, buf, t, name)
        e = S.sgd_errors(p_new, buf_new, p, g, buf, t, name)
        worst = {k: max(worst[k], e[k]) for k in worst}
        p64, buf64, _, _ = S.sgd_update(p64, g, buf64, t, name, abi=True)
        p, buf = p_new, buf_new
    assert np.isfinite(p).all()
    ulps = np.abs(p.astype(np.float64) - p64) / np.spacing(np.maximum(np.abs(p), np.float32(1))).astype(np.float64)
    print(f"sgd fp32 emulation, {name}: worst single update p {worst['p']:.3f} (limit {S.SGD_P_LIMIT}), buf {worst['buf']:.3f} (limit {S.SGD_BUF_LIMIT}) "
          f"EPS32 units; after {STEPS} steps {float(ulps.max()):.2f} ulp(max(|p|, 1)) from the fp64 trajectory")
    assert worst["p"] <= S.SGD_P_LIMIT and worst["buf"] <= S.SGD_BUF_LIMIT


def test_emulation_is_the_documented_sequence_on_hand_values():
    """Values chosen so that every rounding of the sequence is visible: the result differs from the fused / reordered forms."""
    F = np.float32
    o = dict(lr=0.1, momentum=0.9, dampening=0.5, weight_decay=1e-2, grad_scale=1.0 / 3.0)
    p, g, buf = np.asarray([1.2345678], F), np.asarray([0.7654321], F), np.asarray([-0.3456789], F)
    lr, mom, wd, s = F(0.1), F(0.9), F(1e-2), F(1.0 / 3.0)
    gr = F(F(g[0] * s) + F(wd * p[0]))
    b1 = F(F(mom * buf[0]) + F(F(F(1) - F(0.5)) * gr))
    want = F(p[0] - F(lr * b1))
    got_p, got_b = S.sgd_fp32_emulation(p, g, buf, 3, o)
    assert got_b[0] == b1 and got_p[0] == want
    first_p, first_b = S.sgd_fp32_emulation(p, g, buf, 0, o)
    assert first_b[0] == gr and first_p[0] == F(p[0] - F(lr * gr))      # t = 0: the buffer is the gradient, its old content is not read


def test_error_figures_see_a_wrong_update(inputs):
    """The figures are not blind: dampening applied at t = 0, and a buffer that was not set to gr at t = 0, leave the limits."""
    p0, grads = inputs
    o = "dampening"
    lr, mom, omd, _, _ = S.scalars(o, True)
    ok_p, ok_b = S.sgd_fp32_emulation(p0, grads[0], None, 0, o)
    ok = S.sgd_errors(ok_p, ok_b, p0, grads[0], None, 0, o)
    assert ok["p"] <= S.SGD_P_LIMIT and ok["buf"] <= S.SGD_BUF_LIMIT
    # (a) the t > 0 formula from a zero buffer at t = 0: buf = (1 - dampening) gr
    wrong_p, wrong_b = S.sgd_fp32_emulation(p0, grads[0], np.zeros_like(p0), 1, o)
    bad = S.sgd_errors(wrong_p, wrong_b, p0, grads[0], None, 0, o)
    assert bad["p"] > S.SGD_P_LIMIT and bad["buf"] > S.SGD_BUF_LIMIT
    # (b) the first update steps along gr but leaves the buffer at zero: the parameter is right, the buffer is not, and the second
    # update -- judged against the fp64 trajectory's state -- is off in both
    lazy_b = np.zeros_like(p0)
    e0 = S.sgd_errors(ok_p, lazy_b, p0, grads[0], None, 0, o)
    assert e0["p"] <= S.SGD_P_LIMIT and e0["buf"] > S.SGD_BUF_LIMIT
    p2, b2 = S.sgd_fp32_emulation(ok_p, grads[1], lazy_b, 1, o)
    e1 = S.sgd_errors(p2, b2, ok_p, grads[1], ok_b, 1, o)
    assert e1["p"] > S.SGD_P_LIMIT and e1["buf"] > S.SGD_BUF_LIMIT


def test_entry_points_refuse_by_return_code():
    """Every rejected argument set returns CLICA_E_INVALID from host code, before any launch (no GPU needed)."""
    from cl_ica_amd import _lib
    L, a = _lib.load(), 4096
    plain = (0.1, 0.0, 0.0, 0.0, 0, 0, 1.0)
    mom = (0.1, 0.9, 0.0, 0.0, 0, 0, 1.0)
    cases = [
        ((None, a, None, 8) + plain + (a,), b"bad argument"),
        ((a, None, None, 8) + plain + (a,), b"bad argument"),
        ((a, a, None, 8) + plain + (None,), b"bad argument"),
        ((a, a, None, 0) + plain + (a,), b"bad argument"),
        ((a, a, None, -4) + plain + (a,), b"bad argument"),
        ((a + 4, a, None, 8) + plain + (a,), b"16-byte"),
        ((a, a + 8, None, 8) + plain + (a,), b"16-byte"),
        ((a, a, a + 4, 8) + mom + (a,), b"16-byte"),
        ((a, a, None, 8) + mom + (a,), b"momentum buffer"),
        ((a, a, None, 8) + (0.1, 0.0, 0.0, 0.0, 1, 0, 1.0) + (a,), b"nesterov"),
        ((a, a, a, 8) + (0.1, 0.9, 0.5, 0.0, 1, 0, 1.0) + (a,), b"nesterov"),
    ]
    for args, msg in cases:
        assert L.clica_sgd_step(*args, None) == -1, args
        assert msg in L.clica_last_error(), (args, L.clica_last_error())
        assert L.clica_sgd_step_tick(*args, a, None) == -1, args
    assert L.clica_sgd_step_tick(a, a, None, 8, *plain, a, None, None) == -1 and b"ticket" in L.clica_last_error()
