"""csrc/sgd.hip (``ops.sgd_step``) and ``cl_ica_amd.optim.SGD`` on the GPU against tests/sgd_oracle.py's float32 emulation of the
operation sequence documented in include/clica.h -- bit for bit: the sequence is multiplies and adds only, each rounded once.
tests/test_sgd_host.py ties that emulation to torch.optim.SGD."""
import numpy as np
import pytest
import torch

import elementwise_oracle as E
import sgd_oracle as S

pytestmark = pytest.mark.gpu

NAMES = list(S.SGD_OPTION_SETS)
SMALL_COUNTS = [1, 3, 4, 5, 1023, 1025]
WRAP_COUNT = 2 * 1024 * 1024 + 5      # 2048 blocks x 256 threads x 4 floats + 5: one grid-stride wrap of the block cap plus a scalar tail
TICK_WRAP_COUNT = 256 * 256 * 4 + 5   # the fused tick caps the grid at 256 blocks


def dev():
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def gpu(a):
    return torch.tensor(np.asarray(a), device=dev())


def run_steps(count, name, tick, steps=3, pad=0):
    """`steps` updates from t = 0 through ops.sgd_step on arenas of count + pad floats (-0.0 beyond count); returns the per-step
    (p, buf) arrays of the whole arenas, the final counter and ticket, and the inputs."""
    from cl_ica_amd import ops
    o = S.options(name)
    p0, grads = S.sgd_inputs(count, steps, seed=count % 1000 + 13)
    row = lambda a: E.padded(np.asarray(a, np.float32)[None, :], count + pad)[0]
    p = gpu(row(p0))
    buf = gpu(row(np.full(count, np.nan, np.float32))) if o["momentum"] != 0 else None      # NaN: the first update must not read it
    step = torch.zeros(1, dtype=torch.int32, device=dev())
    ticket = torch.zeros(1, dtype=torch.int32, device=dev()) if tick else None
    out = []
    for k in range(steps):
        g = gpu(row(grads[k]))
        ops.sgd_step(p, g, buf, step, o["lr"], momentum=o["momentum"], dampening=o["dampening"], weight_decay=o["weight_decay"],
                     nesterov=o["nesterov"], maximize=o["maximize"], grad_scale=o["grad_scale"], ticket=ticket, count=count)
        if not tick:
            assert int(step.item()) == k      # the plain entry point leaves the counter alone
            ops.tick(step)
        else:
            assert int(step.item()) == k + 1 and int(ticket.item()) == 0
        out.append((p.cpu().numpy(), None if buf is None else buf.cpu().numpy()))
    return out, p0, grads


def assert_matches_emulation(count, name, tick, pad=0):
    out, p0, grads = run_steps(count, name, tick, pad=pad)
    want = S.emulate_steps(p0, grads, name)
    for k, ((gp, gb), (wp, wb)) in enumerate(zip(out, want)):
        assert np.array_equal(bits(gp[:count]), bits(wp)), (name, count, tick, k, "param", int((bits(gp[:count]) != bits(wp)).sum()))
        assert (gb is None) == (wb is None)
        if wb is not None:
            assert np.array_equal(bits(gb[:count]), bits(wb)), (name, count, tick, k, "momentum_buffer")
        if pad:
            assert (bits(gp[count:]) == 0x80000000).all() and (gb is None or (bits(gb[count:]) == 0x80000000).all()), (name, count, k, "padding")


@pytest.mark.parametrize("tick", [False, True], ids=["plain", "tick"])
@pytest.mark.parametrize("name", NAMES)
def test_three_steps_bit_equal_small_counts(name, tick):
    for count in SMALL_COUNTS:
        assert_matches_emulation(count, name, tick, pad=(-count) % 4 + 8)


@pytest.mark.parametrize("count,tick", [(WRAP_COUNT, False), (WRAP_COUNT, True), (TICK_WRAP_COUNT, True)], ids=["wrap", "wrap-tick", "tickwrap-tick"])
def test_three_steps_bit_equal_past_the_block_caps(count, tick):
    for name in ("plain", "nesterov", "momentum_wd", "dampening"):
        assert_matches_emulation(count, name, tick, pad=7)


def test_rejected_arguments_return_the_error():
    from cl_ica_amd import _lib, ops
    p = torch.zeros(16, device=dev()); g = torch.zeros(16, device=dev()); b = torch.zeros(16, device=dev())
    step = torch.zeros(1, dtype=torch.int32, device=dev())
    before = p.clone()
    with pytest.raises(_lib.ClicaError, match="momentum buffer"):
        ops.sgd_step(p, g, None, step, 0.1, momentum=0.9)
    with pytest.raises(_lib.ClicaError, match="nesterov"):
        ops.sgd_step(p, g, None, step, 0.1, nesterov=True)
    with pytest.raises(_lib.ClicaError, match="nesterov"):
        ops.sgd_step(p, g, b, step, 0.1, momentum=0.9, dampening=0.5, nesterov=True)
    with pytest.raises(_lib.ClicaError, match="16-byte"):
        ops.sgd_step(p[1:9], g[:8], None, step, 0.1)
    with pytest.raises(_lib.ClicaError, match="16-byte"):
        ops.sgd_step(p[:8], g[:8], b[2:10], step, 0.1, momentum=0.9)
    with pytest.raises(_lib.ClicaError, match="bad argument"):
        ops.sgd_step(p[:0], g, None, step, 0.1)
    L = _lib.load()
    assert L.clica_sgd_step(None, g.data_ptr(), None, 8, 0.1, 0.0, 0.0, 0.0, 0, 0, 1.0, step.data_ptr(), None) == -1
    assert L.clica_sgd_step(p.data_ptr(), None, None, 8, 0.1, 0.0, 0.0, 0.0, 0, 0, 1.0, step.data_ptr(), None) == -1
    assert L.clica_sgd_step(p.data_ptr(), g.data_ptr(), None, 8, 0.1, 0.0, 0.0, 0.0, 0, 0, 1.0, None, None) == -1
    assert L.clica_sgd_step_tick(p.data_ptr(), g.data_ptr(), None, 8, 0.1, 0.0, 0.0, 0.0, 0, 0, 1.0, step.data_ptr(), None, None) == -1
    torch.cuda.synchronize()
    assert torch.equal(p, before) and int(step.item()) == 0


# ---------------------------------------------------------------------------------------------------------------- optim.SGD
def _model(seed=3):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Linear(3, 2)).to(dev())


def _arena_grads(opt, steps, seed=21):
    """Gradient arenas with zeros in the alignment padding (what autograd leaves there)."""
    rng = np.random.default_rng(seed)
    mask = np.zeros(opt.total, bool)
    for p, off in zip(opt.params, opt.offsets):
        mask[off:off + p.numel()] = True
    return [np.where(mask, rng.normal(size=opt.total), 0.0).astype(np.float32) for _ in range(steps)]


def test_optimizer_repoints_parameters_and_steps_like_the_emulation():
    from cl_ica_amd import optim
    f = _model()
    want0 = [p.detach().cpu().numpy().copy() for p in f.parameters()]
    kw = dict(lr=0.1, momentum=0.9, weight_decay=1e-2)
    opt = optim.SGD(f.parameters(), **kw)
    assert opt.total == 16 + 4 + 8 + 4 and opt.offsets == [0, 16, 20, 28]      # 15 -> 16, 3 -> 4, 6 -> 8, 2 -> 4
    base, gbase = opt.param_arena.data_ptr(), opt.grad_arena.data_ptr()
    for p, off, w in zip(f.parameters(), opt.offsets, want0):
        assert p.data_ptr() == base + 4 * off and p.grad.data_ptr() == gbase + 4 * off and p._clica_grad_view is p.grad
        assert np.array_equal(p.detach().cpu().numpy(), w)
    assert opt.state_dict()["state"] == {}
    grads = _arena_grads(opt, 3)
    want = S.emulate_steps(opt.param_arena.cpu().numpy(), grads, kw)
    for k, g in enumerate(grads):
        opt.zero_grad()
        assert float(opt.grad_arena.abs().max()) == 0.0
        opt.grad_arena.copy_(gpu(g))
        opt.step()
        assert np.array_equal(bits(opt.param_arena.cpu().numpy()), bits(want[k][0])), k
        assert np.array_equal(bits(opt.momentum_buffer.cpu().numpy()), bits(want[k][1])), k
    assert int(opt.step_dev.item()) == 3 and int(opt._ticket.item()) == 0
    # a foreign .grad (model.zero_grad() dropped the views, autograd allocated new tensors) is adopted
    f.zero_grad(set_to_none=True)
    f(torch.ones(4, 5, device=dev())).sum().backward()
    foreign = [p.grad.detach().cpu().numpy().copy() for p in f.parameters()]
    g4 = np.zeros(opt.total, np.float32)
    for a, p, off in zip(foreign, opt.params, opt.offsets):
        g4[off:off + p.numel()] = a.ravel()
    w4 = S.sgd_fp32_emulation(want[2][0], g4, want[2][1], 3, kw)
    opt.step()
    assert np.array_equal(bits(opt.param_arena.cpu().numpy()), bits(w4[0]))
    assert all(p.grad.data_ptr() == gbase + 4 * off for p, off in zip(f.parameters(), opt.offsets))


def test_plain_sgd_has_no_buffer_and_an_empty_state():
    from cl_ica_amd import optim
    f = _model()
    opt = optim.SGD(f.parameters(), lr=0.05)
    assert opt.momentum_buffer is None
    g = _arena_grads(opt, 1)[0]
    want = S.sgd_fp32_emulation(opt.param_arena.cpu().numpy(), g, None, 0, dict(lr=0.05))[0]
    opt.grad_arena.copy_(gpu(g))
    opt.step()
    assert np.array_equal(bits(opt.param_arena.cpu().numpy()), bits(want))
    sd = opt.state_dict()
    assert sd["state"] == {} and sd["param_groups"][0]["momentum"] == 0.0
    torch.optim.SGD(_model().parameters(), lr=1.0).load_state_dict(sd)
    with pytest.raises(ValueError):
        optim.SGD(_model().parameters(), lr=0.1, nesterov=True)


def test_state_dict_round_trips_through_torch():
    from cl_ica_amd import optim
    kw = dict(lr=0.1, momentum=0.9, dampening=0.25, weight_decay=1e-2)
    f = _model()
    opt = optim.SGD(f.parameters(), **kw)
    grads = _arena_grads(opt, 3)
    for g in grads[:2]:
        opt.grad_arena.copy_(gpu(g))
        opt.step()
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0, 1, 2, 3] and all(list(st) == ["momentum_buffer"] for st in sd["state"].values())
    assert {k: sd["param_groups"][0][k] for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize")} == \
        dict(kw, nesterov=False, maximize=False) and sd["param_groups"][0]["params"] == [0, 1, 2, 3]
    # ours -> torch.optim.SGD -> its state_dict -> a fresh flat optimizer over a copy of the parameters
    f2 = _model()
    f2.load_state_dict(f.state_dict())
    topt = torch.optim.SGD(f2.parameters(), lr=1.0)
    topt.load_state_dict(sd)
    tsd = topt.state_dict()
    assert tsd["param_groups"][0]["momentum"] == 0.9 and tsd["param_groups"][0]["dampening"] == 0.25
    for i, p in enumerate(f2.parameters()):
        assert torch.equal(topt.state[p]["momentum_buffer"], sd["state"][i]["momentum_buffer"])
    f3 = _model()
    f3.load_state_dict(f.state_dict())
    opt3 = optim.SGD(f3.parameters(), lr=7.0)      # no momentum at construction: the buffer arrives with the state
    opt3.load_state_dict(tsd)
    assert int(opt3.step_dev.item()) == 1 and opt3.param_groups[0]["lr"] == 0.1 and opt3.param_groups[0]["momentum"] == 0.9
    assert np.array_equal(bits(opt3.momentum_buffer.cpu().numpy()), bits(opt.momentum_buffer.cpu().numpy()))
    for o_ in (opt, opt3):
        o_.grad_arena.copy_(gpu(grads[2]))
        o_.step()
    assert np.array_equal(bits(opt3.param_arena.cpu().numpy()), bits(opt.param_arena.cpu().numpy()))
    # a state without buffers resets the counter: the next update is a first one again
    opt3.load_state_dict(dict(state={}, param_groups=tsd["param_groups"]))
    assert int(opt3.step_dev.item()) == 0


def test_torch_state_dict_loads_and_the_next_step_matches():
    from cl_ica_amd import optim
    kw = dict(lr=0.1, momentum=0.9, nesterov=True)
    f = _model()
    topt = torch.optim.SGD(f.parameters(), **kw)
    f(torch.randn(7, 5, device=dev())).square().sum().backward()
    topt.step()
    tsd = topt.state_dict()
    opt = optim.SGD(f.parameters(), lr=0.5)
    opt.load_state_dict(tsd)
    assert opt.param_groups[0]["nesterov"] is True and int(opt.step_dev.item()) == 1
    for i, p in enumerate(f.parameters()):
        assert torch.equal(opt.momentum_buffer[opt.offsets[i]:opt.offsets[i] + p.numel()].view(p.shape), tsd["state"][i]["momentum_buffer"])
    g = _arena_grads(opt, 1)[0]
    want = S.sgd_fp32_emulation(opt.param_arena.cpu().numpy(), g, opt.momentum_buffer.cpu().numpy(), 1, kw)
    opt.grad_arena.copy_(gpu(g))
    opt.step()
    assert np.array_equal(bits(opt.param_arena.cpu().numpy()), bits(want[0]))
    assert np.array_equal(bits(opt.momentum_buffer.cpu().numpy()), bits(want[1]))


def test_captured_step_replays_to_the_bits_of_eager_steps():
    from cl_ica_amd import optim
    kw = dict(lr=0.1, momentum=0.9, weight_decay=1e-2)
    fa, fb = _model(), _model()
    a, b = optim.SGD(fa.parameters(), **kw), optim.SGD(fb.parameters(), **kw)
    grads = [gpu(g) for g in _arena_grads(a, 3)]
    for g in grads:
        a.grad_arena.copy_(g)
        a.step()
    # warm-up on a side stream, state put back, then the capture on that stream (as Solver.capture does)
    state = (b.param_arena, b.momentum_buffer, b.step_dev)
    snap = [t.clone() for t in state]
    b.grad_arena.copy_(grads[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for dst, src in zip(state, snap):
        dst.copy_(src)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        b.step()
    torch.cuda.synchronize()
    assert int(b.step_dev.item()) == 0      # the capture executed nothing
    for g in grads:
        b.grad_arena.copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    assert int(b.step_dev.item()) == 3 and int(b._ticket.item()) == 0
    assert np.array_equal(bits(b.param_arena.cpu().numpy()), bits(a.param_arena.cpu().numpy()))
    assert np.array_equal(bits(b.momentum_buffer.cpu().numpy()), bits(a.momentum_buffer.cpu().numpy()))
