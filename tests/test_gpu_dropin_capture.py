"""Captured drop-in training steps (`cl_ica_amd.capture_train_step`) at the benchmarked shape, next to other encoder work.

bench.py's `dropin.captured` leg replays the reference's unchanged train_step closure at B = 6144: 12 288 stacked rows take the
whole-encoder kernels, their fragment-order weight packs, weight-gradient slabs and, under `cl_ica_amd.optim.Adam`, the f16x2 arithmetic
with its device-side guard.  Every test walks two worlds in lockstep.  In world C encoder A trains through the replaying callable; in
world E its twin runs the closure eagerly.  Both worlds do the same interfering work in the same order: a second encoder's steps and
evaluation calls, other batch shapes, out-of-range batches.  The same kernels run on the same inputs, so the worlds agree to fp32
rounding, and what the interfering work computes is checked against the fp64 oracle at the weights it ran with.

Before every call of the replaying callable the host checks that every cache-held buffer the capture created (and A's weight pack and
f16x2 state) is still alive and that no other encoder's pack shares its memory: a graph whose buffers were freed or handed to another
encoder is never replayed."""
import weakref

import numpy as np
import pytest
import torch

from conftest import PARITY
from oracle import np_oracle as O
from test_gpu_next_rows import build_mlp_n10

pytestmark = pytest.mark.gpu

N, B, STEPS = 10, 6144, 6
FAM = "dropin_capture_isolation"


@pytest.fixture(params=["f16x2", "bf16x3", "fp32"])
def arith(request, monkeypatch):
    """f16x2: cl_ica_amd.optim.Adam; bf16x3: torch.optim.Adam(capturable=True); fp32: the fp32-MFMA whole-encoder kernels (flat Adam)."""
    _set_arith(request.param, monkeypatch)
    return request.param


def _set_arith(arith, monkeypatch):
    from cl_ica_amd import encoders
    monkeypatch.setenv("CLICA_SPLIT_BF16", "0" if arith == "fp32" else "1")
    monkeypatch.setenv("CLICA_SPLIT_ARITH", "f16")
    monkeypatch.setattr(encoders, "S16_ENABLED", True)
    monkeypatch.setattr(encoders, "FUSED_MODE", "auto")


def _batches(seed, k, rows=B, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(k):
        x1 = torch.rand(rows, N, generator=g)
        x2 = (x1 + 0.05 * torch.randn(rows, N, generator=g)).clamp(0, 1)
        out.append(((x1 * scale).cuda(), (x2 * scale).cuda()))
    return out


class _Enc:
    """One encoder with its optimizer, loss and the reference's train_step closure (main_mlp.py:258-285)."""

    def __init__(self, arith):
        from cl_ica_amd import losses, optim
        self.arith = arith
        self.f = f = build_mlp_n10().cuda()
        self.opt = (torch.optim.Adam(f.parameters(), lr=1e-3, capturable=True) if arith == "bf16x3" else
                    optim.Adam(f.parameters(), lr=1e-3))
        self.loss = losses.LpSimCLRLoss(p=2, tau=1.0, simclr_compatibility_mode=True)

        def train_step(data, loss, optimizer):
            z1, z2_con_z1 = data
            z3 = torch.roll(z1, 1, 0)
            optimizer.zero_grad()
            z1_rec = f(z1)
            z2_con_z1_rec = f(z2_con_z1)
            z3_rec = torch.roll(z1_rec, 1, 0)
            total_loss_value, _, losses_value = loss(z1, z2_con_z1, z3, z1_rec, z2_con_z1_rec, z3_rec)
            total_loss_value.backward()
            optimizer.step()
            return total_loss_value.item(), [v.item() for v in losses_value]
        self.closure = train_step
        self.replay, self.watch = None, None

    def warm(self, data):
        """What capture_train_step's warm-up does: three ordinary steps on `data` (the recording itself launches nothing)."""
        for _ in range(3):
            self.closure(data, self.loss, self.opt)

    def capture(self, data):
        import cl_ica_amd
        before = _cache_tensors()
        self.replay = cl_ica_amd.capture_train_step(self.closure, data, self.loss, self.opt, warmup=3)
        self.watch = _Watch(self, before)

    def call(self, data):
        if self.replay is None:
            return self.closure(data, self.loss, self.opt)
        self.watch.check()              # never replay a graph whose buffers are gone or belong to another encoder now
        return self.replay(data, self.loss, self.opt)

    def step(self, data):
        """An eager training step that keeps what the fp64 check needs: (loss, embeddings z1, z2, parameter gradients)."""
        from cl_ica_amd import lazy
        x1, x2 = data
        self.opt.zero_grad()
        a = self.f(x1)
        b = self.f(x2)
        tot, _, _ = self.loss(None, None, None, a, b, torch.roll(a, 1, 0))
        tot.backward()
        grads = [q.grad.detach().clone() for q in self.f.parameters()]
        lv = tot.item()
        a, b = lazy.plain(a).detach().clone(), b.detach().clone()
        self.opt.step()
        return lv, a, b, grads

    def weight_ptrs(self):
        return tuple(m.weight.data_ptr() for m in self.f if isinstance(m, torch.nn.Linear))


def _weight_ptrs(key):
    return tuple(k[0] for k in key[1:])       # (the weights' data pointers in a pack key: whose weights the entry holds)


def _pack_caches():
    from cl_ica_amd import encoders
    return [c for cls in (encoders._MLPFusedFn, encoders._MLPFusedSplitFn) for c in cls._pack_cache.values()]


def _cache_tensors():
    """Every device buffer the drop-in caches hold (id -> tensor; the dict keeps them alive, so the ids stay unique)."""
    from cl_ica_amd import _lib, encoders
    out = {}
    for c in _pack_caches():
        out[id(c["packed"])] = c["packed"]
        out[id(c["packed_t"])] = c["packed_t"]
    for cls in (encoders._MLPFusedFn, encoders._MLPFusedSplitFn):
        out.update((id(t), t) for t in cls._ws_cache.values())
    out.update((id(t), t) for t in _lib._WS.values())
    return out


class _Watch:
    """Weak references to the buffers a capture created or replaced in the caches, to the captured encoder's weight pack and to its f16x2
    state -- what the recorded launches read and write through raw pointers."""

    def __init__(self, enc, before):
        after = _cache_tensors()
        held = [t for k, t in after.items() if k not in before]
        self.wptrs = enc.weight_ptrs()
        pack = [c[k] for c in _pack_caches() if _weight_ptrs(c["key"]) == self.wptrs for k in ("packed", "packed_t")]
        assert pack, "the captured encoder has no weight pack in the cache"
        lin0 = next(m for m in enc.f if isinstance(m, torch.nn.Linear))
        s16 = lin0.weight.__dict__.get("_clica_s16")
        if s16 is not None:
            held.append(s16.state.buf)
        held = list({id(t): t for t in held + pack}.values())
        self.refs = [weakref.ref(t) for t in held]
        self.pack_ptrs = {t.data_ptr() for t in pack}
        owned = getattr(enc.replay, "owned", None)
        if owned is not None:          # the replaying callable holds them itself
            mine = {id(t) for t in owned}
            assert all(id(t) in mine for t in pack + ([s16.state.buf] if s16 is not None else [])), "replay.owned misses the pack / state"

    def check(self):
        dead = sum(r() is None for r in self.refs)
        assert dead == 0, f"{dead} of {len(self.refs)} buffers the captured graph replays were freed by a cache"
        for c in _pack_caches():
            if _weight_ptrs(c["key"]) != self.wptrs:
                assert c["packed"].data_ptr() not in self.pack_ptrs and c["packed_t"].data_ptr() not in self.pack_ptrs, \
                    "another encoder's weight pack lives in the buffers the captured graph replays"


def _worlds(arith, data0, extra=0):
    """World C: A captured on `data0` (+ `extra` more encoders); world E: A's eager twin after the same three warm-up steps."""
    from cl_ica_amd import encoders
    C = [_Enc(arith) for _ in range(1 + extra)]
    E = [_Enc(arith) for _ in range(1 + extra)]
    for c, e in zip(C, E):
        for q, r in zip(c.f.parameters(), e.f.parameters()):
            assert torch.equal(q, r)
    C[0].capture(data0)
    E[0].warm(data0)
    assert encoders.arith_state(C[0].f)["arith"] == arith and encoders.arith_state(E[0].f)["arith"] == arith
    return C, E


def _lockstep(case, got, ref, ec, ee):
    from cl_ica_amd import encoders
    np.testing.assert_allclose(got[0], ref[0], rtol=2e-6, atol=0, err_msg=case)
    if len(got) > 1 and isinstance(got[1], list):
        np.testing.assert_allclose(got[1], ref[1], rtol=2e-6, atol=0, err_msg=case)
    for q, r in zip(ec.f.parameters(), ee.f.parameters()):
        d = (q.detach() - r.detach()).abs().max().item()
        assert d <= 2e-6 * max(1.0, r.detach().abs().max().item()), (case, d)
    if ec.arith == "f16x2":
        sc, se = encoders.arith_state(ec.f), encoders.arith_state(ee.f)
        for k in ("scales_a", "scales_d", "scales_w", "flags", "skipped"):
            assert sc[k] == se[k], (case, k, sc[k], se[k])


def _params64(f):
    lin = [m for m in f if isinstance(m, torch.nn.Linear)]
    return O.MLPParams([m.weight.detach().cpu().numpy() for m in lin], [m.bias.detach().cpu().numpy() for m in lin])


def _check_step(case, P, data, lv, a=None, b=None, grads=None):
    """Loss (and embeddings, weight gradients) of one training step against the fp64 oracle at the weights `P` it ran with."""
    x = np.concatenate([data[0].cpu().numpy(), data[1].cpu().numpy()]).astype(np.float64)
    y, cache = O.mlp_forward(P, x)
    ref = O.lp_simclr_loss(y[:B], y[B:], np.roll(y[:B], 1, 0), p=2, compat=True, grad=grads is not None)
    PARITY.check(FAM, case, "loss", lv, ref["loss_mean"])
    if a is not None:
        PARITY.check(FAM, case, "embeddings z1", a.cpu().numpy(), y[:B])
        PARITY.check(FAM, case, "embeddings z2", b.cpu().numpy(), y[B:])
    if grads is not None:
        gy = np.concatenate([ref["dz1"] + np.roll(ref["dz3"], -1, 0), ref["dz2"]])
        gr = O.mlp_backward(P, cache, gy)
        # dW / db are sums over the 12 288 rows that cancel (the loss is translation invariant: the last bias's gradient is exactly 0), so
        # they are held to 1e-5 of the size of their summands, sum_r |dz_r| |a_r| -- what an fp32 sum over those rows can resolve
        acts, g = cache["acts"], gy
        for l in reversed(range(len(P.W))):
            dz = np.abs(g)
            PARITY.check(FAM, case, f"dW{l}", grads[2 * l].cpu().numpy(), gr["dW"][l], floor=float((dz.T @ np.abs(acts[l])).max()))
            PARITY.check(FAM, case, f"db{l}", grads[2 * l + 1].cpu().numpy(), gr["db"][l], floor=float(dz.sum(0).max()))
            g = (g @ P.W[l]) * np.where(acts[l] > 0, 1.0, P.slope)


def _check_forward(case, P, x, y):
    PARITY.check(FAM, case, f"embeddings {x.shape[0]} rows", y.detach().cpu().numpy(), O.mlp_forward(P, x.cpu().numpy().astype(np.float64))[0])


def _replay_vs_oracle(case, A, Ae, data):
    P = _params64(A.f)
    got, ref = A.call(data), Ae.call(data)
    _lockstep(case, got, ref, A, Ae)
    _check_step(case, P, data, got[0])


def test_captured_step_at_the_benchmarked_shape(arith):
    """Scenario 1: the captured step at B = 6144 (whole-encoder kernels) in lockstep with the eager closure."""
    batches = _batches(1, STEPS + 2)
    (A,), (Ae,) = _worlds(arith, batches[0])
    for k in range(1, STEPS + 1):
        _lockstep(f"baseline {arith} step{k}", A.call(batches[k]), Ae.call(batches[k]), A, Ae)
    _replay_vs_oracle(f"baseline {arith} replay", A, Ae, batches[STEPS + 1])


def test_captured_step_next_to_a_second_encoder_eager(arith):
    """Scenario 2: between replays of A, eager training steps of a second encoder B of the same shapes and two consecutive no_grad
    forwards of B.  B must neither run on A's weight pack nor hand A its own."""
    batches, other, evals = _batches(2, 6), _batches(3, 4), _batches(4, 1)[0]
    (A, Bc), (Ae, Be) = _worlds(arith, batches[0], extra=1)
    for k in range(1, 5):
        _lockstep(f"2nd eager {arith} A step{k}", A.call(batches[k]), Ae.call(batches[k]), A, Ae)
        P = _params64(Bc.f)
        rc, re = Bc.step(other[k - 1]), Be.step(other[k - 1])
        _lockstep(f"2nd eager {arith} B step{k}", rc, re, Bc, Be)
        gmax = max(v.abs().max().item() for v in re[3])          # (floor: the last bias's gradient is exactly 0 up to rounding)
        for u, v in zip(rc[3], re[3]):
            assert (u - v).abs().max().item() <= 2e-6 * max(v.abs().max().item(), 1e-3 * gmax), f"B's gradients differ from its twin's (step {k})"
        if k == 1:
            # weight gradients against fp64 in the fp32 arithmetic only: the oracle's backward takes the fp64 SIGNS of the hidden
            # activations, and in the split arithmetics a pre-activation within their rounding of 0 flips one row's mask (measured
            # 3e-5 / 4e-4 of the summand scale in f16x2 / bf16x3 on this batch) -- the engine's tests feed the oracle the kernels'
            # own activations for that reason; the drop-in path keeps them packed
            _check_step(f"2nd eager {arith} B step{k}", P, other[k - 1], *(rc if arith == "fp32" else rc[:3]))
        P = _params64(Bc.f)
        with torch.no_grad():
            ys = [Bc.f(x) for x in evals]
            ye = [Be.f(x) for x in evals]
        for y, z in zip(ys, ye):
            assert (y - z).abs().max().item() <= 2e-6 * max(1.0, z.abs().max().item())
        if k == 2:
            for x, y in zip(evals, ys):
                _check_forward(f"2nd eager {arith} B no_grad", P, x, y)
    _replay_vs_oracle(f"2nd eager {arith} A replay", A, Ae, batches[5])


def test_two_captured_steps_alternate(arith):
    """Scenario 3: a second encoder B captured as well; replays of A and B alternate, each in lockstep with its eager twin."""
    batches, other = _batches(5, 6), _batches(6, 6)
    (A, Bc), (Ae, Be) = _worlds(arith, batches[0], extra=1)
    Bc.capture(other[0])
    Be.warm(other[0])
    for k in range(1, 5):
        _lockstep(f"2nd captured {arith} A step{k}", A.call(batches[k]), Ae.call(batches[k]), A, Ae)
        _lockstep(f"2nd captured {arith} B step{k}", Bc.call(other[k]), Be.call(other[k]), Bc, Be)
    _replay_vs_oracle(f"2nd captured {arith} A replay", A, Ae, batches[5])
    _replay_vs_oracle(f"2nd captured {arith} B replay", Bc, Be, other[5])


def test_captured_step_after_other_batch_shapes_and_an_eval_call(arith):
    """Scenario 4: the replaying callable called with four other batch sizes (the closure runs eagerly: more (stream, rows) workspace keys
    than the caches keep) and a no_grad forward of 4 096 rows, then replayed again -- in lockstep with a twin that took the same steps."""
    batches = _batches(7, 6)
    (A,), (Ae,) = _worlds(arith, batches[0])
    for k in (1, 2):
        _lockstep(f"other shapes {arith} step{k}", A.call(batches[k]), Ae.call(batches[k]), A, Ae)
    for i, rows in enumerate((4096, 5120, 7168, 8192)):
        d = _batches(70 + i, 1, rows=rows)[0]
        _lockstep(f"other shapes {arith} fallback {rows}", A.call(d), Ae.call(d), A, Ae)
    x = _batches(80, 1, rows=4096)[0][0]
    P = _params64(A.f)
    with torch.no_grad():
        y, ye = A.f(x), Ae.f(x)
    assert (y - ye).abs().max().item() <= 2e-6 * max(1.0, ye.abs().max().item())
    _check_forward(f"other shapes {arith} no_grad", P, x, y)
    for k in (3, 4):
        _lockstep(f"other shapes {arith} step{k}", A.call(batches[k]), Ae.call(batches[k]), A, Ae)
    _replay_vs_oracle(f"other shapes {arith} replay", A, Ae, batches[5])


def test_guard_inside_the_replay(monkeypatch):
    """Scenario 5 (f16x2): a batch 1 000 x beyond the scales fed to the replay and to the eager twin.  Both withhold the same steps (the guard
    acts on the device, inside the graph), and once a step is applied they agree bit for bit on parameters and moments."""
    from cl_ica_amd import encoders
    _set_arith("f16x2", monkeypatch)
    batches = _batches(9, 6)
    (A,), (Ae,) = _worlds("f16x2", batches[0])
    for k in (1, 2):
        _lockstep(f"guard step{k}", A.call(batches[k]), Ae.call(batches[k]), A, Ae)
    big = (batches[3][0] * 1000.0, batches[3][1] * 1000.0)
    t0 = int(A.opt.step_dev.item())
    assert int(Ae.opt.step_dev.item()) == t0
    for tries in range(1, 13):
        got, ref = A.call(big), Ae.call(big)
        np.testing.assert_allclose(got[0], ref[0], rtol=2e-6, atol=0, equal_nan=True)
        sc, se = encoders.arith_state(A.f), encoders.arith_state(Ae.f)
        assert (sc["skipped"], sc["flags"]) == (se["skipped"], se["flags"]), (tries, sc, se)
        t = int(A.opt.step_dev.item())
        assert t == int(Ae.opt.step_dev.item()), tries
        if t > t0:
            break
    assert t == t0 + 1 and sc["skipped"] >= 1 and (sc["flags"] & 2) and not (sc["flags"] & 4), (tries, sc)
    for u, v in zip((A.opt.param_arena, A.opt.exp_avg, A.opt.exp_avg_sq), (Ae.opt.param_arena, Ae.opt.exp_avg, Ae.opt.exp_avg_sq)):
        assert torch.equal(u, v), "replay and eager closure differ after the guard"
    _replay_vs_oracle("guard replay after", A, Ae, batches[4])


def test_forwards_outside_a_step_leave_the_f16x2_state_alone(monkeypatch):
    """B: evaluation forwards (no_grad of 4 096 and 20 000 rows, inference_mode, no_grad of a 1 000 x batch) between the steps of one of
    two f16x2 encoders in lockstep.  They leave `arith_state` as it was, the two encoders keep agreeing on parameters, moments, scales and
    withheld steps, and every such forward is within 1e-5 of fp64 -- the 1 000 x batch included."""
    from cl_ica_amd import encoders
    _set_arith("f16x2", monkeypatch)
    batches = _batches(11, 5)
    E1, E2 = _Enc("f16x2"), _Enc("f16x2")
    xs = [("no_grad", _batches(12, 1, rows=4096)[0][0]), ("no_grad", _batches(13, 1, rows=20000)[0][0]),
          ("inference_mode", _batches(14, 1)[0][0]), ("no_grad", _batches(15, 1, scale=1000.0)[0][0])]
    for k in range(5):
        _lockstep(f"eval forwards step{k}", E1.step(batches[k]), E2.step(batches[k]), E1, E2)
        assert encoders.arith_state(E1.f)["arith"] == "f16x2"
        if k in (1, 2):
            P = _params64(E1.f)
            for mode, x in xs:
                st = encoders.arith_state(E1.f)
                with (torch.no_grad() if mode == "no_grad" else torch.inference_mode()):
                    y = E1.f(x)
                assert encoders.arith_state(E1.f) == st, (mode, x.shape[0])
                if k == 1:
                    _check_forward(f"eval forwards {mode} x{float(x.abs().max()):.0f}", P, x, y)
    for u, v in zip((E1.opt.param_arena, E1.opt.exp_avg, E1.opt.exp_avg_sq), (E2.opt.param_arena, E2.opt.exp_avg, E2.opt.exp_avg_sq)):
        assert (u - v).abs().max().item() <= 2e-6 * max(1.0, v.abs().max().item())
    s1, s2 = encoders.arith_state(E1.f), encoders.arith_state(E2.f)
    assert s1 == s2 and s1["skipped"] == 0, (s1, s2)
