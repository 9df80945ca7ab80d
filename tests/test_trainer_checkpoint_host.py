"""Checkpoints of the fused trainers without a GPU: the layout of ContrastiveTrainer / SupervisedTrainer.state_dict(), its round trip through
torch.save / torch.load(weights_only=True), interchange of the optimizer slot with torch.optim.Adam, in-place loading, the strict field
checks, the host-side argument checks of the new export / import entry points, and the driver's two flags.  Trainers are built on
device="cpu": host planning only, nothing steps."""
import ctypes
import dataclasses
import os

import pytest
import torch

N, HIDDEN, B = 4, (40, 200, 40), 256
TOP = {"format", "version", "kind", "f", "optimizer", "step", "config", "arith"}
CONFIG = {"sampler", "batch_size", "p", "tau", "alpha", "g_weights", "g_slope", "g_act_kind", "world", "dry_ranks", "layer_shapes", "head"}
ARITH = {"arith", "clica_version", "s16_calibrated", "split16", "loss"}


@pytest.fixture(scope="module")
def lib():
    from cl_ica_amd import _lib
    return _lib.load()


def _gw(seed=0):
    return torch.randn(3, N, N, generator=torch.Generator().manual_seed(seed)) / N ** 0.5


def _f(head=None, hidden=HIDDEN, seed=0):
    from cl_ica_amd import encoders
    torch.manual_seed(seed)
    return encoders.get_mlp(N, N, list(hidden), output_normalization=head)


def _trainer(cls=None, head=None, hidden=HIDDEN, gw=None, spec=None, **kw):
    from cl_ica_amd.engine import ContrastiveTrainer, SamplerSpec
    cls = ContrastiveTrainer if cls is None else cls
    spec = SamplerSpec(n=N, seed=3) if spec is None else spec
    kw.setdefault("batch_size", B)
    return cls(_f(head, hidden), _gw() if gw is None else gw, spec, device="cpu", **kw)


def _stepped(tr, steps=3):
    """What a trainer holds after `steps` steps, as far as the host can tell: moments and a counter (no kernel runs here)."""
    g = torch.Generator().manual_seed(7)
    off = 0
    for prm in tr.f.parameters():
        tr.exp_avg[off:off + prm.numel()].copy_(torch.randn(prm.numel(), generator=g) * 1e-3)
        tr.exp_avg_sq[off:off + prm.numel()].copy_(torch.rand(prm.numel(), generator=g) * 1e-6)
        off += (prm.numel() + 3) // 4 * 4
    tr.step_dev.fill_(steps)
    return tr


def _roundtrip(sd, tmp_path, name="ck.pth"):
    path = os.path.join(str(tmp_path), name)
    torch.save(sd, path)
    return torch.load(path, map_location="cpu", weights_only=True)


def test_state_dict_layout_and_roundtrip(tmp_path):
    from cl_ica_amd import _lib
    from cl_ica_amd.engine import SupervisedTrainer
    tr = _stepped(_trainer(head="learnable_box"))
    sd = tr.state_dict()
    assert set(sd) == TOP and set(sd["config"]) == CONFIG and set(sd["arith"]) == ARITH
    assert (sd["format"], sd["version"], sd["kind"], sd["step"]) == ("cl_ica_amd.trainer", 1, "contrastive", 3)
    assert list(sd["f"]) == list(tr.f.state_dict())
    assert all(v.device.type == "cpu" and torch.equal(v, tr.f.state_dict()[k]) for k, v in sd["f"].items())
    assert sd["config"]["sampler"] == {**dataclasses.asdict(tr.sampler), "box": [0.0, 1.0]}
    assert sd["config"]["layer_shapes"] == [[40, N], [200, 40], [40, 200], [N, 40]] and "learnable" in sd["config"]["head"]
    assert (sd["config"]["batch_size"], sd["config"]["p"], sd["config"]["world"], sd["config"]["dry_ranks"]) == (B, 2.0, 1, 1)
    assert torch.equal(sd["config"]["g_weights"], tr.gW)
    assert sd["arith"]["arith"] == tr.arith_state()["arith"] and sd["arith"]["clica_version"] == _lib.load().clica_version()
    assert sd["arith"]["split16"] is None and sd["arith"]["loss"] is None        # no device state on a host-only trainer
    params = list(tr.f.parameters())
    assert sorted(sd["optimizer"]["state"]) == list(range(len(params))) and sd["optimizer"]["param_groups"][0]["params"] == list(range(len(params)))
    for i, prm in enumerate(params):
        st = sd["optimizer"]["state"][i]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 3.0 and st["exp_avg"].shape == prm.shape
    back = _roundtrip(sd, tmp_path)
    assert set(back) == TOP and back["step"] == 3 and back["config"]["sampler"] == sd["config"]["sampler"]
    assert all(torch.equal(back["f"][k], v) for k, v in sd["f"].items())
    assert all(torch.equal(back["optimizer"]["state"][i]["exp_avg_sq"], sd["optimizer"]["state"][i]["exp_avg_sq"]) for i in range(len(params)))
    # a trainer that has not stepped has no optimizer state, as torch.optim.Adam and cl_ica_amd.optim.Adam
    assert _trainer().state_dict()["optimizer"]["state"] == {}
    sup = _trainer(SupervisedTrainer).state_dict()
    assert sup["kind"] == "supervised" and sup["config"]["p"] is None and set(sup) == TOP


def test_optimizer_slot_loads_into_torch_adam_and_steps(tmp_path):
    tr = _stepped(_trainer())
    sd = _roundtrip(tr.state_dict(), tmp_path)
    f2 = _f(seed=5)
    f2.load_state_dict(sd["f"])                        # the reference's keys: what unsup_f.pth holds
    opt = torch.optim.Adam(f2.parameters(), lr=1e-4)
    m0 = sd["optimizer"]["state"][0]["exp_avg"].clone()      # (torch's optimizer may keep the loaded tensors themselves)
    opt.load_state_dict(sd["optimizer"])
    before = [p.detach().clone() for p in f2.parameters()]
    for p in f2.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    st = opt.state_dict()["state"]
    assert all(float(st[i]["step"]) == 4.0 for i in st)
    assert all(not torch.equal(b, p) for b, p in zip(before, f2.parameters()))
    assert torch.allclose(st[0]["exp_avg"], 0.9 * m0 + 0.1, rtol=0, atol=1e-7)


def test_load_state_dict_writes_in_place(tmp_path):
    src = _stepped(_trainer(head="learnable_box"))
    sd = _roundtrip(src.state_dict(), tmp_path)
    dst = _trainer(head="learnable_box")
    dst.f[0].weight.data.add_(1.0)
    owned = lambda t: [x.data_ptr() for x in (t.param_arena, t.grad_arena, t.exp_avg, t.exp_avg_sq, t.step_dev, t.loss_ws, t.z)] + \
        [p.data_ptr() for p in t.f.parameters()]
    ptrs = owned(dst)
    from cl_ica_amd import ops
    epoch = ops.PARAM_EPOCH
    assert dst.load_state_dict(sd) == "exact"
    assert owned(dst) == ptrs
    assert ops.PARAM_EPOCH == epoch + 1 and dst._versions_seen == dst._param_versions() and not dst._packed_current
    assert torch.equal(dst.param_arena, src.param_arena) and torch.equal(dst.exp_avg, src.exp_avg) and torch.equal(dst.exp_avg_sq, src.exp_avg_sq)
    assert dst.steps_done == 3
    # a checkpoint from before the first step empties the moments again
    assert dst.load_state_dict(_trainer(head="learnable_box").state_dict()) == "exact"
    assert dst.steps_done == 0 and not dst.exp_avg.any() and not dst.exp_avg_sq.any() and owned(dst) == ptrs


def test_portable_domain_is_reported():
    src = _stepped(_trainer())
    sd = src.state_dict()
    sd["arith"] = dict(sd["arith"], arith="f16x2")
    dst = _trainer()
    assert dst.load_state_dict(sd) == "portable"
    assert torch.equal(dst.param_arena, src.param_arena) and torch.equal(dst.exp_avg, src.exp_avg) and dst.steps_done == 3
    sd["arith"] = dict(src.state_dict()["arith"], clica_version=99)
    assert dst.load_state_dict(sd) == "portable"


def _variants():
    from cl_ica_amd.engine import SamplerSpec
    base = dataclasses.asdict(SamplerSpec(n=N, seed=3))
    other = dict(space="real", box=(0.0, 2.0), marginal="normal", m_param=2.0, m_p=1.0, conditional="laplace", c_param=0.1, c_p=1.0, seed=4)
    cases = [("sampler.%s" % k, dict(spec=SamplerSpec(**{**base, k: v}))) for k, v in other.items()]
    cases += [("batch_size", dict(batch_size=128)), ("p", dict(p=1)), ("tau", dict(tau=0.5)), ("alpha", dict(alpha=0.25)),
              ("g_weights", dict(gw=_gw(1))), ("head", dict(head="learnable_box")), ("optimizer.lr", dict(lr=3e-4))]
    return cases


@pytest.mark.parametrize("field,change", _variants(), ids=[c[0] for c in _variants()])
def test_strict_names_the_field_and_lenient_accepts(field, change):
    sd = _stepped(_trainer()).state_dict()
    dst = _trainer(**change)
    if field == "head":
        sd["f"] = {**sd["f"], **{k: v for k, v in dst.f.state_dict().items() if k not in sd["f"]}}     # (the head's own entry: shapes bind always)
    with pytest.raises(ValueError, match=r"`%s`" % field.replace(".", r"\.")):
        dst.load_state_dict(sd, strict=True)
    assert dst.steps_done == 0                          # refused before anything was written
    assert dst.load_state_dict(sd, strict=False) in ("exact", "portable") and dst.steps_done == 3


def test_kind_shapes_world_and_format_bind():
    from cl_ica_amd.engine import SupervisedTrainer
    sd = _stepped(_trainer()).state_dict()
    for strict in (True, False):
        with pytest.raises(ValueError, match="`kind`"):
            _trainer(SupervisedTrainer).load_state_dict(sd, strict=strict)
        with pytest.raises(ValueError, match="`layer_shapes`"):
            _trainer(hidden=(40, 120, 40)).load_state_dict(sd, strict=strict)
        with pytest.raises(ValueError, match="cl_ica_amd.trainer"):
            _trainer().load_state_dict(dict(sd, format="something else"), strict=strict)
        with pytest.raises(ValueError, match="version"):
            _trainer().load_state_dict(dict(sd, version=2), strict=strict)
    for key in ("world", "dry_ranks"):                  # (other values cannot be built here: the saved side is edited)
        bad = dict(sd, config=dict(sd["config"], **{key: 8}))
        with pytest.raises(ValueError, match="`%s`" % key):
            _trainer().load_state_dict(bad, strict=True)
        assert _trainer().load_state_dict(bad, strict=False) == "exact"


def test_new_entry_points_declared_and_sized(lib):
    from cl_ica_amd import _lib
    for name in ("clica_split16_export_bytes", "clica_split16_export", "clica_split16_import", "clica_lp_loss_train_state_bytes",
                 "clica_lp_loss_train_state_export", "clica_lp_loss_train_state_import"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    nb, full = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.clica_split16_export_bytes(ctypes.byref(nb)) == 0 and lib.clica_split16_state_bytes(ctypes.byref(full)) == 0
    assert 7 * 4 + 6 * 9 * 4 <= nb.value <= 1024 < full.value        # the words and scale arrays the issue lists; no slot arrays
    assert lib.clica_split16_export_bytes(None) == -1 and b"NULL" in lib.clica_last_error()
    assert lib.clica_lp_loss_train_state_bytes(ctypes.byref(nb)) == 0 and 256 <= nb.value <= 1024
    assert lib.clica_lp_loss_train_state_bytes(None) == -1 and b"NULL" in lib.clica_last_error()


def test_export_import_argument_checks_fail_loudly(lib):
    """Every check runs on the host before anything is launched or read: dummy device addresses never reach the runtime."""
    from cl_ica_amd import _lib
    P = 1 << 20
    nb = ctypes.c_size_t()
    assert lib.clica_split16_export_bytes(ctypes.byref(nb)) == 0
    n16 = nb.value
    assert lib.clica_split16_export(None, 4, P, n16, None) == -1 and b"NULL" in lib.clica_last_error()
    assert lib.clica_split16_export(P, 4, None, n16, None) == -1 and b"NULL" in lib.clica_last_error()
    assert lib.clica_split16_export(P, 0, P, n16, None) == -1 and b"n_layers" in lib.clica_last_error()
    assert lib.clica_split16_export(P, 4, P, n16 - 4, None) == -1 and b"blob" in lib.clica_last_error()
    assert lib.clica_split16_import(None, P, n16, 4, None) == -1 and b"NULL" in lib.clica_last_error()
    assert lib.clica_split16_import(P, None, n16, 4, None) == -1 and b"NULL" in lib.clica_last_error()
    assert lib.clica_split16_import(P, P, n16, 0, None) == -1 and b"n_layers" in lib.clica_last_error()
    assert lib.clica_split16_import(P, P, n16, 9, None) == -1 and b"n_layers" in lib.clica_last_error()
    assert lib.clica_split16_import(P, P, n16 - 1, 4, None) == -1 and b"blob" in lib.clica_last_error()
    d = _lib.LpLossDesc(B=1024, B3=1024, n=10, p=2.0, tau=1.0, alpha=0.5, compat=1, pow=1)
    ws = ctypes.c_size_t()
    assert lib.clica_lp_loss_train_workspace_bytes(ctypes.byref(d), ctypes.byref(ws)) == 0
    assert lib.clica_lp_loss_train_state_bytes(ctypes.byref(nb)) == 0
    nl = nb.value
    for fn in (lib.clica_lp_loss_train_state_export, lib.clica_lp_loss_train_state_import):
        assert fn(None, P, ws.value, P, nl, None) == -1
        assert fn(ctypes.byref(d), None, ws.value, P, nl, None) == -1 and b"NULL" in lib.clica_last_error()
        assert fn(ctypes.byref(d), P, ws.value, None, nl, None) == -1 and b"NULL" in lib.clica_last_error()
        assert fn(ctypes.byref(d), P, ws.value, P, nl - 4, None) == -1 and b"blob" in lib.clica_last_error()
        bad = _lib.LpLossDesc(B=4, B3=4, n=513, p=2.0, tau=1.0, alpha=0.5, compat=1, pow=1)
        assert fn(ctypes.byref(bad), P, ws.value, P, nl, None) == -1 and b"n=513" in lib.clica_last_error()
    # a shape the matrix-core sweeps never serve has no such words: its import returns before it looks at the blob
    wide = _lib.LpLossDesc(B=256, B3=256, n=40, p=2.0, tau=1.0, alpha=0.5, compat=1, pow=1)
    assert lib.clica_lp_loss_train_state_import(ctypes.byref(wide), P, 1 << 30, P, nl, None) == 0


def test_wrappers_refuse_what_is_not_a_blob():
    from cl_ica_amd import _lib, ops
    assert hasattr(ops.Split16, "export_state") and hasattr(ops.Split16, "import_state")
    d = _lib.LpLossDesc(B=256, B3=256, n=4, p=2.0, tau=1.0, alpha=0.5, compat=1, pow=1)
    with pytest.raises(_lib.ClicaError, match="uint8"):
        ops.lp_loss_train_state_import(d, torch.zeros(8, dtype=torch.uint8), torch.zeros(8))
    # the dot pair carries nothing: an all-zero blob out, a no-op in (no library call, so it runs here)
    dd = _lib.DotLossDesc(B=256, B3=256, n=4, tau=1.0, alpha=0.5, normalize=0)
    blob = ops.lp_loss_train_state_export(dd, torch.zeros(8, dtype=torch.uint8))
    assert blob.dtype == torch.uint8 and not blob.any()
    ops.lp_loss_train_state_import(dd, torch.zeros(8, dtype=torch.uint8), blob)


def test_driver_flags_and_seed_contradiction(tmp_path):
    from cl_ica_amd import train_mlp
    a = train_mlp.parse_args([])
    assert a.checkpoint_every == 0 and a.resume_from == ""
    a = train_mlp.parse_args(["--checkpoint-every", "6", "--save-dir", str(tmp_path), "--n", "4", "--seed", "1"])
    assert a.checkpoint_every == 6
    with pytest.raises(SystemExit):
        train_mlp.parse_args(["--checkpoint-every", "-1"])
    # a checkpoint as the driver writes it (the trainer's dict + the `driver` section), written through the driver's own writer
    sd = _stepped(_trainer()).state_dict()
    sd["driver"] = dict(phase="unsup", phase_done=False, global_step=7, losses=[1.0] * 6, lin_scores=[0.5] * 6, perm_scores=[0.5] * 6,
                        spaces_state=dict(seed=1000003, draw=4), seed=1, torch_rng_state=torch.get_rng_state(),
                        args={k: getattr(a, k) for k in train_mlp._TRAJECTORY})
    path = os.path.join(str(tmp_path), "unsup_trainer.pth")
    train_mlp.write_checkpoint(path, sd)
    assert os.listdir(str(tmp_path)) == ["unsup_trainer.pth"]          # (the temporary name is gone)
    ok = train_mlp.parse_args(["--resume-from", path, "--n", "4", "--seed", "1"])
    assert ok.resume_from == path
    assert train_mlp.parse_args(["--resume-from", path, "--n", "4"]).seed is None        # no --seed: the file's is taken
    with pytest.raises(SystemExit):
        train_mlp.parse_args(["--resume-from", path, "--n", "4", "--seed", "2"])
    with pytest.raises(ValueError, match="--seed 2 contradicts"):
        train_mlp.check_resume(train_mlp.parse_args(["--n", "4", "--seed", "2"]), sd["driver"])
    with pytest.raises(ValueError, match="--batch-size"):
        train_mlp.check_resume(train_mlp.parse_args(["--n", "4", "--seed", "1", "--batch-size", "512"]), sd["driver"])
    with pytest.raises(SystemExit):
        train_mlp.parse_args(["--resume-from", path, "--n", "4", "--tau", "0.5"])
    with pytest.raises(SystemExit):
        train_mlp.parse_args(["--resume-from", os.path.join(str(tmp_path), "missing.pth")])
