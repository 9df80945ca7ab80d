"""The fused trainers' encoder path as a host decision: plan_encoder() maps layer shapes and arguments to an EncoderPlan without a launch or an
allocation, the trainer's flags are copies of its fields, and an encoder the kernels cannot run is refused by name.  No GPU: the rows
with gpu=True only ask the planner what it would decide there."""
import dataclasses

import pytest
import torch

N, B = 10, 200
FLAGS = ("fused_forward", "fused_backward", "mix_in_forward", "split_bf16", "split_f16", "split_wgrad", "split_wgrad_wide", "split_f16_wide")

# Expected values: the attributes of ContrastiveTrainer as constructed at commit bc7c10f (the parent of EncoderPlan), n = 10, B = 200, printed
# there on the CPU (gpu=False: native fp32 and bf16x3 without a chain; f16 falls back to bf16x3 off the GPU) and on an MI355X (gpu=True).
# chain_min was no attribute there: 384 / 1024 / 0 as the parent's _allocate chose it from split_f16_wide / split_wgrad_wide.  Columns:
# hidden widths, fused_forward argument, split_bf16 argument, split_arith argument, keep_fp32_copies, device is a GPU ->
# arith, the flags that are set, kinds, wide_kinds, chain, chain_min, indices of the planes-only acts_out / dz_out entries.
ROWS = [
    ((), True, False, 'f16', False, True, 'native_fp32', 'fused_forward mix_in_forward', (), (), (), 0, (), ()),
    ((), True, False, 'f16', True, True, 'native_fp32', 'fused_forward mix_in_forward', (), (), (), 0, (), ()),
    ((), True, True, 'bf16', False, True, 'native_fp32', 'fused_forward mix_in_forward', (), (), (), 0, (), ()),
    ((), True, True, 'bf16', True, True, 'native_fp32', 'fused_forward mix_in_forward', (), (), (), 0, (), ()),
    ((), True, True, 'f16', False, True, 'native_fp32', 'fused_forward mix_in_forward', (), (), (), 0, (), ()),
    ((), True, True, 'f16', True, True, 'native_fp32', 'fused_forward mix_in_forward', (), (), (), 0, (), ()),
    ((100,), True, False, 'f16', False, True, 'native_fp32', 'fused_forward fused_backward mix_in_forward', (), (), (), 0, (), ()),
    ((100,), True, False, 'f16', True, True, 'native_fp32', 'fused_forward fused_backward mix_in_forward', (), (), (), 0, (), ()),
    ((100,), True, True, 'bf16', False, True, 'bf16x3', 'fused_forward fused_backward mix_in_forward split_bf16', (1, 1), (), (), 0, (), ()),
    ((100,), True, True, 'bf16', True, True, 'bf16x3', 'fused_forward fused_backward mix_in_forward split_bf16', (1, 1), (), (), 0, (), ()),
    ((100,), True, True, 'f16', False, True, 'f16x2', 'fused_forward fused_backward mix_in_forward split_bf16 split_f16', (1, 1), (), (), 0, (), ()),
    ((100,), True, True, 'f16', True, True, 'f16x2', 'fused_forward fused_backward mix_in_forward split_bf16 split_f16', (1, 1), (), (), 0, (), ()),
    ((100, 640, 640, 100), True, False, 'f16', False, True, 'native_fp32', '', (), (), (), 0, (), ()),
    ((100, 640, 640, 100), True, False, 'f16', True, True, 'native_fp32', '', (), (), (), 0, (), ()),
    ((100, 640, 640, 100), True, True, 'bf16', False, True, 'bf16x3', 'split_wgrad_wide', (), (1, 0, 0, 0, 1), (), 1024, (), ()),
    ((100, 640, 640, 100), True, True, 'bf16', True, True, 'bf16x3', 'split_wgrad_wide', (), (1, 0, 0, 0, 1), (), 1024, (), ()),
    ((100, 640, 640, 100), True, True, 'f16', False, True, 'f16x2', 'split_wgrad_wide split_f16_wide', (), (1, 0, 0, 0, 1), (2,), 384, (), ()),
    ((100, 640, 640, 100), True, True, 'f16', True, True, 'f16x2', 'split_wgrad_wide split_f16_wide', (), (1, 0, 0, 0, 1), (2,), 384, (), ()),
    ((100, 600, 100), True, False, 'f16', False, True, 'native_fp32', '', (), (), (), 0, (), ()),
    ((100, 600, 100), True, False, 'f16', True, True, 'native_fp32', '', (), (), (), 0, (), ()),
    ((100, 600, 100), True, True, 'bf16', False, True, 'bf16x3', 'split_wgrad_wide', (), (1, 0, 0, 1), (), 1024, (), ()),
    ((100, 600, 100), True, True, 'bf16', True, True, 'bf16x3', 'split_wgrad_wide', (), (1, 0, 0, 1), (), 1024, (), ()),
    ((100, 600, 100), True, True, 'f16', False, True, 'f16x2', 'split_wgrad_wide split_f16_wide', (), (1, 0, 0, 1), (), 384, (), ()),
    ((100, 600, 100), True, True, 'f16', True, True, 'f16x2', 'split_wgrad_wide split_f16_wide', (), (1, 0, 0, 1), (), 384, (), ()),
    ((100, 500, 500, 100), False, False, 'f16', False, True, 'native_fp32', '', (), (), (), 0, (), ()),
    ((100, 500, 500, 100), False, False, 'f16', True, True, 'native_fp32', '', (), (), (), 0, (), ()),
    ((100, 500, 500, 100), False, True, 'bf16', False, True, 'bf16x3', 'split_wgrad_wide', (), (1, 0, 0, 0, 1), (), 1024, (), ()),
    ((100, 500, 500, 100), False, True, 'bf16', True, True, 'bf16x3', 'split_wgrad_wide', (), (1, 0, 0, 0, 1), (), 1024, (), ()),
    ((100, 500, 500, 100), False, True, 'f16', False, True, 'f16x2', 'split_wgrad_wide split_f16_wide', (), (1, 0, 0, 0, 1), (2,), 384, (), ()),
    ((100, 500, 500, 100), False, True, 'f16', True, True, 'f16x2', 'split_wgrad_wide split_f16_wide', (), (1, 0, 0, 0, 1), (2,), 384, (), ()),
    ((100, 500, 500, 100), True, False, 'f16', False, True, 'native_fp32', 'fused_forward fused_backward mix_in_forward', (), (), (), 0, (), ()),
    ((100, 500, 500, 100), True, False, 'f16', True, True, 'native_fp32', 'fused_forward fused_backward mix_in_forward', (), (), (), 0, (), ()),
    ((100, 500, 500, 100), True, True, 'bf16', False, True, 'bf16x3', 'fused_forward fused_backward mix_in_forward split_bf16 split_wgrad', (1, 0, 0, 0, 1), (), (), 0, (0, 1, 2), (1, 2, 3)),
    ((100, 500, 500, 100), True, True, 'bf16', True, True, 'bf16x3', 'fused_forward fused_backward mix_in_forward split_bf16 split_wgrad', (1, 0, 0, 0, 1), (), (), 0, (), ()),
    ((100, 500, 500, 100), True, True, 'f16', False, True, 'f16x2', 'fused_forward fused_backward mix_in_forward split_bf16 split_f16 split_wgrad', (1, 0, 0, 0, 1), (), (), 0, (0, 1, 2), (1, 2, 3)),
    ((100, 500, 500, 100), True, True, 'f16', True, True, 'f16x2', 'fused_forward fused_backward mix_in_forward split_bf16 split_f16 split_wgrad', (1, 0, 0, 0, 1), (), (), 0, (), ()),
    ((100, 500, 500, 500, 500, 100), True, False, 'f16', False, True, 'native_fp32', 'fused_forward fused_backward mix_in_forward', (), (), (), 0, (), ()),
    ((100, 500, 500, 500, 500, 100), True, False, 'f16', True, True, 'native_fp32', 'fused_forward fused_backward mix_in_forward', (), (), (), 0, (), ()),
    ((100, 500, 500, 500, 500, 100), True, True, 'bf16', False, True, 'bf16x3', 'fused_forward fused_backward mix_in_forward split_bf16 split_wgrad', (1, 0, 0, 0, 0, 0, 1), (), (), 0, (0, 1, 2, 3, 4), (1, 2, 3, 4, 5)),
    ((100, 500, 500, 500, 500, 100), True, True, 'bf16', True, True, 'bf16x3', 'fused_forward fused_backward mix_in_forward split_bf16 split_wgrad', (1, 0, 0, 0, 0, 0, 1), (), (), 0, (), ()),
    ((100, 500, 500, 500, 500, 100), True, True, 'f16', False, True, 'f16x2', 'fused_forward fused_backward mix_in_forward split_bf16 split_f16 split_wgrad', (1, 0, 0, 0, 0, 0, 1), (), (), 0, (0, 1, 2, 3, 4), (1, 2, 3, 4, 5)),
    ((100, 500, 500, 500, 500, 100), True, True, 'f16', True, True, 'f16x2', 'fused_forward fused_backward mix_in_forward split_bf16 split_f16 split_wgrad', (1, 0, 0, 0, 0, 0, 1), (), (), 0, (), ()),
    ((100, 1024, 1024, 1024, 100), True, False, 'f16', False, True, 'native_fp32', '', (), (), (), 0, (), ()),
    ((100, 1024, 1024, 1024, 100), True, False, 'f16', True, True, 'native_fp32', '', (), (), (), 0, (), ()),
    ((100, 1024, 1024, 1024, 100), True, True, 'bf16', False, True, 'bf16x3', 'split_wgrad_wide', (), (1, 0, 0, 0, 0, 1), (2, 3), 1024, (), ()),
    ((100, 1024, 1024, 1024, 100), True, True, 'bf16', True, True, 'bf16x3', 'split_wgrad_wide', (), (1, 0, 0, 0, 0, 1), (2, 3), 1024, (), ()),
    ((100, 1024, 1024, 1024, 100), True, True, 'f16', False, True, 'f16x2', 'split_wgrad_wide split_f16_wide', (), (1, 0, 0, 0, 0, 1), (2, 3), 384, (), ()),
    ((100, 1024, 1024, 1024, 100), True, True, 'f16', True, True, 'f16x2', 'split_wgrad_wide split_f16_wide', (), (1, 0, 0, 0, 0, 1), (2, 3), 384, (), ()),
    ((), True, False, 'f16', False, False, 'native_fp32', 'fused_forward mix_in_forward', (), (), (), 0, (), ()),
    ((), True, False, 'f16', True, False, 'native_fp32', 'fused_forward mix_in_forward', (), (), (), 0, (), ()),
    ((), True, True, 'bf16', False, False, 'native_fp32', 'fused_forward mix_in_forward', (), (), (), 0, (), ()),
    ((), True, True, 'bf16', True, False, 'native_fp32', 'fused_forward mix_in_forward', (), (), (), 0, (), ()),
    ((), True, True, 'f16', False, False, 'native_fp32', 'fused_forward mix_in_forward', (), (), (), 0, (), ()),
    ((), True, True, 'f16', True, False, 'native_fp32', 'fused_forward mix_in_forward', (), (), (), 0, (), ()),
    ((100,), True, False, 'f16', False, False, 'native_fp32', 'fused_forward fused_backward mix_in_forward', (), (), (), 0, (), ()),
    ((100,), True, False, 'f16', True, False, 'native_fp32', 'fused_forward fused_backward mix_in_forward', (), (), (), 0, (), ()),
    ((100,), True, True, 'bf16', False, False, 'bf16x3', 'fused_forward fused_backward mix_in_forward split_bf16', (1, 1), (), (), 0, (), ()),
    ((100,), True, True, 'bf16', True, False, 'bf16x3', 'fused_forward fused_backward mix_in_forward split_bf16', (1, 1), (), (), 0, (), ()),
    ((100,), True, True, 'f16', False, False, 'bf16x3', 'fused_forward fused_backward mix_in_forward split_bf16', (1, 1), (), (), 0, (), ()),
    ((100,), True, True, 'f16', True, False, 'bf16x3', 'fused_forward fused_backward mix_in_forward split_bf16', (1, 1), (), (), 0, (), ()),
    ((100, 640, 640, 100), True, False, 'f16', False, False, 'native_fp32', '', (), (), (), 0, (), ()),
    ((100, 640, 640, 100), True, False, 'f16', True, False, 'native_fp32', '', (), (), (), 0, (), ()),
    ((100, 640, 640, 100), True, True, 'bf16', False, False, 'bf16x3', 'split_wgrad_wide', (), (1, 0, 0, 0, 1), (), 1024, (), ()),
    ((100, 640, 640, 100), True, True, 'bf16', True, False, 'bf16x3', 'split_wgrad_wide', (), (1, 0, 0, 0, 1), (), 1024, (), ()),
    ((100, 640, 640, 100), True, True, 'f16', False, False, 'bf16x3', 'split_wgrad_wide', (), (1, 0, 0, 0, 1), (), 1024, (), ()),
    ((100, 640, 640, 100), True, True, 'f16', True, False, 'bf16x3', 'split_wgrad_wide', (), (1, 0, 0, 0, 1), (), 1024, (), ()),
    ((100, 600, 100), True, False, 'f16', False, False, 'native_fp32', '', (), (), (), 0, (), ()),
    ((100, 600, 100), True, False, 'f16', True, False, 'native_fp32', '', (), (), (), 0, (), ()),
    ((100, 600, 100), True, True, 'bf16', False, False, 'bf16x3', 'split_wgrad_wide', (), (1, 0, 0, 1), (), 1024, (), ()),
    ((100, 600, 100), True, True, 'bf16', True, False, 'bf16x3', 'split_wgrad_wide', (), (1, 0, 0, 1), (), 1024, (), ()),
    ((100, 600, 100), True, True, 'f16', False, False, 'bf16x3', 'split_wgrad_wide', (), (1, 0, 0, 1), (), 1024, (), ()),
    ((100, 600, 100), True, True, 'f16', True, False, 'bf16x3', 'split_wgrad_wide', (), (1, 0, 0, 1), (), 1024, (), ()),
    ((100, 500, 500, 100), False, False, 'f16', False, False, 'native_fp32', '', (), (), (), 0, (), ()),
    ((100, 500, 500, 100), False, False, 'f16', True, False, 'native_fp32', '', (), (), (), 0, (), ()),
    ((100, 500, 500, 100), False, True, 'bf16', False, False, 'bf16x3', 'split_wgrad_wide', (), (1, 0, 0, 0, 1), (), 1024, (), ()),
    ((100, 500, 500, 100), False, True, 'bf16', True, False, 'bf16x3', 'split_wgrad_wide', (), (1, 0, 0, 0, 1), (), 1024, (), ()),
    ((100, 500, 500, 100), False, True, 'f16', False, False, 'bf16x3', 'split_wgrad_wide', (), (1, 0, 0, 0, 1), (), 1024, (), ()),
    ((100, 500, 500, 100), False, True, 'f16', True, False, 'bf16x3', 'split_wgrad_wide', (), (1, 0, 0, 0, 1), (), 1024, (), ()),
    ((100, 500, 500, 100), True, False, 'f16', False, False, 'native_fp32', 'fused_forward fused_backward mix_in_forward', (), (), (), 0, (), ()),
    ((100, 500, 500, 100), True, False, 'f16', True, False, 'native_fp32', 'fused_forward fused_backward mix_in_forward', (), (), (), 0, (), ()),
    ((100, 500, 500, 100), True, True, 'bf16', False, False, 'bf16x3', 'fused_forward fused_backward mix_in_forward split_bf16 split_wgrad', (1, 0, 0, 0, 1), (), (), 0, (0, 1, 2), (1, 2, 3)),
    ((100, 500, 500, 100), True, True, 'bf16', True, False, 'bf16x3', 'fused_forward fused_backward mix_in_forward split_bf16 split_wgrad', (1, 0, 0, 0, 1), (), (), 0, (), ()),
    ((100, 500, 500, 100), True, True, 'f16', False, False, 'bf16x3', 'fused_forward fused_backward mix_in_forward split_bf16 split_wgrad', (1, 0, 0, 0, 1), (), (), 0, (0, 1, 2), (1, 2, 3)),
    ((100, 500, 500, 100), True, True, 'f16', True, False, 'bf16x3', 'fused_forward fused_backward mix_in_forward split_bf16 split_wgrad', (1, 0, 0, 0, 1), (), (), 0, (), ()),
    ((100, 500, 500, 500, 500, 100), True, False, 'f16', False, False, 'native_fp32', 'fused_forward fused_backward mix_in_forward', (), (), (), 0, (), ()),
    ((100, 500, 500, 500, 500, 100), True, False, 'f16', True, False, 'native_fp32', 'fused_forward fused_backward mix_in_forward', (), (), (), 0, (), ()),
    ((100, 500, 500, 500, 500, 100), True, True, 'bf16', False, False, 'bf16x3', 'fused_forward fused_backward mix_in_forward split_bf16 split_wgrad', (1, 0, 0, 0, 0, 0, 1), (), (), 0, (0, 1, 2, 3, 4), (1, 2, 3, 4, 5)),
    ((100, 500, 500, 500, 500, 100), True, True, 'bf16', True, False, 'bf16x3', 'fused_forward fused_backward mix_in_forward split_bf16 split_wgrad', (1, 0, 0, 0, 0, 0, 1), (), (), 0, (), ()),
    ((100, 500, 500, 500, 500, 100), True, True, 'f16', False, False, 'bf16x3', 'fused_forward fused_backward mix_in_forward split_bf16 split_wgrad', (1, 0, 0, 0, 0, 0, 1), (), (), 0, (0, 1, 2, 3, 4), (1, 2, 3, 4, 5)),
    ((100, 500, 500, 500, 500, 100), True, True, 'f16', True, False, 'bf16x3', 'fused_forward fused_backward mix_in_forward split_bf16 split_wgrad', (1, 0, 0, 0, 0, 0, 1), (), (), 0, (), ()),
    ((100, 1024, 1024, 1024, 100), True, False, 'f16', False, False, 'native_fp32', '', (), (), (), 0, (), ()),
    ((100, 1024, 1024, 1024, 100), True, False, 'f16', True, False, 'native_fp32', '', (), (), (), 0, (), ()),
]


def _shapes(hidden):
    widths = [N] + list(hidden) + [N]
    return [(widths[i + 1], widths[i]) for i in range(len(widths) - 1)]


def _encoder(hidden):
    from cl_ica_amd import encoders
    return encoders.get_mlp(N, N, list(hidden)) if hidden else torch.nn.Sequential(torch.nn.Linear(N, N))      # (get_mlp refuses no hidden layer)


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "-".join(str(v) for v in r[:6]))
def test_plan_encoder_decides_as_the_parent_did(row):
    from cl_ica_amd.engine import plan_encoder
    hidden, fused_forward, split, arith_arg, keep, gpu, arith, flags, kinds, wide_kinds, chain, chain_min, acts_only, dz_only = row
    shapes = _shapes(hidden)
    L = len(shapes)
    ep = plan_encoder(shapes, 0.2, gpu, fused_forward, split, arith_arg == "f16", keep_fp32_copies=keep)
    assert {f for f in FLAGS if getattr(ep, f)} == set(flags.split())
    assert (ep.path, ep.arith) == ("whole-stack" if "fused_forward" in flags else "per-layer", arith)
    assert (ep.kinds, ep.wide_kinds, ep.chain, ep.chain_min) == (kinds, wide_kinds, frozenset(chain), chain_min)
    assert ep.acts_planes_only == tuple(l in acts_only for l in range(L))
    assert ep.dz_planes_only == (tuple(l in dz_only for l in range(L - 1)) if ep.fused_backward else ())
    with pytest.raises(dataclasses.FrozenInstanceError):          # frozen: nothing re-decides the path after construction
        ep.split_bf16 = not ep.split_bf16


@pytest.mark.parametrize("row", [r for r in ROWS if not r[5]], ids=lambda r: "-".join(str(v) for v in r[:6]))
def test_cpu_trainer_carries_the_plan(row, monkeypatch):
    from cl_ica_amd.engine import ContrastiveTrainer, SamplerSpec, plan_encoder
    hidden, fused_forward, split, arith_arg, keep = row[:5]
    monkeypatch.setattr(ContrastiveTrainer, "keep_fp32_copies", keep)
    torch.manual_seed(0)
    tr = ContrastiveTrainer(_encoder(hidden), torch.randn(3, N, N) / N ** 0.5, SamplerSpec(n=N, seed=5), batch_size=B, device="cpu",
                            split_bf16=split, split_arith=arith_arg, fused_forward=fused_forward)
    ep = tr.encoder_plan
    assert ep == plan_encoder(_shapes(hidden), tr.slope, False, fused_forward, split, arith_arg == "f16", keep_fp32_copies=keep)
    for f in FLAGS:
        assert getattr(tr, f) is getattr(ep, f), f
    assert tr.grouped_wgrad is ep.fused_backward and tr.wide_kinds == list(ep.wide_kinds) and tr.chain == ep.chain
    assert tr.s16 is None and tr._arith_name() == ep.arith == row[6]
    assert [a is None for a in tr.acts_out] == list(ep.acts_planes_only)
    assert ([d is None for d in tr.dz_out] if tr.dz_out is not None else []) == list(ep.dz_planes_only)
    assert [p is not None for p in tr.dz_planes] == [ep.split_wgrad and k == 0 for k in (ep.kinds or [1] * len(tr.linears))]
    # the per-layer backward body's buffers exist where that body runs, and only there
    assert hasattr(tr, "dbuf") == hasattr(tr, "wgrad_ws") == (not ep.fused_backward)
    assert (tr.group_ws is not None) == ep.fused_backward and tr.plan_summary()["encoder_path"] == ep.path


def test_linear_without_bias_is_refused_by_name():
    from cl_ica_amd.engine import ContrastiveTrainer, SamplerSpec
    f = torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.LeakyReLU(0.2), torch.nn.Linear(8, 4, bias=False))
    with pytest.raises(ValueError, match=r"Linear without bias \(2: Linear"):
        ContrastiveTrainer(f, torch.eye(4).repeat(3, 1, 1), SamplerSpec(n=4), batch_size=8, device="cpu")
