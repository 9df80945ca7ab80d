"""Training driver for the 3DIdent experiment: the counterpart of /root/reference/main_3dident.py on the HIP path, written the way
``train_mlp`` mirrors ``main_mlp.py``.  Same command-line flags (main_3dident.py:30-106), same modes (supervised, unsupervised, test),
same evaluation and log schedule, same log lines and model files.

    python -m cl_ica_amd.train_3dident --offline-dataset /data/3dident/train --mode unsupervised --position-only
    python -m cl_ica_amd.train_3dident --offline-dataset /data/3dident/test --mode test --position-only --load-model f.pth

What runs where: latents are drawn by the device samplers and snapped to the rendered grid by ``clica_nn_search``, image batches are
gathered from a uint8 table in HBM (``cl_ica_amd.datasets``), the encoder is ``threedident.setup_f`` (ResNet-18 with the fused
BatchNorm2d / pool units, HIP head), the objectives are the HIP losses, the optimizer is the flat-arena ``optim.Adam`` or ``optim.SGD``
(``--optimizer``), and the scores come from ``clica_moments``.  Loss values stay on the device between log steps.

Where it differs from the reference (INTEGRATION.md lists the same):
  * ``--approximate-dataset-nn-search`` is accepted and runs the exact search (one line says so);
  * model files carry the ``module.`` key prefix the reference's ``nn.DataParallel`` wrapper writes on a GPU; ``--load-model`` takes files
    with or without it;
  * ``--identity-mixing-and-solution`` does not prompt for a scale at log steps (it stays 1);
  * the combined objective (no mode flag) returns ``(total, parts)`` and crashes the reference's own caller (:441 against :490): the loop
    here takes both shapes and prints ``sigma(loss): nan`` when there is no per-item vector;
  * ``--encoder`` also accepts ``rn152`` (the reference's choices say ``rn151``, its table ``rn152``);
  * ``--no-cuda`` exits: there is no CPU path; ``--workers`` / ``--faiss-omp-threads`` are accepted and unused;
  * extra flags: ``--seed`` (numpy / random / torch / the device samplers), ``--image-cache FILE`` (the decoded image folder, written once);
  * ``--graph`` (default off) replays the whole training iteration -- batch draw, snap, image gather, encoder, loss, backward, optimizer --
    as ONE HIP graph (``threedident.capture_iteration``; the first iteration runs eagerly and trains).  The training batches are then
    drawn under a device clock (``spaces.DeviceClock``), so the batch sequence differs from a run without the flag under the same
    ``--seed``; the evaluation batches still come from the module-level generator.  Log lines, schedule and model files are the same.
    Refused with ``--dummy-mixing`` / ``--identity-solution`` / ``--identity-mixing-and-solution`` (no image batch or nothing to train).
One process, one GPU.
"""
from __future__ import annotations

import argparse
import os
import random
from datetime import datetime

import numpy as np
import torch

from . import disentanglement_utils, invertible_network_utils, latent_spaces, lazy, optim, resnet, spaces, threedident
from .datasets import BatchLoader, SequentialThreeDIdentDataset, ThreeDIdentDataset

__all__ = ["parse_args", "setup_latent_space", "latent_dimensions_to_use", "evaluate", "train_unsupervised", "train_supervised", "test",
           "main", "is_log_step", "strip_module_prefix", "add_module_prefix"]

NORMALIZE = ([0.3292, 0.3278, 0.3215], [0.0778, 0.0776, 0.0771])      # the transforms.Normalize of main_3dident.py:791-793

# the reference's CLI surface (main_3dident.py:30-106): flag -> add_argument keywords
_ARGS = [
    ("--batch-size", dict(default=512, type=int)),
    ("--n-eval-samples", dict(default=4096, type=int)),
    ("--lr", dict(default=1e-4, type=float)),
    ("--optimizer", dict(default="adam", choices=("adam", "sgd"))),
    ("--iterations", dict(default=30000, type=int, help="How long to train the model")),
    ("--n-log-steps", dict(default=100, type=int, help="How often to calculate scores and print them")),
    ("--load-model", dict(default=None, type=str, help="Path from where to load the model")),
    ("--save-model", dict(default=None, type=str, help="Path where to save the model")),
    ("--save-every", dict(default=None, type=int, help="After how many steps to save the model (will always be saved at the end)")),
    ("--no-cuda", dict(action="store_true", help="Exits: there is no CPU path.")),
    ("--position-only", dict(action="store_true")),
    ("--rotation-and-color-only", dict(action="store_true")),
    ("--rotation-only", dict(action="store_true")),
    ("--color-only", dict(action="store_true")),
    ("--no-spotlight-position", dict(action="store_true")),
    ("--no-spotlight-color", dict(action="store_true")),
    ("--no-spotlight", dict(action="store_true")),
    ("--non-periodic-rotation-and-color", dict(action="store_true")),
    ("--dummy-mixing", dict(action="store_true")),
    ("--identity-solution", dict(action="store_true")),
    ("--identity-mixing-and-solution", dict(action="store_true")),
    ("--approximate-dataset-nn-search", dict(action="store_true", help="Accepted: the search that runs is the exact one.")),
    ("--offline-dataset", dict(type=str, required=True)),
    ("--faiss-omp-threads", dict(type=int, default=16, help="Accepted and unused: the nearest-neighbour search is a device kernel.")),
    ("--box-constraint", dict(type=str, required=False, default=None, choices=(None, "fix", "learnable"))),
    ("--sphere-constraint", dict(type=str, required=False, default=None, choices=(None, "fix", "learnable"))),
    ("--workers", dict(default=0, type=int, help="Accepted and unused: batches are gathered on the device.")),
    ("--mode", dict(default="supervised", choices=("supervised", "unsupervised", "test"))),
    ("--supervised-loss", dict(default="mse", type=str, choices=("mse", "r2"))),
    ("--unsupervised-loss", dict(default="l2", type=str, choices=("l1", "l2", "l3", "vmf"))),
    ("--non-periodical-conditional", dict(default="l2", choices=("l1", "l2", "l3"))),
    ("--sigma", dict(default=0.1, type=float, help="Sigma of the conditional distribution (for vMF: 1/kappa)")),
    # the reference's choices say rn151 where its table of constructors says rn152: both spellings of the flag are taken
    ("--encoder", dict(default="rn18", choices=("rn18", "rn50", "rn101", "rn151", "rn152"))),
]
# on top of the reference's
_EXTRA_ARGS = [
    ("--seed", dict(type=int, default=None, help="Seeds numpy, random, torch and the device samplers.")),
    ("--image-cache", dict(type=str, default=None,
                           help=".npy file the decoded image folder is written to once and memory-mapped from afterwards.")),
    ("--amp", dict(default="off", choices=("off", "bf16"),
                   help="bf16: the backbone in bf16 mixed precision (autocast convolutions, channels-last bf16 HIP units between them); "
                        "head, loss, optimizer and model files stay fp32.")),
    ("--graph", dict(default="off", choices=("off", "on"), nargs="?", const="on",
                     help="on (or the bare flag): the training iteration, batch draw included, is recorded once and replayed as one HIP "
                          "graph; the training batches are then drawn under a device clock, so the batch sequence differs from a run "
                          "without the flag under the same --seed.")),
]
# The flags of _EXTRA_ARGS that say HOW the run computes, not what it computes.  They are taken off the command line ahead of the
# table's parser: build_parser() stays the reference's surface plus --seed and --image-cache, the set tests/test_train_3dident_host.py
# pins.
_RUN_ARGS = ("--amp", "--graph")


def build_parser() -> argparse.ArgumentParser:
    run = "; ".join(f"{flag} {{{','.join(kw['choices'])}}} (default {kw['default']}): {kw['help']}" for flag, kw in _EXTRA_ARGS
                    if flag in _RUN_ARGS)
    ap = argparse.ArgumentParser(description="Disentanglement with InfoNCE/Contrastive Learning - 3DIdent (MI355X)",
                                 epilog="Read ahead of the options above, how the run computes: " + run)
    for flag, kw in _ARGS + _EXTRA_ARGS:
        if flag not in _RUN_ARGS:
            ap.add_argument(flag, **kw)
    return ap


def _run_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(add_help=False, allow_abbrev=False, usage=argparse.SUPPRESS)
    for flag, kw in _EXTRA_ARGS:
        if flag in _RUN_ARGS:
            ap.add_argument(flag, **kw)
    return ap


def parse_args(argv=None):
    run, rest = _run_parser().parse_known_args(argv)
    args = build_parser().parse_args(rest, namespace=run)
    if args.no_spotlight:                                                   # :108-111
        args.no_spotlight_color = True
        args.no_spotlight_position = True
    # the assertions of :115-137
    if not (args.save_every is None or args.save_every > 0):
        raise AssertionError("--save-every must be positive")
    if args.save_model is None and args.save_every is not None:
        raise AssertionError("--save-every requires --save-model to be set")
    if args.position_only and args.rotation_and_color_only:
        raise AssertionError("Only one of these flags can be set.")
    if args.position_only and (args.non_periodic_rotation_and_color or args.no_spotlight_color or args.no_spotlight_position):
        raise AssertionError("--position-only excludes --non-periodic-rotation-and-color and the spotlight flags")
    if args.box_constraint is not None and args.sphere_constraint is not None:
        raise AssertionError("only one of --box-constraint / --sphere-constraint")
    if args.save_model is not None and not os.path.exists(os.path.dirname(args.save_model)):
        raise AssertionError(f"Directory {os.path.dirname(args.save_model)} to save model does not exist")
    if args.amp != "off" and (args.dummy_mixing or args.identity_solution or args.identity_mixing_and_solution):
        raise AssertionError(f"--amp {args.amp} is the backbone's mixed precision: --dummy-mixing / --identity-solution / "
                             "--identity-mixing-and-solution have no backbone")
    if args.graph != "off" and (args.dummy_mixing or args.identity_solution or args.identity_mixing_and_solution):
        raise AssertionError("--graph captures the iteration on image batches: --dummy-mixing (latents through an MLP), --identity-solution "
                             "and --identity-mixing-and-solution (nothing to train) have nothing to capture and run without it")
    return args


def _amp(args):
    """What the steps and the evaluation take as ``amp``: None for ``--amp off`` (and for argument objects from before the flag)."""
    amp = getattr(args, "amp", "off")
    return None if amp == "off" else amp


def _graph(args) -> bool:
    """``--graph`` (False for argument objects from before the flag)."""
    return getattr(args, "graph", "off") not in ("off", False, None)


class _GraphedSteps:
    """The loop's training step under ``--graph``: the first call runs one eager clocked iteration (it trains; the find step and the
    workspaces happen there) and records the graph, every later call is one replay.  Returns ``(total, per_item, parts)``; ``total`` is a
    copy, because the graph rewrites its own on the next replay and the loop keeps the values on the device until the next log step."""

    def __init__(self, dataset, loss, optimizer, f, batch_size, supervised, amp):
        self.args = (dataset, loss, optimizer, f, batch_size)
        self.kw = dict(supervised=supervised, amp=amp, warmup=1)
        self.step = None

    def __call__(self):
        if self.step is None:
            first = []
            self.step = threedident.capture_iteration(*self.args, on_warmup=first.append, **self.kw)
            return first[0]
        total, per_item, parts = self.step()
        return total.detach().clone(), per_item, parts


def _amp_batch(x, amp):
    """The image batch as the mixed-precision backbone takes it: dense channels-last.  ``amp`` None: x itself."""
    if amp is None or x is None:
        return x
    return x.contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------------------------------------------------------------ latent space
def setup_latent_space(args, n_objects=1):
    """``(latent_space, n_non_angular, n_angular)`` for the mode flags (main_3dident.py:142-285): a box for the positions, and for
    rotations and colours a sphere with a von Mises-Fisher conditional, or -- ``--non-periodic-rotation-and-color`` -- another box."""
    spot = (0 if args.no_spotlight_color else 1) + (0 if args.no_spotlight_position else 1)
    n_color_and_rotation_variables = n_objects * (4 + spot) + 1
    sigma = args.sigma
    kind = args.non_periodical_conditional

    def non_periodical_conditional(space, z, size, device="cuda"):
        if kind == "l3":
            return space.generalized_normal(z, lbd=sigma, p=3, size=size, device=device)
        if kind == "l2":
            return space.normal(z, std=sigma, size=size, device=device)
        return space.laplace(z, lbd=sigma, size=size, device=device)

    def uniform(space, size, device="cuda"):
        return space.uniform(size, device=device)

    def vmf(space, z, size, device="cuda"):
        return space.von_mises_fisher(z, kappa=1 / sigma, size=size, device=device)

    def box(n):
        return latent_spaces.LatentSpace(spaces.NBoxSpace(n), uniform, non_periodical_conditional)

    def sphere(n):
        return latent_spaces.LatentSpace(spaces.NSphereSpace(n), uniform, vmf)

    position_space = box(n_objects * 3)
    if args.non_periodic_rotation_and_color:
        rotation_and_color_space = box(n_objects * (4 + spot + 1))
        rotation_space = box(n_objects * 3 + (0 if args.no_spotlight_position else 1))
        color_space = box(n_objects * (1 + (0 if args.no_spotlight_color else 1)) + 1)
    else:
        rotation_and_color_space = sphere(n_color_and_rotation_variables + 1)
        rotation_space = sphere(n_objects * 3 + 1)
        color_space = sphere(n_objects * 3 + 1 + 1)

    if args.position_only:
        if args.non_periodic_rotation_and_color:
            raise ValueError()
        chosen = position_space
    elif args.rotation_and_color_only:
        chosen = rotation_and_color_space
    elif args.rotation_only:
        chosen = rotation_space
    elif args.color_only:
        chosen = color_space
    else:
        latent_space = latent_spaces.ProductLatentSpace([position_space, rotation_and_color_space])
        if args.non_periodic_rotation_and_color:
            return latent_space, rotation_and_color_space.dim + position_space.dim, 0
        return latent_space, position_space.dim, rotation_and_color_space.dim
    if args.non_periodic_rotation_and_color or args.position_only:
        return chosen, chosen.dim, 0
    return chosen, 0, chosen.dim


def latent_dimensions_to_use(args):
    """The columns of ``raw_latents.npy`` the mode flags select (main_3dident.py:798-832), or None for all."""
    columns = None
    if args.non_periodic_rotation_and_color:
        if args.rotation_and_color_only:
            columns = [3, 4, 5, 6, 7, 8, 9]
        elif args.rotation_only:
            columns = [3, 4, 5, 6]
        elif args.color_only:
            columns = [7, 8, 9]
        elif args.position_only:
            raise ValueError("Not supported")
        else:
            columns = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
        if args.no_spotlight_position:
            columns = [it for it in columns if it != 6]
        if args.no_spotlight_color:
            columns = [it for it in columns if it != 8]
    else:
        if args.position_only:
            columns = [0, 1, 2]
        elif args.rotation_and_color_only:
            columns = [3, 4, 5, 6, 7, 8, 9, 10]
        if args.no_spotlight_position or args.no_spotlight_color:
            raise NotImplementedError("This is only supported for non-periodic variables at the moment.")
    return columns


# ------------------------------------------------------------------------------------------------------------------ model files
def strip_module_prefix(state_dict):
    """A state dict as ``f`` takes it: the ``module.`` prefix of a ``nn.DataParallel`` wrapper removed where every key carries it."""
    if state_dict and all(k.startswith("module.") for k in state_dict):
        return {k[len("module."):]: v for k, v in state_dict.items()}
    return dict(state_dict)


def add_module_prefix(state_dict):
    """A state dict as the reference writes it on a GPU (``f`` wrapped in ``nn.DataParallel``, :373-383): every key under ``module.``."""
    return {"module." + k: v for k, v in state_dict.items()}


def save_model(f, path):
    torch.save(add_module_prefix({k: v.detach().cpu().clone() for k, v in f.state_dict().items()}), path)


def is_log_step(global_step: int, n_log_steps: int, n_steps: int) -> bool:
    """The reference's schedule (:525, 612), on the 0-based step: every ``n_log_steps``-th step starting with the first."""
    return global_step % n_log_steps == 0 or global_step == n_steps


def _save_due(global_step: int, last_save_at_step: int, save_every) -> bool:
    return save_every is not None and global_step // save_every != last_save_at_step // save_every


def _infinite(loader):
    """The reference's InfiniteIterator: epoch after epoch."""
    while True:
        seen = False
        for batch in loader:
            seen = True
            yield batch
        if not seen:
            raise RuntimeError("the loader yields no batches")


# ------------------------------------------------------------------------------------------------------------------ evaluation
def evaluate(args, f, test_iterator, evaluate_permutation_disentanglement, no_pairs=False, g=None, amp=None):
    """``(MCC, linear R2, mse, linear_fit_mse)`` over ``n_eval_samples // batch_size`` batches (main_3dident.py:656-748): the scores on
    device tensors, the two per-dimension errors as NumPy vectors, ``np.inf`` where the reference returns it.  ``amp``: the encoder
    passes as ``threedident.encode`` runs them."""
    zs, hzs = [], []
    with torch.no_grad():
        for _ in range(args.n_eval_samples // args.batch_size):
            test_data = next(test_iterator)
            if no_pairs:
                batch_z, batch_x = test_data
            else:
                batch_z, batch_x = test_data[0][0], test_data[1][0]
            if args.dummy_mixing:
                batch_x = g(batch_z)
            if args.identity_mixing_and_solution:
                batch_hz = batch_z
            else:
                batch_hz = lazy.plain(threedident.encode(f, _amp_batch(batch_x, amp), amp)).detach()
            zs.append(batch_z)
            hzs.append(batch_hz)
    if not zs:
        return np.inf, np.inf, np.inf, np.inf
    z, hz = torch.cat(zs, 0), torch.cat(hzs, 0)
    (linear_score, _), (test_z, linear_transformed_hz) = disentanglement_utils.linear_disentanglement(z, hz, mode="r2", train_test_split=True)
    if evaluate_permutation_disentanglement:
        (permutation_score, _), _ = disentanglement_utils.permutation_disentanglement(z, hz, mode="pearson", solver="munkres", rescaling=True)
    else:
        permutation_score = np.inf
    mse = ((z - hz) ** 2).mean(0).cpu().numpy() if not args.identity_solution else np.inf
    # the linear fit's error on the samples that were not used to fit it
    test_z = torch.as_tensor(test_z, dtype=torch.float32)
    linear_transformed_hz = torch.as_tensor(linear_transformed_hz, dtype=torch.float32).to(test_z.device)
    linear_fit_mse = ((test_z - linear_transformed_hz) ** 2).mean(0).cpu().numpy()
    return permutation_score, linear_score, mse, linear_fit_mse


def test(args, test_loader, f, g=None):
    scores = evaluate(args, f, _infinite(test_loader), not args.identity_solution, True, g=g, amp=_amp(args))
    permutation_score, linear_score, mse, linear_fit_mse = scores
    print(f"Lin. Disentanglement: {linear_score}, MCC: {permutation_score}, MSE: {mse}, lin. fit MSE: {linear_fit_mse}")
    return scores


# ------------------------------------------------------------------------------------------------------------------ training
def _make_optimizer(args, f):
    if args.optimizer == "adam":
        return optim.Adam(f.parameters(), lr=args.lr)
    if args.optimizer == "sgd":
        return optim.SGD(f.parameters(), lr=args.lr)
    raise ValueError(f"optimizer {args.optimizer!r}")


def _three_values(loss):
    """The single objectives return ``(total, per_item, parts)``, the combined one ``(total, parts)``: one shape for the step."""
    def wrapped(*a):
        out = loss(*a)
        if len(out) == 2:
            return out[0], None, out[1]
        return out
    return wrapped


def _fetch(pending, total_loss_values):
    """Device scalars of the steps since the last log step -> the host list (ONE transfer)."""
    if pending:
        total_loss_values.extend(float(v) for v in torch.stack([p.detach().reshape(()) for p in pending]).cpu())
        del pending[:]


def train_unsupervised(args, train_loader, f, n_non_angular_latents, g=None):
    """main_3dident.py:402-566.  Returns ``dict(losses, optimizer, scores)``."""
    n_log_steps, n_steps = args.n_log_steps, args.iterations
    amp = _amp(args)
    loss = _three_values(threedident.make_unsupervised_loss(args, n_non_angular_latents))
    optimizer = _make_optimizer(args, f)
    total_loss_values, pending = [], []
    linear_scores, permutation_scores = [], []
    train_iterator = _infinite(train_loader)
    identity_scale = 1.0
    last_save_at_step = 0
    scores = None
    graphed = _GraphedSteps(train_loader.dataset, loss, optimizer, f, args.batch_size, False, amp) if _graph(args) else None
    for global_step in range(n_steps):
        if graphed is not None:      # the batch is drawn inside the iteration, under the device clock
            total, per_item, _parts = graphed()
            pending.append(total)
        else:
            data = next(train_iterator)
            (z1, z2_con_z1), (x1, x2_con_x1) = data
            if args.dummy_mixing:
                with torch.no_grad():
                    data = ((z1, z2_con_z1), (g(z1), g(z2_con_z1)))
            if args.identity_mixing_and_solution:      # h = f o g is the identity: the objective on the latents themselves, nothing to train
                z1_rec = z1 * identity_scale
                total, per_item, _parts = loss(None, None, None, z1_rec, z2_con_z1 * identity_scale, torch.roll(z1_rec, 1, 0))
            else:
                if amp is not None:
                    data = ((z1, z2_con_z1), (_amp_batch(data[1][0], amp), _amp_batch(data[1][1], amp)))
                total, per_item, _parts = threedident.train_step(data, loss, optimizer, f, sync=False, amp=amp)
            pending.append(total)
            del data, x1, x2_con_x1
        log = is_log_step(global_step, n_log_steps, n_steps)
        if log:
            scores = evaluate(args, f, train_iterator, True, g=g, amp=amp)
            permutation_score, linear_score, mse, linear_fit_mse = scores
        else:
            linear_score = permutation_score = np.inf
        linear_scores.append(linear_score)
        permutation_scores.append(permutation_score)
        if log:
            _fetch(pending, total_loss_values)
            sigma = float(torch.std(per_item.detach())) if per_item is not None else float("nan")
            print(f"[{datetime.now().strftime('%Y-%m-%d_%H:%M:%S')}] \t",
                  f"Step: {global_step + 1} \t",
                  f"Loss: {total_loss_values[-1]:.6f} \t",
                  f"sigma(loss): {sigma} \t",
                  f"<Loss>: {np.mean(np.array(total_loss_values[-n_log_steps:])):.6f} \t",
                  f"sigma(<Loss>): {np.std(np.array(total_loss_values[-n_log_steps:])):.6f} \t",
                  f"Lin. Disentanglement: {linear_score:.6f} \t",
                  f"Perm. Disentanglement (MCC): {permutation_score:.4f}",
                  f"L2: {mse}",
                  f"lin. L2: {linear_fit_mse}")
        done = global_step + 1
        if _save_due(done, last_save_at_step, args.save_every):
            last_save_at_step = done
            model_path = args.save_model + f".iteration_{done}"
            save_model(f, model_path)
            print("Model saved as", model_path)
    _fetch(pending, total_loss_values)
    return dict(losses=total_loss_values, optimizer=optimizer, scores=scores, linear_scores=linear_scores,
                permutation_scores=permutation_scores)


def train_supervised(args, train_loader, f, g=None):
    """main_3dident.py:569-653 (the evaluation comes BEFORE the step here).  Returns ``dict(losses, optimizer, scores)``."""
    n_log_steps, n_steps = args.n_log_steps, args.iterations
    amp = _amp(args)
    loss = threedident.make_supervised_loss(args)
    optimizer = None if args.identity_solution else _make_optimizer(args, f)
    total_loss_values, pending = [], []
    linear_scores, permutation_scores = [], []
    train_iterator = _infinite(train_loader)
    last_save_at_step = 0
    scores = None
    graphed = _GraphedSteps(train_loader.dataset, loss, optimizer, f, args.batch_size, True, amp) if _graph(args) else None
    for global_step in range(n_steps):
        log = is_log_step(global_step, n_log_steps, n_steps)
        if log:
            scores = evaluate(args, f, train_iterator, False, g=g, amp=amp)
            permutation_score, linear_score, mse, linear_fit_mse = scores
        else:
            linear_score = permutation_score = np.inf
        linear_scores.append(linear_score)
        permutation_scores.append(permutation_score)
        data = next(train_iterator) if graphed is None else None
        if graphed is not None:
            pending.append(graphed()[0])
        elif not args.identity_solution:
            if args.dummy_mixing:
                (z1, z2), _x = data
                with torch.no_grad():
                    data = ((z1, z2), (g(z1), None))
            if amp is not None:
                data = (data[0], (_amp_batch(data[1][0], amp), data[1][1]))
            pending.append(threedident.train_step_supervised(data, loss, optimizer, f, sync=False, amp=amp))
        else:
            _fetch(pending, total_loss_values)
            total_loss_values.append(np.inf)
        del data
        if log:
            _fetch(pending, total_loss_values)
            print(f"[{datetime.now().strftime('%Y-%m-%d_%H:%M:%S')}] \t"
                  f"Step: {global_step} \t",
                  f"Loss: {total_loss_values[-1]:.6f} \t",
                  f"<Loss>: {np.mean(np.array(total_loss_values[-n_log_steps:])):.6f} \t",
                  f"Lin. Disentanglement: {linear_score:.6f} \t",
                  f"L2: {mse}",
                  f"lin. L2: {linear_fit_mse}")
        done = global_step + 1
        if _save_due(done, last_save_at_step, args.save_every):
            last_save_at_step = done
            model_path = args.save_model + f".iteration_{done}"
            save_model(f, model_path)
            print("Model saved as", model_path)
    _fetch(pending, total_loss_values)
    return dict(losses=total_loss_values, optimizer=optimizer, scores=scores, linear_scores=linear_scores,
                permutation_scores=permutation_scores)


# ------------------------------------------------------------------------------------------------------------------ the driver
def main(argv=None, *, images=None, base_encoder=None):
    """Run the driver.  ``images``: a uint8 array ``[N, H, W, C]`` or an ``ImageTable`` handed to the dataset instead of decoding
    ``<offline-dataset>/images``; ``base_encoder``: the backbone constructor ``setup_f`` takes.  Returns what the mode produced
    (``f``, ``args``, and the loop's ``losses`` / ``optimizer`` / ``scores``, or the four test scores)."""
    args = parse_args(argv)
    print(args)
    if args.no_cuda or not torch.cuda.is_available():
        raise SystemExit("cl_ica_amd.train_3dident needs an MI355X: there is no CPU path (--no-cuda cannot be honoured)")
    if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        raise SystemExit("cl_ica_amd.train_3dident runs one process on one GPU: it is not data parallel")
    device = torch.device("cuda", torch.cuda.current_device())
    np.set_printoptions(formatter={"float": lambda x: format(x, "1.5E")})
    if args.seed is not None:
        np.random.seed(args.seed); random.seed(args.seed); torch.manual_seed(args.seed)
        spaces.manual_seed(args.seed)
    if not os.path.exists(args.offline_dataset):
        raise AssertionError(f"{args.offline_dataset} does not exist")
    print("Using dataset:", args.offline_dataset)

    latent_space, n_non_angular_latents, n_angular_latents = setup_latent_space(args)
    if not args.identity_solution:
        print("#Latents:", n_non_angular_latents + n_angular_latents, ", #Non-periodic latents:", n_non_angular_latents,
              ", #Periodic latents:", n_angular_latents)
    f = threedident.setup_f(args, n_non_angular_latents, n_angular_latents, base_encoder=base_encoder)
    if args.load_model is not None:
        print("device", device)
        f.load_state_dict(strip_module_prefix(torch.load(args.load_model, map_location="cpu", weights_only=True)))
        print("Model loaded:", args.load_model)
    f = f.to(device)
    if _amp(args) is not None:
        # parameters stay fp32 (the model file does not change); the kernels between the convolutions take over the bf16 activations
        f = f.to(memory_format=torch.channels_last)
        print(f"Mixed precision: --amp {args.amp}: channels-last model and batches, convolutions under torch.autocast(bfloat16), "
              "resnet NHWC_MODE = NHWC_STEM_MODE = BF16_MODE = 'hip'; head, loss and optimizer in fp32")
        switches = {name: getattr(resnet, name) for name in ("NHWC_MODE", "NHWC_STEM_MODE", "BF16_MODE")}
        for name in switches:
            setattr(resnet, name, "hip")
        try:
            return _run(args, f, device, latent_space, n_non_angular_latents, n_angular_latents, images)
        finally:                                      # (the caller's switches are the caller's)
            for name, value in switches.items():
                setattr(resnet, name, value)
    return _run(args, f, device, latent_space, n_non_angular_latents, n_angular_latents, images)


def _run(args, f, device, latent_space, n_non_angular_latents, n_angular_latents, images):
    """The mode's loop on the model as ``main`` set it up, and the final save."""
    g = None
    if args.dummy_mixing:
        g = invertible_network_utils.construct_invertible_mlp(n_angular_latents + n_non_angular_latents, n_layers=3, act_fct="leaky_relu",
                                                              cond_thresh_ratio=0.0, n_iter_cond_thresh=25000).to(device)
        for p in g.parameters():
            p.requires_grad = False
    if args.identity_mixing_and_solution:
        print("Using identity function for h(z)=f(g(z))")
    if args.approximate_dataset_nn_search:
        print("--approximate-dataset-nn-search: the dataset's nearest-neighbour search is the exact one (a device kernel over the whole table)")
    dummy_images = bool(args.dummy_mixing or args.identity_mixing_and_solution)
    columns = latent_dimensions_to_use(args)
    print("Using latent dimensions:", columns)

    out = dict(args=args, f=f, latent_space=latent_space, n_non_angular_latents=n_non_angular_latents, n_angular_latents=n_angular_latents)
    if args.mode in ("supervised", "unsupervised"):
        train_dataset = ThreeDIdentDataset(args.offline_dataset, latent_space, latent_dimensions_to_use=columns, normalize=NORMALIZE,
                                           images=None if dummy_images else images, dummy_images=dummy_images, device=device,
                                           cache=args.image_cache)
        train_loader = BatchLoader(train_dataset, args.batch_size)
        if args.mode == "supervised":
            out.update(train_supervised(args, train_loader, f, g=g))
        else:
            out.update(train_unsupervised(args, train_loader, f, n_non_angular_latents, g=g))
    elif args.mode == "test":
        if dummy_images:
            raise NotImplementedError("--mode test reads the rendered images: --dummy-mixing / --identity-mixing-and-solution have none")
        test_dataset = SequentialThreeDIdentDataset(args.offline_dataset, latent_dimensions_to_use=columns, normalize=NORMALIZE, images=images,
                                                    device=device, cache=args.image_cache)
        test_loader = BatchLoader(test_dataset, args.batch_size, shuffle=True, seed=args.seed)
        out.update(scores=test(args, test_loader, f, g=g))
    else:
        raise ValueError()
    if args.save_model is not None:
        save_model(f, args.save_model)
        print(f"Saving final model at: {args.save_model}")
    return out


if __name__ == "__main__":
    main()
