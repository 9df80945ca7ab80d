"""Training driver for the KITTI-masks experiment: the counterpart of /root/reference/main_kitti.py on the HIP path, written the way
``train_3dident`` mirrors ``main_3dident.py``.  Same command-line flags with the same defaults and types (main_kitti.py:103-242), same
directory rules (:25-52: ``output_dir/experiment_dir/seed``, ``ckpt_dir/experiment_dir/seed``, ``experiment_dir`` derived as
``{dataset}_{param}/{p}_{box_norm}``), the ``args`` JSON file (:62-63), the seeding (:64-66), train -> evaluate or ``--evaluate`` alone
(:67-79), and the ``--random-seeds`` loop over ``--num_runs`` (:258-261).

    python -m cl_ica_amd.train_kitti --cuda --data-dir /data/kitti --box-norm 1 --p 1 --z-dim 10 --kitti-max-delta-t 5
    python -m cl_ica_amd.train_kitti --cuda --data-dir /data/kitti --box-norm 1 --p 1 --z-dim 10 --kitti-max-delta-t 5 --evaluate

What runs where: all frames live in HBM once; one launch per iteration (``clica_kitti_sample_pairs``) draws the next batch of the
shuffled stream and gathers it; the encoder is ``kitti_masks.BetaVAE_H`` on the HIP conv stack, the loss ``LpSimCLRLoss``, the optimizer
the flat-arena Adam; by default a whole iteration, data included, is one replay of a HIP graph (``Solver.capture_stream``).  The
evaluation is the mean correlation coefficient from ``clica_moments`` (``kitti_masks.mcc_metric``).

Where it differs from the reference (INTEGRATION.md lists the same):
  * the ``pip install`` calls at import are not carried over;
  * without ``--cuda`` and a visible GPU it exits: there is no CPU path;
  * the SlowVAE-era flags ``--beta --gamma --rate-prior --data-distribution --rate-data --data-k --betavae --search-beta
    --natural-discrete --num-workers --log-dir`` are accepted, recorded in ``args`` and otherwise unused;
  * ``--use-writer`` is accepted and says in one line that nothing is written to TensorBoard;
  * ``--random-search`` exits with a message: it is an endless loop over parameters the contrastive solver never reads;
  * the reference's tail, which re-parses ``sys.argv`` and touches an unbound name after ``--evaluate``, is not reproduced: every run
    starts from a copy of the parsed arguments;
  * extra flags: ``--data-dir`` (where ``kitti_peds_v2.pickle`` lies; nothing is downloaded), ``--no-graph`` (issue the iteration's
    launches eagerly), ``--mcc-num-train`` / ``--mcc-correlation`` (what the reference reads from ``metric_configs/mcc.gin``, a file its
    tree does not contain: the defaults 10000 / Pearson are this project's choice).
One process, one GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import time

import numpy as np
import torch

__all__ = ["build_parser", "parse_args", "experiment_dir", "prepare_directories", "run", "main"]

# the reference's CLI surface (main_kitti.py:103-242): flag -> add_argument keywords
_ARGS = [
    ("--box-norm", dict(type=int, default=0)),
    ("--p", dict(type=int, default=1)),
    ("--experiment-dir", dict(type=str, default="", help="specify path")),
    ("--evaluate", dict(action="store_true", default=False, help="evaluate instead of train")),
    ("--specify", dict(default="", type=str, help="use argument to only compute a subset of metrics")),
    ("--random-search", dict(action="store_true", default=False, help="Exits: the searched parameters are not read by the contrastive solver.")),
    ("--random-seeds", dict(action="store_true", default=False, help="whether to go over random seeds with UDR params")),
    ("--seed", dict(default=2, type=int, help="random seed")),
    ("--beta", dict(default=1, type=float, help="Accepted and unused.")),
    ("--gamma", dict(default=10, type=float, help="Accepted and unused.")),
    ("--rate-prior", dict(default=6, type=float, help="Accepted and unused.")),
    ("--data-distribution", dict(default="laplace", type=str, help="Accepted and unused.")),
    ("--rate-data", dict(default=1, type=float, help="Accepted and unused.")),
    ("--data-k", dict(default=-1, type=int, help="Accepted and unused.")),
    ("--betavae", dict(action="store_true", default=False, help="Accepted and unused.")),
    ("--search-beta", dict(action="store_true", default=False, help="Accepted and unused.")),
    ("--output-dir", dict(default="outputs", type=str, help="output directory")),
    ("--log-dir", dict(default="logs", type=str, help="Accepted and unused.")),
    ("--ckpt-dir", dict(default="checkpoints", type=str, help="checkpoint directory")),
    ("--max-iter", dict(default=300000, type=float, help="maximum training iteration")),
    ("--dataset", dict(default="kittimasks", type=str, help="dataset name (kittimasks)")),
    ("--batch-size", dict(default=64, type=int, help="batch size (images: twice the number of pairs)")),
    ("--num-workers", dict(default=2, type=int, help="Accepted and unused: batches are drawn on the device.")),
    ("--image-size", dict(default=64, type=int, help="image size. now only (64,64) is supported")),
    ("--use-writer", dict(action="store_true", default=False, help="Accepted: nothing is written to TensorBoard.")),
    ("--z-dim", dict(default=10, type=int, help="dimension of the representation z")),
    ("--lr", dict(default=1e-4, type=float, help="learning rate")),
    ("--beta1", dict(default=0.9, type=float, help="Adam optimizer beta1")),
    ("--beta2", dict(default=0.999, type=float, help="Adam optimizer beta2")),
    ("--ckpt-name", dict(default="last", type=str, help="load previous checkpoint. insert checkpoint filename")),
    ("--log-step", dict(default=1000, type=int, help="numer of iterations after which data is logged")),
    ("--save-step", dict(default=10000, type=int, help="number of iterations after which a checkpoint is saved")),
    ("--kitti-max-delta-t", dict(default=1, type=int, help="max t difference between frames sampled from kitti data loader.")),
    ("--natural-discrete", dict(action="store_true", default=False, help="Accepted and unused.")),
    ("--verbose", dict(action="store_true", default=False, help="for evaluation")),
    ("--cuda", dict(action="store_true", default=False)),
    ("--num_runs", dict(default=10, type=int, help="when searching over seeds, do 10")),
]
# on top of the reference's
_EXTRA_ARGS = [
    ("--data-dir", dict(default="./data/kitti/", type=str, help="Directory that holds kitti_peds_v2.pickle (nothing is downloaded).")),
    ("--no-graph", dict(action="store_true", default=False, help="Issue every iteration's launches eagerly instead of replaying one graph.")),
    ("--mcc-num-train", dict(default=10000, type=int, help="Points the mean correlation coefficient is computed from.")),
    ("--mcc-correlation", dict(default="Pearson", choices=("Pearson", "Spearman"), help="Correlation the MCC is built on.")),
]


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Disentanglement with InfoNCE/Contrastive Learning - KITTI Masks (MI355X)")
    for flag, kw in _ARGS + _EXTRA_ARGS:
        ap.add_argument(flag, **kw)
    return ap


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    # the assertions of main_kitti.py:246-247
    if args.random_search and args.betavae and not args.search_beta:
        raise AssertionError("--random-search with --betavae needs --search-beta")
    if (args.random_search or args.random_seeds) and args.evaluate:
        raise AssertionError("--random-search / --random-seeds exclude --evaluate")
    return args


def _randint(low, high):
    return int(np.random.randint(low, high, 1)[0])          # main_kitti.py:87-88


def experiment_dir(args) -> str:
    """``--experiment-dir`` or the derived ``{dataset}_{param}/{p}_{box_norm}`` (main_kitti.py:25-35)."""
    if args.experiment_dir:
        return args.experiment_dir
    if "kitti" in args.dataset:
        dataset_param = args.kitti_max_delta_t
    elif "natural" in args.dataset:
        dataset_param = args.natural_discrete
    else:
        dataset_param = args.data_distribution
    return os.path.join(f"{args.dataset}_{dataset_param}", f"{args.p}_{args.box_norm}")


def prepare_directories(args):
    """main_kitti.py:25-52 on `args` in place: ``experiment_dir``, ``output_dir/experiment_dir/seed`` and ``ckpt_dir/experiment_dir/seed``
    (both created); with ``--random-seeds`` a seed whose output directory exists is replaced by an unused one."""
    args.experiment_dir = experiment_dir(args)
    args.output_dir = os.path.join(args.output_dir, args.experiment_dir)
    os.makedirs(args.output_dir, exist_ok=True)
    existing = os.listdir(args.output_dir)
    if args.random_search or args.random_seeds:
        while str(args.seed) in existing:
            args.seed = _randint(1000000, 9999999)
    args.output_dir = os.path.join(args.output_dir, str(args.seed))
    os.makedirs(args.output_dir, exist_ok=True)
    args.ckpt_dir = os.path.join(args.ckpt_dir, args.experiment_dir, str(args.seed))
    os.makedirs(args.ckpt_dir, exist_ok=True)
    return args


def _last_logged_loss(output_dir):
    path = os.path.join(output_dir, "log.csv")
    if not os.path.exists(path):
        return None
    values = [line.strip() for line in open(path) if line.strip() and line.strip() != "Total Loss"]
    return float(values[-1]) if values else None


def run(args, dataset):
    """One pass of the reference's ``main(args, data_loader)`` (:23-79) on a copy of `args`: directories, the ``args`` file, seeding,
    then the evaluation alone or training followed by it.  Returns the dictionary of paths, last logged loss and MCC result."""
    from .kitti_masks.dataset import StreamPairSampler
    from .kitti_masks.evaluate_disentanglement import main as eval_dis
    from .kitti_masks.solver import Solver
    t0 = time.time()
    args = prepare_directories(argparse.Namespace(**vars(args)))
    if args.use_writer:
        print("--use-writer: nothing is written to TensorBoard (log.csv holds the loss)")
    args_file = os.path.join(args.output_dir, "args")
    with open(args_file, "w") as f:
        json.dump(args.__dict__, f)
    torch.manual_seed(args.seed)
    torch.cuda.manual_seed(args.seed)
    np.random.seed(args.seed)
    out = dict(output_dir=args.output_dir, ckpt_dir=args.ckpt_dir, args_file=args_file, log_file=os.path.join(args.output_dir, "log.csv"),
               seed=args.seed, last_loss=None, mcc=None)
    if args.evaluate:
        out["mcc"] = eval_dis(args, dataset)
    else:
        sampler = StreamPairSampler(dataset, args.batch_size // 2, seed=args.seed)
        failure = Solver(args, data_loader=sampler).train()
        if failure:
            print("failed in %.2fs" % (time.time() - t0))
            shutil.rmtree(args.output_dir)
            return out
        args.evaluate = True
        out["mcc"] = eval_dis(args, dataset)
        print("done in %.2fs" % (time.time() - t0))
    out["last_loss"] = _last_logged_loss(args.output_dir)
    return out


def main(argv=None, *, data=None):
    """``data``: the unpickled ``kitti_peds_v2.pickle`` dictionary (tests); otherwise it is read from ``--data-dir``."""
    from .kitti_masks.dataset import KittiMasks
    args = parse_args(argv)
    if args.random_search:
        sys.exit("--random-search is not built: it loops forever over beta / gamma / rate-prior, which the contrastive solver never reads")
    if not (args.cuda and torch.cuda.is_available()):
        sys.exit("cl_ica_amd.train_kitti needs --cuda and a visible GPU: there is no CPU path")
    assert args.image_size == 64, "currently only image size of 64 is supported"
    assert not (args.batch_size % 2)
    if args.dataset.lower() != "kittimasks":
        raise NotImplementedError(f"--dataset {args.dataset}: only kittimasks is built")
    if data is None and not os.path.exists(os.path.join(args.data_dir, "kitti_peds_v2.pickle")):
        sys.exit(f"{os.path.join(args.data_dir, 'kitti_peds_v2.pickle')} not found: put the file there (--data-dir); nothing is downloaded")
    dataset = KittiMasks(path=args.data_dir, max_delta_t=args.kitti_max_delta_t, transform=None, data=data)
    args.num_channel = 1                                      # what the reference's return_data reports for this data set
    args.graph = not args.no_graph
    if not args.random_seeds:
        return run(args, dataset)
    runs = []
    for _ in range(args.num_runs):                            # main_kitti.py:258-261
        args.seed = _randint(1000000, 9999999)
        runs.append(run(args, dataset))
    return dict(runs[-1], runs=runs) if runs else dict(runs=runs)


if __name__ == "__main__":
    main()
