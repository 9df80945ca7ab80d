"""Evaluation of a trained KITTI-masks encoder: the counterpart of /root/reference/kitti_masks/evaluate_disentanglement.py for the one
metric the reference computes on this data set (continuous factors: ``mcc`` only, :65-72), without gin / disentanglement_lib.

``main(args, dataset)`` loads ``ckpt_dir/last`` into ``BetaVAE_H(z_dim, num_channel, box_norm)`` (:21-26), takes the encoder output as
the mean representation (:28-33), seeds the metric with ``np.random.RandomState(0).randint(2 ** 32)`` (:55, :84: the first draw of
that generator, the mcc config being the only one evaluated), runs ``mcc_metric.compute_mcc``, adds ``elapsed_time`` (:52) and writes
the dictionary as JSON under ``output_dir/evaluation/<ckpt_name>/mean/mcc/`` (:90-92).

Unpinned: the file name and sub-folders disentanglement_lib's ``update_result_directory`` would use below that directory cannot be
checked here; this module writes ``results/json/evaluation_results.json``.  ``num_train`` / ``correlation_fn`` come from
``args.mcc_num_train`` / ``args.mcc_correlation`` (the reference reads them from ``metric_configs/mcc.gin``, not part of its tree).
"""
from __future__ import annotations

import json
import os
import time

import numpy as np
import torch

from . import mcc_metric
from .model import BetaVAE_H

__all__ = ["main", "RESULT_FILE"]

RESULT_FILE = os.path.join("results", "json", "evaluation_results.json")


def _plain(v):
    return v.item() if isinstance(v, np.generic) else v


def main(args, dataset):
    if not (getattr(args, "cuda", False) and torch.cuda.is_available()):
        raise RuntimeError("cl_ica_amd.kitti_masks.evaluate_disentanglement runs on the GPU only (args.cuda and a visible MI355X)")
    device = torch.device("cuda", torch.cuda.current_device())
    net = BetaVAE_H(args.z_dim, args.num_channel, args.box_norm).to(device)
    checkpoint = torch.load(os.path.join(args.ckpt_dir, "last"), map_location=device)
    net.load_state_dict(checkpoint["model_states"]["net"])
    mean_rep = mcc_metric.EncoderRepresentation(net, device)

    random_seed = np.random.RandomState(0).randint(2 ** 32)
    if getattr(args, "verbose", False):
        print("Computing metric 'mcc' on 'mean'...")
    experiment_timer = time.time()
    results_dict = mcc_metric.compute_mcc(dataset, mean_rep, random_state=np.random.RandomState(random_seed),
                                          num_train=args.mcc_num_train, correlation_fn=args.mcc_correlation)
    results_dict = {k: _plain(v) for k, v in results_dict.items()}
    results_dict["elapsed_time"] = time.time() - experiment_timer
    output_dir = os.path.join(args.output_dir, "evaluation", args.ckpt_name, "mean", "mcc")
    path = os.path.join(output_dir, RESULT_FILE)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(results_dict, fh, indent=1, sort_keys=True)
    if getattr(args, "verbose", False):
        print("took", results_dict["elapsed_time"], "s")
    return results_dict
