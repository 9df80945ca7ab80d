"""cl_ica_amd.train_kitti end to end on the GPU, on a synthetic data dictionary (17 sequences of 64 x 64 masks) handed over through
``main(data=...)``: the captured run, the eager run (same log and checkpoint, bit for bit), ``--evaluate`` alone, and the MCC evaluation
against tests/kitti_mcc_oracle.py."""
import json
import os

import numpy as np
import pytest
import torch

import kitti_mcc_oracle as MO
from conftest import PARITY, conv_formula, fill_formula

pytestmark = pytest.mark.gpu

FLAGS = ["--z-dim", "4", "--batch-size", "16", "--max-iter", "6", "--log-step", "2", "--save-step", "3", "--p", "1", "--box-norm", "1",
         "--mcc-num-train", "64", "--cuda"]


def _synthetic_kitti(rng, n_seq=17, hw=64):
    lens = rng.integers(2, 40, size=n_seq)
    data = [rng.random((int(T), hw, hw)) < 0.1 for T in lens]
    lat = [rng.normal(size=(int(T), 3)).astype(np.float32) for T in lens]
    return {"pedestrians": data, "pedestrians_latents": lat}


@pytest.fixture(scope="module")
def raw():
    return _synthetic_kitti(np.random.default_rng(5))


def _run(raw, root, extra=()):
    from cl_ica_amd import train_kitti as T
    out = T.main(FLAGS + ["--output-dir", os.path.join(root, "out"), "--ckpt-dir", os.path.join(root, "ck")] + list(extra), data=raw)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def run_a(raw, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("kitti_a"))
    return root, _run(raw, root)


def _log_lines(out):
    return open(out["log_file"]).read().splitlines()


def test_captured_run_writes_what_the_reference_writes(run_a):
    root, out = run_a
    assert out["output_dir"] == os.path.join(root, "out", "kittimasks_1", "1_1", "2")
    assert out["ckpt_dir"] == os.path.join(root, "ck", "kittimasks_1", "1_1", "2")
    args = json.load(open(os.path.join(out["output_dir"], "args")))
    assert args["z_dim"] == 4 and args["batch_size"] == 16 and args["max_iter"] == 6.0 and args["num_channel"] == 1 and args["graph"] is True
    assert args["output_dir"] == out["output_dir"] and args["ckpt_dir"] == out["ckpt_dir"] and args["beta"] == 1 and args["num_runs"] == 10
    lines = _log_lines(out)
    assert lines[0] == "Total Loss" and len(lines) == 4
    values = [float(v) for v in lines[1:]]
    assert all(np.isfinite(v) and v > 0 for v in values) and out["last_loss"] == values[-1]
    ck = torch.load(os.path.join(out["ckpt_dir"], "last"), map_location="cpu")
    assert set(ck) == {"iter", "model_states", "optim_states"} and ck["iter"] == 6
    assert set(ck["model_states"]) == {"net"} and set(ck["optim_states"]) == {"optim"}
    assert "encoder.0.weight" in ck["model_states"]["net"] and "encoder.12.max_abs_bound" in ck["model_states"]["net"]
    path = os.path.join(out["output_dir"], "evaluation", "last", "mean", "mcc", "results", "json", "evaluation_results.json")
    res = json.load(open(path))
    assert res == out["mcc"]
    assert 0.0 <= res["meanabscorr"] <= 1.0 and res["elapsed_time"] >= 0.0
    assert len([k for k in res if k.startswith("corr_sorted_")]) == 16 and len([k for k in res if k.startswith("sort_idx_")]) == 4
    assert sorted(res["sort_idx_%d" % i] for i in range(4)) == [0.0, 1.0, 2.0, 3.0]


def _tensors(tree, prefix=""):
    if torch.is_tensor(tree):
        yield prefix, tree
    elif isinstance(tree, dict):
        for k in sorted(tree, key=str):
            yield from _tensors(tree[k], f"{prefix}/{k}")
    elif isinstance(tree, (list, tuple)):
        for i, v in enumerate(tree):
            yield from _tensors(v, f"{prefix}/{i}")


def test_eager_run_writes_the_same_log_and_checkpoint(raw, run_a, tmp_path):
    """--no-graph issues the same launches eagerly: log.csv equal as written (both loops sum the loss in one device fp32 scalar, in the
    same order), every checkpoint tensor bit-equal."""
    _, a = run_a
    b = _run(raw, str(tmp_path), ["--no-graph"])
    assert json.load(open(os.path.join(b["output_dir"], "args")))["graph"] is False
    assert open(a["log_file"]).read() == open(b["log_file"]).read()
    ca = torch.load(os.path.join(a["ckpt_dir"], "last"), map_location="cpu")
    cb = torch.load(os.path.join(b["ckpt_dir"], "last"), map_location="cpu")
    ta, tb = dict(_tensors(ca)), dict(_tensors(cb))
    assert ca["iter"] == cb["iter"] == 6 and set(ta) == set(tb) and len(ta) >= 14
    for name in ta:
        assert torch.equal(ta[name], tb[name]), name
    assert {k: v for k, v in a["mcc"].items() if k != "elapsed_time"} == {k: v for k, v in b["mcc"].items() if k != "elapsed_time"}


def test_evaluate_alone_reproduces_the_evaluation(raw, run_a):
    root, a = run_a
    log_before = open(a["log_file"]).read()
    e = _run(raw, root, ["--evaluate"])
    assert e["output_dir"] == a["output_dir"] and e["ckpt_dir"] == a["ckpt_dir"]
    assert {k: v for k, v in e["mcc"].items() if k != "elapsed_time"} == {k: v for k, v in a["mcc"].items() if k != "elapsed_time"}
    assert open(a["log_file"]).read() == log_before                                  # nothing was trained


def test_driver_refusals(raw, tmp_path):
    from cl_ica_amd import train_kitti as T
    base = ["--output-dir", str(tmp_path / "o"), "--ckpt-dir", str(tmp_path / "c")]
    with pytest.raises(SystemExit):
        T.main(base, data=raw)                                                       # no --cuda
    with pytest.raises(SystemExit):
        T.main(base + ["--cuda", "--random-search"], data=raw)
    with pytest.raises(SystemExit):
        T.main(base + ["--cuda", "--data-dir", str(tmp_path / "nowhere")])           # no pickle, no download
    assert not os.path.exists(tmp_path / "o")


@pytest.fixture(scope="module")
def mcc_setup(raw):
    from cl_ica_amd.kitti_masks import dataset as D
    from cl_ica_amd.kitti_masks.model import BetaVAE_H
    net = BetaVAE_H(4, 1, True).cuda()
    fill_formula(net, conv_formula)
    return D.KittiMasks(data=raw, max_delta_t=3), net


@pytest.mark.parametrize("method", ["Pearson", "Spearman"])
def test_mcc_matches_the_oracle(raw, mcc_setup, method):
    """num_train 64 at batch_size 16.  The bulk path's factors are bit-equal to the oracle's restatement of the sample loop for the same
    RandomState, its images to the oracle's first frames; with the device codes copied to the host as the oracle's input, meanabscorr and
    the corr_sorted matrix agree at the project's 1e-5 (ranks are taken from identical fp32 codes: no allowance for Spearman) and sort_idx
    is equal."""
    from cl_ica_amd import ops
    from cl_ica_amd.kitti_masks import mcc_metric as M
    ds, net = mcc_setup
    rep = M.EncoderRepresentation(net)
    mus, ys = M.generate_batch_factor_code(ds, rep, 64, np.random.RandomState(17), 16)
    assert torch.is_tensor(mus) and mus.is_cuda and mus.shape == (4, 64) and ys.shape == (3, 64)
    cum = np.cumsum([len(s) - 1 for s in raw["pedestrians"]])
    items = MO.sampled_items(len(ds), 64, 16, np.random.RandomState(17))
    frames, labs = MO.first_frames(raw["pedestrians"], raw["pedestrians_latents"], cum, items)
    assert np.array_equal(ys, labs.T)
    got_frames, _ = ops.kitti_gather_frames(ds.frames, torch.as_tensor(ds.first_frame_ids(items)))
    assert np.array_equal(got_frames.cpu().numpy(), frames)
    codes = mus.cpu().numpy()
    assert np.isfinite(codes).all() and (codes.std(1) > 0).all()
    got = M._compute_mcc(mus, ys, method, np.random.RandomState(1))
    ref = MO.compute_mcc_from_codes(codes, ys, method, np.random.RandomState(1))
    assert set(got) == set(ref) and len(got) == 1 + 16 + 4
    mat = lambda d: np.array([[d["corr_sorted_%d%d" % (i, j)] for j in range(4)] for i in range(4)])      # noqa: E731
    print(method, "meanabscorr", got["meanabscorr"], ref["meanabscorr"], "max |corr diff|", np.abs(mat(got) - mat(ref)).max())
    assert [got["sort_idx_%d" % i] for i in range(4)] == [ref["sort_idx_%d" % i] for i in range(4)]
    PARITY.check("kitti_mcc", method, "meanabscorr", got["meanabscorr"], ref["meanabscorr"])
    PARITY.check("kitti_mcc", method, "corr_sorted", mat(got), mat(ref))
    # compute_mcc end to end = the same two steps on the same RandomState
    full = M.compute_mcc(ds, rep, np.random.RandomState(17), num_train=64, correlation_fn=method)
    rs = np.random.RandomState(17)
    mus2, ys2 = M.generate_batch_factor_code(ds, rep, 64, rs, 16)
    assert full == M._compute_mcc(mus2, ys2, method, rs)


@pytest.mark.parametrize("method", ["Pearson", "Spearman"])
def test_host_callable_representation_gives_the_same_result(mcc_setup, method):
    """An arbitrary host callable (numpy in, numpy out) is served chunk by chunk through KittiMasks.sample; with the encoder behind it
    the dictionary equals the bulk path's: same factors, same assignment, correlations at 1e-5 (the encoder sees 16 images per call
    instead of 64 and its split arithmetic scales by per-batch maxima: bit equality of the codes is not promised)."""
    from cl_ica_amd.kitti_masks import mcc_metric as M
    ds, net = mcc_setup
    rep = M.EncoderRepresentation(net)
    shapes = []

    def host_rep(x):
        assert isinstance(x, np.ndarray)
        shapes.append(x.shape)
        return rep(x)

    bulk = M.compute_mcc(ds, rep, np.random.RandomState(17), num_train=64, correlation_fn=method)
    host = M.compute_mcc(ds, host_rep, np.random.RandomState(17), num_train=64, correlation_fn=method)
    assert shapes == [(16, 1, 64, 64)] * 4 and set(bulk) == set(host)
    keys = sorted(k for k in bulk if not k.startswith("sort_idx_"))
    print(method, "max diff", max(abs(bulk[k] - host[k]) for k in keys))
    assert [bulk["sort_idx_%d" % i] for i in range(4)] == [host["sort_idx_%d" % i] for i in range(4)]
    PARITY.check("kitti_mcc", method, "host callable vs bulk", np.array([host[k] for k in keys]), np.array([bulk[k] for k in keys]))
    # with the bulk path's encoder chunk set to the host path's 16 images per call -- the same images in the same order -- the two
    # dictionaries are THE SAME
    same = M.compute_mcc(ds, M.EncoderRepresentation(net, chunk=16), np.random.RandomState(17), num_train=64, correlation_fn=method)
    assert same == host
