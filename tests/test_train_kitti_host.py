"""Host side of the KITTI-masks driver (no GPU): the command line against the reference's parser table (g29, read from main_kitti.py
with `ast`), the directory rules, and the parts of the MCC evaluation that are host arithmetic -- the assignment, the padding rows and
the sampling loop -- against tests/kitti_mcc_oracle.py and a brute-force search over all permutations."""
import argparse
import json
import os

import numpy as np
import pytest

import kitti_mcc_oracle as MO
from conftest import GOLDEN

EXTRA = {"--data-dir", "--no-graph", "--mcc-num-train", "--mcc-correlation"}


def _actions(parser):
    return {a.option_strings[0]: a for a in parser._actions if a.option_strings and a.option_strings[0] != "-h"}


def test_parser_matches_reference_table():
    from cl_ica_amd import train_kitti as T
    table = json.load(open(os.path.join(GOLDEN, "g29_main_kitti.json")))["cli"]
    acts = _actions(T.build_parser())
    assert len(table) == 37
    assert set(acts) == {r["flag"] for r in table} | EXTRA
    for row in table:
        a = acts[row["flag"]]
        assert a.default == row["default"] and type(a.default) is type(row["default"]), (row, a.default)
        if row["action"] == "store_true":
            assert isinstance(a, argparse._StoreTrueAction), row
        else:
            assert row["action"] is None and a.type is not None and a.type.__name__ == row["type"], (row, a.type)
        assert (list(a.choices) if a.choices is not None else None) == row["choices"], row
    args = T.parse_args([])
    # (argparse leaves a non-string default alone: the default stays the int 300000, a given value goes through float)
    assert args.max_iter == 300000 and args.num_runs == 10 and args.kitti_max_delta_t == 1
    given = T.parse_args(["--max-iter", "6"]).max_iter
    assert isinstance(given, float) and given == 6.0
    # on top of the reference's
    assert args.data_dir == "./data/kitti/" and args.no_graph is False and args.mcc_num_train == 10000 and args.mcc_correlation == "Pearson"
    with pytest.raises(SystemExit):
        T.parse_args(["--mcc-correlation", "Kendall"])
    with pytest.raises(AssertionError):
        T.parse_args(["--random-seeds", "--evaluate"])
    with pytest.raises(AssertionError):
        T.parse_args(["--random-search", "--betavae"])


def test_directory_rules(tmp_path):
    from cl_ica_amd import train_kitti as T
    base = ["--output-dir", str(tmp_path / "out"), "--ckpt-dir", str(tmp_path / "ck")]
    a = T.prepare_directories(T.parse_args(base + ["--kitti-max-delta-t", "5", "--p", "1", "--box-norm", "1", "--seed", "7"]))
    assert a.experiment_dir == os.path.join("kittimasks_5", "1_1")
    assert a.output_dir == str(tmp_path / "out" / "kittimasks_5" / "1_1" / "7") and os.path.isdir(a.output_dir)
    assert a.ckpt_dir == str(tmp_path / "ck" / "kittimasks_5" / "1_1" / "7") and os.path.isdir(a.ckpt_dir)
    # an explicit experiment directory wins; other data-set names pick their own parameter
    b = T.prepare_directories(T.parse_args(base + ["--experiment-dir", "mine"]))
    assert b.output_dir == str(tmp_path / "out" / "mine" / "2") and b.ckpt_dir == str(tmp_path / "ck" / "mine" / "2")
    assert T.experiment_dir(T.parse_args(["--dataset", "natural", "--natural-discrete", "--p", "2"])) == os.path.join("natural_True", "2_0")
    assert T.experiment_dir(T.parse_args(["--dataset", "dsprites"])) == os.path.join("dsprites_laplace", "1_0")
    # --random-seeds: a seed whose directory exists is replaced by an unused one; without the flag it is reused
    np.random.seed(0)
    c = T.prepare_directories(T.parse_args(base + ["--experiment-dir", "mine", "--random-seeds"]))
    assert c.seed != 2 and 1000000 <= c.seed <= 9999999 and os.path.basename(c.output_dir) == str(c.seed)
    d = T.prepare_directories(T.parse_args(base + ["--experiment-dir", "mine"]))
    assert d.seed == 2 and d.output_dir == b.output_dir


@pytest.mark.parametrize("method", ["Pearson", "Spearman"])
@pytest.mark.parametrize("dim", [1, 2, 3, 4, 5])
def test_assignment_is_the_brute_force_optimum(dim, method):
    """Continuous inputs (no ties): the assignment on -|corr| -- the oracle's and the package's -- is the optimum over all dim!
    permutations, and corr_sort is the correlation matrix with that column order."""
    from cl_ica_amd.kitti_masks import mcc_metric as M
    rng = np.random.default_rng(100 * dim + len(method))
    N = 50
    y = rng.normal(size=(dim, N))
    mix = rng.normal(size=(dim, dim))
    x = (mix @ y + 0.5 * rng.normal(size=(dim, N)))[rng.permutation(dim)]
    corr = MO.corr_matrix(x, y, method)
    perm, best = MO.brute_force_assignment(corr)
    corr_sort, sort_idx, x_sort = MO.correlation(x, y, method)
    assert np.array_equal(sort_idx, perm.astype(np.float64))
    assert np.array_equal(x_sort, x[perm])
    assert np.allclose(corr_sort, corr[:, perm], rtol=0, atol=1e-12)
    assert abs(np.abs(np.diag(corr_sort)).sum() - best) < 1e-12
    assert np.array_equal(M._assign(corr), perm)


def test_padding_rows_and_random_state_order():
    """Factors [3, N] padded to the code dimension 5: rows 3 and 4 are the next two normal(size=N) draws, in that order; both
    restatements leave the generator in the same state."""
    from cl_ica_amd.kitti_masks import mcc_metric as M
    rng = np.random.default_rng(3)
    N = 40
    mus, ys = rng.normal(size=(5, N)), rng.normal(size=(3, N))
    ra, rb, rc = (np.random.RandomState(11) for _ in range(3))
    got, ref = M._pad_factors(mus, ys, ra), MO.pad_factors(mus, ys, rb)
    assert np.array_equal(got, ref) and np.array_equal(got[:3], ys)
    assert np.array_equal(got[3], rc.normal(size=N)) and np.array_equal(got[4], rc.normal(size=N))
    assert ra.randint(2 ** 31) == rb.randint(2 ** 31) == rc.randint(2 ** 31)
    # nothing is drawn when the factors fill the code dimension
    rd = np.random.RandomState(11)
    M._pad_factors(ys, ys, rd)
    assert rd.randint(2 ** 31) == np.random.RandomState(11).randint(2 ** 31)


class _StubData:
    """Records every sample() call; factors [n, 2], observations [n, 1, 2, 2] derived from the item numbers it draws."""

    def __init__(self):
        self.calls = []

    def sample(self, num, random_state):
        items = random_state.choice(1000, num, replace=False)
        self.calls.append((num, items.copy()))
        factors = np.stack([items, -items], 1).astype(np.float64)
        return factors, np.tile(items.astype(np.float32).reshape(num, 1, 1, 1), (1, 1, 2, 2))


def test_sampling_loop_call_sequence():
    """num_train 40 at batch_size 16: sample(16), sample(16), sample(8) on the caller's RandomState, in that order, codes and factors
    stacked and transposed -- with a host callable as representation function (no GPU involved)."""
    from cl_ica_amd.kitti_masks import mcc_metric as M
    assert MO.chunk_sizes(40, 16) == [16, 16, 8] and list(M._chunks(40, 16)) == [16, 16, 8]
    seen = []

    def rep(x):
        seen.append(x.shape)
        return np.stack([x[:, 0, 0, 0], 2.0 * x[:, 0, 1, 1], x[:, 0, 0, 1] + 1.0], 1)

    data = _StubData()
    mus, ys = M.generate_batch_factor_code(data, rep, 40, np.random.RandomState(5), 16)
    assert [c[0] for c in data.calls] == [16, 16, 8] and seen == [(16, 1, 2, 2), (16, 1, 2, 2), (8, 1, 2, 2)]
    ref = np.random.RandomState(5)
    items = np.concatenate([ref.choice(1000, n, replace=False) for n in (16, 16, 8)])
    assert np.array_equal(np.concatenate([c[1] for c in data.calls]), items)
    assert mus.shape == (3, 40) and ys.shape == (2, 40)
    assert np.array_equal(ys, np.stack([items, -items]).astype(np.float64))
    assert np.array_equal(mus, np.stack([items, 2.0 * items, items + 1.0]).astype(np.float32))
    assert np.array_equal(MO.sampled_items(1000, 40, 16, np.random.RandomState(5)), items)
    with pytest.raises(TypeError):
        M.compute_mcc(data, rep, np.random.RandomState(5))          # num_train / correlation_fn have no defaults
