"""cl_ica_amd.train_3dident without a GPU: its command line, latent-space set-up and column selection against what the reference's own
driver does (tests/golden/g28_main_3dident.json, recorded by tests/golden/gen_goldens_3dident_driver.py), the `module.`-prefix handling
and the log schedule."""
import argparse
import json
import os

import pytest

from conftest import GOLDEN

BASE = ["--offline-dataset", "somewhere"]


@pytest.fixture(scope="module")
def fixture():
    return json.load(open(os.path.join(GOLDEN, "g28_main_3dident.json")))


@pytest.fixture(scope="module")
def T():
    from cl_ica_amd import train_3dident
    return train_3dident


def _namespace(flags):
    """The flags as the fixture's generator handed them to the reference's function: no parse_args assertions in between."""
    keys = ["position_only", "rotation_and_color_only", "rotation_only", "color_only", "non_periodic_rotation_and_color",
            "no_spotlight_position", "no_spotlight_color"]
    return argparse.Namespace(sigma=0.1, non_periodical_conditional="l2", **{k: bool(flags.get(k)) for k in keys})


def test_importing_runs_nothing(T, capsys):
    assert callable(T.main) and capsys.readouterr().out == ""
    for name in ("parse_args", "setup_latent_space", "latent_dimensions_to_use", "evaluate", "train_unsupervised", "train_supervised", "test", "main"):
        assert callable(getattr(T, name))


def test_cli_table_matches_the_reference(T, fixture):
    actions = {a.option_strings[0]: a for a in T.build_parser()._actions if a.option_strings and a.option_strings[0] != "-h"}
    rows = {r["flag"]: r for r in fixture["cli"]}
    assert len(rows) == 33 and set(rows) <= set(actions)
    assert set(actions) - set(rows) == {"--seed", "--image-cache"}
    for flag, r in rows.items():
        a = actions[flag]
        if r["action"] == "store_true":
            assert isinstance(a, argparse._StoreTrueAction) and a.default is False, flag
            continue
        assert a.default == r["default"] and type(a.default) is type(r["default"]), (flag, a.default, r["default"])
        assert (a.type.__name__ if a.type is not None else None) == r["type"], flag
        assert bool(a.required) == bool(r["required"]), flag
        want = r["choices"]
        if flag == "--encoder":
            assert list(a.choices) == want + ["rn152"]      # the reference's choices say rn151, its table rn152
        else:
            assert (list(a.choices) if a.choices is not None else None) == want, flag


def test_defaults_and_choices_parse(T, fixture):
    args = T.parse_args(BASE)
    for r in fixture["cli"]:
        name = r["flag"][2:].replace("-", "_")
        if r["flag"] == "--offline-dataset":
            assert args.offline_dataset == "somewhere"
        elif r["action"] == "store_true":
            assert getattr(args, name) is False
        else:
            assert getattr(args, name) == r["default"], r["flag"]
        for c in r["choices"] or []:
            if c is not None:
                assert getattr(T.parse_args(BASE + [r["flag"], c]), name) == c
    assert args.seed is None and args.image_cache is None
    assert T.parse_args(BASE + ["--encoder", "rn152"]).encoder == "rn152"
    for flag, bad in (("--optimizer", "lbfgs"), ("--mode", "train"), ("--unsupervised-loss", "l4"), ("--encoder", "rn34"), ("--box-constraint", "soft")):
        with pytest.raises(SystemExit):
            T.parse_args(BASE + [flag, bad])
    with pytest.raises(SystemExit):
        T.parse_args([])                                    # --offline-dataset is required
    assert T.parse_args(BASE + ["--no-cuda", "--workers", "3", "--faiss-omp-threads", "2", "--approximate-dataset-nn-search"]).no_cuda is True


def test_no_spotlight_implies_both(T):
    a = T.parse_args(BASE + ["--no-spotlight"])
    assert a.no_spotlight_color is True and a.no_spotlight_position is True
    b = T.parse_args(BASE + ["--no-spotlight-color"])
    assert b.no_spotlight_color is True and b.no_spotlight_position is False and b.no_spotlight is False


def test_parse_assertions(T, tmp_path):
    ok = str(tmp_path / "f.pth")
    assert T.parse_args(BASE + ["--save-model", ok, "--save-every", "3"]).save_every == 3
    for extra in (["--save-every", "3"],                                                 # needs --save-model
                  ["--save-model", ok, "--save-every", "0"],
                  ["--save-model", ok, "--save-every", "-2"],
                  ["--position-only", "--rotation-and-color-only"],
                  ["--position-only", "--non-periodic-rotation-and-color"],
                  ["--position-only", "--no-spotlight-color"],
                  ["--position-only", "--no-spotlight-position"],
                  ["--position-only", "--no-spotlight"],
                  ["--box-constraint", "fix", "--sphere-constraint", "fix"],
                  ["--save-model", str(tmp_path / "missing" / "f.pth")],
                  ["--save-model", "f.pth"]):                                            # dirname "" does not exist, as in the reference
        with pytest.raises(AssertionError):
            T.parse_args(BASE + extra)


def test_latent_space_against_the_reference(T, fixture):
    import torch
    from cl_ica_amd import latent_spaces, spaces
    assert len(fixture["latent"]) == 40
    initialised, seen = torch.cuda.is_initialized(), set()
    for row in fixture["latent"]:
        args = _namespace(row["flags"])
        seen.add(tuple(sorted(row["flags"])))
        if "error" in row:
            with pytest.raises(ValueError) as ei:
                T.setup_latent_space(args)
            assert type(ei.value).__name__ == row["error"]
            continue
        ls, n_non_angular, n_angular = T.setup_latent_space(args)
        assert (ls.dim, n_non_angular, n_angular, type(ls).__name__) == (row["dim"], row["n_non_angular"], row["n_angular"], row["cls"]), row
        factors = ls.spaces if isinstance(ls, latent_spaces.ProductLatentSpace) else [ls]
        assert [[type(f.space).__name__, f.space.dim] for f in factors] == row["factors"], row
        for f in factors:
            assert isinstance(f.space, (spaces.NBoxSpace, spaces.NSphereSpace)) and callable(f.sample_marginal) and callable(f.sample_conditional)
    assert len(seen) == 40
    assert torch.cuda.is_initialized() == initialised                          # construction touched no device
    # the three conditionals are all accepted
    for kind in ("l1", "l2", "l3"):
        a = _namespace({"position_only": True}); a.non_periodical_conditional = kind
        assert T.setup_latent_space(a)[0].dim == 3
    assert T.setup_latent_space(_namespace({}), n_objects=2)[0].dim == 6 + 14


def test_latent_dimensions_against_the_reference(T, fixture):
    n_errors = 0
    for row in fixture["latent"]:
        args = _namespace(row["flags"])
        if "columns_error" in row:
            n_errors += 1
            with pytest.raises((ValueError, NotImplementedError)) as ei:
                T.latent_dimensions_to_use(args)
            assert type(ei.value).__name__ == row["columns_error"], row
        else:
            assert T.latent_dimensions_to_use(args) == row["columns"], row
    assert n_errors >= 4


def test_module_prefix_handling(T):
    plain = {"0.weight": 1, "2.bias": 2, "3.r": 3}
    wrapped = T.add_module_prefix(plain)
    assert list(wrapped) == ["module.0.weight", "module.2.bias", "module.3.r"] and list(wrapped.values()) == [1, 2, 3]
    assert T.strip_module_prefix(wrapped) == plain
    assert T.strip_module_prefix(plain) == plain and T.strip_module_prefix(plain) is not plain
    mixed = {"module.a": 1, "b": 2}                      # not a DataParallel file: left alone
    assert T.strip_module_prefix(mixed) == mixed
    assert T.strip_module_prefix({}) == {}
    nested = T.add_module_prefix({"module.x": 1})        # only ONE level is taken off
    assert T.strip_module_prefix(nested) == {"module.x": 1}


def test_log_schedule(T):
    assert [s for s in range(6) if T.is_log_step(s, 3, 6)] == [0, 3]
    assert [s for s in range(7) if T.is_log_step(s, 100, 7)] == [0]
    assert [s for s in range(5) if T.is_log_step(s, 1, 5)] == [0, 1, 2, 3, 4]
    assert T.is_log_step(6, 4, 6)                                         # the reference's second clause (never reached by range(n_steps))
    # saving: every --save-every completed steps
    due, last = [], 0
    for done in range(1, 8):
        if T._save_due(done, last, 3):
            due.append(done); last = done
    assert due == [3, 6] and not T._save_due(5, 0, None)
