"""The driver's --amp flag on a CPU-only host: the parser, and the refusals that come before any device work."""
import inspect

import pytest

BASE = ["--offline-dataset", "somewhere"]


@pytest.fixture(scope="module")
def T():
    from cl_ica_amd import train_3dident
    return train_3dident


def test_the_parser_takes_amp(T):
    assert T.parse_args(BASE).amp == "off"
    assert T.parse_args(BASE + ["--amp", "bf16"]).amp == "bf16" and T.parse_args(BASE + ["--amp", "off"]).amp == "off"
    assert "--amp" in [flag for flag, _ in T._EXTRA_ARGS] and "--amp" not in [flag for flag, _ in T._ARGS]
    assert "--amp {off,bf16}" in T.build_parser().format_help()           # read ahead of the table's parser, named in its help
    assert T.parse_args(["--amp", "bf16"] + BASE + ["--position-only"]).position_only is True
    for bad in ("fp16", "on", "BF16"):
        with pytest.raises(SystemExit):
            T.parse_args(BASE + ["--amp", bad])
    assert T._amp(T.parse_args(BASE)) is None and T._amp(T.parse_args(BASE + ["--amp", "bf16"])) == "bf16"
    import argparse
    assert T._amp(argparse.Namespace()) is None                       # argument objects from before the flag


@pytest.mark.parametrize("flag", ["--dummy-mixing", "--identity-solution", "--identity-mixing-and-solution"])
def test_bf16_without_a_backbone_is_refused_while_parsing(T, flag):
    with pytest.raises(AssertionError, match="no backbone"):
        T.parse_args(BASE + ["--amp", "bf16", flag])
    with pytest.raises(AssertionError, match="no backbone"):          # main refuses before it looks for a device or the dataset
        T.main(BASE + ["--amp", "bf16", flag])
    assert T.parse_args(BASE + ["--amp", "off", flag]).amp == "off"    # "off" goes with everything


def test_the_steps_take_amp_and_none_is_the_plain_call():
    from cl_ica_amd import threedident
    for fn in (threedident.train_step, threedident.train_step_supervised):
        assert inspect.signature(fn).parameters["amp"].default is None
    from cl_ica_amd import train_3dident
    assert inspect.signature(train_3dident.evaluate).parameters["amp"].default is None
    calls = []
    f = lambda x: calls.append(x) or x + 1  # noqa: E731
    assert threedident.encode(f, 2) == 3 and threedident.encode(f, 2, None) == 3 and calls == [2, 2]
    with pytest.raises(ValueError, match="amp="):
        threedident.encode(f, 2, "fp16")
    assert calls == [2, 2]
