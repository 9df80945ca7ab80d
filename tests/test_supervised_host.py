"""The supervised phase's fused step without a GPU: the MSE objective's C ABI is declared, bound and exported, its host-side argument
checks fail loudly, and SupervisedTrainer is part of the engine's public surface (and refuses data parallelism)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "clica.h")
NEW = ("clica_mse_loss_workspace_bytes", "clica_mse_loss_fwd_bwd")


@pytest.fixture(scope="module")
def lib():
    from cl_ica_amd import _lib
    return _lib.load()


def test_mse_entry_points_declared_bound_exported(lib):
    from cl_ica_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    # the chain's descriptor carries the objective as its LAST field (older callers that leave it zero keep today's behaviour)
    tail = re.search(r"typedef struct clica_chain_tail \{(.*?)\} clica_chain_tail;", text, flags=re.S).group(1)
    assert tail.strip().splitlines()[-1].strip().startswith("const clica_mse_target* mse;")
    assert [f[0] for f in _lib.ChainTail._fields_][-1] == "mse"
    assert [f[0] for f in _lib.MseTarget._fields_] == ["y", "ldy", "target", "ldt", "loss_out", "tick", "workspace", "workspace_bytes"]


def test_mse_workspace_query(lib):
    nb = ctypes.c_size_t()
    assert lib.clica_mse_loss_workspace_bytes(6144, 10, ctypes.byref(nb)) == 0
    # header + one float per wave of the chain's 128 panels (or of the stand-alone grid)
    assert 256 + 128 * 8 * 4 <= nb.value < 1 << 20
    assert lib.clica_mse_loss_workspace_bytes(6144, 0, ctypes.byref(nb)) == -1
    assert b"n=0" in lib.clica_last_error()
    assert lib.clica_mse_loss_workspace_bytes(0, 10, ctypes.byref(nb)) == -1
    assert lib.clica_mse_loss_workspace_bytes(64, 10, None) == -1


def test_mse_launch_argument_checks_fail_loudly(lib):
    """Every check runs on the host before anything is launched: dummy device addresses never reach a kernel."""
    nb = ctypes.c_size_t()
    assert lib.clica_mse_loss_workspace_bytes(256, 10, ctypes.byref(nb)) == 0
    P = 1 << 20          # (never dereferenced: the call returns before any launch)

    def call(ldy=10, ldt=10, lddy=10, n=10, M=256, ws_bytes=nb.value, y=P, ws=P):
        return lib.clica_mse_loss_fwd_bwd(y, ldy, P, ldt, M, n, P, lddy, P, None, ws, ws_bytes, None)

    assert call(ldy=9) == -1 and b"leading dimension" in lib.clica_last_error()
    assert call(ldt=4) == -1 and b"leading dimension" in lib.clica_last_error()
    assert call(lddy=1) == -1 and b"leading dimension" in lib.clica_last_error()
    assert call(n=0) == -1 and b"n=0" in lib.clica_last_error()
    assert call(M=0) == -1
    assert call(y=None) == -1 and b"NULL" in lib.clica_last_error()
    assert call(ws_bytes=nb.value - 4) == -1 and b"workspace" in lib.clica_last_error()
    assert call(ws=P + 4) == -1 and b"aligned" in lib.clica_last_error()


def test_supervised_trainer_is_public_and_refuses_data_parallelism():
    import torch
    from cl_ica_amd import engine
    from cl_ica_amd.engine import SamplerSpec, SupervisedTrainer
    assert "SupervisedTrainer" in engine.__all__
    # the two objectives are siblings on the shared step machinery: neither carries the other's loss
    shared = set(SupervisedTrainer.__mro__) & set(engine.ContrastiveTrainer.__mro__) - {object}
    assert shared and not issubclass(SupervisedTrainer, engine.ContrastiveTrainer)
    assert all(hasattr(c, "step") and hasattr(c, "capture") and hasattr(c, "load_state_dict") for c in shared)
    assert not hasattr(SupervisedTrainer, "loss_guard") and SupervisedTrainer.loss_spread(None) == 0.0
    f = torch.nn.Sequential(torch.nn.Linear(4, 4))
    with pytest.raises(NotImplementedError, match="one rank"):
        SupervisedTrainer(f, torch.eye(4).repeat(3, 1, 1), SamplerSpec(n=4), batch_size=8, device="cpu", force_collectives=True)
    with pytest.raises(NotImplementedError, match="data parallelism"):
        SupervisedTrainer(f, torch.eye(4).repeat(3, 1, 1), SamplerSpec(n=4), batch_size=8, device="cpu", dry_ranks=2)
