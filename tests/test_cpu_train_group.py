"""The host side of the sweep trainer (train.group_schedule, train.train_nn_controllers' argument checks, the C ABI's new
symbols): nothing here touches a device."""
import re
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP_SYMBOLS = ["nnmpc_train_group_" + s for s in (
    "create", "destroy", "set_data", "epoch", "eval", "get_weights", "set_weights", "snapshot", "restore", "padding_max",
    "last_ms", "last_launches")]


def test_group_schedule():
    from industrial_nnmpc_2021_amd.train import group_schedule
    assert group_schedule([950, 665, 285], 256) == [[256, 256, 256, 182], [256, 256, 153], [256, 29]]
    assert group_schedule([0, 512, 1], 256) == [[], [256, 256], [1]]
    assert group_schedule([], 256) == []


def _data(n, nx, nu):
    rng = np.random.default_rng(0)
    return dict(x=rng.standard_normal((n, nx)), uprev=rng.standard_normal((n, nu)), xs=rng.standard_normal((n, nx)),
                us=rng.standard_normal((n, nu)), u=rng.standard_normal((n, nu)))


def test_mismatched_models_and_unknown_backends_are_rejected_before_the_library_is_loaded(monkeypatch):
    from industrial_nnmpc_2021_amd import _lib, train
    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    M = train.RegulatorModel
    ok = M(4, 2, [None, 8, 8, 2])
    d = _data(64, 4, 2)
    for other in (M(5, 2, [None, 8, 8, 2]), M(4, 3, [None, 8, 8, 3]), M(4, 2, [None, 8, 8, 2], nnwithuprev=False),
                  M(4, 2, [None, 8, 2])):
        with pytest.raises(ValueError, match="agree in Nx, Nu, nnwithuprev and depth"):
            train.train_nn_controllers([ok, other], d, epochs=1)
    with pytest.raises(ValueError, match="unknown backend"):
        train.train_nn_controllers([ok], d, epochs=1, backend="triton")
    with pytest.raises(ValueError, match="num_samples"):
        train.train_nn_controllers([ok, ok], d, num_samples=[64], epochs=1)
    with pytest.raises(ValueError, match="num_samples"):
        train.train_nn_controllers([ok], d, num_samples=[65], epochs=1)


def test_the_torch_backend_loops_over_train_nn_controller():
    import copy
    from industrial_nnmpc_2021_amd import train
    a = train.RegulatorModel(4, 2, [None, 8, 8, 2])
    b = copy.deepcopy(a)
    d = _data(64, 4, 2)
    models, ttime, hists = train.train_nn_controllers([a], d, num_samples=[40], epochs=2, batch_size=16, seed=3,
                                                      backend="torch")
    part = {k: v[:40] for k, v in d.items()}
    b, _, hist = train.train_nn_controller(b, part, epochs=2, batch_size=16, seed=3, device="cpu")
    assert len(models) == 1 and ttime > 0 and len(hists[0]) == 2
    if next(models[0].parameters()).device.type == "cpu":                       # same device, same arithmetic
        assert hists[0] == hist


def test_header_bindings_and_library_agree_on_the_group_symbols():
    import ctypes
    from industrial_nnmpc_2021_amd import _lib
    header = open(os.path.join(ROOT, "include", "nnmpc.h")).read()
    declared = set(re.findall(r"\bint\s+(nnmpc_train_group_\w+)\s*\(", header))
    assert declared == set(GROUP_SYMBOLS)
    assert set(GROUP_SYMBOLS) <= set(_lib.EXPORTS)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in GROUP_SYMBOLS:
        getattr(lib, name)


def test_create_rejects_bad_groups_before_it_looks_for_a_device():
    """NNMPC_EINVAL with a message, with or without a device: these checks come first."""
    from industrial_nnmpc_2021_amd import _lib
    from industrial_nnmpc_2021_amd.train import HipGroupTrainer
    rng = np.random.default_rng(0)
    W = [rng.standard_normal((16, 8)), rng.standard_normal(8), rng.standard_normal((8, 3))]      # nx 5, nu 3, uprev
    for ws, nx, nu, kw in (([], 5, 3, {}), ([W, W], 6, 3, {}), ([W], 5, 2, {}), ([W], 5, 3, dict(eps=0.0))):
        with pytest.raises(_lib.NnmpcError, match=r"\(code -1\): \S"):
            HipGroupTrainer(ws, nx, nu, max_batch=128, **kw)
    with pytest.raises(ValueError, match="same depth"):
        HipGroupTrainer([W, W[:2] + [rng.standard_normal((8, 8)), rng.standard_normal(8)] + W[2:]], 5, 3)
