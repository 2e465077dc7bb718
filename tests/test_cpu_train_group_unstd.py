"""The grouped trainer's unstructured forms without a GPU: the new export (header, bindings, library), the C ABI's rejections
that come before a device is looked for, the host-side refusals of train.train_unstd_nn_controllers (each before the library is
loaded) and its torch backend."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

from tests import unstd_train_helpers as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "nnmpc_train_create_group_ex"
NX, NU = 4, 2


def test_header_bindings_and_library_agree_on_the_new_export():
    from industrial_nnmpc_2021_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nnmpc.h")).read()
    assert "int " + NAME + "(" in hdr
    assert NAME in _lib.EXPORTS
    getattr(C.CDLL(_lib.LIB_PATH), NAME)
    lib = _lib.load()
    assert len(getattr(lib, NAME).argtypes) == len(lib.nnmpc_train_group_create.argtypes) + 1


def _members(G, rng):
    """G unstructured networks [12, 16, 2] (nx 4, nu 2, uprev) as per-member (Ws, bs), every bias present."""
    out = []
    for _ in range(G):
        W = T.weights(NX, NU, True, [16], rng)
        out.append(([np.ascontiguousarray(w) for w in W[0::2]], [np.ascontiguousarray(b) for b in W[1::2]]))
    return out


def _create(members, form, G=None, nx=NX, nu=NU):
    """(return code, message) of the new create through ctypes alone."""
    from industrial_nnmpc_2021_amd import _lib
    lib = _lib.load()
    G = len(members) if G is None else G
    flat = lambda k: [a for m in members for a in m[k]]
    pl = lambda arr: (C.c_void_p * max(1, len(arr)))(*[None if a is None else a.ctypes.data for a in arr])
    dims = [d for Ws, _ in members for d in [Ws[0].shape[0]] + [w.shape[1] for w in Ws]]
    h = C.c_void_p()
    rc = getattr(lib, NAME)(C.byref(h), G, 2, (C.c_int32 * max(1, len(dims)))(*dims), pl(flat(0)), pl(flat(1)), nx, nu, 1, 128,
                            1e-3, 0.9, 0.999, 1e-7, form)
    msg = lib.nnmpc_last_error().decode()
    if h.value:                                              # only where a device exists and the arguments were valid
        lib.nnmpc_train_group_destroy(h)
    return rc, msg, bool(h.value)


def test_create_rejects_what_needs_no_device_first():
    """NNMPC_EINVAL, with or without a device; every message starts with the function that was called."""
    from industrial_nnmpc_2021_amd import _lib
    mem = _members(2, np.random.default_rng(0))
    rc, msg, made = _create(mem, 7)
    assert rc == _lib.EINVAL and not made and msg.startswith(NAME + ": form 7"), msg
    for form in (_lib.NN_UNSTD, _lib.NN_UNSTD_RELU):
        nobias = [mem[0], (mem[1][0], [mem[1][1][0], None])]                        # member 1 without its head bias
        rc, msg, made = _create(nobias, form)
        assert rc == _lib.EINVAL and not made and msg.startswith(NAME + ": member 1: "), msg
        assert "bias of layer 1" in msg, msg
    rc, msg, made = _create(nobias, _lib.NN_STRUCTURED)                             # the structured head has none: no such refusal
    assert not (rc == _lib.EINVAL and "bias" in msg), msg
    rc, msg, made = _create(mem, _lib.NN_UNSTD, G=0)
    assert rc == _lib.EINVAL and not made and msg.startswith(NAME + ": a group of 0"), msg
    rc, msg, made = _create(mem, _lib.NN_UNSTD, nx=NX + 1)
    assert rc == _lib.EINVAL and not made and msg.startswith(NAME + ": member 0: dims[0]=12 (want 14)"), msg


def test_the_old_create_keeps_its_name_in_its_messages():
    from industrial_nnmpc_2021_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    one = (C.c_void_p * 1)()
    rc = lib.nnmpc_train_group_create(C.byref(h), 0, 2, (C.c_int32 * 3)(12, 16, 2), one, one, NX, NU, 1, 128, 1e-3, 0.9, 0.999, 1e-7)
    assert rc == _lib.EINVAL and lib.nnmpc_last_error().decode().startswith("nnmpc_train_group_create: a group of 0")


def test_no_cpu_fallback_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from industrial_nnmpc_2021_amd import _lib, train
    rc, msg, made = _create(_members(2, np.random.default_rng(1)), _lib.NN_UNSTD_RELU)
    assert rc != 0 and not made and msg.startswith(NAME + ": ") and "no HIP device" in msg, msg
    data = T.fit_data(np.random.default_rng(2), 64, NX, NU)
    with pytest.raises(_lib.NnmpcError, match="no HIP device"):
        train.train_unstd_nn_controllers([train.UnstdRegulatorModel(NX, NU, [0, 8, NU])], data, epochs=1)


def _no_library():
    raise AssertionError("the library must not be loaded before the host-side checks")


def test_host_refusals_come_before_the_library_is_loaded(monkeypatch):
    from industrial_nnmpc_2021_amd import _lib, train
    monkeypatch.setattr(_lib, "load", _no_library)
    data = T.fit_data(np.random.default_rng(2), 64, NX, NU)
    un = lambda nx=NX, nu=NU, dims=(0, 8, 8), **kw: train.UnstdRegulatorModel(nx, nu, list(dims) + [nu], **kw)
    fit = train.train_unstd_nn_controllers
    with pytest.raises(ValueError, match="UnstdRegulatorModel"):
        fit([un(), train.RegulatorModel(NX, NU, [0, 8, 8, NU])], data, epochs=1)
    for other in (un(nx=NX + 1), un(nu=NU + 1), un(nnwithuprev=False), un(dims=(0, 8)), un(head_relu=False)):
        with pytest.raises(ValueError, match="agree in Nx, Nu, nnwithuprev, depth and head_relu"):
            fit([un(), other], data, epochs=1)
    with pytest.raises(ValueError, match="num_samples"):
        fit([un(), un()], data, num_samples=[64], epochs=1)
    with pytest.raises(ValueError, match="num_samples"):
        fit([un()], data, num_samples=[65], epochs=1)
    with pytest.raises(ValueError, match="num_samples"):
        fit([un()], data, num_samples=[0], epochs=1)
    with pytest.raises(ValueError, match="unknown backend"):
        fit([un()], data, epochs=1, backend="triton")
    with pytest.raises(ValueError, match="no models"):
        fit([], data, epochs=1)
    with pytest.raises(ValueError, match="form"):                                   # the handle's own check, host side too
        train.HipGroupTrainer([un().get_weights()], NX, NU, form=7)
    with pytest.raises(ValueError, match="torch"):                                  # the structured sweep still refuses them
        train.train_nn_controllers([un()], data, epochs=1)


def test_the_torch_backend_loops_over_train_unstd_nn_controller():
    import torch
    from industrial_nnmpc_2021_amd import train
    torch.manual_seed(0)
    data = T.fit_data(np.random.default_rng(1), 64, NX, NU)
    a = train.UnstdRegulatorModel(NX, NU, [0, 16, NU], head_relu=False)
    b = copy.deepcopy(a)
    models, ttime, hists = train.train_unstd_nn_controllers([a], data, num_samples=[40], epochs=3, batch_size=16, lr=1e-2,
                                                            seed=3, backend="torch")
    part = {k: v[:40] for k, v in data.items()}
    b, _, hist = train.train_unstd_nn_controller(b, part, epochs=3, batch_size=16, lr=1e-2, seed=3, device="cpu", backend="torch")
    assert len(models) == 1 and ttime > 0 and len(hists[0]) == 3 and len(models[0].get_weights()) == 4
    if next(models[0].parameters()).device.type == "cpu":                           # same device, same arithmetic
        assert hists[0] == hist
        assert T.bytes_of(models[0].get_weights()) == T.bytes_of(b.get_weights())
