"""The tangent loss with D directions per row and whole-input directions in the native training step (csrc/nn_train.hip:
nnmpc_train_create_tan_ex, train.HipTrainer(tangents=True, tan_dirs=D, tan_whole_input=...)) against the float64 reference of
tests/tanx_helpers.py -- stock torch on the CPU, never the code under test.

Bars, by the rule of tests/test_tan_train_gpu.py.  Gradients, per parameter tensor in Keras layout: max|g_hip - g64| / max|g64|
<= max(8 x the same figure of the reference run in torch float32 on the CPU with the same weights and rows, measured on every
run, sqrt(M) 2^-24), M = (2 + D) Bp or (2 + 2D) Bp the stacked rows a dot product of the weight gradient runs over.  L, mse and
tan_mse: the same rule with floor 2^-20 relative.  The exact case (tests/test_cpu_tanx_inputs.py proves its condition) has no
bar.  The measured figures are printed (pytest -s)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from tests import tan_helpers as H
from tests import tanx_helpers as X
from tests import test_train_hip_gpu as P

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS, W = P.LR, P.B1, P.B2, P.EPS, X.W_TAN


@functools.lru_cache(maxsize=None)
def _case(name, D, whole):
    return X.case(name, D, whole)


def _trainer(Wk, nx, nu, uprev, d, max_batch, D, whole, w=W, load=True):
    from industrial_nnmpc_2021_amd.train import HipTrainer
    tr = HipTrainer(Wk, nx, nu, nnwithuprev=uprev, max_batch=max_batch, lr=LR, betas=(B1, B2), eps=EPS, tangents=True, tan_dirs=D,
                    tan_whole_input=whole)
    if load:
        tr.set_data(d)
        tr.set_tangents(d)
        tr.set_tan_weight(w)
    return tr


def _ex_trainer(Wk, nx, nu, uprev, max_batch):
    """A HipTrainer whose handle comes from nnmpc_train_create_tan_ex with dirs = 1, whole_input = 0 (the constructor sends
    those values through nnmpc_train_create_tan) and whose tangents go through nnmpc_train_set_tangents_ex."""
    from industrial_nnmpc_2021_amd import _lib
    from industrial_nnmpc_2021_amd.train import HipTrainer, _split_keras
    Ws, bs = _split_keras(Wk, _lib.NN_STRUCTURED)
    tr = object.__new__(HipTrainer)
    tr.form, tr.tangents, tr.tan_dirs, tr.tan_whole, tr._tan_ex = _lib.NN_STRUCTURED, True, 1, 0, True
    tr.dims = [Ws[0].shape[0]] + [w.shape[1] for w in Ws]
    tr.L, tr.nx, tr.nu, tr.nnwithuprev, tr.n = len(Ws), nx, nu, bool(uprev), 0
    tr._lib, tr._h = _lib.load(), C.c_void_p()
    _lib.check(tr._lib.nnmpc_train_create_tan_ex(C.byref(tr._h), tr.L, (C.c_int32 * (tr.L + 1))(*tr.dims), tr._plist(Ws), tr._plist(bs),
                                                 nx, nu, int(uprev), int(max_batch), LR, B1, B2, EPS, tr.form, 1, 0), "nnmpc_train_create_tan_ex")
    return tr


def _bytes(weights):
    return b"".join(np.ascontiguousarray(w).tobytes() for w in weights)


def _rel(a, ref):
    return np.abs(a - ref).max() / np.abs(ref).max()


def _check(tag, tr, Wk, uprev, d, rows, D, whole, w=W):
    """Loss parts and every gradient tensor of tr.grad(rows) at the weights Wk (those the handle holds) within their bars."""
    import torch
    M = X.stacked_rows((len(rows) + 127) // 128 * 128, D, whole)
    r64 = X.ref_loss_grad(Wk, uprev, d, rows, w)
    r32 = X.ref_loss_grad(Wk, uprev, d, rows, w, dtype=torch.float32)
    L, g = tr.grad(rows)
    mse, tan = tr.last_losses()
    fails = []
    for what, got, i in (("L", L, 0), ("mse", mse, 1), ("tan_mse", tan, 2)):
        e, e32 = abs(got - r64[i]) / abs(r64[i]), abs(r32[i] - r64[i]) / abs(r64[i])
        print(f"[{tag}] {what} {r64[i]:.6e}: hip {e:.2e}, torch f32 {e32:.2e}, bar {max(8 * e32, 2.0 ** -20):.2e}")
        if not e <= max(8 * e32, 2.0 ** -20):
            fails.append((what, e))
    for i, (a, b32, b64) in enumerate(zip(g, r32[3], r64[3])):
        assert a.shape == b64.shape
        e, e32 = _rel(a, b64), _rel(b32, b64)
        bar = max(8 * e32, np.sqrt(M) * 2.0 ** -24)
        print(f"[{tag}] tensor {i} {b64.shape}: hip {e:.2e}, torch f32 {e32:.2e}, bar {bar:.2e}")
        if not e <= bar:
            fails.append((i, e, bar))
    assert not fails, fails
    return L, mse, tan


@pytest.mark.parametrize("name,D,whole", X.RUNS)
def test_gradient_parity(name, D, whole):
    nx, nu, uprev, hidden, B = X.CASES[name]
    Wk, d, rows = _case(name, D, whole)
    tr = _trainer(Wk, nx, nu, uprev, d, B, D, whole)
    try:
        L, mse, tan = _check(f"{name} D={D} whole={whole}", tr, Wk, uprev, d, rows, D, whole)
        assert L == mse + W * tan and tan > 0                                # in double, as the device adds them
        assert tr.padding_max() == 0.0
    finally:
        tr.close()


def test_gradient_parity_with_three_slices_across_block_borders(monkeypatch):
    name, D, whole = X.RUN_E
    nx, nu, uprev, hidden, B = X.CASES[name]
    Wk, d, rows = _case(name, D, whole)
    monkeypatch.setenv("NNMPC_TRAIN_DW_SLICES", "3")                         # 6 Bp = 3840 rows = 120 chunks: three slices of 1280 rows, Bp = 640
    tr = _trainer(Wk, nx, nu, uprev, d, B, D, whole)
    try:
        L, mse, tan = _check("e", tr, Wk, uprev, d, rows, D, whole)
        assert L == mse + W * tan
        assert tr.dw_slices() == [3] * (len(hidden) + 1)
        assert tr.padding_max() == 0.0
    finally:
        tr.close()


@pytest.mark.parametrize("name", sorted(X.EXACT))
def test_exact_case(name):
    """D = 2, whole input, w = 1: mse, tan_mse, L and every gradient entry equal the int64 result, whatever the order the
    device adds in.  A mask from the wrong block, a missing dus, a wrong sign on the pass-2 rows or another denominator changes
    numbers (tests/test_cpu_tanx_inputs.py shows it for the reference's variants)."""
    Wk, d, rows = X.exact_case(name)
    L, mse, tan, g, peak = X.exact_int(Wk, d, rows)
    assert peak < 2 ** 24
    tr = _trainer(Wk, X.EX_NX, X.EX_NU, True, d, X.EX_B, X.EX_D, True, w=X.EX_W)
    try:
        Lh, gh = tr.grad(rows)
        assert (Lh,) + tr.last_losses() == (L, mse, tan)
        for i, (a, b) in enumerate(zip(gh, g)):
            assert np.array_equal(a, b), (i, np.abs(a - b).max())
        assert tr.padding_max() == 0.0
    finally:
        tr.close()


def _one_direction_epoch_data():
    nx, nu, uprev, Wk, d = P._epoch_data()
    return nx, nu, uprev, Wk, H.add_tangents(d, nx, nu, np.random.default_rng(2)), np.random.default_rng(3).permutation(950)


def test_an_ex_handle_with_one_direction_gives_the_bytes_of_create_tan():
    """An epoch of 950 rows at batch 256 at w > 0: losses, weights, last_losses and eval, byte for byte."""
    from tests.test_tan_train_gpu import _trainer as old_trainer
    nx, nu, uprev, Wk, d, perm = _one_direction_epoch_data()
    a, b = _ex_trainer(Wk, nx, nu, uprev, 256), old_trainer(Wk, nx, nu, uprev, d, 256)
    try:
        a.set_data(d); a.set_tangents(d); a.set_tan_weight(W)
        la, lb = a.epoch(perm, 256), b.epoch(perm, 256)
        assert la == lb and a.last_losses() == b.last_losses() and a.last_losses()[1] > 0
        assert _bytes(a.get_weights()) == _bytes(b.get_weights())
        assert a.eval(950, 50) == b.eval(950, 50) and a.last_losses() == b.last_losses()
        assert a.dw_slices() == b.dw_slices()
    finally:
        a.close(); b.close()


def test_weight_zero_gives_the_bytes_of_a_plain_handle():
    nx, nu, uprev, Wk, d = P._epoch_data()
    d = X.add_tangents(d, nx, nu, np.random.default_rng(2), 3, True)
    perm = np.random.default_rng(3).permutation(950)
    a, b = _trainer(Wk, nx, nu, uprev, d, 256, 3, True, w=0.0), P._trainer(Wk, nx, nu, uprev, d, 256)
    try:
        la, lb = a.epoch(perm, 256), b.epoch(perm, 256)
        assert la == lb and _bytes(a.get_weights()) == _bytes(b.get_weights())
        assert a.last_losses() == (la, 0.0)
        assert a.eval(950, 50) == b.eval(950, 50)
    finally:
        a.close(); b.close()


def test_two_handles_hold_the_same_bytes_and_an_epoch_equals_its_steps():
    nx, nu, uprev, Wk, d = P._epoch_data()
    d = X.add_tangents(d, nx, nu, np.random.default_rng(2), 3, True)
    perm = np.random.default_rng(3).permutation(950)
    parts = [perm[i:i + 256] for i in range(0, 950, 256)]
    a, b, c = (_trainer(Wk, nx, nu, uprev, d, 256, 3, True) for _ in range(3))
    try:
        for p in parts[:2]:
            assert a.step(p) == b.step(p)
        assert _bytes(a.get_weights()) == _bytes(b.get_weights())
        b.close()
        b = _trainer(Wk, nx, nu, uprev, d, 256, 3, True)
        losses = [(b.step(p),) + b.last_losses() for p in parts]
        le = c.epoch(perm, 256)
        assert _bytes(b.get_weights()) == _bytes(c.get_weights())
        got = (le,) + c.last_losses()
        for k, what in enumerate(("L", "mse", "tan_mse")):
            want = sum(l[k] * len(p) for l, p in zip(losses, parts)) / 950
            print(f"[epoch] {what} {got[k]:.9e}, from the steps {want:.9e}")
            assert abs(got[k] - want) <= 2.0 ** -20 * abs(want)
        assert c.padding_max() == 0.0
        v = c.eval(950, 50)
        mse, tan = c.last_losses()
        assert abs(v - (mse + W * tan)) <= 2.0 ** -50 * v and tan > 0
    finally:
        a.close(); b.close(); c.close()


def test_the_fan_equals_the_row_repeated_per_direction():
    """D = 3 partial on the B rows of case (a) against the merged one-direction handle fed each row three times, tan_weight
    unchanged.  That handle's tangent mean runs over 3 B nu too, but its primal term counts every row three times, so what is
    compared is tan_mse and the tangent part of the gradient, grad at w minus grad at 0, the two handles against each other within
    the gradient bar at the repeated handle's stacked rows."""
    import torch
    from tests.test_tan_train_gpu import _trainer as old_trainer
    D = 3
    nx, nu, uprev, hidden, B = X.CASES["a"]
    Wk, d, rows = _case("a", D, False)
    rep = X.repeat_rows(d, D)
    rrows = (D * rows[:, None] + np.arange(D)[None, :]).ravel()
    part = lambda g1, g0: [a - b for a, b in zip(g1, g0)]
    r64, r32 = (part(X.ref_loss_grad(Wk, uprev, d, rows, W, dtype=t)[3], X.ref_loss_grad(Wk, uprev, d, rows, 0.0, dtype=t)[3])
                for t in (torch.float64, torch.float32))
    a, b = _trainer(Wk, nx, nu, uprev, d, B, D, False), old_trainer(Wk, nx, nu, uprev, rep, D * B)
    try:
        ga = a.grad(rows)[1]
        tan_a = a.last_losses()[1]
        gb = b.grad(rrows)[1]
        tan_b = b.last_losses()[1]
        a.set_tan_weight(0.0); b.set_tan_weight(0.0)
        ta, tb = part(ga, a.grad(rows)[1]), part(gb, b.grad(rrows)[1])
    finally:
        a.close(); b.close()
    t64 = X.ref_loss_grad(Wk, uprev, d, rows, W)[2]
    t32 = X.ref_loss_grad(Wk, uprev, d, rows, W, dtype=torch.float32)[2]
    e, bar = abs(tan_a - tan_b) / t64, max(8 * abs(t32 - t64) / t64, 2.0 ** -20)
    print(f"[fan] tan_mse fan {tan_a:.9e} repeated {tan_b:.9e}: {e:.2e}, bar {bar:.2e}")
    assert e <= bar
    M = 3 * ((D * B + 127) // 128 * 128)
    for i, (x, y, q32, q64) in enumerate(zip(ta, tb, r32, r64)):
        if not np.abs(q64).max() > 0:                                        # a bias: tangent rows send nothing into it, and db runs over
            assert not x.any() and not y.any(), i                            # the primal rows alone, whose dZ does not depend on w
            continue
        e, bar = np.abs(x - y).max() / np.abs(q64).max(), max(8 * _rel(q32, q64), np.sqrt(M) * 2.0 ** -24)
        print(f"[fan] tangent part of tensor {i}: fan against repeated {e:.2e}, against float64 {_rel(x, q64):.2e}, bar {bar:.2e}")
        assert e <= bar, (i, e, bar)


def test_zero_dxs_and_dus_give_the_partial_handle():
    D = 2
    nx, nu, uprev, hidden, B = X.CASES["a"]
    Wk, d, rows = _case("a", D, False)
    z = dict(d, dxs=np.zeros_like(d["dx"]), dus=np.zeros_like(d["du"]))
    a, b = _trainer(Wk, nx, nu, uprev, z, B, D, True), _trainer(Wk, nx, nu, uprev, d, B, D, False)
    try:
        _check("zero whole", a, Wk, uprev, z, rows, D, True)
        La, ga = a.grad(rows)
        Lb, gb = b.grad(rows)
        assert a.last_losses() == b.last_losses() and La == Lb               # the same sums in the same order: dus = 0, a'' = 0 exactly
        for i, (x, y) in enumerate(zip(ga, gb)):
            bar = np.sqrt(X.stacked_rows(256, D, True)) * 2.0 ** -24         # the same products, exact zeros added, other slices
            assert np.abs(x - y).max() <= bar * np.abs(y).max(), (i, _rel(x, y), bar)
    finally:
        a.close(); b.close()


def test_a_nan_in_one_direction_is_isolated_and_not_hidden():
    D = 3
    nx, nu, uprev, hidden, B = X.CASES["a"]
    Wk, d, rows = _case("a", D, True)
    bad = dict(d, dus=d["dus"].copy())
    bad["dus"][rows[3], 1, 0] = np.nan
    tr = _trainer(Wk, nx, nu, uprev, bad, B, D, True)
    try:
        L, _ = tr.grad(rows[:16])                                            # not an error
        mse, tan = tr.last_losses()
        assert np.isnan(L) and np.isnan(tan) and np.isfinite(mse)
        assert np.isfinite(tr.grad(rows[4:20])[0])                           # the other rows are unaffected
        tr.grad(rows[:16])
        L2, g2 = tr.grad(rows[4:6])                                          # the NaN row's places are padding now, in every block
        assert np.isfinite(L2) and all(np.isfinite(a).all() for a in g2)
    finally:
        tr.close()


def _einval(fn, who):
    from industrial_nnmpc_2021_amd import _lib
    with pytest.raises(_lib.NnmpcError) as ei:
        fn()
    assert re.search(r"\(code -1\): \S", str(ei.value)) and who in str(ei.value), str(ei.value)


def test_error_paths_launch_nothing():
    from industrial_nnmpc_2021_amd import _lib
    D = 2
    nx, nu, uprev, hidden, B = X.CASES["a"]
    Wk, d, rows = _case("a", D, True)
    n = d["x"].shape[0]
    p = lambda a: None if a is None else np.ascontiguousarray(a, np.float64).ctypes.data_as(C.c_void_p)
    tr = _trainer(Wk, nx, nu, uprev, d, B, D, True, load=False)
    part = _trainer(Wk, nx, nu, uprev, d, B, D, False, load=False)
    plain = P._trainer(Wk, nx, nu, uprev, d, B)
    try:
        ex = lambda h, nn, dirs, dx, dup, dxs, dus, t: _lib.check(
            h._lib.nnmpc_train_set_tangents_ex(h._h, nn, dirs, p(dx), p(dup), p(dxs), p(dus), p(t), _lib.HOST), "nnmpc_train_set_tangents_ex")
        full = lambda h, **kw: ex(h, **dict(dict(nn=n, dirs=D, dx=d["dx"], dup=d["duprev"], dxs=d["dxs"], dus=d["dus"], t=d["du"]), **kw))
        _einval(lambda: full(plain), "nnmpc_train_set_tangents_ex")                          # a plain handle
        _einval(lambda: full(tr), "nnmpc_train_set_tangents_ex")                             # before set_data
        tr.set_data(d); part.set_data(d)
        _einval(lambda: full(tr, dirs=3), "nnmpc_train_set_tangents_ex")                     # another D than the handle's
        _einval(lambda: full(tr, nn=n - 1), "nnmpc_train_set_tangents_ex")
        _einval(lambda: full(tr, dup=None), "nnmpc_train_set_tangents_ex")
        _einval(lambda: full(tr, dus=None), "nnmpc_train_set_tangents_ex")                   # whole input without dus / dxs
        _einval(lambda: full(tr, dxs=None), "nnmpc_train_set_tangents_ex")
        _einval(lambda: full(part), "nnmpc_train_set_tangents_ex")                           # dxs / dus on a partial handle
        for h in (tr, part):                                                                 # the old call names the new one
            _einval(lambda: _lib.check(h._lib.nnmpc_train_set_tangents(h._h, n, p(d["dx"]), p(d["duprev"]), p(d["du"]), _lib.HOST),
                                       "nnmpc_train_set_tangents"), "nnmpc_train_set_tangents_ex")
        with pytest.raises(ValueError, match="set_tangents"):
            tr.set_tangents({k: (v[:, 0] if v.ndim == 3 else v) for k, v in d.items()})      # no direction axis at D = 2
        before = _bytes(tr.get_weights())
        l0 = tr.grad(rows)[0]                                                                # w is still 0: the plain step
        tr.set_tan_weight(W)
        for call, who in ((lambda: tr.grad(rows), "nnmpc_train_grad"), (lambda: tr.step(rows), "nnmpc_train_step"),
                          (lambda: tr.epoch(rows, 64), "nnmpc_train_epoch"), (lambda: tr.eval(0, 16), "nnmpc_train_eval")):
            _einval(call, who)                                                               # w > 0 and no tangents
        assert _bytes(tr.get_weights()) == before and tr.last_losses() == (l0, 0.0)          # nothing ran
        tr.set_tangents(d)
        assert tr.grad(rows)[0] > l0
        tr.set_data(d)                                                                       # drops the tangents
        _einval(lambda: tr.grad(rows), "nnmpc_train_grad")
    finally:
        tr.close(); part.close(); plain.close()


def test_device_resident_tangents_give_the_same_bytes():
    from industrial_nnmpc_2021_amd import _lib
    D = 3
    nx, nu, uprev, hidden, B = X.CASES["c"]
    Wk, d, rows = _case("c", D, True)
    a, b = _trainer(Wk, nx, nu, uprev, d, B, D, True), _trainer(Wk, nx, nu, uprev, d, B, D, True, load=False)
    bufs = {k: _lib.DeviceArray.from_host(np.ascontiguousarray(d[k], np.float64)) for k in ("dx", "duprev", "du", "dxs", "dus")}
    try:
        b.set_data(d)
        b.set_tangents_device(d["x"].shape[0], bufs["dx"], bufs["duprev"], bufs["du"], bufs["dxs"], bufs["dus"])
        b.set_tan_weight(W)
        la, ga = a.grad(rows)
        lb, gb = b.grad(rows)
        assert la == lb and _bytes(ga) == _bytes(gb) and a.last_losses() == b.last_losses()
    finally:
        a.close(); b.close()
        for v in bufs.values():
            v.free()


def test_tangent_data_with_three_whole_input_directions_on_a_golden_plant(golden_dir):
    """64 seeded rows around the stable golden plant: du - dus is, bit for bit, sensitivity_batch(first_move_only=True) of the
    same solve along whole_input_perturbation(...); it agrees with the gains of first_move_gain_batch(bounds=True) -- the adjoint
    kernels, a second implementation -- applied to the same perturbation within the bar of tests/test_adj_solve_gpu.py (8 x the
    gap of the two float64 routes on these sets, floor 64 2^-53 (n + n_aug), times the scale of the sums); flagged rows are zero."""
    from industrial_nnmpc_2021_amd.train import tangent_data, whole_input_perturbation
    from tests import adj_helpers as A
    from tests import mult_helpers as M
    from tests import sens_helpers as S
    g = np.load(os.path.join(golden_dir, "regulator_stable_s0.npz"))
    reg = M.golden_regulator(g, max_batch=128)
    try:
        nx, nu, D, B = g["A"].shape[0], g["B"].shape[1], 3, 64
        rng = np.random.default_rng(64)
        ulb, uub = g["ulb"].ravel(), g["uub"].ravel()
        us = ulb + (uub - ulb) * rng.uniform(0.3, 0.7, (B, nu))
        xs = 0.1 * rng.standard_normal((B, nx))
        raw = dict(x=xs + 2.0 * rng.standard_normal((B, nx)), uprev=us + 0.1 * (uub - ulb) * rng.standard_normal((B, nu)), xs=xs, us=us)
        xscale = rng.uniform(0.5, 2.0, nx)
        td = tangent_data(reg, raw, xscale, ulb=ulb, uub=uub, seed=3, directions=D, whole_input=True)
        assert all(td[k].shape == (B, D, w) for k, w in (("dx", nx), ("duprev", nu), ("dxs", nx), ("dus", nu), ("du", nu)))
        _, info = reg.solve_batch(np.hstack((raw["x"] - xs, raw["uprev"] - us)), ulb - us, uub - us, first_move_only=True)
        dX0, dlb, dub = whole_input_perturbation(td["dx"], td["duprev"], td["dxs"], td["dus"], xscale)
        out = reg.sensitivity_batch(info, dX0, dulb=dlb, duub=dub, first_move_only=True)
        ok = (out["flag"] == 0) & (info["status"] == 0)
        print(f"[golden] {int(ok.sum())} of {B} rows carry a slope, {int(info['active'].any(axis=1).sum())} with active bounds")
        assert np.array_equal(td["flag"], out["flag"]) and ok.sum() >= B // 2
        assert np.array_equal(td["du"][ok], (td["dus"] + out["du"])[ok]) and np.abs(out["du"][ok]).max() > 0   # du - dus IS that call's du
        for k in ("dx", "duprev", "dxs", "dus", "du"):
            assert (td[k][~ok] == 0.0).all(), k
        K, Klb, Kub, flag = reg.first_move_gain_batch(info, bounds=True)
        Pb, tqb = reg._box_form()
        Pb = np.tril(Pb) + np.tril(Pb, -1).T
        n, n_aug = Pb.shape[0], nx + nu
        Hinv = np.linalg.inv(Pb)
        Hinv = 0.5 * (Hinv + Hinv.T)
        Kunc = -Hinv @ tqb
        words = M.pack_rows(info["active"], n)
        r = np.random.default_rng(5)
        v, qx, ql, qu = r.standard_normal((B, 4, n)), r.standard_normal((B, 4, n_aug)), r.standard_normal((B, 4, nu)), r.standard_normal((B, 4, nu))
        gap, scale = A.identity_gap(v, S.sens_route_f64(Hinv, Kunc, words, qx, ql, qu, nu), A.adjoint_route_f64(Hinv, Kunc, words, v, nu), qx, ql, qu)
        tol = A.tolerance(float((gap / scale)[ok].max()), n, n_aug)
        ein = lambda G, q: np.einsum("bjk,bdk->bdj", G, q)
        pred = ein(K, dX0) + ein(Klb, dlb) + ein(Kub, dub)
        sc = ein(np.abs(K), np.abs(dX0)) + ein(np.abs(Klb), np.abs(dlb)) + ein(np.abs(Kub), np.abs(dub)) + np.abs(out["du"])
        ratio = (np.abs(pred - out["du"]) / sc)[ok & (flag == 0)]
        print(f"[golden] max |gains . perturbation - sensitivity| / scale {ratio.max():.2e}, tol {tol:.2e}")
        assert ratio.max() <= tol
    finally:
        reg._solver().close()
