"""The tangent loss of the native training step (csrc/nn_train.hip: nnmpc_train_create_tan, train.HipTrainer(tangents=True))
against the float64 reference of tests/tan_helpers.py -- stock torch on the CPU, never the code under test.

Bars.  Gradients, per parameter tensor in Keras layout: max|g_hip - g64| / max|g64| <= max(8 x the same figure of the
reference run in torch float32 on the CPU with the same weights and rows, measured on every run, sqrt(3 Bp) 2^-24): the rule
tests/test_train_hip_gpu.py derives, at the 3 Bp stacked rows a dot product of the weight gradient now runs over.  L, mse and
tan_mse: the same rule with floor 2^-20 relative.  Rows are kink-free by that file's rule.  The exact case (integer and dyadic
data, tests/test_cpu_tan_inputs.py proves its condition) has no bar: every number must equal the int64 result.  The measured
figures are printed (pytest -s)."""
import functools
import re

import numpy as np
import pytest

from tests import tan_helpers as H
from tests import test_train_hip_gpu as P

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS, W = P.LR, P.B1, P.B2, P.EPS, H.W_TAN


@functools.lru_cache(maxsize=None)
def _case(name):
    return H.case(name)


def _trainer(Wk, nx, nu, uprev, d, max_batch, w=W, tangents=True):
    from industrial_nnmpc_2021_amd.train import HipTrainer
    tr = HipTrainer(Wk, nx, nu, nnwithuprev=uprev, max_batch=max_batch, lr=LR, betas=(B1, B2), eps=EPS, tangents=tangents)
    tr.set_data(d)
    if tangents:
        tr.set_tangents(d)
        tr.set_tan_weight(w)
    return tr


def _bytes(weights):
    return b"".join(np.ascontiguousarray(w).tobytes() for w in weights)


def _check(tag, tr, Wk, uprev, d, rows, w=W):
    """Loss parts and every gradient tensor of tr.grad(rows) at the weights Wk (those the handle holds) within their bars."""
    import torch
    Bp = (len(rows) + 127) // 128 * 128
    r64 = H.ref_loss_grad(Wk, uprev, d, rows, w)
    r32 = H.ref_loss_grad(Wk, uprev, d, rows, w, dtype=torch.float32)
    L, g = tr.grad(rows)
    mse, tan = tr.last_losses()
    rel = lambda a, ref: np.abs(a - ref).max() / np.abs(ref).max()
    fails = []
    for what, got, i in (("L", L, 0), ("mse", mse, 1), ("tan_mse", tan, 2)):
        if r64[i] == 0.0:
            assert got == 0.0, (what, got)
            continue
        e, e32 = abs(got - r64[i]) / abs(r64[i]), abs(r32[i] - r64[i]) / abs(r64[i])
        print(f"[{tag}] {what} {r64[i]:.6e}: hip {e:.2e}, torch f32 {e32:.2e}, bar {max(8 * e32, 2.0 ** -20):.2e}")
        if not e <= max(8 * e32, 2.0 ** -20):
            fails.append((what, e))
    for i, (a, b32, b64) in enumerate(zip(g, r32[3], r64[3])):
        assert a.shape == b64.shape
        e, e32 = rel(a, b64), rel(b32, b64)
        bar = max(8 * e32, np.sqrt(3 * Bp) * 2.0 ** -24)
        print(f"[{tag}] tensor {i} {b64.shape}: hip {e:.2e}, torch f32 {e32:.2e}, bar {bar:.2e}")
        if not e <= bar:
            fails.append((i, e, bar))
    assert not fails, fails
    return L, mse, tan


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_gradient_parity(name):
    nx, nu, uprev, hidden, B = H.CASES[name]
    Wk, d, rows = _case(name)
    tr = _trainer(Wk, nx, nu, uprev, d, B)
    try:
        L, mse, tan = _check(name, tr, Wk, uprev, d, rows)
        assert L == mse + W * tan and tan > 0                                # in double, as the device adds them
        if name == "a":
            assert tr.dw_slices() == [1] * (len(hidden) + 1)                 # what case (e) is compared with
        assert tr.padding_max() == 0.0
    finally:
        tr.close()


def test_gradient_parity_with_three_slices_of_the_stacked_rows(monkeypatch):
    nx, nu, uprev, hidden, B = H.CASES["e"]
    Wk, d, rows = _case("e")
    monkeypatch.setenv("NNMPC_TRAIN_DW_SLICES", "3")                         # 3 Bp = 1920 rows = 60 chunks: three slices of 20
    tr = _trainer(Wk, nx, nu, uprev, d, B)
    try:
        _check("e", tr, Wk, uprev, d, rows)
        assert tr.dw_slices() == [3] * (len(hidden) + 1)
        assert tr.padding_max() == 0.0
    finally:
        tr.close()


@pytest.mark.parametrize("name", sorted(H.EXACT))
def test_exact_case(name):
    """Every quantity is a small multiple of a power of two: mse, tan_mse, L and every gradient entry equal the int64 result,
    whatever the order the device adds in.  Zeros of the pass-1 pre-activation, both signs, and a pass 2 with other signs are
    in it (tests/test_cpu_tan_inputs.py), so a mask taken from the wrong place, or a bias on the tangent rows, changes numbers."""
    Wk, d, rows = H.exact_case(name)
    L, mse, tan, g, peak = H.exact_int(Wk, d, rows)
    assert peak < 2 ** 24
    tr = _trainer(Wk, H.EX_NX, H.EX_NU, True, d, H.EX_B)
    try:
        Lh, gh = tr.grad(rows)
        assert (Lh,) + tr.last_losses() == (L, mse, tan)
        for i, (a, b) in enumerate(zip(gh, g)):
            assert np.array_equal(a, b), (i, np.abs(a - b).max())
        assert tr.padding_max() == 0.0
    finally:
        tr.close()


def test_weight_zero_gives_the_bytes_of_a_plain_handle():
    """An epoch of 950 rows at batch 256 (three full batches and one of 182) on a tangent handle at w = 0, tangents loaded."""
    nx, nu, uprev, Wk, d = P._epoch_data()
    d = H.add_tangents(d, nx, nu, np.random.default_rng(2))
    perm = np.random.default_rng(3).permutation(950)
    a, b = _trainer(Wk, nx, nu, uprev, d, 256, w=0.0), P._trainer(Wk, nx, nu, uprev, d, 256)
    try:
        la, lb = a.epoch(perm, 256), b.epoch(perm, 256)
        assert la == lb and _bytes(a.get_weights()) == _bytes(b.get_weights())
        assert a.last_losses() == (la, 0.0) and b.last_losses() == (lb, 0.0)
        assert a.eval(950, 50) == b.eval(950, 50)
        assert a.dw_slices() == b.dw_slices()
    finally:
        a.close(); b.close()


def test_the_primal_part_is_the_plain_loss():
    """At w > 0 the first set of partials is computed exactly as today: mse equals the plain handle's loss as a double."""
    nx, nu, uprev, hidden, B = H.CASES["a"]
    Wk, d, rows = _case("a")
    a, b = _trainer(Wk, nx, nu, uprev, d, B), P._trainer(Wk, nx, nu, uprev, d, B)
    try:
        a.grad(rows)
        assert a.last_losses()[0] == b.grad(rows)[0]
        a.eval(P.FILL, B)
        assert a.last_losses()[0] == b.eval(P.FILL, B)
    finally:
        a.close(); b.close()


def test_two_handles_hold_the_same_bytes_and_an_epoch_equals_its_steps():
    nx, nu, uprev, Wk, d = P._epoch_data()
    d = H.add_tangents(d, nx, nu, np.random.default_rng(2))
    perm = np.random.default_rng(3).permutation(950)
    parts = [perm[i:i + 256] for i in range(0, 950, 256)]
    a, b, c = (_trainer(Wk, nx, nu, uprev, d, 256) for _ in range(3))
    try:
        for p in parts[:3]:
            assert a.step(p) == b.step(p)
        assert _bytes(a.get_weights()) == _bytes(b.get_weights())
        b.close()
        b = _trainer(Wk, nx, nu, uprev, d, 256)
        losses = [(b.step(p),) + b.last_losses() for p in parts]
        le = c.epoch(perm, 256)
        assert _bytes(b.get_weights()) == _bytes(c.get_weights())
        got = (le,) + c.last_losses()
        for k, what in enumerate(("L", "mse", "tan_mse")):
            want = sum(l[k] * len(p) for l, p in zip(losses, parts)) / 950
            print(f"[epoch] {what} {got[k]:.9e}, from the steps {want:.9e}")
            assert abs(got[k] - want) <= 2.0 ** -20 * abs(want)
        assert np.abs(np.concatenate([w.ravel() for w in c.get_weights()]) - np.concatenate([w.ravel() for w in Wk])).max() > LR
        assert c.padding_max() == 0.0
        v = c.eval(950, 50)
        mse, tan = c.last_losses()
        assert abs(v - (mse + W * tan)) <= 2.0 ** -50 * v and tan > 0
    finally:
        a.close(); b.close(); c.close()


def test_adam_step_applies_the_gradient_grad_returns():
    """One step at w > 0: every entry within 4 * 2^-24 * max(|W_ref|, lr) of torch's formula applied to grad's gradient."""
    nx, nu, uprev, hidden, B = H.CASES["a"]
    Wk, d, rows = _case("a")
    tr = _trainer(Wk, nx, nu, uprev, d, B)
    try:
        W0 = tr.get_weights()
        _, g = tr.grad(rows)
        tr.step(rows)
        W1 = tr.get_weights()
        worst = 0.0
        for i in range(len(Wk)):
            m, v = g[i] * (1 - B1), (1 - B2) * g[i] * g[i]
            ref = W0[i] - LR / (1 - B1) * m / (np.sqrt(v) / np.sqrt(1 - B2) + EPS)
            worst = max(worst, (np.abs(W1[i] - ref) / (4 * 2.0 ** -24 * np.maximum(np.abs(ref), LR))).max())
            assert np.abs(W1[i] - W0[i]).max() > 0.1 * LR
        print(f"[adam] worst |W_hip - W_ref| / bar = {worst:.3f}")
        assert worst <= 1.0
        assert tr.padding_max() == 0.0
    finally:
        tr.close()


def test_zero_directions_leave_the_plain_gradient():
    import torch
    nx, nu, uprev, hidden, B = H.CASES["a"]
    Wk, d, rows = _case("a")
    z = dict(d, dx=np.zeros_like(d["dx"]), duprev=np.zeros_like(d["duprev"]), du=np.zeros_like(d["du"]))
    tr = _trainer(Wk, nx, nu, uprev, z, B)
    try:
        L, g = tr.grad(rows)
        mse, tan = tr.last_losses()
        assert tan == 0.0 and L == mse
        l64, g64 = P._torch_grad(Wk, nx, nu, uprev, d, rows, torch.float64)
        l32, g32 = P._torch_grad(Wk, nx, nu, uprev, d, rows, torch.float32)
        rel = lambda a, ref: np.abs(a - ref).max() / np.abs(ref).max()
        assert abs(L - l64) / l64 <= max(8 * abs(l32 - l64) / l64, 2.0 ** -20)
        for i, (a, b32, b64) in enumerate(zip(g, g32, g64)):
            e, bar = rel(a, b64), max(8 * rel(b32, b64), np.sqrt(3 * 256) * 2.0 ** -24)
            print(f"[zero] tensor {i}: hip {e:.2e}, bar {bar:.2e}")
            assert e <= bar, (i, e, bar)
    finally:
        tr.close()


def _signs(Wc, uprev, d, rows, npdtype):
    """Sign pattern of every hidden pre-activation of both passes on ``rows``, computed in ``npdtype``."""
    z1, z2, _ = H.stack(d, rows, uprev)
    out = []
    for z in (z1.astype(npdtype), z2.astype(npdtype)):
        for l in range(0, len(Wc) - 1, 2):
            p = z @ Wc[l].astype(npdtype) + Wc[l + 1].astype(npdtype)
            out.append(p > 0)
            z = np.maximum(p, 0)
    return np.concatenate([o.ravel() for o in out])


def _adam_run(Wk, uprev, d, rows, steps, dtype):
    """The reference's trajectory: ``steps`` Adam updates on the batch ``rows`` with the gradients of ref_loss_grad in ``dtype``;
    in float32 the weights and moments are rounded to f32 after every update, as the device stores them.  Returns the final
    (L, mse, tan_mse) in ``dtype``; per row of ``rows`` the smallest kink margin (smallest / largest |pre-activation|, as
    tests/test_train_hip_gpu.py measures it) met at the weights of any step, the last included; and the sign patterns there."""
    import torch
    f32 = dtype == torch.float32
    rnd = (lambda a: P._f32(a)) if f32 else (lambda a: a)
    Wc = [w.copy() for w in Wk]
    m, v = [np.zeros_like(w) for w in Wk], [np.zeros_like(w) for w in Wk]
    lo, hi = P._kink_margin(Wc, d, uprev)
    margin, signs = lo[rows] / hi[rows], []
    for t in range(1, steps + 1):
        g = H.ref_loss_grad(Wc, uprev, d, rows, W, dtype=dtype)[3]
        for i in range(len(Wc)):
            m[i] = rnd(m[i] + (g[i] - m[i]) * (1 - B1))
            v[i] = rnd(B2 * v[i] + (1 - B2) * g[i] * g[i])
            Wc[i] = rnd(Wc[i] - LR / (1 - B1 ** t) * m[i] / (np.sqrt(v[i]) / np.sqrt(1 - B2 ** t) + EPS))
        lo, hi = P._kink_margin(Wc, d, uprev)
        margin = np.minimum(margin, lo[rows] / hi[rows])
        signs.append(_signs(Wc, uprev, d, rows, np.float32 if f32 else np.float64))
    return H.ref_loss_grad(Wc, uprev, d, rows, W, dtype=dtype)[:3], margin, signs


def test_five_steps_follow_the_float64_trajectory():
    """Five steps at w > 0 on the kink-free rows of case (a); the final L and tan_mse against the float64 reference run from
    the same weights and batches, the bar 8 x what the float32 reference run leaves (measured, no floor).  The weights move
    and the margins of the first choice shrink with them (printed), so the reference checks what matters: its float32 run
    takes the float64 run's side of every kink of every row at the weights of every step, so the two -- and a device that
    rounds like float32 -- differentiate the same branch.  Were that to fail, the run is to be shortened, not the bar widened."""
    import torch
    nx, nu, uprev, hidden, B = H.CASES["a"]
    Wk, d, rows = _case("a")
    steps = 5
    r64, m64, s64 = _adam_run(Wk, uprev, d, rows, steps, torch.float64)
    r32, m32, s32 = _adam_run(Wk, uprev, d, rows, steps, torch.float32)
    assert len(s64) == steps and all(np.array_equal(a, b) for a, b in zip(s32, s64))
    print(f"[trajectory] smallest kink margin on the way {m64.min():.2e} (f64) {m32.min():.2e} (f32)")
    tr = _trainer(Wk, nx, nu, uprev, d, B)
    try:
        for _ in range(steps):
            tr.step(rows)
        L, _ = tr.grad(rows)
        mse, tan = tr.last_losses()
    finally:
        tr.close()
    for what, got, i in (("L", L, 0), ("tan_mse", tan, 2)):
        e, e32 = abs(got - r64[i]) / r64[i], abs(r32[i] - r64[i]) / r64[i]
        print(f"[trajectory] {what} {r64[i]:.6e}: hip {e:.2e}, torch f32 {e32:.2e}, bar {8 * e32:.2e}")
        assert e <= 8 * e32, (what, e, e32)
    assert L < H.ref_loss_grad(Wk, uprev, d, rows, W)[0]                     # and it went down


def test_a_nan_tangent_is_not_hidden():
    nx, nu, uprev, hidden, B = H.CASES["a"]
    Wk, d, rows = _case("a")
    bad = dict(d, dx=d["dx"].copy())
    bad["dx"][rows[3], 1] = np.nan
    tr = _trainer(Wk, nx, nu, uprev, bad, B)
    try:
        L, _ = tr.grad(rows[:16])                                            # not an error
        mse, tan = tr.last_losses()
        assert np.isnan(L) and np.isnan(tan) and np.isfinite(mse)
        assert np.isfinite(tr.grad(rows[4:20])[0])                           # the other rows are unaffected
        tr.grad(rows[:16])
        L2, g2 = tr.grad(rows[4:6])                                          # the NaN row's place is padding now: rewritten to zero,
        assert np.isfinite(L2) and all(np.isfinite(a).all() for a in g2)     # or 0 * NaN would reach the weight gradient
        assert np.isnan(tr.step(rows[:16]))
    finally:
        tr.close()


def _einval(fn, who):
    from industrial_nnmpc_2021_amd import _lib
    with pytest.raises(_lib.NnmpcError) as ei:
        fn()
    assert re.search(r"\(code -1\): \S", str(ei.value)) and who in str(ei.value), str(ei.value)


def test_error_paths_launch_nothing():
    from industrial_nnmpc_2021_amd.train import HipTrainer
    nx, nu, uprev, hidden, B = H.CASES["a"]
    Wk, d, rows = _case("a")
    n = d["x"].shape[0]
    plain = P._trainer(Wk, nx, nu, uprev, d, B)
    try:
        _einval(lambda: plain.set_tangents(d), "nnmpc_train_set_tangents")                   # a plain handle
        _einval(lambda: plain.set_tan_weight(0.5), "nnmpc_train_set_tan_weight")
        assert np.isfinite(plain.grad(rows)[0])
    finally:
        plain.close()
    tr = HipTrainer(Wk, nx, nu, nnwithuprev=uprev, max_batch=B, lr=LR, betas=(B1, B2), eps=EPS, tangents=True)
    try:
        _einval(lambda: tr.set_tangents(d), "nnmpc_train_set_tangents")                      # before set_data
        _einval(lambda: tr.last_losses(), "nnmpc_train_last_losses")
        tr.set_data(d)
        _einval(lambda: tr.set_tangents({k: v[:n - 1] for k, v in d.items()}), "nnmpc_train_set_tangents")     # a wrong n
        _einval(lambda: tr.set_tangents({k: v for k, v in d.items() if k != "duprev"}), "nnmpc_train_set_tangents")
        for w in (-0.5, float("nan"), float("inf")):
            _einval(lambda: tr.set_tan_weight(w), "nnmpc_train_set_tan_weight")
        before = _bytes(tr.get_weights())
        l0 = tr.grad(rows)[0]                                                                # w is still 0: the plain step
        tr.set_tan_weight(W)

        def refused():                                                                       # w > 0 and no tangents
            _einval(lambda: tr.grad(rows), "nnmpc_train_grad")
            _einval(lambda: tr.step(rows), "nnmpc_train_step")
            _einval(lambda: tr.epoch(rows, 64), "nnmpc_train_epoch")
            _einval(lambda: tr.eval(0, 16), "nnmpc_train_eval")
            assert _bytes(tr.get_weights()) == before and tr.last_losses() == (l0, 0.0)      # nothing ran: the loss words are grad's

        refused()
        tr.set_tangents(d)
        assert tr.grad(rows)[0] > l0
        tr.set_data(d)                                                                       # drops the tangents
        tr.set_tan_weight(0.0)
        l0 = tr.grad(rows)[0]
        tr.set_tan_weight(W)
        refused()
    finally:
        tr.close()


def test_device_resident_tangents_give_the_same_bytes():
    from industrial_nnmpc_2021_amd import _lib
    nx, nu, uprev, hidden, B = H.CASES["c"]
    Wk, d, rows = _case("c")
    a, b = _trainer(Wk, nx, nu, uprev, d, B), None
    bufs = {k: _lib.DeviceArray.from_host(np.ascontiguousarray(d[k], np.float64)) for k in ("dx", "duprev", "du")}
    try:
        from industrial_nnmpc_2021_amd.train import HipTrainer
        b = HipTrainer(Wk, nx, nu, nnwithuprev=uprev, max_batch=B, lr=LR, betas=(B1, B2), eps=EPS, tangents=True)
        b.set_data(d)
        b.set_tangents_device(d["x"].shape[0], bufs["dx"], bufs["duprev"], bufs["du"])
        b.set_tan_weight(W)
        la, ga = a.grad(rows)
        lb, gb = b.grad(rows)
        assert la == lb and _bytes(ga) == _bytes(gb) and a.last_losses() == b.last_losses()
    finally:
        a.close()
        if b is not None:
            b.close()
        for v in bufs.values():
            v.free()


def test_tangent_data_on_a_golden_plant(golden_dir):
    """64 seeded rows around the stable golden plant: du is, bit for bit, sensitivity_batch(first_move_only=True) of the same
    solve along [dx * xscale; duprev]; rows without a certified slope are zero in direction and target."""
    import os
    from industrial_nnmpc_2021_amd.train import tangent_data
    from tests import mult_helpers as M
    g = np.load(os.path.join(golden_dir, "regulator_stable_s1.npz"))
    reg = M.golden_regulator(g, max_batch=128)
    try:
        nx, nu = g["A"].shape[0], g["B"].shape[1]
        rng = np.random.default_rng(64)
        ulb, uub = g["ulb"].ravel(), g["uub"].ravel()
        us = ulb + (uub - ulb) * rng.uniform(0.3, 0.7, (64, nu))
        xs = 0.1 * rng.standard_normal((64, nx))
        raw = dict(x=xs + 2.0 * rng.standard_normal((64, nx)), uprev=us + 0.1 * (uub - ulb) * rng.standard_normal((64, nu)), xs=xs, us=us)
        xscale = rng.uniform(0.5, 2.0, nx)
        td = tangent_data(reg, raw, xscale, ulb=ulb, uub=uub, seed=3)
        _, info = reg.solve_batch(np.hstack((raw["x"] - xs, raw["uprev"] - us)), ulb - us, uub - us, first_move_only=True)
        out = reg.sensitivity_batch(info, np.hstack((td["dx"] * xscale, td["duprev"])), first_move_only=True)
        ok = (out["flag"] == 0) & (info["status"] == 0)
        print(f"[golden] {int(ok.sum())} of 64 rows carry a slope, {int(info['active'].any(axis=1).sum())} with active bounds")
        assert np.array_equal(td["flag"], out["flag"]) and ok.sum() >= 32
        assert np.array_equal(td["du"][ok], out["du"][ok]) and np.abs(td["du"][ok]).max() > 0
        assert np.abs(td["dx"][ok]).min() > 0 and np.abs(td["duprev"][ok]).min() > 0
        for k in ("dx", "duprev", "du"):
            assert (td[k][~ok] == 0.0).all(), k
    finally:
        reg._solver().close()
