"""The tangent loss without a device: the float64 reference of tests/tan_helpers.py against autograd (jvp of the project's
RegulatorModel, double backward through it, a central difference), train_nn_controller(backend="torch", tan_weight=...)
against that reference, train.tangent_data against a stub regulator, the exact case's inputs against their own condition,
and the four ABI names."""
import os
import re

import numpy as np
import pytest
import torch

from industrial_nnmpc_2021_amd import _lib
from industrial_nnmpc_2021_amd import train as T
from tests import tan_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["nnmpc_train_create_tan", "nnmpc_train_set_tangents", "nnmpc_train_set_tan_weight", "nnmpc_train_last_losses"]
W = H.W_TAN


def _model(Wk, nx, nu, uprev):
    m = T.RegulatorModel(nx, nu, [None] + [w.shape[1] for w in Wk[0:-1:2]] + [nu], nnwithuprev=uprev)
    m.set_weights(Wk)
    return m


def _keras_grads(m):
    g = []
    for lin in m.layers:
        g.append(lin.weight.grad.numpy().T.copy())
        if lin.bias is not None:
            g.append(lin.bias.grad.numpy().copy())
    return g


def _rel(a, ref):
    return np.abs(a - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize("name", ["a", "d"])
def test_reference_equals_autograd_through_the_models_jvp(name):
    """The explicit propagation IS the derivative of RegulatorModel along [dx, (duprev)]: tan_mse, L and every gradient
    tensor equal what torch gets from functional.jvp(create_graph=True) of the model and a backward pass through it."""
    nx, nu, uprev, hidden, B = H.CASES[name]
    Wk, d, rows = H.case(name)
    L, mse, tan, g = H.ref_loss_grad(Wk, uprev, d, rows, W)
    m = _model(Wk, nx, nu, uprev)
    t = lambda k: torch.as_tensor(d[k][rows], dtype=torch.float64)
    f = lambda x, up: m(x, up, t("xs"), t("us"))
    pred, jd = torch.autograd.functional.jvp(f, (t("x"), t("uprev")),
                                             (t("dx"), t("duprev") if uprev else torch.zeros_like(t("us"))), create_graph=True)
    mse_a, tan_a = torch.mean((pred - t("u")) ** 2), torch.mean((jd - t("du")) ** 2)
    (mse_a + W * tan_a).backward()
    print(f"[{name}] mse {abs(float(mse_a) - mse) / mse:.2e} tan_mse {abs(float(tan_a) - tan) / tan:.2e}")
    assert abs(float(mse_a) - mse) <= 1e-12 * mse and abs(float(tan_a) - tan) <= 1e-12 * tan
    assert abs(float(mse_a + W * tan_a) - L) <= 1e-12 * L
    for i, (a, r) in enumerate(zip(_keras_grads(m), g)):
        print(f"[{name}] tensor {i}: {_rel(a, r):.2e}")
        assert _rel(a, r) <= 1e-12
    # and the product's own torch loss is that propagation too
    Lp, mp, tp = T.tangent_loss(m, *(t(k) for k in ("x", "uprev", "xs", "us", "u", "dx", "duprev", "du")), W)
    assert abs(float(Lp) - L) <= 1e-12 * L and abs(float(mp) - mse) <= 1e-12 * mse and abs(float(tp) - tan) <= 1e-12 * tan


def test_reference_gradient_equals_a_central_difference():
    """On kink-free rows L is smooth around W: (L(W + hV) - L(W - hV)) / 2h against <g, V> to 1e-6 relative, float64."""
    nx, nu, uprev, hidden, B = H.CASES["d"]
    Wk, d, rows = H.case("d")
    rng = np.random.default_rng(5)
    V = [rng.standard_normal(w.shape) * np.abs(w).max() for w in Wk]
    _, _, _, g = H.ref_loss_grad(Wk, uprev, d, rows, W)
    want = sum(float((a * v).sum()) for a, v in zip(g, V))
    h = 1e-6
    Lp = H.ref_loss_grad([w + h * v for w, v in zip(Wk, V)], uprev, d, rows, W)[0]
    Lm = H.ref_loss_grad([w - h * v for w, v in zip(Wk, V)], uprev, d, rows, W)[0]
    got = (Lp - Lm) / (2 * h)
    print(f"[fd] <g, V> {want:.9e}, central difference {got:.9e}: {abs(got - want) / abs(want):.2e}")
    assert abs(got - want) <= 1e-6 * abs(want)


def _small():
    nx, nu, uprev, hidden, B = H.CASES["d"]
    Wk, d, rows = H.case("d")
    return nx, nu, Wk, {k: v[rows] for k, v in d.items()}


@pytest.mark.parametrize("uprev", [True, False])
def test_torch_backend_takes_the_references_adam_step(uprev):
    """One epoch of one full batch with tan_weight > 0: every tensor moved by Adam's first update of the reference's gradient."""
    nx, nu, hidden = 4, 2, [16, 24]
    rng = np.random.default_rng(3)
    Wk = H._weights(nx, nu, uprev, hidden, rng)
    d = H.add_tangents(H._kink_free(Wk, nx, nu, uprev, 48, rng), nx, nu, rng)
    n, lr = d["x"].shape[0], 1e-3
    _, _, _, g = H.ref_loss_grad(Wk, uprev, d, np.arange(n), W)
    data = dict(d) if uprev else {k: v for k, v in d.items() if k not in ("uprev", "duprev")}
    m, _, hist = T.train_nn_controller(_model(Wk, nx, nu, uprev), data, epochs=1, batch_size=n, validation_split=0.0, lr=lr,
                                       device="cpu", tan_weight=W)
    L = H.ref_loss_grad(Wk, uprev, d, np.arange(n), W)[0]
    assert abs(hist[0][0] - L) <= 1e-12 * L
    for w0, w1, gi in zip(Wk, m.get_weights(), g):
        ref = w0 - lr * gi / (np.abs(gi) + 1e-7)               # t = 1: m / (1 - b1) = g, sqrt(v / (1 - b2)) = |g|
        assert np.abs(w1 - ref).max() <= 1e-12 and np.abs(w1 - w0).max() > 0.1 * lr


def test_torch_backend_without_the_weight_is_todays_loop():
    """tan_weight = 0 (and the argument left out): the state dict of the plain loop -- written out here as it stood before
    the argument existed -- after two epochs from the same seed, bit for bit."""
    nx, nu, Wk, d = _small()
    n, bs, seed, lr = d["x"].shape[0], 48, 4, 1e-3
    ntr = n - int(n * 0.25)
    want = _model(Wk, nx, nu, False)
    torch.manual_seed(seed)
    t = {k: torch.as_tensor(d[k], dtype=torch.float64) for k in ("x", "xs", "us", "u")}
    up = torch.zeros_like(t["us"])
    opt = torch.optim.Adam(want.parameters(), lr=lr, eps=1e-7)
    best, best_state = float("inf"), None
    for _ in range(2):
        perm = torch.randperm(ntr)
        for i in range(0, ntr, bs):
            idx = perm[i:i + bs]
            loss = torch.mean((want(t["x"][idx], up[idx], t["xs"][idx], t["us"][idx]) - t["u"][idx]) ** 2)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        with torch.no_grad():
            vl = float(torch.mean((want(t["x"][ntr:], up[ntr:], t["xs"][ntr:], t["us"][ntr:]) - t["u"][ntr:]) ** 2))
        if vl < best:
            best, best_state = vl, {k: v.clone() for k, v in want.state_dict().items()}
    for kw in ({}, {"tan_weight": 0.0}):
        m, _, hist = T.train_nn_controller(_model(Wk, nx, nu, False), d, epochs=2, batch_size=bs, validation_split=0.25, lr=lr,
                                           device="cpu", seed=seed, **kw)
        assert min(h[1] for h in hist) == best
        for k, v in m.state_dict().items():
            assert torch.equal(v, best_state[k]), k


def test_tan_weight_arguments_are_checked_on_the_host():
    nx, nu, Wk, d = _small()
    plain = {k: v for k, v in d.items() if k not in ("dx", "duprev", "du")}
    for backend in ("torch", "hip"):
        with pytest.raises(ValueError, match="tangent_data"):
            T.train_nn_controller(_model(Wk, nx, nu, False), plain, epochs=1, tan_weight=0.5, backend=backend)
        with pytest.raises(ValueError, match="tan_weight"):
            T.train_nn_controller(_model(Wk, nx, nu, False), d, epochs=1, tan_weight=-1.0, backend=backend)
    um = T.UnstdRegulatorModel(nx, nu, [None, 8, nu], nnwithuprev=False)
    with pytest.raises(ValueError, match="structured"):
        T.train_nn_controller(um, d, epochs=1, tan_weight=0.5)


class _StubRegulator:
    """u0 = K x0 everywhere; row ``flagged`` comes back with sensitivity flag 1, row ``failed`` with solve status 1."""

    def __init__(self, K, flagged, failed):
        self.K, self.flagged, self.failed, self.calls = K, flagged, failed, []

    def solve_batch(self, X0, ulb=None, uub=None, first_move_only=False, **kw):
        assert first_move_only
        self.calls.append((np.array(X0), np.array(ulb), np.array(uub)))
        st = np.zeros(X0.shape[0], np.int32)
        st[self.failed] = 1
        return X0 @ self.K.T, dict(status=st, active=np.zeros((X0.shape[0], 4), bool))

    def sensitivity_batch(self, info, dX0, first_move_only=False, **kw):
        assert first_move_only and dX0.ndim == 2
        self.dX0 = np.array(dX0)
        flag = np.zeros(dX0.shape[0], np.int32)
        flag[self.flagged] = 1
        return dict(du=dX0 @ self.K.T, flag=flag)


@pytest.mark.parametrize("uprev", [True, False])
def test_tangent_data_with_a_stub_regulator(uprev):
    rng = np.random.default_rng(9)
    n, nx, nu = 12, 4, 2
    K = rng.standard_normal((nu, nx + nu))
    raw = dict(x=rng.standard_normal((n, nx)), uprev=rng.standard_normal((n, nu)), xs=rng.standard_normal((n, nx)),
               us=rng.uniform(-.5, .5, (n, nu)))
    xscale = rng.uniform(0.5, 3.0, nx)
    ulb, uub = -np.ones(nu), 2 * np.ones(nu)
    reg = _StubRegulator(K, flagged=3, failed=7)
    out = T.tangent_data(reg, raw, xscale, ulb=ulb, uub=uub, seed=2, nnwithuprev=uprev)
    X0, lb, ub = reg.calls[0]
    assert np.array_equal(X0, np.hstack((raw["x"] - raw["xs"], raw["uprev"] - raw["us"])))
    assert np.array_equal(lb, ulb - raw["us"]) and np.array_equal(ub, uub - raw["us"])
    assert out["dx"].shape == (n, nx) and out["duprev"].shape == (n, nu) and out["du"].shape == (n, nu)
    ok = np.ones(n, bool)
    ok[[3, 7]] = False
    assert out["flag"][3] == 1 and (out["flag"][ok] == 0).all()
    assert np.array_equal(out["du"][ok], (np.hstack((out["dx"] * xscale, out["duprev"])) @ K.T)[ok])
    assert np.abs(out["du"][ok]).min() > 0 and np.abs(out["dx"][ok]).min() > 0
    for k in ("dx", "duprev", "du"):
        assert (out[k][~ok] == 0.0).all(), k                    # flagged, or not solved: the row says nothing
    if uprev:
        assert np.abs(out["duprev"][ok]).min() > 0
    else:
        assert (out["duprev"] == 0.0).all() and (reg.dX0[:, nx:] == 0.0).all()
    again = T.tangent_data(_StubRegulator(K, 3, 7), raw, xscale, ulb=ulb, uub=uub, seed=2, nnwithuprev=uprev)
    assert all(np.array_equal(out[k], again[k]) for k in out)   # seeded


@pytest.mark.parametrize("name", sorted(H.EXACT))
def test_exact_case_meets_its_own_condition(name):
    """Every f32 quantity of the step is a whole count of UNIT and no absolute-value sum reaches 2^24 of it (int64), the
    float64 reference agrees with the int64 recomputation exactly, pre-activations of pass 1 are positive, zero and negative,
    pass 2 differs, and each wrong reference differs from the right one in tan_mse and in some gradient entry."""
    Wk, d, rows = H.exact_case(name)
    assert len(rows) == H.EX_B == 64 and d["us"].shape[1] == 2
    assert max(w.shape[-1] for w in Wk) == max(H.EXACT[name]) and (max(H.EXACT[name]) <= 64) == (name == "narrow")
    assert all(np.isin(w, (-1.0, 0.0, 1.0)).all() and (w == 0).mean() > 0.4 for w in Wk[0::2])
    L, mse, tan, g, peak = H.exact_int(Wk, d, rows)
    print(f"[exact {name}] L {L} mse {mse} tan_mse {tan}, peak {peak} = 2^{np.log2(peak):.1f} counts of 2^-8")
    assert peak < 2 ** 24
    assert all((a == np.asarray(a, np.float32)).all() for a in g)
    Lr, mr, tr_, gr = H.ref_loss_grad(Wk, True, d, rows, W)
    assert (Lr, mr, tr_) == (L, mse, tan) and tan > 0 and mse > 0
    assert all(np.array_equal(a, b) for a, b in zip(g, gr)) and all(np.abs(a).max() > 0 for a in g)
    z1, z2, _ = H.stack(d, rows, True)
    p1, p2 = z1 @ Wk[0] + Wk[1], z2 @ Wk[0] + Wk[1]
    r0 = int(np.flatnonzero(rows == 0)[0])
    assert (p1[r0, :6] == 0).all() and (p1 > 0).mean() > 0.1 and (p1 < 0).mean() > 0.1
    assert ((p1 > 0) != (p2 > 0)).mean() > 0.1
    for v in H.VARIANTS:
        Lv, mv, tv, gv, _ = H.exact_int(Wk, d, rows, variant=v)
        Lq, mq, tq, gq = H.ref_loss_grad(Wk, True, d, rows, W, variant=v)
        assert (Lv, mv, tv) == (Lq, mq, tq) and all(np.array_equal(a, b) for a, b in zip(gv, gq)), v
        assert tv != tan and mv == mse, v
        assert any(not np.array_equal(a, b) for a, b in zip(g, gv)), v


def test_the_four_names_are_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nnmpc.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", text), n
        assert n in _lib.EXPORTS and not n.startswith("nnmpc_train_group_")
        assert hasattr(_lib.load(), n), n


def test_create_tan_refuses_an_unstructured_form_without_a_device():
    """NNMPC_EINVAL with its message, checked before a device is looked for: the same on a machine without one."""
    rng = np.random.default_rng(0)
    Wu = [rng.standard_normal((10, 8)), np.zeros(8), rng.standard_normal((8, 2)), np.zeros(2)]
    for form in (_lib.NN_UNSTD, _lib.NN_UNSTD_RELU):
        with pytest.raises(_lib.NnmpcError) as ei:
            T.HipTrainer(Wu, 3, 2, nnwithuprev=True, max_batch=128, form=form, tangents=True)
        msg = str(ei.value)
        assert "(code -1)" in msg and "nnmpc_train_create_tan" in msg and "structured form only" in msg, msg
