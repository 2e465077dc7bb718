"""nnmpc_qp_adjoint behind real solves: DenseQPRegulator.adjoint_batch, first_move_gain_batch and the torch wrapper
(industrial_nnmpc_2021_amd/torch_qp.py), on the 24 golden regulator problems tests/test_sens_solve_gpu.py uses (four plants, both
unstable ones re-parameterised).

The gain against the forward: K (B, Nu, n_aug) of first_move_gain_batch against sensitivity_batch(first_move_only=True) with the n_aug
unit directions of x0, Klb / Kub against the Nu unit directions of each bound -- entry (j, k) of a gain and entry j of the forward's
first move along direction k are the two sides of the adjoint identity with unit vectors, so they agree within tol x scale,
tol = max(8 x the identity's gap of the two float64 routes on the same problems, 64 2^-53 (n + n_aug)) and scale that of the sums
an entry is formed from (the scales of e_x and e_w of tests/adj_helpers.errors for the unit cotangent).

The torch wrapper: the autograd gradient of sum(c . u0) equals adjoint_batch with v = c bit for bit, and every coordinate of it
equals the central difference of two GPU solves at a step of 1e-4 of the region radius along that coordinate within 1e-7 |gradient|_inf
(step and bound of test_du_is_the_derivative_central_differences).  A problem whose set changes under a step is left out; at most a
quarter of the 24 may be.
"""
import os

import numpy as np
import pytest

from tests import adj_helpers as A
from tests import mult_helpers as M
from tests import sens_helpers as S

pytestmark = pytest.mark.gpu

_RUNS = {}


def golden_run(golden_dir, case):
    if case not in _RUNS:
        g = np.load(os.path.join(golden_dir, f"regulator_{case}.npz"))
        reg = M.golden_regulator(g, max_batch=128)
        X0, lb, ub = M.golden_box_inputs(g)
        Pb, tqb = reg._box_form()
        Pb = np.tril(Pb) + np.tril(Pb, -1).T
        U, info = reg.solve_batch(X0, ulb=lb, uub=ub)
        _RUNS[case] = dict(reg=reg, X0=X0, lb=lb, ub=ub, Pb=Pb, tqb=tqb, U=U, info=info)
    return _RUNS[case]


@pytest.fixture(scope="module", autouse=True)
def _close_solvers():
    yield
    for r in _RUNS.values():
        r["reg"]._solver().close()
    _RUNS.clear()


@pytest.mark.parametrize("case", M.GOLDEN_CASES)
def test_gain_equals_the_forward_with_unit_directions(golden_dir, case):
    r = golden_run(golden_dir, case)
    reg, info, Pb, tqb = r["reg"], r["info"], r["Pb"], r["tqb"]
    B, n = r["U"].shape
    nu, n_aug = reg.Nu, r["X0"].shape[1]
    assert reg.reparameterize == case.startswith("unstable") and (info["status"] == 0).all()
    K, Klb, Kub, flag = reg.first_move_gain_batch(info, bounds=True)
    assert K.shape == (B, nu, n_aug) and Klb.shape == Kub.shape == (B, nu, nu) and (flag == 0).all()
    assert np.array_equal(reg.first_move_gain_batch(info), K)
    eye = lambda k: np.ascontiguousarray(np.broadcast_to(np.eye(k), (B, k, k)))
    zx, zb = np.zeros((B, nu, n_aug)), np.zeros((B, nu, nu))
    fx = reg.sensitivity_batch(info, eye(n_aug), first_move_only=True)["du"]                        # (B, n_aug, nu)
    fl = reg.sensitivity_batch(info, zx, dulb=eye(nu), duub=zb, first_move_only=True)["du"]         # (B, nu, nu)
    fu = reg.sensitivity_batch(info, zx, dulb=zb, duub=eye(nu), first_move_only=True)["du"]
    # the tolerance: the identity's gap of the two float64 routes with one inverse pair, seeded cotangents and directions
    Hinv = np.linalg.inv(Pb)
    Hinv = 0.5 * (Hinv + Hinv.T)
    Kunc = -Hinv @ tqb
    words = M.pack_rows(info["active"], n)
    rng = np.random.default_rng(5)
    v, dx0, dlb, dub = rng.standard_normal((B, 4, n)), rng.standard_normal((B, 4, n_aug)), rng.standard_normal((B, 4, nu)), rng.standard_normal((B, 4, nu))
    gap, scale = A.identity_gap(v, S.sens_route_f64(Hinv, Kunc, words, dx0, dlb, dub, nu), A.adjoint_route_f64(Hinv, Kunc, words, v, nu), dx0, dlb, dub)
    tol = A.tolerance(float((gap / scale).max()), n, n_aug)
    # Scale: with unit vectors both sides of the identity are single entries, and an entry may be the small rest of a cancellation
    # (the gain row of a first-stage active input is Kunc_j - Kunc[A, :]' w with w = e_j: zero up to rounding, where the forward copies
    # an exact 0.0).  The rounding of an entry is relative to the terms of its sum: the scales of e_x and e_w (tests/adj_helpers.errors)
    # for the unit cotangent e_j, from the float64 route.
    unit = A.adjoint_route_f64(Hinv, Kunc, words, eye(nu), nu)
    mag = np.abs(A.extend(eye(nu), n)) + np.abs(unit["gbound"])                                    # (B, nu, n)
    sx = (mag @ np.abs(Kunc)).max(axis=2)[:, :, None]
    sw = (np.abs(unit["gbound"]).max(axis=2) + 1.0)[:, :, None]
    worst = 0.0
    for name, gain, fwd, sc in (("K", K, fx, sx), ("Klb", Klb, fl, sw), ("Kub", Kub, fu, sw)):
        diff = np.abs(gain - np.swapaxes(fwd, 1, 2))
        worst = max(worst, float((diff / sc).max()))
        assert (diff <= tol * sc).all(), name
    print(case, "n", n, "sets", S.set_size(words, n, nu).tolist(), "max |gain - forward| / scale", worst, "tol", tol,
          "float64 routes", float((gap / scale).max()))
    # the whole sequence: adjoint_batch against sensitivity_batch, the identity itself
    du = reg.sensitivity_batch(info, dx0, dulb=dlb, duub=dub)["du"]
    g = reg.adjoint_batch(info, v, bounds=True, per_variable=True)
    assert (g["flag"] == 0).all() and g["gbound"].shape == (B, 4, n)
    gap_g, scale_g = A.identity_gap(v, du, g, dx0, dlb, dub)
    assert (gap_g <= tol * scale_g).all()


@pytest.mark.parametrize("case", M.GOLDEN_CASES)
def test_torch_gradient_is_the_adjoint_and_the_derivative(golden_dir, case):
    import torch
    from industrial_nnmpc_2021_amd.torch_qp import first_move
    r = golden_run(golden_dir, case)
    reg, info, X0, lb, ub, Pb, tqb = r["reg"], r["info"], r["X0"], r["lb"], r["ub"], r["Pb"], r["tqb"]
    B, n = r["U"].shape
    nu, n_aug = reg.Nu, X0.shape[1]
    rng = np.random.default_rng(600 + M.GOLDEN_CASES.index(case))
    c = rng.standard_normal((B, nu))
    tx, tl, tu = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (X0, lb, ub))
    u0 = first_move(reg, tx, tl, tu)
    assert u0.shape == (B, nu) and np.array_equal(u0.detach().numpy(), r["U"][:, :nu])
    (torch.as_tensor(c) * u0).sum().backward()
    g = reg.adjoint_batch(info, c, first_move_only=True, bounds=True)
    assert (g["flag"] == 0).all()
    same = lambda t, a: t.shape == a.shape and t.numpy().tobytes() == np.ascontiguousarray(a).tobytes()
    assert same(tx.grad, g["gx0"]) and same(tl.grad, g["glb"]) and same(tu.grad, g["gub"])
    # central differences along every coordinate of (x0, lb, ub): two solves per coordinate, all problems in one batch
    K = n_aug + 2 * nu
    E = np.eye(K)
    grad = np.concatenate((g["gx0"], g["glb"], g["gub"]), axis=1)                                   # (B, K)
    radius = np.empty((B, K))
    for k in range(K):
        d = [np.broadcast_to(E[k, a:b], (B, b - a)) for a, b in ((0, n_aug), (n_aug, n_aug + nu), (n_aug + nu, K))]
        fwd = S.golden_step(Pb, tqb, nu, X0, lb, ub, r["U"], info["active"], d[0], d[1], d[2])[0]
        bwd = S.golden_step(Pb, tqb, nu, X0, lb, ub, r["U"], info["active"], -d[0], -d[1], -d[2])[0]
        radius[:, k] = np.minimum(2 * np.minimum(fwd, bwd), 1.0)                                    # (a coordinate that never leaves the region: 1)
    assert (radius > 0).all()
    h = 1e-4 * radius
    sgn = np.array([1.0, -1.0])[None, None, :, None]
    step = sgn * h[:, :, None, None] * E[None, :, None, :]                                          # (B, K, 2, K)
    base = np.concatenate((X0, lb, ub), axis=1)[:, None, None, :]
    pts = (base + step).reshape(B * K * 2, K)
    U2, info2 = reg.solve_batch(pts[:, :n_aug], ulb=pts[:, n_aug:n_aug + nu], uub=pts[:, n_aug + nu:], first_move_only=True)
    inside = (info2["status"].reshape(B, K * 2) == 0).all(axis=1) & \
        (info2["active"].reshape(B, K * 2, 2 * n) == info["active"][:, None, :]).all(axis=(1, 2))
    loss = (U2.reshape(B, K, 2, nu) * c[:, None, None, :]).sum(axis=3)
    quot = (loss[:, :, 0] - loss[:, :, 1]) / (2 * h)
    err = np.abs(quot - grad).max(axis=1) / np.abs(grad).max(axis=1)
    print(case, "problems left out (set changed under a step)", int((~inside).sum()), "of", B,
          "\n max |central difference - gradient| / |gradient|_inf per problem", err)
    assert (~inside).sum() <= B // 4
    assert (err[inside] <= 1e-7).all()


def test_flagged_rows_give_nan_gradients_for_that_row_only(golden_dir):
    import torch
    from industrial_nnmpc_2021_amd.torch_qp import first_move
    r = golden_run(golden_dir, M.GOLDEN_CASES[0])
    reg, X0, lb, ub = r["reg"], r["X0"].copy(), r["lb"], r["ub"]
    B, nu = X0.shape[0], reg.Nu
    clean = torch.tensor(X0, requires_grad=True)
    first_move(reg, clean, torch.tensor(lb), torch.tensor(ub)).sum().backward()
    X0[2, 0] = np.nan                                                           # not solved: status NNMPC_ST_NUMERIC, flag 2
    tx = torch.tensor(X0, requires_grad=True)
    tl = torch.tensor(lb, requires_grad=True)
    u0 = first_move(reg, tx, tl, torch.tensor(ub))
    assert torch.isnan(u0[2]).all()
    keep = [b for b in range(B) if b != 2]
    u0[keep].sum().backward()
    assert torch.isnan(tx.grad[2]).all() and torch.isnan(tl.grad[2]).all()
    assert tx.grad[keep].numpy().tobytes() == clean.grad[keep].numpy().tobytes()
    # bounds shared by the batch, float32 tensors: the gradient comes back in their shape and dtype
    tb = torch.tensor(reg.uub.reshape(1, -1), dtype=torch.float32, requires_grad=True)
    first_move(reg, torch.tensor(r["X0"], dtype=torch.float32), None, tb).sum().backward()
    assert tb.grad.shape == tb.shape and tb.grad.dtype == torch.float32 and torch.isfinite(tb.grad).all()
