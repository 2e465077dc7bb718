"""nnmpc_qp_sensitivity behind real solves: DenseQPRegulator.sensitivity_batch and BatchedBoxQP.sensitivity.

Per-row step, exactness of the extrapolation (the four golden plants, both re-parameterisations): solve_batch with multipliers,
sensitivity_batch with seeded directions in x0 and in both bounds, and per row a step tau = half the largest step that keeps
u + tau du inside the bounds on the non-active rows and mult + tau dmult >= 0, taken from the float64 route on the CPU
(tests/test_cpu_sens_inputs.py: the 24 problems are strictly complementary, tau > 0 for every one).  Inside the critical region the
law is affine, so the GPU solve of the perturbed problem must return the same active set and
    |u(x0 + tau dx0, ...) - (u + tau du)| <= 1e-9 max(1, |u|_inf)             (1e-9 = bound_tol, the slack a certified solve carries),
and its multipliers must agree with mult + tau dmult within the dot-product bounds of the three evaluations (mult_bound of the base
point, of the perturbed point and tau times that of the direction) plus |P_i|_1 times the distance just measured -- mult is linear
in u.  In the reference's variables v the extrapolated point (v', z + tau dz) satisfies the reference's own stationarity
P v' + q' + G'z' = 0 with the perturbed q: the box residual is bounded row by row by those dot-product bounds plus |P_i|_1 times the
distance of u from the golden optimum and tau |P_i|_1 times the distance of du from the float64 route, and the reference's residual
is Mg' times the box residual.

Derivative, not only the point: on the synthetic CSTRs-size plant (n = 540) with sets of 20 to 60 bounds, eight directions per
problem, du against central differences of two GPU solves per direction at a step of 1e-4 of the region radius: 1e-7 |du|_inf.
"""
import os

import numpy as np
import pytest

from tests import mult_helpers as M
from tests import sens_helpers as S

pytestmark = pytest.mark.gpu

_RUNS = {}


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def golden_run(golden_dir, case):
    """Base solve, sensitivities, the step and the perturbed solve of one golden plant; shared by the tests."""
    if case not in _RUNS:
        g, e = _load(golden_dir, f"regulator_{case}.npz"), _load(golden_dir, f"qp_exact_{case}.npz")
        reg = M.golden_regulator(g, max_batch=128)
        X0, lb, ub = M.golden_box_inputs(g)
        Pb, tqb = reg._box_form()
        Pb = np.tril(Pb) + np.tril(Pb, -1).T
        B, nu = X0.shape[0], reg.Nu
        U, info = reg.solve_batch(X0, ulb=lb, uub=ub, multipliers=True)
        dX0, dlb, dub = S.golden_directions(case, B, X0.shape[1], nu)
        out = reg.sensitivity_batch(info, dX0, dulb=dlb, duub=dub, multipliers=True)
        first = reg.sensitivity_batch(info, dX0, dulb=dlb, duub=dub, first_move_only=True)
        tau, du64, dmult64, mult64 = S.golden_step(Pb, tqb, nu, X0, lb, ub, U, info["active"], dX0, dlb, dub)
        t = tau[:, None]
        U2, info2 = reg.solve_batch(X0 + t * dX0, ulb=lb + t * dlb, uub=ub + t * dub, multipliers=True)
        _RUNS[case] = dict(g=g, e=e, reg=reg, X0=X0, lb=lb, ub=ub, Pb=Pb, tqb=tqb, U=U, info=info, dX0=dX0, dlb=dlb, dub=dub, out=out,
                           first=first, tau=tau, du64=du64, U2=U2, info2=info2)
        reg._solver().close()
    return _RUNS[case]


@pytest.mark.parametrize("case", M.GOLDEN_CASES)
def test_extrapolation_is_exact_inside_the_region(golden_dir, case):
    r = golden_run(golden_dir, case)
    info, out, tau, U = r["info"], r["out"], r["tau"], r["U"]
    B, n = U.shape
    assert B == 6 and (info["status"] == 0).all() and np.array_equal(info["active"], r["e"]["active"])
    assert out["du"].shape == (B, n) and out["dmult"].shape == (B, n) and out["dz"].shape == (B, 2 * n)     # one direction: no D axis
    assert (out["flag"] == 0).all()
    assert (tau > 0).all() and np.isfinite(tau).all()                           # every row: none is left out
    assert r["first"]["du"].shape == (B, r["reg"].Nu) and (r["first"]["flag"] == 0).all()
    t = tau[:, None]
    assert (r["info2"]["status"] == 0).all()
    assert np.array_equal(r["info2"]["active"], info["active"])                 # the same critical region
    want = U + t * out["du"]
    err = np.abs(r["U2"] - want).max(axis=1)
    lim = 1e-9 * np.maximum(1.0, np.abs(U).max(axis=1))
    print(case, "tau", tau, "\n max |u(perturbed) - (u + tau du)| / limit", err / lim, "max |du - float64 route|", float(np.abs(out["du"] - r["du64"]).max()))
    assert (err <= lim).all()


@pytest.mark.parametrize("case", M.GOLDEN_CASES)
def test_multipliers_extrapolate_too(golden_dir, case):
    r = golden_run(golden_dir, case)
    info, out, U, X0, Pb, tqb = r["info"], r["out"], r["U"], r["X0"], r["Pb"], r["tqb"]
    t = r["tau"][:, None]
    want = info["mult"] + t * out["dmult"]
    dw = np.abs(r["U2"] - (U + t * out["du"])).max(axis=1, keepdims=True)
    tol = (M.mult_bound(Pb, tqb, X0, U) + M.mult_bound(Pb, tqb, X0 + t * r["dX0"], r["U2"]) + t * M.mult_bound(Pb, tqb, r["dX0"], out["du"])
           + np.abs(Pb).sum(axis=1)[None, :].astype(np.longdouble) * dw)
    err = np.abs(r["info2"]["mult"].astype(np.longdouble) - want)
    act = M.sides(M.pack_rows(info["active"], Pb.shape[0]), Pb.shape[0], r["reg"].Nu) > 0
    print(case, "max |mult(perturbed) - (mult + tau dmult)| / tol on the active rows", float((err[act] / tol[act]).max()))
    assert (err <= tol).all()
    assert (want[act] >= -tol[act]).all()                                       # still dual feasible: tau is half the way out
    assert np.array_equal(out["dz"], M.z_rows(out["dmult"], info["active"], r["reg"].Nu))
    assert (out["dmult"][~act].view(np.uint64) == 0).all()


@pytest.mark.parametrize("case", M.GOLDEN_CASES)
def test_reference_stationarity_at_the_extrapolated_point(golden_dir, case):
    """In the reference's variables (both unstable plants are re-parameterised; the stable ones have Mg = I)."""
    from industrial_nnmpc_2021_amd import condense
    r = golden_run(golden_dir, case)
    g, e, reg, info, out, U, X0, Pb, tqb = r["g"], r["e"], r["reg"], r["info"], r["out"], r["U"], r["X0"], r["Pb"], r["tqb"]
    assert reg.reparameterize == case.startswith("unstable")
    t = r["tau"][:, None]
    X0p, Up = X0 + t * r["dX0"], U + t * out["du"]
    vp = M.v_of_sequence(reg, Up, X0p)
    zp = info["z"] + t * out["dz"]
    tq_ref = np.asarray(reg.tq)
    qp_ = g["q"][:, :, 0] + t * (r["dX0"] @ tq_ref.T)                           # the reference's q = tq x0 is linear in x0
    assert np.abs(g["q"][:, :, 0] - X0 @ tq_ref.T).max() <= 1e-9 * max(1.0, np.abs(g["q"]).max())
    res = M.reference_kkt(dict(P=g["P"], q=qp_[:, :, None], G=g["G"]), vp, zp)
    w_star = M.sequence_of_v(reg, e["v"], X0)
    p1 = np.abs(Pb).sum(axis=1)[None, :].astype(np.longdouble)
    tol_box = (M.mult_bound(Pb, tqb, X0, U) + t * M.mult_bound(Pb, tqb, r["dX0"], out["du"])
               + p1 * (np.abs(U - w_star).max(axis=1, keepdims=True) + t * np.abs(out["du"] - r["du64"]).max(axis=1, keepdims=True)))
    if reg.reparameterize:
        Mg, _ = condense.constraint_map(reg.A, reg.B, reg.Krep, reg.N)
        tol = tol_box @ np.abs(Mg).astype(np.longdouble)                        # residual in v = Mg' (residual in w)
    else:
        tol = tol_box
    print(case, "max |P v' + q' + G'z'| / tol", float((np.abs(res) / tol).max()))
    assert (np.abs(res) <= tol).all()
    # primal and dual feasibility of the extrapolated point with the perturbed h
    up, lo = M.row_index(U.shape[1], reg.Nu)
    c = np.arange(U.shape[1]) % reg.Nu
    ubp, lbp = (r["ub"] + t * r["dub"])[:, c], (r["lb"] + t * r["dlb"])[:, c]
    assert (Up <= ubp + 1e-9).all() and (Up >= lbp - 1e-9).all()


@pytest.fixture(scope="module")
def cstrs_size():
    from industrial_nnmpc_2021_amd import linearMPC as lm, synthetic
    pl = synthetic.plant("cstrs", 0)
    reg = lm.LinearMPCController.setup_regulator(pl["A"], pl["B"], pl["Q"], pl["R"], pl["S"], pl["N"], pl["ulb"], pl["uub"], max_batch=256)
    yield pl, reg
    reg._solver().close()


def test_du_is_the_derivative_central_differences(cstrs_size):
    pl, reg = cstrs_size
    from industrial_nnmpc_2021_amd import synthetic
    s = synthetic.samples(pl, 24, seed=21, sx=3.0)
    x0 = np.concatenate((s["x"] - s["xs"], s["uprev"] - s["us"]), axis=1)
    lb, ub = pl["ulb"].T - s["us"], pl["uub"].T - s["us"]
    qp = reg._solver()
    n, nu, n_aug = qp.n, qp.nu, qp.n_aug
    assert 300 <= n <= 600 and not reg.reparameterize
    base = qp.solve_batch(x0, lb, ub, multipliers=True)
    sizes = S.set_size(qp.active_to_words(base["active"]), n, nu)
    pick = np.flatnonzero((base["status"] == 0) & (sizes >= 20) & (sizes <= 60))[:8]
    print("set sizes of the batch", sizes.tolist(), "taken", pick.tolist())
    assert pick.size == 8
    x0, lb, ub, U, act = x0[pick], lb[pick], ub[pick], base["u"][pick], base["active"][pick]
    B, D = 8, 8
    rng = np.random.default_rng(77)
    dx0, dlb, dub = rng.standard_normal((B, D, n_aug)), 0.1 * rng.standard_normal((B, D, nu)), 0.1 * rng.standard_normal((B, D, nu))
    words = qp.active_to_words(act)
    out = qp.sensitivity(words, dx0, dlb=dlb, dub=dub, status=base["status"][pick], multipliers=True)
    assert (out["flag"] == 0).all() and out["du"].shape == (B, D, n)
    # the region radius of every (problem, direction): the smaller of the two ways out, from the float64 route
    Pb, tqb = reg._box_form()
    Pb = np.tril(Pb) + np.tril(Pb, -1).T
    radius = np.empty((B, D))
    for d in range(D):
        fwd = S.golden_step(Pb, tqb, nu, x0, lb, ub, U, act, dx0[:, d], dlb[:, d], dub[:, d])[0]
        bwd = S.golden_step(Pb, tqb, nu, x0, lb, ub, U, act, -dx0[:, d], -dlb[:, d], -dub[:, d])[0]
        radius[:, d] = 2 * np.minimum(fwd, bwd)
    assert (radius > 0).all() and np.isfinite(radius).all()
    h = 1e-4 * radius
    sgn = np.array([1.0, -1.0])[None, None, :, None]
    hh = h[:, :, None, None]
    rep = lambda a: np.broadcast_to(a[:, None, None, :], (B, D, 2, a.shape[1]))
    xs = (rep(x0) + sgn * hh * dx0[:, :, None, :]).reshape(B * D * 2, n_aug)
    lbs = (rep(lb) + sgn * hh * dlb[:, :, None, :]).reshape(B * D * 2, nu)
    ubs = (rep(ub) + sgn * hh * dub[:, :, None, :]).reshape(B * D * 2, nu)
    pert = qp.solve_batch(xs, lbs, ubs)
    assert (pert["status"] == 0).all()
    assert np.array_equal(pert["active"].reshape(B, D, 2, 2 * n), np.broadcast_to(act[:, None, None, :], (B, D, 2, 2 * n)))   # inside the region
    up = pert["u"].reshape(B, D, 2, n)
    quot = (up[:, :, 0] - up[:, :, 1]) / (2 * h[:, :, None])
    err = np.abs(quot - out["du"]).max(axis=2) / np.abs(out["du"]).max(axis=2)
    print("region radius", radius.min(), radius.max(), "\n max |central difference - du| / |du|_inf per (problem, direction)\n", err)
    assert (err <= 1e-7).all()
