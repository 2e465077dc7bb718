"""The inputs and evaluators of the sensitivity tests (tests/sens_helpers.py), held to the conditions the GPU tests rest on -- no
device needed.

1. The case tables produce exactly the set sizes they claim, on both sides of the LDS / slab hand-over (160 | 161) and of the
   ceiling (768 | 784), with sets confined to the first stage, sets that include the last variable and mixed sides.
2. The exact cases are exact: P = diag(4^e) with its exact inverse pair, integer perturbations; every expected value is a dyadic
   number far below 2^53, and the expected du satisfies the definition with no rounding at all.
3. sens_route_f64 (the library's route through Hinv and Kunc) agrees with an independent np.linalg.solve on P_FF: the residual of
   either on the free rows is within 1e-9 scale, and so is P times their difference.
4. The longdouble evaluator flags a deliberately wrong du: one active row shifted, one side flipped, one free entry perturbed by 1e-6.
5. The golden conditions the solve test rests on: every problem of the four golden plants is strictly complementary -- smallest
   active multiplier >= 0.04, smallest slack of a non-active row >= 0.004 (measured: 0.047 and 0.0045 over the 24 problems) -- and the
   step of the extrapolation test is positive for every one of them.
"""
import os

import numpy as np
import pytest

from tests import mult_helpers as M
from tests import sens_helpers as S


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: "n%d_nu%d_aug%d" % s)
def test_family_table_has_the_sizes_it_claims(shape):
    n, nu, n_aug = shape
    rng = np.random.default_rng(1)
    fams = S.families(n, nu)
    assert len(set(fams)) == len(fams)
    for name, m in fams:
        rows = S.family_rows(name, m, n, nu, rng)
        words = M.pack_rows(rows[None, :], n)
        s = M.sides(words, n, nu)[0]
        assert (s < 3).all()
        assert (s > 0).sum() == m == S.set_size(words, n, nu)[0], (name, m)
        v = np.flatnonzero(s)
        if name == "first_stage":
            assert v.max() < nu
        if name in ("tail", "spread") and m > 1:
            assert v[-1] == n - 1
        if name == "head":
            assert np.array_equal(v, np.arange(m))
        if m >= 15 and name != "all_alternating":
            assert (s[v] == 1).any() and (s[v] == 2).any()                   # sides mixed
    sizes = {m for _, m in fams}
    assert sizes >= {m for m in S.SET_SIZES if m < n} | {n}
    if n > S.M_OVER:
        assert S.M_OVER in sizes and S.M_MAX in sizes and S.M_LDS in sizes and S.M_LDS + 1 in sizes
    # a batch of 129 holds every family of the shape, whatever D
    for D in S.DIRECTIONS:
        assert {fams[(b + 7 * D + 129) % len(fams)] for b in range(129)} == set(fams)


def test_real_case_table_covers_every_set_size():
    table = S.real_case_table()
    assert [m for m, _ in table[:len(S.SET_SIZES)]] == S.SET_SIZES
    for m, shape in table:
        n, nu, n_aug = shape
        assert m < n
        c = S.real_case(m, shape)
        assert (S.set_size(c["words"], n, nu) == m).all() and c["words"].shape[0] == S.REAL_B and c["dx0"].shape[1] == S.REAL_D
        s = M.sides(c["words"], n, nu)
        assert (s < 3).all()
        if m:
            assert (s[3][s[3] > 0] == 1).all() and (s[4][s[4] > 0] == 2).all()
            assert s[1, n - 1] > 0 and (s[2, n - 1] > 0 or m == 1)               # the last variable
    assert any(m == S.M_LDS + 1 and sh == S.SHAPES[-1] for m, sh in table)


@pytest.mark.parametrize("shape", [S.SHAPES[1], S.SHAPES[4], S.SHAPES[6]], ids=lambda s: "n%d" % s[0])
def test_exact_cases_are_exact(shape):
    n, nu, n_aug = shape
    mats = S.exact_matrices(n, nu, n_aug)
    d = np.diag(mats["P"])
    assert set(np.unique(d)) <= {1, 4, 16} and np.array_equal(mats["P"], np.diag(d))
    assert np.array_equal(mats["Hinv"] @ mats["P"], np.eye(n))               # the exact inverse
    assert np.array_equal(mats["P"] @ mats["Kunc"], -mats["tq"].astype(float))
    for B, D in ((5, 3), (129, 9)):
        c = S.exact_case(n, nu, n_aug, B, D)
        ok = c["flag"] == 0
        assert np.array_equal(c["flag"] == 1, S.set_size(c["words"], n, nu) > S.M_MAX)
        if n > S.M_OVER and B == 129:
            assert (c["flag"] == 1).sum() >= 2                               # 784 bounds, and all 1028
        for k in ("dx0", "dlb", "dub"):
            assert np.abs(c[k]).max() <= 16 and np.array_equal(c[k], np.round(c[k]))
        du, dm = c["du"][ok], c["dmult"][ok]
        assert np.array_equal(du * 16, np.round(du * 16)) and np.abs(du).max() <= 256 * n_aug     # dyadic, small
        assert np.array_equal(dm * 16, np.round(dm * 16)) and np.abs(dm).max() < 2.0 ** 20
        # the definition, with no rounding anywhere: P du + tq dx0 = 0 on the free rows, = -/+ dmult on the active ones
        g = du @ mats["P"].T.astype(float) + c["dx0"][ok] @ mats["tq"].T.astype(float)
        s = np.broadcast_to(M.sides(c["words"], n, nu)[ok][:, None, :], g.shape)
        assert (g[s == 0] == 0).all() and (dm[s == 0] == 0).all()
        assert np.array_equal(dm[s == 1], -g[s == 1]) and np.array_equal(dm[s == 2], g[s == 2])
        pert = S.tile_pert(c["dlb"], c["dub"], c["words"], n, nu)[ok]
        assert np.array_equal(du[s > 0], pert[s > 0])
        assert np.isnan(c["du"][~ok]).all() and np.isnan(c["dmult"][~ok]).all()
        assert S.SENTINEL * 16 != np.round(S.SENTINEL * 16) and S.SENTINEL != 0.0   # no value of a case: they are sixteenths
        # ... and the library's route in float64 reproduces it exactly on this data
        route = S.sens_route_f64(mats["Hinv"], mats["Kunc"], c["words"][ok], c["dx0"][ok], c["dlb"][ok], c["dub"][ok], nu)
        assert np.array_equal(route, du)


@pytest.mark.parametrize("m,shape", S.real_case_table(), ids=lambda v: str(v) if isinstance(v, int) else "n%d" % v[0])
def test_route_agrees_with_direct_solve(m, shape):
    n, nu, n_aug = shape
    mats = S.real_matrices(*shape)
    if m == 0:
        ev = np.linalg.eigvalsh(mats["P"])
        assert 0.9e3 < ev[-1] / ev[0] < 1.1e3                                # cond ~ 1e3
        assert np.abs(mats["P"] @ mats["Hinv"] - np.eye(n)).max() < 1e-10
    c = S.real_case(m, shape)
    route = S.sens_route_f64(mats["Hinv"], mats["Kunc"], c["words"], c["dx0"], c["dlb"], c["dub"], nu)
    direct = S.direct_f64(mats["P"], mats["tq"], c["words"], c["dx0"], c["dlb"], c["dub"], nu)
    free = np.broadcast_to((M.sides(c["words"], n, nu) == 0)[:, None, :], route.shape)
    sc = S.scale(mats["P"], mats["tq"], c["dx0"], direct)
    for name, du in (("route", route), ("direct", direct)):
        r = np.abs(S.free_residual(mats["P"], mats["tq"], c["dx0"], du))
        print(f"m {m} n {n} {name}: max free residual / scale = {float((r[free] / sc[free]).max()):.3g}")
        assert (r[free] <= 1e-9 * sc[free]).all()
    diff = np.abs((route - direct).astype(np.longdouble) @ mats["P"].astype(np.longdouble).T)
    assert (diff[free] <= 1e-9 * sc[free]).all()
    assert np.array_equal(route[~free], direct[~free])                      # the copied perturbations
    assert np.abs(route - direct).max() <= 1e-9 * max(1.0, np.abs(direct).max())


def test_longdouble_evaluator_flags_wrong_results():
    shape = S.SHAPES[4]
    n, nu, n_aug = shape
    mats = S.real_matrices(*shape)
    c = S.real_case(63, shape)
    du = S.sens_route_f64(mats["Hinv"], mats["Kunc"], c["words"], c["dx0"], c["dlb"], c["dub"], nu)
    P, tq = mats["P"], mats["tq"]
    good = S.free_ratio(P, tq, c["words"], c["dx0"], du, nu)
    tol = max(8 * good, S.FLOOR * (n + n_aug))
    assert good < 1e-12 and good <= tol
    s = M.sides(c["words"], n, nu)
    b = 2
    act, free = np.flatnonzero(s[b] > 0), np.flatnonzero(s[b] == 0)
    # one active row shifted: the free rows no longer balance
    bad = du.copy()
    bad[b, :, act[5]] += 1.0
    assert S.free_ratio(P, tq, c["words"], c["dx0"], bad, nu) > 1e3 * tol
    # one side flipped: the copied value is the other bound's
    pert = S.tile_pert(c["dlb"], c["dub"], c["words"], n, nu)
    flipped = S.tile_pert(c["dub"], c["dlb"], c["words"], n, nu)
    assert not np.array_equal(pert[b][:, act[3]], flipped[b][:, act[3]])
    bad = du.copy()
    bad[b, :, act[3]] = flipped[b][:, act[3]]
    assert not np.array_equal(bad[s[:, None, :].repeat(S.REAL_D, 1) > 0], pert[~np.isnan(pert)])
    assert S.free_ratio(P, tq, c["words"], c["dx0"], bad, nu) > 1e3 * tol
    # one free entry perturbed by 1e-6
    bad = du.copy()
    bad[b, 4, free[7]] += 1e-6
    assert S.free_ratio(P, tq, c["words"], c["dx0"], bad, nu) > 1e3 * tol


def golden_problem(golden_dir, case):
    g, e = _load(golden_dir, f"regulator_{case}.npz"), _load(golden_dir, f"qp_exact_{case}.npz")
    reg = M.golden_regulator(g)
    Pb, tqb = reg._box_form()
    Pb = np.tril(Pb) + np.tril(Pb, -1).T
    X0, lb, ub = M.golden_box_inputs(g)
    w = M.sequence_of_v(reg, e["v"], X0)
    return g, e, reg, Pb, tqb, X0, lb, ub, w


@pytest.mark.parametrize("case", M.GOLDEN_CASES)
def test_golden_problems_are_strictly_complementary(golden_dir, case):
    g, e, reg, Pb, tqb, X0, lb, ub, w = golden_problem(golden_dir, case)
    n, nu = Pb.shape[0], reg.Nu
    words = M.pack_rows(e["active"], n)
    s = M.sides(words, n, nu)
    mult = M.mult_ref(Pb, tqb, X0, w, words, nu, dtype=np.float64)
    c = np.arange(n) % nu
    slack = np.minimum(ub[:, c] - w, w - lb[:, c])
    # a variable at one bound: its other row is non-active too (slack ub - lb); every non-active row counts
    other = (ub - lb)[:, c]
    min_mult = mult[s > 0].min()
    min_slack = min(slack[s == 0].min(), other[s > 0].min())
    print(case, "min active multiplier", float(min_mult), "min slack of a non-active row", float(min_slack), "problems", X0.shape[0])
    assert X0.shape[0] == 6 and (s > 0).any()
    assert min_mult >= 0.04 and min_slack >= 0.004
    dX0, dlb, dub = S.golden_directions(case, X0.shape[0], X0.shape[1], nu)
    tau, du, dmult, _ = S.golden_step(Pb, tqb, nu, X0, lb, ub, w, e["active"], dX0, dlb, dub)
    print(case, "tau", tau)
    assert (tau > 0).all() and np.isfinite(tau).all()
