"""The evaluators of the adjoint tests (tests/adj_helpers.py), held to the conditions the GPU tests rest on -- no device needed.

1. The adjoint identity <v, du> = <gx0, dx0> + <glb, dlb> + <gub, dub> of adjoint_route_f64 against sens_route_f64 (the forward's
   float64 route) on every entry of real_case_table(), sequence and first-move cotangents: the gap stays below 1e-12 of the sum of
   the absolute terms (measured: <= 3.0e-14).
2. exact_case_adj's expectations equal adjoint_route_f64 entry for entry, are sixteenths far below 2^53, and in first-move mode w
   is exactly zero behind the first stage.
3. Three float64 evaluation orders of the route (np.linalg.solve | Cholesky and two triangular solves | the same with the list
   reversed) stay within the GPU tests' tolerance of each other, measured against adjoint_ref_ld: each one's (e_x, e_w) is below
   the tolerance formed from the first one's.
4. adjoint_ref_ld's refinement has converged: its last correction is below 2^-60 of |y| (its residuals are exact beyond
   np.longdouble: adj_helpers.residual_exact).
5. Every family of sens_helpers.families appears in the exact batches of 129, whatever D.
"""
import numpy as np
import pytest

from tests import adj_helpers as A
from tests import mult_helpers as M
from tests import sens_helpers as S

_IDS = lambda v: str(v) if isinstance(v, int) else "n%d" % v[0]


@pytest.mark.parametrize("m,shape", S.real_case_table(), ids=_IDS)
def test_adjoint_identity_against_the_forward_route(m, shape):
    n, nu, n_aug = shape
    mats = S.real_matrices(*shape)
    c = S.real_case(m, shape)
    du = S.sens_route_f64(mats["Hinv"], mats["Kunc"], c["words"], c["dx0"], c["dlb"], c["dub"], nu)
    for first in (False, True):
        v = A.real_cotangents(m, shape, first)
        g = A.adjoint_route_f64(mats["Hinv"], mats["Kunc"], c["words"], v, nu)
        gap, scale = A.identity_gap(A.extend(v, n), du, g, c["dx0"], c["dlb"], c["dub"])
        print(f"m {m} n {n} first {first}: identity gap / scale = {float((gap / scale).max()):.3g}")
        assert (gap <= 1e-12 * scale).all()
        # gbound: zero off the set, and glb / gub are its column sums
        assert (g["gbound"][np.broadcast_to((M.sides(c["words"], n, nu) == 0)[:, None, :], g["gbound"].shape)] == 0).all()
        assert np.allclose(g["glb"].sum(axis=2) + g["gub"].sum(axis=2), g["gbound"].sum(axis=2), rtol=0, atol=1e-9 * (1 + np.abs(g["gbound"]).sum(axis=2).max()))


@pytest.mark.parametrize("shape", [S.SHAPES[1], S.SHAPES[4], S.SHAPES[6]], ids=lambda s: "n%d" % s[0])
def test_exact_expectations_equal_the_route(shape):
    n, nu, n_aug = shape
    for B, D in ((5, 3), (129, 9)):
        for first in (False, True):
            c = A.exact_case_adj(n, nu, n_aug, B, D, first)
            ok = c["flag"] == 0
            assert np.abs(c["v"]).max() <= 16 and np.array_equal(c["v"], np.round(c["v"]))
            g = A.adjoint_route_f64(c["mats"]["Hinv"], c["mats"]["Kunc"], c["words"][ok], c["v"][ok], nu)
            for k in ("gx0", "gbound", "glb", "gub"):
                assert np.array_equal(g[k], c[k][ok]), k
                assert np.array_equal(c[k][ok] * 16, np.round(c[k][ok] * 16)) and np.abs(c[k][ok]).max() < 2.0 ** 30
                assert np.isnan(c[k][~ok]).all()
            if first:
                assert (c["gbound"][ok][:, :, nu:] == 0).all()
            assert A.SENTINEL * 16 != np.round(A.SENTINEL * 16)


@pytest.mark.parametrize("m,shape", S.real_case_table(), ids=_IDS)
def test_evaluation_orders_and_converged_reference(m, shape):
    n, nu, n_aug = shape
    mats = S.real_matrices(*shape)
    c = S.real_case(m, shape)
    for first in (False, True):
        v = A.real_cotangents(m, shape, first)
        ref = A.real_reference(m, shape, first)
        vals = {}
        for order in A.ORDERS:
            g = A.adjoint_route_f64(mats["Hinv"], mats["Kunc"], c["words"], v, nu, order=order)
            vals[order] = A.errors(mats["Kunc"], c["words"], v, nu, g["gx0"], g["gbound"], ref)
        tol_x, tol_w = (A.tolerance(vals["solve"][i], n, n_aug) for i in (0, 1))
        print(f"m {m} n {n} first {first}: (e_x, e_w) " + ", ".join(f"{o} ({vals[o][0]:.3g}, {vals[o][1]:.3g})" for o in A.ORDERS)
              + f"  tol ({tol_x:.3g}, {tol_w:.3g})")
        for o in A.ORDERS:
            assert vals[o][0] <= tol_x and vals[o][1] <= tol_w, o


def test_reference_refinement_has_converged():
    """The last of the four corrections of adjoint_ref_ld, relative to max |y|, over real_case_table() and both modes: below 2^-60 =
    8.7e-19 (measured: at most 4.9e-20, the last bit of np.longdouble).  With residuals formed in np.longdouble alone the corrections
    stall at cond(P_FF) 2^-64 |y| -- 2.35e-17 at worst was measured, above the bound -- which is why residual_exact forms them from
    exact float64 products of 21-bit chunks."""
    worst = 0.0
    for m, shape in S.real_case_table():
        for first in (False, True):
            last = A.real_reference(m, shape, first)["last"]
            print(f"m {m} n {shape[0]} first {first}: last correction / max |y| = {last:.3g}")
            worst = max(worst, last)
    assert worst < 2.0 ** -60, worst


def test_every_family_appears_in_the_exact_batches():
    for shape in S.SHAPES:
        n, nu, n_aug = shape
        fams = set(S.families(n, nu))
        for D in S.DIRECTIONS:
            assert set(A.exact_case_adj(n, nu, n_aug, 129, D)["fam"]) == fams
