"""The inputs of tests/test_pdip_factor_gpu.py and tests/test_pdip_paths_gpu.py, held to their conditions on the CPU.

  * pdip_unit_spd: eigenvalue extremes 1 and 1e2 exactly before the rescaling, a unit diagonal after it, and a condition number
    that the rescaling leaves within a factor 2 of 1e2 (50 .. 150 asserted; for a 2 x 2 matrix the unit-diagonal scaling is the
    optimal one, so it can only lower it); every tile couples with every other (no off-diagonal tile is small);
  * pdip_factor_case: the f32-rounded K of every row is positive definite with a smallest eigenvalue >= 1e-7 |K|max -- the f32
    factorisation of the kernels and of the LAPACK yardstick cannot meet a non-positive pivot --, the masks are what the docstring
    says, and pdip_pivot_rows puts a negative diagonal entry where it says;
  * pdip_family: cond(P) = 1e3, every row's optimal set holds 10 - 50 % of the variables (row 1: the empty set), the flipped
    guesses differ from the oracle's set in 10 % of the variables, and the oracle's answers pass the independent fp64 KKT check
    the GPU tests of the large sets use as their referee.
"""
import numpy as np
import pytest

from tests import helpers as H

SIZES = sorted({n for n, _ in H.PDIP_FACTOR_SHAPES})


@pytest.mark.parametrize("n", SIZES)
def test_factor_hessian_has_the_stated_cond_and_a_unit_diagonal(n):
    P, P0 = H.pdip_unit_spd(n, 7000 + n)
    ev0, ev = np.linalg.eigvalsh(P0), np.linalg.eigvalsh(P)
    assert abs(ev0[-1] / ev0[0] / H.PDIP_FACTOR_COND - 1.0) < 1e-9
    assert (np.diag(P) == 1.0).all() and (P == P.T).all()
    assert 0.5 * H.PDIP_FACTOR_COND <= ev[-1] / ev[0] <= 1.5 * H.PDIP_FACTOR_COND, ev[-1] / ev[0]
    assert np.array_equal(H.pdip_factor_case(n)["P"], P)
    # the library's normalisation (upper median of the diagonal) is exactly 1
    assert np.sort(np.diag(P))[n // 2] == 1.0
    for i in range(0, n, 64):                                  # dense coupling: every 64 x 64 tile carries entries of the typical size
        for j in range(0, i, 64):
            assert np.abs(P[i:i + 64, j:j + 64]).max() >= 1.0 / np.sqrt(n), (i, j)


@pytest.mark.parametrize("n", SIZES)
def test_factor_rows_are_positive_definite_in_f32(n):
    c = H.pdip_factor_case(n)
    dvec, mask = c["dvec"], c["mask"]
    assert dvec.dtype == np.float32 and mask.dtype == np.float32 and c["rhs"].dtype == np.float32
    assert (dvec[0] == 0).all() and (mask[:3] == 1).all() and (dvec[1] == np.float32(1e-6)).all()
    assert dvec[2].min() >= np.float32(np.exp(-3.0)) * (1 - 1e-6) and dvec[2].max() <= np.float32(np.exp(3.0)) * (1 + 1e-6)
    for b in (3, 4, 5):
        assert np.array_equal(dvec[b], np.where(mask[b] == 0, np.float32(1.0), np.float32(1e-6)))
    assert int((mask[4] == 1).sum()) == min(3, n)
    if n >= 128:
        assert np.array_equal(mask[5] == 0, np.arange(n) // 64 == 1)
    if n >= 31:
        assert 0.1 * n <= (mask[3] == 0).sum() <= 0.5 * n
    for b in range(H.PDIP_FACTOR_ROWS):
        K32 = H.pdip_K(c["P"], dvec[b], mask[b]).astype(np.float32).astype(np.float64)
        assert np.linalg.eigvalsh(K32)[0] >= 1e-7 * np.abs(K32).max(), (n, b)
    dv2, mk2, _ = H.pdip_second_call(c)
    assert not np.array_equal(dv2, dvec) and not np.array_equal(mk2, mask)
    for b in range(H.PDIP_FACTOR_ROWS):
        K32 = H.pdip_K(c["P"], dv2[b], mk2[b]).astype(np.float32).astype(np.float64)
        assert np.linalg.eigvalsh(K32)[0] >= 1e-7 * np.abs(K32).max(), (n, b)


def test_pivot_rows_are_negative_where_intended():
    n, nb = H.PDIP_PIVOT_SHAPE
    c = H.pdip_factor_case(n)
    assert [a // nb for a in H.PDIP_PIVOT_AT] == [0, 0, 1] and [a % nb // 32 for a in H.PDIP_PIVOT_AT[:2]] == [0, 1]
    for at in H.PDIP_PIVOT_AT:
        dvec, mask = H.pdip_pivot_rows(c, at)
        good = np.arange(H.PDIP_FACTOR_ROWS) != H.PDIP_PIVOT_ROW
        assert np.array_equal(dvec[good], c["dvec"][good]) and np.array_equal(mask[good], c["mask"][good])
        K = H.pdip_K(c["P"], dvec[H.PDIP_PIVOT_ROW], mask[H.PDIP_PIVOT_ROW])
        d = np.diag(K)
        assert d[at] == -2.0 and (np.delete(d, at) == 1.0).all()
        assert np.linalg.eigvalsh(K)[0] < -1.0                 # ... so no pivot order could factor it


@pytest.fixture(scope="module")
def fam():
    f = H.pdip_family()
    f["U"], f["act"] = H.pdip_family_oracle(f)
    return f


def test_family_shares_and_conditioning(fam):
    ev = np.linalg.eigvalsh(fam["P"])
    assert 0.5 * fam["cond"] <= ev[-1] / ev[0] <= fam["cond"]
    assert (fam["n"], fam["nu"], fam["N"], fam["x0"].shape[0]) == (130, 2, 65, 24)
    share = fam["act"].sum(axis=1) / fam["n"]
    assert share[1] == 0 and (fam["x0"][1] == 0).all()
    rest = np.delete(share, 1)
    assert (rest >= 0.10).all() and (rest <= 0.50).all(), np.round(share, 2)


def test_family_oracle_passes_the_independent_kkt_check(fam):
    H.kkt_check(fam["P"], fam["tq"], fam["nu"], fam["N"], fam["x0"], fam["lb"], fam["ub"], dict(u=fam["U"], active=fam["act"]), 1e-9)


def test_flipped_guesses_differ_from_the_oracles_set(fam):
    state = H.active_to_state(fam["act"], fam["nu"])
    g = H.pdip_flipped_guess(state)
    assert ((g != state).sum(axis=1) == fam["n"] // 10).all()
    assert g.max() <= 2
    assert np.array_equal(g, H.pdip_flipped_guess(state))      # a function of the seed alone


def test_indefinite_hessian_has_a_positive_diagonal_and_no_factor():
    P = H.pdip_indefinite()
    ev = np.linalg.eigvalsh(P)
    assert (np.diag(P) == 1.0).all() and ev[0] < -0.5 and (ev[1:] > 0).all()
