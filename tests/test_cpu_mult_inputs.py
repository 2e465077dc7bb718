"""The inputs and the reference evaluator of the bound-multiplier tests (tests/mult_helpers.py), held to the conditions the GPU
tests rest on -- no device needed.

1. mult_ref is the definition: checked against a loop written from include/nnmpc.h, bit unpacking included.
2. On the committed goldens (regulator_<case>.npz / qp_exact_<case>.npz: stable and unstable, S = 0 and S != 0) the multipliers of
   the golden optimum and active set are >= 0 and satisfy P v* + q + G'z = 0 with the reference's own P, q, G, both up to the
   rounding bound of mult_bound, row by row: this pins the sign convention, and that the box problem of a re-parameterised
   plant hands out the z of the reference's G v <= h untransformed.
3. The integer table of the kernel test: every expected value is an int64 product whose partial sums stay below 2^53 in any
   order, so the fp64 kernel must reproduce it exactly.
4. The structural inputs of the solve test really are what they are called: no bound active / every variable held, and the
   oracle solves every one of them.
"""
import os

import numpy as np
import pytest

from tests import mult_helpers as M


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def test_evaluator_is_the_definition():
    rng = np.random.default_rng(5)
    n, nu, n_aug, B = 12, 3, 4, 7
    A = rng.standard_normal((n, n))
    P, tq = A @ A.T, rng.standard_normal((n, n_aug))
    x0, u = rng.standard_normal((B, n_aug)), rng.standard_normal((B, n))
    rows = rng.random((B, 2 * n)) < 0.3
    up, lo = M.row_index(n, nu)
    rows[:, lo] &= ~rows[:, up]                                  # one side per variable
    words = M.pack_rows(rows, n)
    assert words.shape == (B, M.n_words(n)) and words.dtype == np.uint32
    assert np.array_equal(M.unpack_words(words, n), rows)
    got = M.mult_ref(P, tq, x0, u, words, nu)
    assert got.dtype == np.longdouble
    for b in range(B):
        g = P @ u[b] + tq @ x0[b]
        for i in range(n):
            k, c = divmod(i, nu)
            bu, bl = k * 2 * nu + c, k * 2 * nu + nu + c
            bit = lambda j: (int(words[b, j // 32]) >> (j % 32)) & 1
            want = -g[i] if bit(bu) else (g[i] if bit(bl) else 0.0)
            assert abs(float(got[b, i]) - want) <= 1e-13 * max(1.0, abs(want)), (b, i)
            assert M.sides(words, n, nu)[b, i] == bit(bu) + 2 * bit(bl)
    z = M.z_rows(got, rows, nu)
    assert np.array_equal(z != 0, rows & (z != 0)) and np.array_equal(z[:, up] + z[:, lo], got)


@pytest.mark.parametrize("case", M.GOLDEN_CASES)
def test_golden_optimum_has_nonnegative_multipliers_and_reference_stationarity(golden_dir, case):
    g, e = _load(golden_dir, f"regulator_{case}.npz"), _load(golden_dir, f"qp_exact_{case}.npz")
    reg = M.golden_regulator(g)
    assert reg.reparameterize == bool(g["reparameterize"]) == case.startswith("unstable")
    Pb, tqb = reg._box_form()
    Pb = np.tril(Pb) + np.tril(Pb, -1).T
    X0, _, _ = M.golden_box_inputs(g)
    v = e["v"]
    w = M.sequence_of_v(reg, v, X0)
    words = M.pack_rows(e["active"], Pb.shape[0])
    assert (M.sides(words, Pb.shape[0], reg.Nu) < 3).all()
    mult = M.mult_ref(Pb, tqb, X0, w, words, reg.Nu)
    bound = M.mult_bound(Pb, tqb, X0, w)
    print(case, "min mult / bound", float((mult / bound).min()), "active", int(e["active"].sum()))
    assert (mult >= -bound).all()
    assert (mult[M.sides(words, Pb.shape[0], reg.Nu) > 0] > 0).any()
    z = M.z_rows(mult, e["active"], reg.Nu)
    r = M.reference_kkt(g, v, z)
    print(case, "max |P v + q + G'z| / bound", float((np.abs(r) / bound).max()))
    assert (np.abs(r) <= bound).all()


@pytest.mark.parametrize("shape", M.KERNEL_SHAPES)
def test_integer_table_of_the_kernel_test(shape):
    n, nu, n_aug = shape
    assert n % nu == 0
    P, tq = M.kernel_matrices(n, nu, n_aug)
    off = P - np.diag(np.diag(P))
    assert np.array_equal(P, P.T) and np.abs(off).max() <= 8 and (np.diag(P) > np.abs(off).sum(axis=1)).all()
    assert np.abs(tq).max() <= 16
    for B in M.KERNEL_BATCHES:
        c = M.kernel_case(n, nu, n_aug, B)
        assert c["want"].dtype == np.int64 and c["want"].shape == (B, n)
        for k in ("x0", "u"):
            assert c[k].dtype == np.int64 and np.abs(c[k]).max() <= 16
        # every partial sum of |P_i| |u| + |tq_i| |x0|, in any order, stays an integer below 2^53
        assert (np.abs(c["u"]) @ np.abs(P).T + np.abs(c["x0"]) @ np.abs(tq).T).max() < 2 ** 53
        s = M.sides(c["words"], n, nu)
        assert (s < 3).all()
        count = (s > 0).sum(axis=1)
        pats = [M.pattern_of_row(b) for b in range(B)]
        for b, p in enumerate(pats):
            if p == "none":
                assert count[b] == 0
            elif p == "first_upper":
                assert count[b] == 1 and s[b, 0] == 1
            elif p == "last_lower":
                assert count[b] == 1 and s[b, n - 1] == 2
            elif p == "all_alternating":
                assert count[b] == n and (s[b, 0::2] == 1).all() and (s[b, 1::2] == 2).all()
        assert set(pats) == set(M.PATTERNS) if B >= 5 else pats == ["all_alternating"]
        assert np.array_equal(c["want"] != 0, (s > 0) & (c["want"] != 0))        # zero wherever the variable is free
        # the sentinel is no value a case can produce: not zero, not an integer
        assert M.SENTINEL != 0.0 and M.SENTINEL != int(M.SENTINEL) and not (c["want"] == M.SENTINEL).any()
        assert all(0 < r < B for r in M.bad_rows(B))


def test_structural_inputs_are_all_free_and_all_held():
    from oracle import qp as oqp
    s = M.structural_problem()
    P, tq, nu = s["P"], s["tq"], s["nu"]
    n = P.shape[0]
    N = n // nu
    assert n == 21
    for name, want_active in (("free", 0), ("held", n)):
        lb, ub = s[name]
        for b in range(s["x0"].shape[0]):
            info = {"nu": nu}
            q = tq @ s["x0"][b]
            l, u_ = np.tile(lb[b], N), np.tile(ub[b], N)
            x = oqp.solve_exact_box(P, q, l, u_, info=info)
            # status 0 from the oracle's point of view: a KKT point of the box problem
            grad = P @ x + q
            at_ub, at_lb = x == u_, x == l
            assert np.isfinite(x).all() and (x >= l).all() and (x <= u_).all()
            assert (np.abs(grad[~at_ub & ~at_lb]) <= 1e-9 * max(1.0, np.abs(q).max())).all()
            assert (grad[at_ub] <= 0).all() and (grad[at_lb] >= 0).all()
            assert len(info["active"]) == want_active, (name, b, len(info["active"]))
            if want_active:
                assert (at_ub | at_lb).all()
