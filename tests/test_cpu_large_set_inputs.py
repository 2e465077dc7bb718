"""The inputs and the referee of tests/test_large_sets_gpu.py, judged on the CPU by the fp64 oracle alone.

  * large_set_problem: at every size named by a kernel threshold of the active-set pass (144 | 145, 176 | 177, 256 | 257,
    384 | 385, 768 | 769, and 800) the oracle's active set is exactly the pushed set, with the pushed signs, and every free
    variable stays well inside the box -- the set the first round sees (the bounds x_unc violates) is the same set;
  * strain_problem (cond(P) = 1e4): the oracle's sets put at least three problems into 257 .. 384 and three into 385 .. 768 bounds;
  * kkt_check, the GPU tests' referee, accepts the oracle's answer and rejects it with one bound state flipped or with one free
    variable moved by 1e-6.
"""
import numpy as np
import pytest

from tests import helpers as H

N_, NU = 1024, 8
NAMED = [144, 145, 176, 177, 256, 257, 384, 385, 768, 769, 800]


@pytest.fixture(scope="module")
def named():
    P, q, lb, ub, state, xref = H.large_set_problem(N_, NU, 5, NAMED)
    return P, q, lb, ub, state, xref, H.oracle_rows(P, q, lb, ub, NU, range(len(NAMED)))


def test_named_sizes_give_exactly_the_pushed_set(named):
    P, q, lb, ub, state, xref, ref = named
    assert np.linalg.cond(P) < 6.0
    expect = H.state_to_active(state, NU)
    xunc = np.linalg.solve(P, -q.T).T
    for r, m in enumerate(NAMED):
        x, act = ref[r]
        assert int(act.sum()) == m and (act == expect[r]).all(), (m, int(act.sum()))
        assert np.abs(x[state[r] == 0]).max() <= 0.68, m                                 # free variables: far from a bound
        assert np.array_equal(np.where(xunc[r] > 1, 1, np.where(xunc[r] < -1, 2, 0)), state[r]), m   # the first set is the final one
        assert np.abs(xref[r] - x).max() <= 1e-12, m                                     # the builder's own optimum


def test_strain_family_covers_both_large_classes():
    P, q, lb, ub = H.strain_problem(N_, NU)
    ev = np.linalg.eigvalsh(P)
    assert 0.5 * H.STRAIN_COND < ev[-1] / ev[0] <= 1.001 * H.STRAIN_COND
    sizes = np.array([int(act.sum()) for _, act in H.oracle_rows(P, q, lb, ub, NU, range(q.shape[0]))])
    assert ((sizes >= 257) & (sizes <= 384)).sum() >= 3 and ((sizes >= 385) & (sizes <= 768)).sum() >= 3, sizes
    assert (sizes > np.array(H.STRAIN_PUSHES)).all(), sizes                              # the couplings add bounds to the pushed ones


def _answer(named, r):
    P, q, lb, ub, state, xref, ref = named
    x, act = ref[r]
    return dict(u=x[None, :].copy(), active=act[None, :].copy())


@pytest.mark.parametrize("r", [0, 6, 8])
def test_kkt_check_rejects_a_flipped_state_and_a_moved_variable(named, r):
    P, q, lb, ub, state, xref, ref = named
    args = (P, np.eye(N_), NU, N_ // NU, q[r:r + 1], lb[None, :], ub[None, :])
    H.kkt_check(*args, _answer(named, r), 1e-7)                                          # the oracle's own answer passes
    on, free = np.flatnonzero(state[r] != 0), np.flatnonzero(state[r] == 0)
    k, c = np.arange(N_) // NU, np.arange(N_) % NU
    row = lambda i, s: k[i] * 2 * NU + (0 if s == 1 else NU) + c[i]
    for i in (on[0], on[-1]):                                                            # an active bound reported free
        bad = _answer(named, r)
        bad["active"][0, row(i, state[r, i])] = False
        with pytest.raises(AssertionError):
            H.kkt_check(*args, bad, 1e-7)
        bad = _answer(named, r)                                                          # ... and reported on the other side
        bad["active"][0, row(i, state[r, i])] = False
        bad["active"][0, row(i, 3 - state[r, i])] = True
        with pytest.raises(AssertionError):
            H.kkt_check(*args, bad, 1e-7)
    for i in (free[0], free[-1]):                                                        # a free variable reported on a bound
        bad = _answer(named, r)
        bad["active"][0, row(i, 1)] = True
        with pytest.raises(AssertionError):
            H.kkt_check(*args, bad, 1e-7)
    # a free variable moved by 1e-6: its own gradient entry moves by 1e-6 P_ii, against a tolerance of 1e-7 max(1, |q|inf) -- the
    # variable with the largest P_ii (~4) is one the check must see (|q|inf is ~12 here: asserted, with a factor 2 to spare)
    i = free[np.argmax(np.diag(P)[free])]
    assert 1e-6 * P[i, i] > 2 * 1e-7 * max(1.0, np.abs(q[r]).max())
    for d in (1e-6, -1e-6):
        bad = _answer(named, r)
        bad["u"][0, i] += d
        with pytest.raises(AssertionError):
            H.kkt_check(*args, bad, 1e-7)
