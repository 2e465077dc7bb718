"""Self-certifying fp64 references for the reduced steady-state target problem (TEST ORACLE)

    min 1/2 us' Pr us + q' us   s.t.  E us = e,  lb <= us <= ub,      Pr symmetric positive definite.

Strictly convex, so a KKT point is THE optimum.  Multiplier convention (include/nnmpc.h states the same one):

    Pr us + q + E' lam_eq + mu_ub - mu_lb = 0,   mu_ub, mu_lb >= 0,   mu_ub (ub - us) = 0,  mu_lb (us - lb) = 0.

Bound states are coded like the library's ``active`` output: 0 free, 1 at ub, 2 at lb.

* ``enumerate_states``  tries all 3^nu bound states (nu <= 7), independent of every active-set strategy;
* ``certify``           takes a candidate point of any size, fixes its bound state, re-solves the KKT system of that state and
                        reports margins and the conditioning of that system -- or raises when the state is not a KKT point.
"""
import itertools

import numpy as np
import scipy.linalg as sla

EPS = np.finfo(np.float64).eps


def _as(Pr, q, E, e, lb, ub):
    Pr = np.asarray(Pr, float)
    nu = Pr.shape[0]
    E = np.zeros((0, nu)) if E is None else np.asarray(E, float).reshape(-1, nu)
    return (Pr, np.asarray(q, float), E, np.asarray(e, float), np.asarray(lb, float).ravel(), np.asarray(ub, float).ravel())


def kkt_matrix(Pr, E, state):
    """KKT matrix of the free inputs and the equalities of a bound state: [[Pr_ff, E_f'], [E_f, 0]]."""
    f = np.asarray(state) == 0
    nz = E.shape[0]
    return np.block([[Pr[np.ix_(f, f)], E[:, f].T], [E[:, f], np.zeros((nz, nz))]])


def solve_state(Pr, Q, E, Ee, lb, ub, state):
    """Solve the KKT system of one bound state for a batch of right-hand sides Q (M, nu), Ee (M, nz).
    Returns (us (M, nu), lam_eq (M, nz), mu (M, nu): multiplier of the held bound, 0 on free inputs, K) or None when the
    system of this state is singular (fewer free inputs than equalities, or E_f rank deficient)."""
    state = np.asarray(state)
    f = state == 0
    h = ~f
    nu, nz, nf = Pr.shape[0], E.shape[0], int(f.sum())
    if nf < nz:
        return None
    M = Q.shape[0]
    xb = np.where(state == 1, ub, lb)
    us = np.tile(np.where(h, xb, 0.0), (M, 1))
    lam = np.zeros((M, nz))
    K = kkt_matrix(Pr, E, state)
    if nf + nz:
        if nz:                                           # Pr_ff > 0: K is singular exactly when E_f loses row rank
            sv = np.linalg.svd(E[:, f], compute_uv=False)
            if not sv[-1] > 1e-12 * max(sv[0], np.abs(E).max()):
                return None
        rhs = np.concatenate((-Q[:, f] - (Pr[np.ix_(f, h)] @ xb[h])[None, :], Ee - (E[:, h] @ xb[h])[None, :]), axis=1)
        lu = sla.lu_factor(K)
        sol = sla.lu_solve(lu, rhs.T)
        for _ in range(2):                               # refinement: LU is backward stable in norm, not row by row, and
            sol += sla.lu_solve(lu, rhs.T - K @ sol)     # the rows of K differ by max|Pr| / max|E| in size
        sol = sol.T
        us[:, f] = sol[:, :nf]
        lam = sol[:, nf:]
    g = us @ Pr.T + Q + lam @ E
    mu = np.where(state == 1, -g, np.where(state == 2, g, 0.0))
    return us, lam, mu, K


def _row_size(Pr, Q, E, us, lam):
    """Size of the terms of every stationarity row (what its rounding error scales with)."""
    return np.abs(us) @ np.abs(Pr).T + np.abs(Q) + np.abs(lam) @ np.abs(E)


def enumerate_states(Pr, Q, E, Ee, lb, ub, ptol=1e-9, dtol=1e-9):
    """All KKT bound states of every problem of a batch that shares Pr, E, lb, ub (nu <= 7).

    Q (M, nu), Ee (M, nz) -> list of M lists of dicts(state, us, lam_eq, mu, primal_margin, dual_margin, cond).  A state
    counts when its free inputs lie inside the box within ``ptol`` and its bound multipliers are >= -``dtol`` max(1, |q|inf);
    a non-degenerate problem has exactly one, a degenerate one several that share ``us``, an infeasible one none."""
    Pr, Q, E, Ee, lb, ub = _as(Pr, Q, E, Ee, lb, ub)
    nu = Pr.shape[0]
    if nu > 7:
        raise ValueError("enumeration is meant for nu <= 7")
    Q = Q.reshape(-1, nu)
    M = Q.shape[0]
    Ee = Ee.reshape(M, E.shape[0])
    out = [[] for _ in range(M)]
    for state in itertools.product((0, 1, 2), repeat=nu):
        state = np.array(state)
        r = solve_state(Pr, Q, E, Ee, lb, ub, state)
        if r is None:
            continue
        us, lam, mu, K = r
        f = state == 0
        pm = np.minimum(us - lb, ub - us)[:, f].min(axis=1) if f.any() else np.full(M, np.inf)
        dm = mu[:, ~f].min(axis=1) if (~f).any() else np.full(M, np.inf)
        dok = (mu >= -dtol * _row_size(Pr, Q, E, us, lam))[:, ~f].all(axis=1)
        eq = np.abs(us @ E.T - Ee).max(axis=1) if E.shape[0] else np.zeros(M)
        ok = (pm >= -ptol) & dok & (eq <= 1e-9 * np.maximum(1.0, np.abs(Ee).max(axis=1) if E.shape[0] else 1.0))
        if not ok.any():
            continue
        cond = np.linalg.cond(K) if K.size else 1.0
        for i in np.flatnonzero(ok):
            out[i].append(dict(state=state.astype(np.uint8), us=us[i], lam_eq=lam[i], mu=mu[i], primal_margin=float(pm[i]),
                               dual_margin=float(dm[i]), cond=float(cond)))
    return out


def enumerate_solve(Pr, q, E, e, lb, ub, **kw):
    """One problem by enumeration: the KKT state with the largest smaller margin (the clearest one of a degenerate point), with
    ``states`` = every KKT state found.  Raises ArithmeticError when there is none (infeasible) and when two states disagree on
    ``us`` (impossible for Pr > 0; it would mean the enumeration itself is wrong)."""
    found = enumerate_states(Pr, np.asarray(q, float)[None, :], E, np.asarray(e, float)[None, :], lb, ub, **kw)[0]
    return pick_state(found)


def pick_state(found):
    if not found:
        raise ArithmeticError("no bound state satisfies the KKT conditions: the problem is infeasible")
    best = max(found, key=lambda s: min(s["primal_margin"], s["dual_margin"]))
    for s in found:
        if np.abs(s["us"] - best["us"]).max() > 1e-7 * max(1.0, np.abs(best["us"]).max()):
            raise ArithmeticError("two KKT states with different us")
    return dict(best, states=[s["state"] for s in found])


def certify(Pr, q, E, e, lb, ub, us=None, snap=1e-9, ptol=1e-9, dtol=1e-9, state=None):
    """Certify a candidate optimum of any size.

    The bound state is ``state`` when given, else read off the candidate ``us`` (at a bound within ``snap``; an input with lb == ub goes to the side its multiplier
    asks for), the KKT system of that state is re-solved in fp64, and the result is checked: free inputs inside the box within
    ``ptol``, bound multipliers >= -``dtol`` times the size of the terms of their row, equalities.  Returns dict(us, lam_eq, mu, state, primal_margin
    (smallest distance of a free input to its bounds; inf when none is free), dual_margin (smallest bound multiplier; inf
    when none is held), cond (cond_2 of the KKT matrix of the free inputs and the equalities; 1 when it is empty)).
    Raises ArithmeticError when the state is not a KKT point."""
    Pr, q, E, e, lb, ub = _as(Pr, q, E, e, lb, ub)
    if state is None:
        us = np.asarray(us, float).ravel()
        if not np.all(np.isfinite(us)):
            raise ArithmeticError("candidate is not finite")
        state = np.where(us >= ub - snap, 1, np.where(us <= lb + snap, 2, 0))
    state = np.array(state, int)
    fixed = lb == ub
    for _ in range(2):
        r = solve_state(Pr, q[None, :], E, e[None, :], lb, ub, state)
        if r is None:
            raise ArithmeticError("the KKT system of the candidate's bound state is singular")
        x, lam, mu, K = (a[0] if i < 3 else a for i, a in enumerate(r))
        flip = fixed & (state != 0) & (mu < 0.0)
        if not flip.any():
            break
        state = np.where(flip, 3 - state, state)
    f = state == 0
    pm = float(np.minimum(x - lb, ub - x)[f].min()) if f.any() else np.inf
    dm = float(mu[~f].min()) if (~f).any() else np.inf
    if pm < -ptol:
        raise ArithmeticError(f"not a KKT point: a free input leaves the box by {-pm:.3e}")
    if not (mu >= -dtol * _row_size(Pr, q, E, x, lam))[~f].all():
        raise ArithmeticError(f"not a KKT point: bound multiplier {dm:.3e}")
    if E.shape[0] and np.abs(E @ x - e).max() > 1e-9 * max(1.0, np.abs(e).max()):
        raise ArithmeticError("not a KKT point: equalities violated")
    cond = float(np.linalg.cond(K)) if K.size else 1.0
    return dict(us=x, lam_eq=lam, mu=mu, state=state.astype(np.uint8), primal_margin=pm, dual_margin=dm, cond=cond)


def dual_active_set(Pr, q, E, e, lb, ub, iters=2000):
    """Bound state by a Goldfarb-Idnani dual active-set iteration from the optimum under the equalities alone, plain numpy, one
    dense KKT solve per step.  It only PROPOSES a state: nothing here is trusted, ``certify`` judges the result.  Returns the
    state, or None when no step is possible (no point of the box satisfies the equalities) or the budget runs out."""
    nu, nz = Pr.shape[0], E.shape[0]
    state = np.zeros(nu, int)
    r = solve_state(Pr, q[None, :], E, e[None, :], lb, ub, state)
    if r is None:
        return None
    x, mu = r[0][0].copy(), np.zeros(nu)
    it = 0
    while it < iters:
        viol = np.where(state == 0, np.maximum(x - ub, lb - x), -np.inf)
        p = int(viol.argmax())
        if not viol[p] > 1e-13:
            return state
        sp, bp = (1.0, ub[p]) if x[p] > ub[p] else (-1.0, lb[p])
        while it < iters:
            it += 1
            f = state == 0
            rhs = np.zeros(int(f.sum()) + nz)
            rhs[int(f[:p].sum())] = -sp
            sol = np.linalg.solve(kkt_matrix(Pr, E, state), rhs)
            z = np.zeros(nu)
            z[f] = sol[:int(f.sum())]
            g = Pr @ z + E.T @ sol[int(f.sum()):]
            vi = np.where(state == 1, -g, np.where(state == 2, g, 0.0))
            t2 = (bp - x[p]) / z[p] if abs(z[p]) * Pr[p, p] > 1e-10 and (bp - x[p]) / z[p] > 0.0 else np.inf
            cand = np.where((state != 0) & (vi < 0.0), mu / np.where(vi < 0.0, -vi, 1.0), np.inf)
            kb = int(cand.argmin())
            t1 = cand[kb]
            t = min(t1, t2)
            if not np.isfinite(t):
                return None
            x = np.where(f, x + t * z, x)
            mu = np.where(f, mu, mu + t * vi)
            mu[p] += t
            if t2 <= t1:
                state[p] = 1 if sp > 0 else 2
                x[p] = bp
                break
            state[kb], mu[kb] = 0, 0.0
    return None


def _interior_point(Pr, q, E, e, lb, ub):
    from . import qp as oqp
    nu = Pr.shape[0]
    if E.shape[0] == 0:
        x = oqp.solve_exact_box(Pr, q, lb, ub)
    else:
        G = np.vstack((np.eye(nu), -np.eye(nu)))
        x = oqp.solve_exact_eq(Pr, q, G, np.concatenate((ub, -lb)), E, e)
    return certify(Pr, q, E, e, lb, ub, x)


def _active_set(Pr, q, E, e, lb, ub):
    state = dual_active_set(Pr, q, E, e, lb, ub)
    if state is None:
        raise ArithmeticError("no bound state proposed: infeasible, rank deficient or out of budget")
    return certify(Pr, q, E, e, lb, ub, state=state)


def solve(Pr, q, E, e, lb, ub, propose="interior_point"):
    """Certified optimum of one problem of any size.  The candidate comes from oracle.qp.solve_exact_box (nz = 0) /
    solve_exact_eq (``propose="interior_point"``) or from ``dual_active_set`` (``"active_set"``, ten times faster at 64
    unknowns); either way ``certify`` judges it, and when it refuses -- solve_exact_eq can stop short of the optimal bound
    state on ill-conditioned problems, its polish does not certify itself -- the other proposer gets its turn.  Raises
    ArithmeticError when neither candidate is a KKT point."""
    Pr, q, E, e, lb, ub = _as(Pr, q, E, e, lb, ub)
    order = (_interior_point, _active_set) if propose == "interior_point" else (_active_set, _interior_point)
    try:
        return order[0](Pr, q, E, e, lb, ub)
    except (ArithmeticError, ValueError, np.linalg.LinAlgError):
        pass
    try:
        return order[1](Pr, q, E, e, lb, ub)
    except (ValueError, np.linalg.LinAlgError) as ex:
        raise ArithmeticError(f"no certified optimum: {ex}")
