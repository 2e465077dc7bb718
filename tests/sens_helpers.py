"""Inputs and evaluators of the sensitivity tests (tests/test_cpu_sens_inputs.py holds them to the conditions the GPU tests rest on;
tests/test_sens_kernel_gpu.py and tests/test_sens_solve_gpu.py use them).  Built on tests/mult_helpers.py.

Definition (include/nnmpc.h, nnmpc_qp_sensitivity): problem b, variable i = k nu + c, direction d; A = variables with a bit set:
    du_i = dub_c (upper bit) | dlb_c (lower bit),      du_F = -P_FF^-1 (tq_F dx0 + P_FA du_A)
evaluated by the library as  t = Kunc dx0,  lam = (Hinv_AA)^-1 (t_A - du_A),  du = t - Hinv[:, A] lam.
"""
import functools

import numpy as np

from tests import mult_helpers as M

SHAPES = list(M.KERNEL_SHAPES)               # (n, nu, n_aug); the last one, (1028, 4, 12), carries the large-set family
BATCHES = [1, 5, 129]
DIRECTIONS = [1, 3, 8, 9, 17]                # both sides of the kernel's chunk of 8 directions
SET_SIZES = [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 159, 160, 161, 176, 256, 257, 512, 768]
M_LDS, M_MAX, M_OVER = 160, 768, 784         # largest set of the LDS instance, largest set at all, a set beyond it (flag 1)
KINDS = ["head", "tail", "spread"]           # the first m variables | the last m (the last variable included) | m spread over all n
FLOOR = 64 * M.U53
# what the output buffers hold before a call: mult_helpers.SENTINEL moved off the grid of sixteenths every exact result lies on
# (-7.25 itself is a value an exact case can produce)
SENTINEL = M.SENTINEL + 2.0 ** -5


def families(n, nu):
    """The set families of a shape, in a fixed order: (name, m).  Every SET_SIZES entry below n appears (one placement each, all
    three at the LDS / slab hand-over and at the ceiling), `none`, `all_alternating` (m = n), a set confined to the first stage, and
    at n > M_OVER one set of M_OVER bounds."""
    fam = [("none", 0), ("all_alternating", n), ("first_stage", nu)]
    for j, m in enumerate(s for s in SET_SIZES if 0 < s < n):
        kinds = KINDS if m in (M_LDS, M_LDS + 1, M_MAX) else [KINDS[j % 3]]
        fam += [(k, m) for k in kinds]
    if n > M_OVER:
        fam.append(("head", M_OVER))
    return fam


def family_variables(name, m, n, nu):
    if name == "none":
        return np.zeros(0, int)
    if name == "all_alternating":
        return np.arange(n)
    if name == "first_stage":
        return np.arange(nu)
    if name == "head":
        return np.arange(m)
    if name == "tail":
        return np.arange(n - m, n)
    v = np.unique(np.round(np.linspace(0, n - 1, m)).astype(int))            # spread: ends included
    extra = np.setdiff1d(np.arange(n), v)[:m - v.size]
    return np.sort(np.concatenate((v, extra)))


def family_rows(name, m, n, nu, rng, lower=None):
    """One problem's (2n,) bool active rows: the family's variables, upper and lower sides mixed (`lower`: (n,) bool to fix them)."""
    if name == "all_alternating":
        return M.pattern_rows(name, n, nu, rng)
    a = np.zeros(2 * n, bool)
    v = family_variables(name, m, n, nu)
    low = (rng.random(n) < 0.5) if lower is None else lower
    up, lo = M.row_index(n, nu)
    a[up[v[~low[v]]]] = True
    a[lo[v[low[v]]]] = True
    return a


def set_size(words, n, nu):
    return (M.sides(words, n, nu) > 0).sum(axis=1)


def tile_pert(dlb, dub, words, n, nu):
    """du on the active entries: (B, D, n) with dub_c / dlb_c where the upper / lower bit of i = k nu + c is set, NaN elsewhere."""
    s = M.sides(words, n, nu)[:, None, :]
    c = np.arange(n) % nu
    return np.where(s == 1, dub[:, :, c], np.where(s == 2, dlb[:, :, c], np.nan))


# ---- exact cases: P = diag(4^e), integer data
def exact_matrices(n, nu, n_aug):
    """P = diag(4^e_i), e_i in {0, 1, 2} (int64), tq integers of at most 16 in size; with them the exact inverse pair
    Hinv = diag(4^-e_i), Kunc = -Hinv tq (dyadic, exact in float64)."""
    rng = np.random.default_rng(3000 + n)
    e = rng.integers(0, 3, n)
    tq = rng.integers(-16, 17, (n, n_aug)).astype(np.int64)
    d = 4 ** e.astype(np.int64)
    return dict(e=e, P=np.diag(d), tq=tq, Hinv=np.diag(1.0 / d), Kunc=-(tq / d[:, None].astype(np.float64)))


def exact_case(n, nu, n_aug, B, D):
    """Integer inputs of one exact case and the results every entry must EQUAL.  Row b takes family (b + 7 D + B) mod the number of
    families, so a batch of 129 holds all of them and the small batches walk through them with D.
    dict(words, fam, dx0, dlb, dub (float64 holding integers), du (B, D, n), dmult (B, D, n), flag (B,))."""
    mats = exact_matrices(n, nu, n_aug)
    fams = families(n, nu)
    rng = np.random.default_rng(11 * n + 5 * B + D)
    fam = [fams[(b + 7 * D + B) % len(fams)] for b in range(B)]
    rows = np.array([family_rows(name, m, n, nu, rng) for name, m in fam])
    words = M.pack_rows(rows, n)
    dx0 = rng.integers(-16, 17, (B, D, n_aug)).astype(np.int64)
    dlb = rng.integers(-16, 17, (B, D, nu)).astype(np.int64)
    dub = rng.integers(-16, 17, (B, D, nu)).astype(np.int64)
    d = 4 ** mats["e"].astype(np.int64)
    q = dx0 @ mats["tq"].T                                                    # int64, |q| <= 256 n_aug
    du = -q / d.astype(np.float64)                                            # a power of two divides exactly
    pert = tile_pert(dlb.astype(np.float64), dub.astype(np.float64), words, n, nu)
    du = np.where(np.isnan(pert), du, pert)
    g = d * du + q                                                            # dyadic, far below 2^53: exact
    s = M.sides(words, n, nu)[:, None, :]
    dmult = np.where(s == 1, -g, np.where(s == 2, g, 0.0))
    flag = np.where(set_size(words, n, nu) > M_MAX, 1, 0).astype(np.int32)
    du[flag == 1] = np.nan
    dmult[flag == 1] = np.nan
    return dict(mats=mats, fam=fam, words=words, dx0=dx0.astype(np.float64), dlb=dlb.astype(np.float64), dub=dub.astype(np.float64),
                du=du, dmult=dmult, flag=flag)


# ---- real cases: seeded SPD P with cond ~ 1e3
@functools.lru_cache(maxsize=None)
def real_matrices(n, nu, n_aug):
    """P = Q diag(1 .. 1e3) Q' (symmetric), tq, and the pair (Hinv, Kunc) the handle is given (set_inverse): Hinv = Q diag^-1 Q'
    made exactly symmetric (the library averages Hinv and its transpose), Kunc = -Hinv tq."""
    rng = np.random.default_rng(4000 + n)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.logspace(0, 3, n)
    P = (Q * lam) @ Q.T
    P = 0.5 * (P + P.T)
    Hinv = (Q / lam) @ Q.T
    Hinv = 0.5 * (Hinv + Hinv.T)
    tq = rng.standard_normal((n, n_aug))
    return dict(P=P, tq=tq, Hinv=Hinv, Kunc=-Hinv @ tq)


def real_case_table():
    """(m, shape) of the real cases: every set size at the smallest shape that leaves a variable free, and the hand-over and two large
    sets once more at n = 1028, where the sets reach past 1024."""
    table = []
    for m in SET_SIZES:
        table.append((m, next(s for s in SHAPES if s[0] > m)))
    table += [(m, SHAPES[-1]) for m in (M_LDS, M_LDS + 1, 512)]
    return table


REAL_B, REAL_D = 5, 9


def real_case(m, shape):
    """Five problems with sets of exactly m bounds (head, tail, spread with mixed sides; head all upper; spread all lower), nine
    directions in x0 and both bounds."""
    n, nu, n_aug = shape
    rng = np.random.default_rng(13 * n + m)
    plan = [("head", None), ("tail", None), ("spread", None), ("head", np.zeros(n, bool)), ("spread", np.ones(n, bool))]
    rows = np.array([family_rows(k if m else "none", m, n, nu, rng, lower=low) for k, low in plan])
    return dict(words=M.pack_rows(rows, n), dx0=rng.standard_normal((REAL_B, REAL_D, n_aug)),
                dlb=rng.standard_normal((REAL_B, REAL_D, nu)), dub=rng.standard_normal((REAL_B, REAL_D, nu)))


def sens_route_f64(Hinv, Kunc, words, dx0, dlb, dub, nu):
    """The library's formula in numpy float64 with the very Hinv / Kunc the handle was given: du (B, D, n)."""
    n = Hinv.shape[0]
    B, D = dx0.shape[:2]
    pert = tile_pert(dlb, dub, words, n, nu)
    du = np.empty((B, D, n))
    for b in range(B):
        A = np.flatnonzero(~np.isnan(pert[b, 0]))
        t = dx0[b] @ Kunc.T                                                   # (D, n)
        if A.size:
            lam = np.linalg.solve(Hinv[np.ix_(A, A)], (t[:, A] - pert[b][:, A]).T)
            t = t - lam.T @ Hinv[A, :]
            t[:, A] = pert[b][:, A]
        du[b] = t
    return du


def direct_f64(P, tq, words, dx0, dlb, dub, nu):
    """The definition itself, independent of any inverse: du_F = -P_FF^-1 (tq_F dx0 + P_FA du_A) by np.linalg.solve."""
    n = P.shape[0]
    B, D = dx0.shape[:2]
    pert = tile_pert(dlb, dub, words, n, nu)
    du = np.empty((B, D, n))
    for b in range(B):
        act = ~np.isnan(pert[b, 0])
        A, F = np.flatnonzero(act), np.flatnonzero(~act)
        du[b][:, A] = pert[b][:, A]
        if F.size:
            rhs = tq[F] @ dx0[b].T + P[np.ix_(F, A)] @ pert[b][:, A].T
            du[b][:, F] = -np.linalg.solve(P[np.ix_(F, F)], rhs).T
    return du


def free_residual(P, tq, dx0, du):
    """P du + tq dx0 in np.longdouble, (B, D, n); the caller looks at the free entries."""
    ld = np.longdouble
    return du.astype(ld) @ P.astype(ld).T + dx0.astype(ld) @ tq.astype(ld).T


def scale(P, tq, dx0, du):
    """(|P| |du| + |tq| |dx0|)_i, (B, D, n)."""
    return np.abs(du) @ np.abs(P).T + np.abs(dx0) @ np.abs(tq).T


def free_ratio(P, tq, words, dx0, du, nu):
    """max over the free entries of |free_residual| / scale (0.0 when no variable is free)."""
    free = (M.sides(words, P.shape[0], nu) == 0)[:, None, :] & np.ones(du.shape, bool)
    if not free.any():
        return 0.0
    r = np.abs(free_residual(P, tq, dx0, du))[free] / scale(P, tq, dx0, du)[free]
    return float(r.max())


def dmult_ref(P, tq, words, dx0, du, nu, dtype=np.longdouble):
    """The multiplier definition applied to (dx0, du, active): (B, D, n)."""
    B, D, n = du.shape
    w = np.repeat(words, D, axis=0)
    return M.mult_ref(P, tq, dx0.reshape(B * D, -1), du.reshape(B * D, n), w, nu, dtype=dtype).reshape(B, D, n)


# ---- the golden plants: the step of the extrapolation test
def golden_directions(case, B, n_aug, nu):
    """Seeded directions in x0 and in both bounds, the same in the CPU and the GPU test."""
    rng = np.random.default_rng(500 + M.GOLDEN_CASES.index(case))
    return rng.standard_normal((B, n_aug)), 0.1 * rng.standard_normal((B, nu)), 0.1 * rng.standard_normal((B, nu))


def golden_step(reg_Pb, tqb, nu, X0, lb, ub, w, active_rows, dX0, dlb, dub):
    """Per problem the largest step t such that w + t du stays inside the bounds on the non-active rows and mult + t dmult >= 0, from
    the float64 route (np.linalg): returns (tau = t / 2 (B,), du (B, n), dmult (B, n), mult (B, n), slack (B, 2n) of the rows)."""
    n = reg_Pb.shape[0]
    words = M.pack_rows(active_rows, n)
    du = direct_f64(reg_Pb, tqb, words, dX0[:, None, :], dlb[:, None, :], dub[:, None, :], nu)[:, 0]
    mult = M.mult_ref(reg_Pb, tqb, X0, w, words, nu, dtype=np.float64)
    dmult = M.mult_ref(reg_Pb, tqb, dX0, du, words, nu, dtype=np.float64)
    c = np.arange(n) % nu
    s = M.sides(words, n, nu)
    tau = np.full(X0.shape[0], np.inf)
    for b in range(X0.shape[0]):
        free = s[b] == 0
        # upper slack ub + t dub - (w + t du) >= 0, lower slack likewise, on the non-active rows
        for slack, rate in ((ub[b, c] - w[b], dub[b, c] - du[b]), (w[b] - lb[b, c], du[b] - dlb[b, c])):
            shrink = free & (rate < 0)
            if shrink.any():
                tau[b] = min(tau[b], (slack[shrink] / -rate[shrink]).min())
        drop = ~free & (dmult[b] < 0)
        if drop.any():
            tau[b] = min(tau[b], (mult[b][drop] / -dmult[b][drop]).min())
    return 0.5 * tau, du, dmult, mult
