"""Inputs and evaluators of the adjoint tests (tests/test_cpu_adj_inputs.py holds them to the conditions the GPU tests rest on;
tests/test_adj_kernel_gpu.py, tests/test_adj_solve_gpu.py and tests/test_adj_staging_gpu.py use them).  Built on tests/sens_helpers.py
and tests/mult_helpers.py.

Definition (include/nnmpc.h, nnmpc_qp_adjoint): problem b, cotangent d, A = variables with a bit set, F = the rest:
    w = (Hinv_AA)^-1 (Hinv[A, :] v),   z = v - E_A w,   gx0 = Kunc' z,   gbound = w on A and +0.0 on F,   gub / glb = w summed per input
    and side,  so that  <v, du> = <gx0, dx0> + <glb, dlb> + <gub, dub>  for du of nnmpc_qp_sensitivity.
In first-move mode v has nu entries and stands for the sequence cotangent with zeros behind the first stage (extend).
"""
import functools

import numpy as np
import scipy.linalg

from tests import mult_helpers as M
from tests import sens_helpers as S

FLOOR = S.FLOOR
SENTINEL = S.SENTINEL
ORDERS = ["solve", "chol", "perm"]


def extend(v, n):
    """(B, D, nu) first-stage cotangents -> (B, D, n), zeros behind the first stage; (B, D, n) comes back as it is."""
    if v.shape[2] == n:
        return v
    out = np.zeros(v.shape[:2] + (n,))
    out[:, :, :v.shape[2]] = v
    return out


def column_sums(w, words, n, nu):
    """gub, glb (B, D, nu) of gbound w (B, D, n): the sums over the variables of each input whose upper / lower bit is set."""
    s = M.sides(words, n, nu)[:, None, :]
    fold = lambda a: a.reshape(a.shape[0], a.shape[1], n // nu, nu).sum(axis=2)
    return fold(np.where(s == 1, w, 0.0)), fold(np.where(s == 2, w, 0.0))


def adjoint_route_f64(Hinv, Kunc, words, v, nu, order="solve"):
    """The library's formula in numpy float64 with the very Hinv / Kunc the handle was given.  v (B, D, n) or (B, D, nu).
    order: how w = M^-1 r is evaluated -- np.linalg.solve | Cholesky and two triangular solves | the same with the list reversed (every
    sum of the factorisation and of the substitutions in another order).  dict(gx0 (B, D, n_aug), gbound (B, D, n), glb, gub)."""
    n = Hinv.shape[0]
    v = extend(v, n)
    B, D = v.shape[:2]
    act = M.sides(words, n, nu) > 0
    gx0, gb = np.empty((B, D, Kunc.shape[1])), np.zeros((B, D, n))
    for b in range(B):
        A = np.flatnonzero(act[b])
        z = v[b].copy()                                                       # (D, n)
        if A.size:
            if order == "perm":
                A = A[::-1]
            Mx, r = Hinv[np.ix_(A, A)], Hinv[A, :] @ v[b].T                   # (m, m), (m, D)
            if order == "solve":
                w = np.linalg.solve(Mx, r)
            else:
                L = np.linalg.cholesky(Mx)
                w = scipy.linalg.solve_triangular(L.T, scipy.linalg.solve_triangular(L, r, lower=True), lower=False)
            gb[b][:, A] = w.T
            z[:, A] -= w.T
        gx0[b] = z @ Kunc
    gub, glb = column_sums(gb, words, n, nu)
    return dict(gx0=gx0, gbound=gb, glb=glb, gub=gub)


def _chunks(x, count, bits=21):
    """x (float64 or longdouble) as a sum of `count` arrays of integers of at most `bits` bits (float64) times powers of two:
    [(c_k, scale_k)], x = sum c_k scale_k up to 2^-(bits count) max |x|."""
    ld = np.longdouble
    top = float(np.abs(x).max())
    if top == 0.0:
        return []
    e = int(np.ceil(np.log2(top))) + 1
    r = x.astype(ld) / ld(2.0) ** e                                           # |r| <= 1/2, exact
    out = []
    for k in range(count):
        r = r * ld(2.0) ** bits
        c = np.trunc(r)
        r = r - c                                                             # exact: both are multiples of the last bit of r
        out.append((c.astype(np.float64), ld(2.0) ** (e - bits * (k + 1))))
    return out


def residual_exact(A, y, v):
    """v - A y for float64 A (k x k, k < 2048), longdouble y and v, to far below the last bit of longdouble: A in five and y in four
    chunks of 21 bits, so that every float64 product of two chunks is a sum of k integers below 2^42 -- exact whatever the order --,
    and the twenty partial products are taken from v one after the other with an error-free two-sum, the errors summed beside it.
    (A residual formed in longdouble alone carries 2^-64 |A| |y|, which the solve turns into cond(A) 2^-64 |y|.)"""
    assert A.shape[0] < 2048
    s, comp = v.copy(), np.zeros_like(v)
    for ca, sa in _chunks(A, 5):
        for cy, sy in _chunks(y, 4):
            t = -((ca @ cy).astype(np.longdouble) * (sa * sy))
            new = s + t
            bb = new - s
            comp = comp + ((s - (new - bb)) + (t - bb))
            s = new
    return s + comp


def adjoint_ref_ld(P, tq, words, v, nu):
    """Independent of any inverse: y = P_FF^-1 v_F by an LU solve and four refinement steps with residuals exact beyond
    np.longdouble (residual_exact), gx0 = -tq_F' y, w = v_A - P_AF y in np.longdouble.
    dict(gx0, gbound (float64), last: the largest last correction / max |y|)."""
    ld = np.longdouble
    n = P.shape[0]
    v = extend(v, n)
    B, D = v.shape[:2]
    act = M.sides(words, n, nu) > 0
    Pl, tql = P.astype(ld), tq.astype(ld)
    gx0, gb, last = np.empty((B, D, tq.shape[1])), np.zeros((B, D, n)), 0.0
    for b in range(B):
        A, F = np.flatnonzero(act[b]), np.flatnonzero(~act[b])
        y = np.zeros((F.size, D), ld)
        if F.size:
            PFF, vF = P[np.ix_(F, F)], v[b][:, F].T.astype(ld)
            lu = scipy.linalg.lu_factor(PFF)
            y = scipy.linalg.lu_solve(lu, v[b][:, F].T).astype(ld)
            for _ in range(4):
                dy = scipy.linalg.lu_solve(lu, residual_exact(PFF, y, vF).astype(np.float64)).astype(ld)
                y = y + dy
            last = max(last, float(np.abs(dy).max() / max(np.abs(y).max(), np.finfo(float).tiny)))
        gx0[b] = (-(tql[F].T @ y)).T.astype(np.float64)
        if A.size:
            gb[b][:, A] = (v[b][:, A].T.astype(ld) - Pl[np.ix_(A, F)] @ y).T.astype(np.float64)
    return dict(gx0=gx0, gbound=gb, last=last)


def errors(Kunc, words, v, nu, got_gx0, got_w, ref):
    """(e_x, e_w) of a result against ref (adjoint_ref_ld's dict), the largest over the rows (b, d):
    e_x = max_i |gx0 - ref|_i / max_i (|Kunc|' (|v| + E_A |w_ref|))_i,     e_w = max_i |w - w_ref|_i / (max |w_ref| + max |v|)."""
    n = Kunc.shape[0]
    v = extend(v, n)
    sx = (np.abs(v) + np.abs(ref["gbound"])) @ np.abs(Kunc)                   # (B, D, n_aug); gbound is zero off A
    e_x = np.abs(got_gx0 - ref["gx0"]).max(axis=2) / sx.max(axis=2)
    e_w = np.abs(got_w - ref["gbound"]).max(axis=2) / (np.abs(ref["gbound"]).max(axis=2) + np.abs(v).max(axis=2))
    return float(e_x.max()), float(e_w.max())


def tolerance(route_value, n, n_aug):
    return max(8 * route_value, FLOOR * (n + n_aug))


def real_cotangents(m, shape, first=False):
    """Seeded normal cotangents of a real case (sens_helpers.real_case gives its sets): (REAL_B, REAL_D, n) or (..., nu)."""
    n, nu, n_aug = shape
    rng = np.random.default_rng(17 * n + m + (1 if first else 0))
    return rng.standard_normal((S.REAL_B, S.REAL_D, nu if first else n))


@functools.lru_cache(maxsize=None)
def real_reference(m, shape, first=False):
    """adjoint_ref_ld of a real case and its seeded cotangents, computed once and shared (treat it as read-only)."""
    mats, c = S.real_matrices(*shape), S.real_case(m, shape)
    return adjoint_ref_ld(mats["P"], mats["tq"], c["words"], real_cotangents(m, shape, first), shape[1])


def identity_gap(v, du, g, dx0, dlb, dub):
    """Per row (b, d): |<v, du> - <gx0, dx0> - <glb, dlb> - <gub, dub>| and the scale |v|'|du| + |gx0|'|dx0| + |glb|'|dlb| + |gub|'|dub|."""
    dot = lambda a, b: (a * b).sum(axis=2)
    gap = np.abs(dot(v, du) - dot(g["gx0"], dx0) - dot(g["glb"], dlb) - dot(g["gub"], dub))
    scale = dot(np.abs(v), np.abs(du)) + dot(np.abs(g["gx0"]), np.abs(dx0)) + dot(np.abs(g["glb"]), np.abs(dlb)) + dot(np.abs(g["gub"]), np.abs(dub))
    return gap, scale


# ---- exact cases: P = diag(4^e), integer data
def exact_case_adj(n, nu, n_aug, B, D, first=False):
    """Integer cotangents in [-16, 16] on the sets of sens_helpers.exact_case (the same families in the same rows) and the results every
    entry must EQUAL: with Hinv diagonal w = v on A, so gx0 = Kunc' (v masked to F), gbound = v on A, glb / gub its column sums -- all
    multiples of 1/16 far below 2^53.  In first-move mode the terms of first-stage active variables cancel exactly and w is exactly
    zero behind the first stage.  dict(mats, fam, words, v, gx0, gbound, glb, gub, flag)."""
    c = S.exact_case(n, nu, n_aug, B, D)
    rng = np.random.default_rng(19 * n + 3 * B + D + (1 if first else 0))
    v = rng.integers(-16, 17, (B, D, nu if first else n)).astype(np.float64)
    ve = extend(v, n)
    act = (M.sides(c["words"], n, nu) > 0)[:, None, :]
    gbound = np.where(act, ve, 0.0)
    gx0 = np.where(act, 0.0, ve) @ c["mats"]["Kunc"]
    gub, glb = column_sums(gbound, c["words"], n, nu)
    out = dict(mats=c["mats"], fam=c["fam"], words=c["words"], v=v, gx0=gx0, gbound=gbound, glb=glb, gub=gub, flag=c["flag"])
    for k in ("gx0", "gbound", "glb", "gub"):
        out[k][c["flag"] == 1] = np.nan
    return out
