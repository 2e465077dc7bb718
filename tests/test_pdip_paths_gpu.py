"""The PDIP path's state machine (refill_k, stage_pre_k, cg_alpha, kkt_check) under method "pdip", against the exact oracle.

One family (tests/helpers.py: pdip_family -- the generic SPD construction of tests/test_random_shapes_gpu.py at n = 130, nu = 2,
N = 65: three tiles of 64 with 62 pad rows, cond(P) = 1e3, 24 problems, the oracle's sets hold 19 - 45 % of the variables, row 1 is
the empty set; tests/test_cpu_pdip_inputs.py holds it to that) through every option of the path no other test sets, a warm start
(`guess`) under "pdip", the budgets, slot reuse, and an indefinite Hessian.

"Certified exact": status 0, |u - u*| <= 1e-8 max(1, |u*|inf) and the active rows equal to those of oracle.qp.solve_exact_box.
"""
import time

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

OPTIONS = {
    "default": {},
    "nb128": dict(nb=128),
    "no_reuse": dict(stale_max_changes=-1),
    "reuse_always_cg2": dict(stale_max_changes=1000, stale_cg_limit=2),
    "sub_steps2": dict(sub_steps=2),
    "max_refine5": dict(max_refine=5),
    "max_ipm_iters1": dict(max_ipm_iters=1),          # the polish must repair a poor first set
}
_runs = {}


@pytest.fixture(scope="module")
def fam():
    f = H.pdip_family()
    f["U"], f["act"] = H.pdip_family_oracle(f)
    f["state"] = H.active_to_state(f["act"], f["nu"])
    return f


def _solver(f, **kw):
    from industrial_nnmpc_2021_amd.qp import BatchedBoxQP
    return BatchedBoxQP(f["P"], f["tq"], f["nu"], max_batch=128, method="pdip", **kw)


def _run(f, name):
    """The family under OPTIONS[name], cold; solved once per module."""
    if name not in _runs:
        qp = _solver(f, **OPTIONS[name])
        _runs[name] = qp.solve_batch(f["x0"], f["lb"], f["ub"])
        qp.close()
    return _runs[name]


def _exact(out, U, act):
    """Per row: certified exact?"""
    err = np.abs(out["u"] - U).max(axis=1) / np.maximum(1.0, np.abs(U).max(axis=1))
    return (out["status"] == 0) & (err <= 1e-8) & (out["active"] == act).all(axis=1)


def _assert_exact(out, U, act, what):
    ok = _exact(out, U, act)
    err = np.abs(out["u"] - U).max(axis=1) / np.maximum(1.0, np.abs(U).max(axis=1))
    assert ok.all(), (what, "rows", np.flatnonzero(~ok)[:10], "status", out["status"][~ok][:10], "err", err[~ok][:10],
                      "set differs in", (out["active"] != act).sum(axis=1)[~ok][:10])


@pytest.mark.parametrize("name", list(OPTIONS))
def test_every_option_gives_the_exact_optimum(fam, name):
    out = _run(fam, name)
    print(f"\n{name}: factorizations {out['factorizations'].tolist()} ipm_iters {out['ipm_iters'].tolist()}")
    _assert_exact(out, fam["U"], fam["act"], name)
    assert (out["factorizations"] >= 1).all()
    if name == "max_ipm_iters1":
        assert (out["ipm_iters"] <= 1).all(), out["ipm_iters"]


def test_factor_reuse_is_reached(fam):
    """Without reuse every set change costs a factorisation: never fewer than the default, and more in at least one row --
    otherwise the family does not reach the stale-preconditioner path and has to be drawn again."""
    base, none = _run(fam, "default")["factorizations"], _run(fam, "no_reuse")["factorizations"]
    assert (none >= base).all() and (none > base).any(), (base, none)
    # With stale_max_changes = 1000 (> n) every set change keeps its factor: beyond the PDIP iterations' factors and the polish's
    # first one, only cg_alpha's fallback (a reused factor that has not converged after stale_cg_limit = 2 steps) factors again.
    always = _run(fam, "reuse_always_cg2")
    assert (always["factorizations"] > always["ipm_iters"] + 1).any(), (always["factorizations"], always["ipm_iters"])


def test_warm_start_under_pdip(fam):
    """One batch, side by side: the oracle's set as guess (no PDIP iteration, at least one factorisation), a guess with 10 % of
    the states flipped, an all-free guess, and rows whose guess starts with 255 (= no guess: the bytes of the cold run)."""
    B, n = fam["x0"].shape[0], fam["n"]
    flipped = H.pdip_flipped_guess(fam["state"])
    ignored = np.ones((B, n), np.uint8)                 # would be a terrible guess if it were read
    ignored[:, 0] = 255
    guess = np.concatenate((fam["state"], flipped, np.zeros((B, n), np.uint8), ignored))
    rep = lambda a: np.tile(a, (4, 1))
    qp = _solver(fam)
    cold = qp.solve_batch(fam["x0"], fam["lb"], fam["ub"])
    out = qp.solve_batch(rep(fam["x0"]), rep(fam["lb"]), rep(fam["ub"]), guess=guess)
    qp.close()
    _assert_exact(out, rep(fam["U"]), rep(fam["act"]), "warm batch")
    assert (out["ipm_iters"][:3 * B] == 0).all(), out["ipm_iters"][:3 * B]
    assert (out["factorizations"][:3 * B] >= 1).all()
    for k in ("u", "active", "status", "ipm_iters", "factorizations"):
        assert out[k][3 * B:].tobytes() == cold[k].tobytes(), k
    print(f"\nwarm start: factorizations oracle-set {out['factorizations'][:B].tolist()} flipped {out['factorizations'][B:2 * B].tolist()} "
          f"all-free {out['factorizations'][2 * B:3 * B].tolist()} cold {cold['factorizations'].tolist()}")


def _loud_never_wrong(out, f, what):
    ok = _exact(out, f["U"], f["act"])
    assert np.isfinite(out["u"]).all(), what
    assert (out["status"] != 2).all(), (what, out["status"])
    assert (ok | (out["status"] == 1)).all(), (what, np.flatnonzero(~ok & (out["status"] != 1)), out["status"])
    assert (out["status"] == 1).any(), (what, "no row met its budget: nothing was tested")
    print(f"\n{what}: status 1 in {int((out['status'] == 1).sum())} of {out['status'].size} rows")


def test_budgets_are_loud_never_wrong(fam):
    qp = _solver(fam, max_polish_rounds=1)
    out = qp.solve_batch(fam["x0"], fam["lb"], fam["ub"], guess=H.pdip_flipped_guess(fam["state"]))
    qp.close()
    _loud_never_wrong(out, fam, "max_polish_rounds=1, flipped guess")
    qp = _solver(fam, max_rounds=3)
    out = qp.solve_batch(fam["x0"], fam["lb"], fam["ub"])
    qp.close()
    _loud_never_wrong(out, fam, "max_rounds=3, cold")


def test_slot_reuse_with_rejected_rows_between(fam):
    """300 problems on 128 slots: every slot is refilled at least once, rejected rows (NaN in x0, lb > ub) in between."""
    B, total = fam["x0"].shape[0], 300
    src = np.arange(total) % B
    x0, lb, ub = fam["x0"][src].copy(), fam["lb"][src].copy(), fam["ub"][src].copy()
    nan_rows, swap_rows = np.arange(5, total, 13), np.arange(9, total, 17)
    x0[nan_rows, 0] = np.nan
    lb[swap_rows, 0], ub[swap_rows, 0] = ub[swap_rows, 0].copy(), lb[swap_rows, 0].copy()
    bad = np.zeros(total, bool)
    bad[nan_rows] = bad[swap_rows] = True
    qp = _solver(fam)
    out = qp.solve_batch(x0, lb, ub)
    qp.close()
    assert (out["status"][bad] == 2).all() and np.isnan(out["u"][bad]).all()
    good = {k: v[~bad] for k, v in out.items()}
    _assert_exact(good, fam["U"][src[~bad]], fam["act"][src[~bad]], "300 on 128 slots")
    for b in range(B):
        rows = np.flatnonzero(~bad & (src == b))
        assert rows.size >= 8
        u = out["u"][rows]
        assert np.abs(u - u[0]).max() <= 1e-12 * max(1.0, np.abs(u[0]).max()), b


def test_indefinite_hessian_is_refused_per_row(fam):
    """Unit diagonal, one negative eigenvalue: the handle is created (only the diagonal is checked); every row comes back within
    the budget with NNMPC_ST_NUMERIC -- chol_diag_k's non-positive pivot, as include/nnmpc.h documents it -- and a good handle
    created afterwards solves the family as before."""
    from industrial_nnmpc_2021_amd.qp import BatchedBoxQP
    P = H.pdip_indefinite()
    n = P.shape[0]
    rng = np.random.default_rng(2)
    tq = 0.1 * rng.standard_normal((n, 4))
    x0 = rng.standard_normal((12, 4))
    qp = BatchedBoxQP(P, tq, 2, max_batch=128, method="pdip", Kunc=None, max_rounds=30)
    t0 = time.perf_counter()
    out = qp.solve_batch(x0, -10.0 * np.ones(2), 10.0 * np.ones(2))
    dt = time.perf_counter() - t0
    stats = qp.stats()
    qp.close()
    print(f"\nindefinite P: status {out['status'].tolist()} rounds {stats['rounds']} in {dt:.2f} s")
    assert (out["status"] != 0).all(), out["status"]
    assert stats["rounds"] <= 30 + 2, stats["rounds"]                       # max_rounds = 30: within the budget
    assert (out["status"] == 2).all(), out["status"]
    qp = _solver(fam)
    again = qp.solve_batch(fam["x0"], fam["lb"], fam["ub"])
    qp.close()
    _assert_exact(again, fam["U"], fam["act"], "good handle after the indefinite one")
