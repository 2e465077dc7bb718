"""Bound multipliers through nnmpc_qp_solve_batch_dual and the Python layers (BatchedBoxQP, DenseQPRegulator, cvxopt_shim).

On the four golden plants (tests/golden/regulator_<case>.npz, qp_exact_<case>.npz), for method auto / pdip / asm on a handle each
(nnmpc_qp_get_stats says which path ran), and once more with the device tail taking the whole call:
  * mult against mult_ref (np.longdouble) on the DELIVERED u and active set, row by row within
    2 (n + n_aug + 2) 2^-53 (|P_i| |u| + |tq_i| |x0|) -- the bound of a dot product in any order, derived, not chosen;
  * active sets equal to the golden ones; with the reference's own P, q, G, h: |P v + q + G'z| below that bound plus
    |P_i|_1 max|u - u*| (u* from the golden file; v recovered from the delivered sequence as DenseQPRegulator's box form defines
    it), every z >= minus the same quantity, s = h - G v >= -bound_tol, z = 0 on the free rows;
  * the shim's "s" and "z" for one stable and one unstable problem against the same quantities.
Structural cases (inputs checked on the CPU by tests/test_cpu_mult_inputs.py): no bound active -> mult exactly zero; every variable
held (n = 21) -> all status 0, every multiplier within its bound of mult_ref and >= -bound; a NaN in one row's x0 -> that mult row
NaN, the neighbours' bytes unchanged; first_move_only with multipliers -> ValueError / NNMPC_EINVAL; and nnmpc_qp_solve_batch_dual
returns u, active, status, iters byte-identical to nnmpc_qp_solve_batch_ex on the same handle, cold and with a guess.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import mult_helpers as M

pytestmark = pytest.mark.gpu

BOUND_TOL = 1e-9                      # nnmpc_qp_opts.bound_tol, the default
_RUNS = {}


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def golden_run(golden_dir, case, method):
    """One solve of the six golden problems of `case` with multipliers, on a handle of its own; shared by the tests."""
    if (case, method) not in _RUNS:
        g, e = _load(golden_dir, f"regulator_{case}.npz"), _load(golden_dir, f"qp_exact_{case}.npz")
        reg = M.golden_regulator(g, max_batch=128, solver_options=dict(method=method))
        X0, lb, ub = M.golden_box_inputs(g)
        qp = reg._solver()
        qp.stats(reset=True)
        U, info = reg.solve_batch(X0, ulb=lb, uub=ub, multipliers=True)
        stats = qp.stats()
        Pb, tqb = reg._box_form()
        _RUNS[(case, method)] = dict(g=g, e=e, reg=reg, X0=X0, U=U, info=info, stats=stats,
                                     Pb=np.tril(Pb) + np.tril(Pb, -1).T, tqb=tqb)
        qp.close()
    return _RUNS[(case, method)]


def check_against_mult_ref(qp_n_nu, Pb, tqb, X0, U, active_rows, mult, label):
    n, nu = qp_n_nu
    words = M.pack_rows(active_rows, n)
    ref = M.mult_ref(Pb, tqb, X0, U, words, nu)
    bound = M.mult_bound(Pb, tqb, X0, U)
    err = np.abs(mult.astype(np.longdouble) - ref)
    print(f"{label}: {int(active_rows.sum())} active bounds, max |mult - ref| / bound = {float((err / bound).max()):.3g}, "
          f"min mult / bound = {float((mult / bound).min()):.3g}")
    assert (err <= bound).all()
    assert (mult[M.sides(words, n, nu) == 0].view(np.uint64) == 0).all()       # free: +0.0
    return bound


def reference_checks(r, v, z, active_rows, rows, label):
    """The reference's own KKT system for problems `rows`: v (len(rows), n), z (len(rows), 2n)."""
    g, e, reg = r["g"], r["e"], r["reg"]
    sub = {k: g[k][rows] for k in ("q", "h")}
    X0 = r["X0"][rows]
    w = M.sequence_of_v(reg, v, X0)
    w_star = M.sequence_of_v(reg, e["v"][rows], X0)
    bound = M.mult_bound(r["Pb"], r["tqb"], X0, w)
    dw = np.abs(w - w_star).max(axis=1, keepdims=True)
    tol = bound + np.abs(r["Pb"]).sum(axis=1)[None, :].astype(np.longdouble) * dw           # row by row
    res = M.reference_kkt(dict(P=g["P"], q=sub["q"], G=g["G"]), v, z)
    print(f"{label}: max |P v + q + G'z| / tol = {float((np.abs(res) / tol).max()):.3g}, max |u - u*| = {float(dw.max()):.3g}")
    assert (np.abs(res) <= tol).all()
    up, lo = M.row_index(v.shape[1], reg.Nu)
    assert (z[:, up] >= -tol).all() and (z[:, lo] >= -tol).all()
    assert (z[~active_rows] == 0).all()                                         # z s = 0 on the free rows by construction
    s = sub["h"][:, :, 0] - v @ g["G"].T
    assert (s >= -BOUND_TOL).all()
    return s


@pytest.mark.parametrize("method", ["auto", "pdip", "asm"])
@pytest.mark.parametrize("case", M.GOLDEN_CASES)
def test_golden_plants_every_method(golden_dir, case, method):
    r = golden_run(golden_dir, case, method)
    reg, info, st, B = r["reg"], r["info"], r["stats"], r["X0"].shape[0]
    n = r["Pb"].shape[0]
    assert n <= 704                                                             # the small-problem kernel takes these shapes
    print(case, method, {k: st[k] for k in ("problems", "asm_solved", "asm_small_passes", "asm_rounds", "ipm_iterations", "factorizations")})
    assert (info["status"] == 0).all()
    assert st["problems"] == B
    if method == "pdip":
        assert st["ipm_iterations"] > 0 and st["asm_solved"] == 0 and st["asm_small_passes"] == 0
    elif method == "asm":
        assert st["asm_solved"] == B and st["asm_small_passes"] == 1 and st["ipm_iterations"] == 0
    else:
        # the active-set pass first; what it leaves (nothing, on these plants) shows as PDIP iterations
        assert st["asm_small_passes"] == 1 and st["asm_solved"] > 0 and (st["asm_solved"] == B or st["ipm_iterations"] > 0)
    assert np.array_equal(info["active"], r["e"]["active"])
    assert info["mult"].shape == (B, n) and info["z"].shape == (B, 2 * n)
    check_against_mult_ref((n, reg.Nu), r["Pb"], r["tqb"], r["X0"], r["U"], info["active"], info["mult"], f"{case} {method}")
    assert np.array_equal(info["z"], M.z_rows(info["mult"], info["active"], reg.Nu))
    v = M.v_of_sequence(reg, r["U"], r["X0"])
    reference_checks(r, v, info["z"], info["active"], np.arange(B), f"{case} {method}")


def test_device_tail_takes_the_whole_call(golden_dir, monkeypatch):
    """A batch of at most 256 problems with the small-problem kernel switched off: asm_tail_k from the first set to the end."""
    monkeypatch.setenv("NNMPC_NO_SMALL", "1")
    g, e = _load(golden_dir, "regulator_stable_s0.npz"), _load(golden_dir, "qp_exact_stable_s0.npz")
    reg = M.golden_regulator(g, max_batch=128, solver_options=dict(method="asm"))
    X0, lb, ub = M.golden_box_inputs(g)
    qp = reg._solver()
    qp.stats(reset=True)
    U, info = reg.solve_batch(X0, ulb=lb, uub=ub, multipliers=True)
    st = qp.stats()
    qp.close()
    print({k: st[k] for k in ("problems", "asm_solved", "asm_small_passes", "asm_rounds", "ipm_iterations")})
    assert (info["status"] == 0).all() and X0.shape[0] <= 256
    # (tail_only_pass counts itself as the call's one round; no lock-step round, no small pass, nothing left for the PDIP path)
    assert st["asm_small_passes"] == 0 and st["asm_rounds"] == 1 and st["asm_solved"] == X0.shape[0] and st["ipm_iterations"] == 0
    assert np.array_equal(info["active"], e["active"])
    Pb, tqb = reg._box_form()
    check_against_mult_ref((Pb.shape[0], reg.Nu), np.tril(Pb) + np.tril(Pb, -1).T, tqb, X0, U, info["active"], info["mult"], "tail")


@pytest.mark.parametrize("case", ["stable_s1", "unstable_s0"])
def test_shim_returns_s_and_z(golden_dir, case):
    from industrial_nnmpc_2021_amd import cvxopt_shim as cvx
    r = golden_run(golden_dir, case, "auto")
    g, e = r["g"], r["e"]
    n = g["P"].shape[0]
    b = 0
    sol = cvx.solvers.qp(*[cvx.matrix(a) for a in (g["P"], g["q"][b], g["G"], g["h"][b])])
    x, s, z = (np.asarray(sol[k]) for k in ("x", "s", "z"))
    assert sol["status"] == "optimal" and x.shape == (n, 1) and s.shape == (2 * n, 1) and z.shape == (2 * n, 1)
    active = e["active"][b:b + 1]
    assert np.array_equal(z[:, 0] != 0, active[0] & (z[:, 0] != 0))
    s_ref = reference_checks(r, x.T, z.T, active, np.array([b]), f"shim {case}")
    # s = h - G x: two fp64 evaluations of a row of n + 1 terms, each within (n + 2) 2^-53 (|h| + |G| |x|) of the exact value
    assert (np.abs(s[:, 0] - s_ref[0]) <= 2 * (n + 2) * 2.0 ** -53 * (np.abs(g["h"][b][:, 0]) + np.abs(g["G"]) @ np.abs(x[:, 0]))).all()


@pytest.fixture(scope="module")
def structural():
    from industrial_nnmpc_2021_amd.qp import BatchedBoxQP
    s = M.structural_problem()
    qp = BatchedBoxQP(s["P"], s["tq"], s["nu"], max_batch=128, seg_max=128)
    yield s, qp
    qp.close()


def test_all_free_gives_exact_zeros(structural):
    s, qp = structural
    out = qp.solve_batch(s["x0"], *s["free"], multipliers=True)
    assert (out["status"] == 0).all() and not out["active"].any()
    assert (out["mult"].view(np.uint64) == 0).all()


def test_all_held_and_a_bad_row(structural):
    s, qp = structural
    n, B = qp.n, s["x0"].shape[0]
    out = qp.solve_batch(s["x0"], *s["held"], multipliers=True)
    assert (out["status"] == 0).all()                                           # all of them, no share left out
    assert (out["active"].sum(axis=1) == n).all()
    bound = check_against_mult_ref((n, qp.nu), s["P"], s["tq"], s["x0"], out["u"], out["active"], out["mult"], "all held")
    assert (out["mult"] >= -bound).all() and (out["mult"] > 0).all()
    # the stand-alone call on what was delivered: the same bytes
    assert same_bits(qp.multipliers(s["x0"], out["u"], qp.active_to_words(out["active"]), out["status"]), out["mult"])
    x0 = s["x0"].copy()
    x0[3, 1] = np.nan
    out2 = qp.solve_batch(x0, *s["held"], multipliers=True)
    assert out2["status"][3] == 2 and np.isnan(out2["mult"][3]).all()
    keep = np.arange(B) != 3
    assert (out2["status"][keep] == 0).all()
    assert same_bits(out2["mult"][keep], out["mult"][keep]) and same_bits(out2["u"][keep], out["u"][keep])


def test_first_move_with_multipliers_is_refused(structural):
    from industrial_nnmpc_2021_amd import _lib
    s, qp = structural
    with pytest.raises(ValueError):
        qp.solve_batch(s["x0"], *s["held"], first_move_only=True, multipliers=True)
    B = s["x0"].shape[0]
    u, mult = np.full((B, qp.nu), 5.0), np.full((B, qp.n), 5.0)
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    lb, ub = (np.ascontiguousarray(a) for a in s["held"])
    rc = qp._lib.nnmpc_qp_solve_batch_dual(qp._h, B, p(s["x0"]), p(lb), p(ub), None, p(u), None, None, None, p(mult), _lib.HOST,
                                           _lib.OUT_FIRST_MOVE)
    assert rc == _lib.EINVAL and b"FIRST_MOVE" in qp._lib.nnmpc_last_error()
    assert (u == 5.0).all() and (mult == 5.0).all()                             # nothing written
    # without mult it is nnmpc_qp_solve_batch_ex: the first moves
    assert qp._lib.nnmpc_qp_solve_batch_dual(qp._h, B, p(s["x0"]), p(lb), p(ub), None, p(u), None, None, None, None, _lib.HOST,
                                             _lib.OUT_FIRST_MOVE) == 0
    assert same_bits(u, qp.solve_batch(s["x0"], lb, ub, first_move_only=True)["u"])


def _call(qp, fn, x0, lb, ub, guess, mult):
    from industrial_nnmpc_2021_amd import _lib
    B = x0.shape[0]
    u, act = np.full((B, qp.n), 9.0), np.full((B, qp.words), 0xFFFFFFFF, np.uint32)
    st, it = np.full(B, 9, np.int32), np.full((B, 2), 9, np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    if fn == "ex":
        rc = qp._lib.nnmpc_qp_solve_batch_ex(qp._h, B, p(x0), p(lb), p(ub), p(guess), p(u), p(act), p(st), p(it), _lib.HOST, _lib.OUT_SEQUENCE)
    else:
        rc = qp._lib.nnmpc_qp_solve_batch_dual(qp._h, B, p(x0), p(lb), p(ub), p(guess), p(u), p(act), p(st), p(it), p(mult), _lib.HOST,
                                               _lib.OUT_SEQUENCE)
    assert rc == 0
    return u, act, st, it


def test_dual_is_byte_identical_to_ex(structural):
    from industrial_nnmpc_2021_amd import _lib
    s, qp = structural
    B = s["x0"].shape[0]
    x0 = np.ascontiguousarray(s["x0"])
    # half of the rows held, half with a box a few bounds of which are active
    lb = np.ascontiguousarray(np.where(np.arange(B)[:, None] % 2 == 0, s["held"][0], -5.0))
    ub = np.ascontiguousarray(np.where(np.arange(B)[:, None] % 2 == 0, s["held"][1], 5.0))
    cold = _call(qp, "ex", x0, lb, ub, None, None)
    assert (cold[2] == 0).all()
    bits = M.unpack_words(cold[1], qp.n)
    assert 0 < bits[1::2].sum() < (B // 2) * qp.n                               # the wide box: some bounds active, not all
    guess = np.ascontiguousarray(qp.active_to_state(bits))
    for g in (None, guess):
        ex = _call(qp, "ex", x0, lb, ub, g, None)
        mult = np.full((B, qp.n), 9.0)
        du = _call(qp, "dual", x0, lb, ub, g, mult)
        for a, b, what in zip(ex, du, ("u", "active", "status", "iters")):
            assert same_bits(a, b), (what, g is not None)
        assert not (mult == 9.0).any()
        assert same_bits(mult, qp.multipliers(x0, du[0], du[1], du[2]))
        nomult = _call(qp, "dual", x0, lb, ub, g, None)                        # mult = NULL behaves as _ex
        for a, b in zip(ex, nomult):
            assert same_bits(a, b)
        if g is None:
            # device buffers, active and status not asked for: the library keeps the words itself
            D = _lib.DeviceArray
            dx, dl, db = D.from_host(x0), D.from_host(lb), D.from_host(ub)
            du_, dm = D((B, qp.n), np.float64), D.from_host(np.full((B, qp.n), 9.0))
            qp.solve_batch_device(B, dx, dl, db, du_, mult=dm)
            assert same_bits(du_.to_host(), ex[0]) and same_bits(dm.to_host(), mult)
            for d in (dx, dl, db, du_, dm):
                d.free()
