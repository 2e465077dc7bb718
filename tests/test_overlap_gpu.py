"""The full-width pass beside the round (csrc/qp_solver.hip: launch_pass / finish_pass in the loop of solve_segment_asm; opts.asm_overlap).

A far-field full-width pass runs on a side stream while the problems that did not settle run their next round (or the device
tail) in a second, small row space.  That changes the ORDER of the work and nothing else: status, active sets and u* must equal the
serial order's (active sets bit for bit, |du| <= 1e-10 max(1, max|u|), as in test_predict_gpu.py), the oracle's to 1e-8.

Plant: mid_cdu (n = 1024, nu = 16: the predictor's window of 512 columns is below n, the far-field pass has four column tiles),
B = 4096 problems in one segment, never the tail-only path, far-field factors of every window up to 512 prepared before the calls.
"""
import functools

import numpy as np
import pytest

from tests.helpers import batch_inputs, oracle_box_rows

pytestmark = pytest.mark.gpu

B = 4096
# statistics of a call that must not depend on the order when no problem re-entered the rounds from a pass
SAME_STATS = ("asm_gemm_flops", "asm_far_passes", "asm_solved", "asm_full_checks", "problems")


@functools.lru_cache(maxsize=None)
def _mid():
    from industrial_nnmpc_2021_amd import synthetic
    from industrial_nnmpc_2021_amd.linearMPC_build import build_regulator_matrices
    pl = synthetic.plant("mid_cdu", 0)
    P, tq, nu = build_regulator_matrices(pl)
    return pl, P, tq, nu


def _handle(P, tq, nu, overlap, **kw):
    from industrial_nnmpc_2021_amd.qp import BatchedBoxQP
    qp = BatchedBoxQP(P, tq, nu, max_batch=1024, seg_max=B, asm_tail_batch=-1, asm_overlap=0 if overlap else -1, **kw)
    qp.prepare_farfield_windows(hi=512)
    qp.set_profiling(True)                                    # (the flop statistics are only kept with profiling on)
    return qp


def _call(qp, x0, lb, ub, first_move_only=False):
    qp.stats(reset=True)
    out = qp.solve_batch(x0, lb, ub, first_move_only=first_move_only)
    out["stats"] = qp.stats()
    return out


def _assert_same(on, off, what=""):
    assert (on["status"] == 0).all() and (off["status"] == 0).all(), what
    assert np.array_equal(on["active"], off["active"]), what
    assert np.abs(on["u"] - off["u"]).max() <= 1e-10 * max(1.0, np.abs(off["u"]).max()), what


def _assert_oracle(out, P, tq, nu, N, x0, lb, ub, rows):
    n = P.shape[0]
    Ps = np.tril(P) + np.tril(P, -1).T
    for r, (xe, active) in zip(rows, oracle_box_rows(Ps, tq, nu, N, x0, lb, ub, rows)):
        ref = np.zeros(2 * n, bool)
        ref[active] = True
        assert np.abs(out["u"][r] - xe).max() <= 1e-8 * max(1.0, np.abs(xe).max()), r
        assert np.array_equal(out["active"][r], ref), r


@pytest.mark.parametrize("first_move_only", [False, True])
def test_overlapped_order_equals_serial_order(first_move_only):
    """sx = 2: the bulk settles in round 1, the stragglers' round 2 and their tail run beside the passes.  Sequence calls, and
    first-move calls (asm_wide_tnorm_k and the tile skip on the side stream)."""
    pl, P, tq, nu = _mid()
    s, x0, lb, ub = batch_inputs(pl, B, 3, 2.0)
    out = {}
    for tag in ("on", "off"):
        qp = _handle(P, tq, nu, tag == "on")
        out[tag] = _call(qp, x0, lb, ub, first_move_only)
        qp.close()
    _assert_same(out["on"], out["off"])
    son, soff = out["on"]["stats"], out["off"]["stats"]
    print("overlapped passes", son["asm_overlapped_passes"], "far passes", son["asm_far_passes"], "rounds", son["asm_rounds"], soff["asm_rounds"])
    assert son["asm_overlapped_passes"] >= 1 and soff["asm_overlapped_passes"] == 0
    assert son["asm_solved"] == B
    for k in SAME_STATS:
        assert son[k] == soff[k], (k, son[k], soff[k])


def test_environment_switch_turns_the_overlap_off(monkeypatch):
    """NNMPC_OVERLAP=0 (A/B runs of an untouched benchmark) is read per call."""
    pl, P, tq, nu = _mid()
    s, x0, lb, ub = batch_inputs(pl, B, 3, 2.0)
    qp = _handle(P, tq, nu, True)
    on = _call(qp, x0, lb, ub)
    monkeypatch.setenv("NNMPC_OVERLAP", "0")
    off = _call(qp, x0, lb, ub)
    monkeypatch.delenv("NNMPC_OVERLAP")
    again = _call(qp, x0, lb, ub)
    qp.close()
    assert on["stats"]["asm_overlapped_passes"] >= 1 and off["stats"]["asm_overlapped_passes"] == 0
    assert again["stats"]["asm_overlapped_passes"] == on["stats"]["asm_overlapped_passes"]
    _assert_same(on, off)
    _assert_same(again, off)


FAR_COL = 61 * 16 + 5             # input 5 of stage 61: column 981 of 1024
FAR_GAIN = 0.025


def test_problems_sent_back_by_a_pass_that_ran_beside_a_round(monkeypatch):
    """Re-entry: asm_wide_k finds a bound violated beyond column 512 and sends the problem back to ASM_RUN after the overlapped
    round has run; the next iteration's count must pick it up.

    No sx of this plant gives such rows: x_unc decays along the horizon (sx = 1 .. 20: the last violated column is 119 .. 279, and
    no x0 at all that keeps columns 0 .. 511 inside the box moves a column >= 512 by more than 2e-4).  The nearest case that does
    keeps the plant, its Hessian and the sx = 2 batch of the other tests and adds a linear term on one late input -- row 981 of tq
    gets FAR_GAIN P[981, 981] v', v a fixed unit vector -- which the numpy count below puts beyond its bound in x_unc for 0.1 % ..
    5 % of the rows (FAR_GAIN = 0.025: 57 rows of 4096, 1.4 %; 0.02: 18 rows, 0.04: 301).  Those rows look like any other inside
    the window.  They settle with the bulk in the first fp64 round, when a good part of the 4096 problems is still running: the
    second row space gets 4096 rows here (the test-only variable) so that this pass, the only one of the call -- a set that reaches
    column 981 makes the window all columns -- runs beside their round."""
    monkeypatch.setenv("NNMPC_OVERLAP_ROWS", str(B))          # (read when the handle is created)
    pl, P, tq, nu = _mid()
    N, n = pl["N"], P.shape[0]
    s, x0, lb, ub = batch_inputs(pl, B, 3, 2.0)
    v = np.random.default_rng(12).standard_normal(tq.shape[1])
    tq2 = tq.copy()
    tq2[FAR_COL] += FAR_GAIN * P[FAR_COL, FAR_COL] * v / np.linalg.norm(v)
    import scipy.linalg as sla
    Ps = np.tril(P) + np.tril(P, -1).T
    xu = -x0 @ sla.cho_solve(sla.cho_factor(Ps, lower=True), tq2).T
    viol = (xu > np.tile(ub, (1, N)) + 1e-9) | (xu < np.tile(lb, (1, N)) - 1e-9)
    far = np.flatnonzero(viol[:, 512:].any(axis=1))
    print("rows with an x_unc-violated bound at a column >= 512:", far.size, "of", B)
    assert 0.001 * B <= far.size <= 0.05 * B, far.size
    out = {}
    for tag in ("on", "off"):
        qp = _handle(P, tq2, nu, tag == "on")
        out[tag] = _call(qp, x0, lb, ub)
        qp.close()
    _assert_same(out["on"], out["off"])
    son = out["on"]["stats"]
    print("overlapped passes", son["asm_overlapped_passes"], "far passes", son["asm_far_passes"], "rounds", son["asm_rounds"], out["off"]["stats"]["asm_rounds"])
    assert son["asm_overlapped_passes"] >= 1 and son["asm_solved"] == B
    # the far bound can only have joined through a full-width pass: x_unc beyond column 512 never exists before one
    k, c = FAR_COL // nu, FAR_COL % nu
    far_active = out["on"]["active"][:, k * 2 * nu + c] | out["on"]["active"][:, k * 2 * nu + nu + c]
    reentered = far[far_active[far]]
    assert reentered.size >= 1
    rows = list(reentered[:2]) + [r for r in (0, 1, 2, 3) if r not in reentered[:2]][:2]
    _assert_oracle(out["on"], P, tq2, nu, N, x0, lb, ub, rows)


def test_rounds_too_large_for_the_second_row_space_fall_back(monkeypatch):
    """Predictor off: the first sets are the bounds x_unc violates, the rounds are many, and while most problems still run the
    early passes find more of them than the second row space has rows (1024 here): they keep the serial order, only the late
    rounds run beside their pass.  A handle whose second row space is forced down to 128 rows declines more often, one without it
    always; all give the serial order's answers."""
    pl, P, tq, nu = _mid()
    s, x0, lb, ub = batch_inputs(pl, B, 3, 2.0)
    qp = _handle(P, tq, nu, False, asm_predict_iters=-1)
    off = _call(qp, x0, lb, ub)
    qp.close()
    qp = _handle(P, tq, nu, True, asm_predict_iters=-1)
    on = _call(qp, x0, lb, ub)
    qp.close()
    monkeypatch.setenv("NNMPC_OVERLAP_ROWS", "128")           # (tests only; read when the handle is created)
    qp = _handle(P, tq, nu, True, asm_predict_iters=-1)
    tiny = _call(qp, x0, lb, ub)
    qp.close()
    monkeypatch.setenv("NNMPC_OVERLAP_ROWS", "0")
    qp = _handle(P, tq, nu, True, asm_predict_iters=-1)
    none = _call(qp, x0, lb, ub)
    qp.close()
    monkeypatch.delenv("NNMPC_OVERLAP_ROWS")
    for tag, o in (("on", on), ("tiny", tiny), ("none", none)):
        print(tag, "overlapped passes", o["stats"]["asm_overlapped_passes"], "far passes", o["stats"]["asm_far_passes"], "rounds", o["stats"]["asm_rounds"])
        _assert_same(o, off, tag)
        assert o["stats"]["asm_solved"] == B
    assert 1 <= on["stats"]["asm_overlapped_passes"] < on["stats"]["asm_far_passes"]
    assert tiny["stats"]["asm_overlapped_passes"] <= on["stats"]["asm_overlapped_passes"]
    assert tiny["stats"]["asm_overlapped_passes"] < tiny["stats"]["asm_far_passes"]
    assert none["stats"]["asm_overlapped_passes"] == 0 and off["stats"]["asm_overlapped_passes"] == 0


def test_second_call_on_one_handle_equals_a_fresh_handle():
    """The rows of LAM of the second row space are back to zero after a call: a second, different batch on the same handle gives
    what a fresh handle gives (a stale multiplier would enter the next round's GEMM)."""
    pl, P, tq, nu = _mid()
    s, x0a, lba, uba = batch_inputs(pl, B, 3, 2.0)
    s, x0b, lbb, ubb = batch_inputs(pl, B, 8, 2.5)
    qp = _handle(P, tq, nu, True)
    first = _call(qp, x0a, lba, uba)
    second = _call(qp, x0b, lbb, ubb)
    qp.close()
    qp = _handle(P, tq, nu, True)
    fresh = _call(qp, x0b, lbb, ubb)
    qp.close()
    assert first["stats"]["asm_overlapped_passes"] >= 1 and second["stats"]["asm_overlapped_passes"] >= 1
    _assert_same(second, fresh)
