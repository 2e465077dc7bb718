"""A second iteration beside the same full-width pass, in a third row space (csrc/qp_solver.hip: PassFifo, finish_passes and the
chain in the loop of solve_segment_asm; NNMPC_VIEWS, nnmpc_qp_stats.asm_shared_passes).

After a round that ran beside a pass the loop no longer joins that pass at once: the round's own pass queues behind it on the side
stream, the problems still running are counted in the view neither pass holds and run their next round (or the device tail) there,
and then both passes are finished in launch order.  As with the pass beside the round (tests/test_overlap_gpu.py) that changes the
ORDER of the work and nothing else: status, active sets and u* must equal the two-view order's (NNMPC_VIEWS=2) and the serial
order's (asm_overlap = -1) -- active sets bit for bit, |du| <= 1e-10 max(1, max|u|) --, the oracle's to 1e-8.

Plant and calls as in that file: mid_cdu (n = 1024, nu = 16, window 512 < n), B = 4096 problems in one segment, never the
tail-only path, far-field factors of every window up to 512.  At sx = 2 only ~55 problems still run after the round the bulk
settles in and go to the device tail at once (tail_max = 256); the chain "round beside pass 1, then a second iteration beside
the same pass" needs more than 256 of them: sx = SX.
"""
import functools

import numpy as np
import pytest

from tests.helpers import batch_inputs, oracle_box_rows
from tests.test_overlap_gpu import B, FAR_COL, FAR_GAIN, SAME_STATS, _assert_oracle, _assert_same, _call, _handle, _mid

pytestmark = pytest.mark.gpu

SX = 3.0
ORACLE_ROWS = (0, 1, 2, 3, 1000, 2047, 3000, B - 1)


@functools.lru_cache(maxsize=None)
def _batch(seed=3, sx=SX):
    pl, P, tq, nu = _mid()
    s, x0, lb, ub = batch_inputs(pl, B, seed, sx)
    return x0, lb, ub


@functools.lru_cache(maxsize=None)
def _oracle():
    """u* and active rows of ORACLE_ROWS of the sx = SX batch, computed once."""
    pl, P, tq, nu = _mid()
    x0, lb, ub = _batch()
    Ps = np.tril(P) + np.tril(P, -1).T
    return oracle_box_rows(Ps, tq, nu, pl["N"], x0, lb, ub, ORACLE_ROWS)


def _views(monkeypatch, three):
    if three:
        monkeypatch.delenv("NNMPC_VIEWS", raising=False)
    else:
        monkeypatch.setenv("NNMPC_VIEWS", "2")                # (read per call)


def _show(tag, o):
    s = o["stats"]
    print("VIEWS3", tag, "shared", s["asm_shared_passes"], "overlapped", s["asm_overlapped_passes"], "far passes", s["asm_far_passes"],
          "rounds", s["asm_rounds"], "gemm flops", s["asm_gemm_flops"])


@pytest.mark.parametrize("first_move_only", [False, True])
def test_three_view_order_equals_two_view_and_serial_order(monkeypatch, first_move_only):
    """Sequence calls and first-move calls (asm_wide_tnorm_k and the tile skip, twice on the side stream)."""
    pl, P, tq, nu = _mid()
    x0, lb, ub = _batch()
    n = P.shape[0]
    qp = _handle(P, tq, nu, True)
    _views(monkeypatch, True)
    three = _call(qp, x0, lb, ub, first_move_only)
    _views(monkeypatch, False)
    two = _call(qp, x0, lb, ub, first_move_only)
    _views(monkeypatch, True)
    qp.close()
    qp = _handle(P, tq, nu, False)
    serial = _call(qp, x0, lb, ub, first_move_only)
    qp.close()
    for tag, o in (("three", three), ("two", two), ("serial", serial)):
        _show(tag, o)
    assert three["stats"]["asm_shared_passes"] >= 1
    assert two["stats"]["asm_shared_passes"] == 0 and serial["stats"]["asm_shared_passes"] == 0
    assert two["stats"]["asm_overlapped_passes"] >= 1 and serial["stats"]["asm_overlapped_passes"] == 0
    _assert_same(three, two, "three views against two")
    _assert_same(three, serial, "three views against the serial order")
    assert three["stats"]["asm_solved"] == B
    for k in SAME_STATS:
        assert three["stats"][k] == two["stats"][k] == serial["stats"][k], (k, three["stats"][k], two["stats"][k], serial["stats"][k])
    ncol = three["u"].shape[1]
    for r, (xe, active) in zip(ORACLE_ROWS, _oracle()):
        ref = np.zeros(2 * n, bool)
        ref[active] = True
        assert np.abs(three["u"][r] - xe[:ncol]).max() <= 1e-8 * max(1.0, np.abs(xe).max()), r
        assert np.array_equal(three["active"][r], ref), r


def test_a_pass_of_a_chain_sends_problems_back(monkeypatch):
    """The re-entry construction of tests/test_overlap_gpu.py (a bound violated at column 981, beyond the window): the pass that
    finds it is the first of a chain here -- the stragglers' round and the iteration after it both ran beside it -- and the problems
    its asm_wide_k sends back must be found by the count after finish_passes."""
    monkeypatch.setenv("NNMPC_OVERLAP_ROWS", str(B))          # (read when the handle is created: both free views)
    pl, P, tq, nu = _mid()
    N = pl["N"]
    s, x0, lb, ub = batch_inputs(pl, B, 3, 2.0)
    v = np.random.default_rng(12).standard_normal(tq.shape[1])
    tq2 = tq.copy()
    tq2[FAR_COL] += FAR_GAIN * P[FAR_COL, FAR_COL] * v / np.linalg.norm(v)
    qp = _handle(P, tq2, nu, True)
    _views(monkeypatch, True)
    three = _call(qp, x0, lb, ub)
    _views(monkeypatch, False)
    two = _call(qp, x0, lb, ub)
    _views(monkeypatch, True)
    qp.close()
    qp = _handle(P, tq2, nu, False)
    serial = _call(qp, x0, lb, ub)
    qp.close()
    for tag, o in (("three", three), ("two", two), ("serial", serial)):
        _show("re-entry " + tag, o)
    assert three["stats"]["asm_shared_passes"] >= 1 and two["stats"]["asm_shared_passes"] == 0
    _assert_same(three, two, "three views against two")
    _assert_same(three, serial, "three views against the serial order")
    assert three["stats"]["asm_solved"] == B
    # the far bound can only have joined through a full-width pass: x_unc beyond column 512 never exists before one
    k, c = FAR_COL // nu, FAR_COL % nu
    far_active = three["active"][:, k * 2 * nu + c] | three["active"][:, k * 2 * nu + nu + c]
    reentered = np.flatnonzero(far_active)
    assert reentered.size >= 1
    rows = list(reentered[:2]) + [r for r in (0, 1, 2, 3) if r not in reentered[:2]][:2]
    _assert_oracle(three, P, tq2, nu, N, x0, lb, ub, rows)


def test_free_views_too_small_fall_back(monkeypatch):
    """NNMPC_OVERLAP_ROWS=128: the counts beside the passes find more problems than a free view has rows -- the passes are finished
    and the count repeated in view 0.  Same outputs as with the default views."""
    pl, P, tq, nu = _mid()
    x0, lb, ub = _batch()
    qp = _handle(P, tq, nu, True)
    full = _call(qp, x0, lb, ub)
    qp.close()
    monkeypatch.setenv("NNMPC_OVERLAP_ROWS", "128")           # (tests only; read when the handle is created)
    qp = _handle(P, tq, nu, True)
    tiny = _call(qp, x0, lb, ub)
    qp.close()
    monkeypatch.delenv("NNMPC_OVERLAP_ROWS")
    _show("full", full)
    _show("tiny", tiny)
    # (a chain starts with a ROUND beside a pass; from round 2 on a round has more than tail_max = 256 problems, which 128 rows cannot
    # hold, and rounds 0 and 1 hold the whole batch: no chain with the tiny views)
    assert full["stats"]["asm_shared_passes"] >= 1 and tiny["stats"]["asm_shared_passes"] == 0
    _assert_same(tiny, full)
    assert np.array_equal(tiny["u"], full["u"])
    for k in SAME_STATS:
        assert tiny["stats"][k] == full["stats"][k], (k, tiny["stats"][k], full["stats"][k])


def test_second_call_on_one_handle_equals_a_fresh_handle():
    """No event, counter or multiplier row is left over from the passes of the first call: a second, different batch on the same
    handle gives what a fresh handle gives, and chains as a fresh handle's call does."""
    pl, P, tq, nu = _mid()
    x0a, lba, uba = _batch()
    x0b, lbb, ubb = _batch(8, SX + 0.5)
    qp = _handle(P, tq, nu, True)
    first = _call(qp, x0a, lba, uba)
    second = _call(qp, x0b, lbb, ubb)
    qp.close()
    qp = _handle(P, tq, nu, True)
    fresh = _call(qp, x0b, lbb, ubb)
    qp.close()
    _show("first", first)
    _show("second", second)
    _show("fresh", fresh)
    assert first["stats"]["asm_shared_passes"] >= 1 and second["stats"]["asm_shared_passes"] >= 1
    _assert_same(second, fresh)
    assert np.array_equal(second["u"], fresh["u"])
    for k in SAME_STATS + ("asm_shared_passes", "asm_overlapped_passes", "asm_rounds"):
        assert second["stats"][k] == fresh["stats"][k], (k, second["stats"][k], fresh["stats"][k])


def test_carry_and_views_commute(monkeypatch):
    """Carry on / off x three views on / off on one handle: the same outputs bit for bit (the carry's flags live from round 0 to
    round 1; the chain starts after round 1 at the earliest), the same carried problems whatever the order."""
    pl, P, tq, nu = _mid()
    x0, lb, ub = _batch()
    qp = _handle(P, tq, nu, True)
    out = {}
    for three in (True, False):
        for car in (True, False):
            _views(monkeypatch, three)
            if car:
                monkeypatch.delenv("NNMPC_CARRY", raising=False)
            else:
                monkeypatch.setenv("NNMPC_CARRY", "0")
            out[three, car] = _call(qp, x0, lb, ub)
    qp.close()
    ref = out[False, False]
    for k, o in out.items():
        _show("views3, carry %s" % (k,), o)
        assert (o["status"] == 0).all(), k
        for key in ("u", "active", "status"):
            assert np.array_equal(o[key], ref[key]), (k, key)
        assert (o["stats"]["asm_carried"] > 0) == k[1] and (o["stats"]["asm_shared_passes"] > 0) == k[0], k
    assert out[True, True]["stats"]["asm_carried"] == out[False, True]["stats"]["asm_carried"]
    assert out[True, True]["stats"]["asm_rounds"] == out[False, True]["stats"]["asm_rounds"]
