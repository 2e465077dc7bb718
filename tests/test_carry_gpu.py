"""Carried multipliers (csrc/qp_asm.h: AsmDev::carry, asm_carry_copy).

Behind predicted first sets round 0 is a plain f32 screen and round 1 solves the sets that screen left unchanged once more, in f32
with one fp64 correction.  With the carry round 0 runs that correction too and keeps its result; round 1 copies it into the
problem's fp64 row instead of solving again.  The copy holds the very bits the second solve would have produced -- same kernel
instance, same inputs -- so NOTHING may differ from a run with NNMPC_CARRY=0: u, active sets, status, iteration counts and the
number of rounds are compared with np.array_equal, never with a tolerance.

Plant: mid_cdu (n = 1024, nu = 16), B = 4096 problems in one segment, never the tail-only path: the shape of
tests/test_predict_gpu.py, with its three kinds of box (ordinary, a tiny one whose set is beyond 176 bounds, a wide one whose set
is empty).  Sets of a chosen size: the family of tests/test_large_sets_gpu.py with the pushes inside the predictor's 512 columns.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers as H
from tests.helpers import batch_inputs

pytestmark = pytest.mark.gpu

B = 4096
KEYS = ("u", "active", "status", "ipm_iters", "factorizations")


@functools.lru_cache(maxsize=None)
def _mid():
    from industrial_nnmpc_2021_amd import synthetic
    from industrial_nnmpc_2021_amd.linearMPC_build import build_regulator_matrices
    pl = synthetic.plant("mid_cdu", 0)
    P, tq, nu = build_regulator_matrices(pl)
    return pl, P, tq, nu


@functools.lru_cache(maxsize=None)
def _batch(seed=3, sx=2.0, nprob=B):
    """The batch of tests/test_predict_gpu.py: ordinary boxes, a tiny one (row 7), a wide one (row 11)."""
    pl = _mid()[0]
    s, x0, lb, ub = batch_inputs(pl, nprob, seed, sx)
    if nprob == B:
        ub[7] = 0.02; lb[7] = -0.02
        lb[11] = -50.0; ub[11] = 50.0
    return x0, lb, ub


def _handle(**kw):
    from industrial_nnmpc_2021_amd.qp import BatchedBoxQP
    pl, P, tq, nu = _mid()
    return BatchedBoxQP(P, tq, nu, **{"max_batch": 1024, "seg_max": B, "asm_tail_batch": -1, **kw})


def _call(qp, x0, lb, ub):
    qp.stats(reset=True)
    out = qp.solve_batch(x0, lb, ub)
    out["stats"] = qp.stats()
    return out


def _carry(monkeypatch, on):
    """NNMPC_CARRY is read at every call."""
    if on:
        monkeypatch.delenv("NNMPC_CARRY", raising=False)
    else:
        monkeypatch.setenv("NNMPC_CARRY", "0")


def _assert_bit_equal(a, b, what=""):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))
    assert a["stats"]["asm_rounds"] == b["stats"]["asm_rounds"], (what, a["stats"]["asm_rounds"], b["stats"]["asm_rounds"])


def _flops(m):
    m = np.asarray(m, dtype=np.float64)
    return m ** 3 / 3.0 + 2.0 * m ** 2


@functools.lru_cache(maxsize=None)
def _on_off():
    """Carry on and NNMPC_CARRY=0 on one handle each (shared by the tests that need the pair; nobody writes to it)."""
    x0, lb, ub = _batch()
    out = {}
    old = os.environ.pop("NNMPC_CARRY", None)
    try:
        for tag in ("on", "off"):
            if tag == "off":
                os.environ["NNMPC_CARRY"] = "0"
            qp = _handle()
            out[tag] = _call(qp, x0, lb, ub)
            qp.close()
    finally:
        os.environ.pop("NNMPC_CARRY", None)
        if old is not None:
            os.environ["NNMPC_CARRY"] = old
    return out


def test_carry_on_equals_carry_off_bit_for_bit():
    out = _on_off()
    on, off = out["on"], out["off"]
    print("CARRY carried", on["stats"]["asm_carried"], "of", B, "rounds", on["stats"]["asm_rounds"], off["stats"]["asm_rounds"],
          "status", np.bincount(on["status"], minlength=4))
    _assert_bit_equal(on, off)
    assert (on["status"] == 0).all()
    assert off["stats"]["asm_carried"] == 0
    assert 0 < on["stats"]["asm_carried"] <= on["stats"]["problems"] == B
    assert on["status"][11] == 0 and not on["active"][11].any()          # the wide box: an empty set
    assert on["active"][7].sum() > 176                                    # the tiny box: beyond the classes that carry


def test_statistics_count_executed_factorisations_only():
    """asm_lambda32_flops falls by the carried problems' m^3 / 3 + 2 m^2.  Which problems were carried the library does not say;
    a carried problem's round-1 set is its delivered set unless a later round or the full-width pass moved it (a few in a
    thousand), so the sum over the asm_carried SMALLEST delivered non-empty sets of at most 176 bounds is a floor of the
    difference.  asm_lambda_flops (all precisions) falls by the same amount."""
    out = _on_off()
    on, off = out["on"], out["off"]
    K = on["stats"]["asm_carried"]
    m = on["active"].sum(axis=1)
    f = np.sort(_flops(m[(m > 0) & (m <= 176)]))
    floor = f[:K].sum()
    d32 = off["stats"]["asm_lambda32_flops"] - on["stats"]["asm_lambda32_flops"]
    d = off["stats"]["asm_lambda_flops"] - on["stats"]["asm_lambda_flops"]
    print(f"CARRY flops: f32 {on['stats']['asm_lambda32_flops']:.4e} (off {off['stats']['asm_lambda32_flops']:.4e}) difference {d32:.4e}, "
          f"all {d:.4e}, floor from the {K} smallest delivered sets {floor:.4e}")
    assert K > 0 and f.size >= K
    assert on["stats"]["asm_lambda32_flops"] < off["stats"]["asm_lambda32_flops"]
    assert d32 >= floor and d >= floor
    assert on["stats"]["asm_lambda_bytes"] < off["stats"]["asm_lambda_bytes"]


def test_predictor_off_nothing_is_carried(monkeypatch):
    x0, lb, ub = _batch()
    out = {}
    for tag in ("on", "off"):
        _carry(monkeypatch, tag == "on")
        qp = _handle(asm_predict_iters=-1)
        out[tag] = _call(qp, x0, lb, ub)
        qp.close()
    assert out["on"]["stats"]["asm_predict_launches"] == 0
    assert out["on"]["stats"]["asm_carried"] == 0 and out["off"]["stats"]["asm_carried"] == 0
    _assert_bit_equal(out["on"], out["off"])
    ref = _on_off()["on"]                                     # (the predictor changes the rounds, not the sets)
    assert np.array_equal(out["on"]["status"], ref["status"]) and np.array_equal(out["on"]["active"], ref["active"])


# ---- sets of a chosen size ------------------------------------------------------------------------------------------------------

N_, NU, PSEED, PRED_COLS = 1024, 8, 5, 512


def _leading_rows(P, seed, sizes):
    """tests/helpers.py: pushed_rows(exact=True) with the m pushed indices drawn inside the predictor's window (the leading 512
    columns), so that the predicted first set, the set of the f32 screen and the optimum's set all have exactly m bounds."""
    rng = np.random.default_rng(seed)
    n = P.shape[0]
    Ps = np.tril(P) + np.tril(P, -1).T
    lb, ub = -np.ones(NU), np.ones(NU)
    q = np.empty((len(sizes), n))
    state = np.zeros((len(sizes), n), np.uint8)
    for b, m in enumerate(sizes):
        base = 0.05 * rng.standard_normal(n)
        for attempt in range(50):
            xu, st = base.copy(), np.zeros(n, np.uint8)
            idx = rng.choice(PRED_COLS, int(m), replace=False)
            sgn = rng.choice([-1.0, 1.0], int(m))
            xu[idx] = sgn * rng.uniform(1.5, 3.0, int(m))
            st[idx] = np.where(sgn > 0, 1, 2)
            qb = -Ps @ xu
            x = H.solve_on_set(Ps, qb, lb, ub, st)
            g = Ps @ x + qb
            if np.abs(x[st == 0]).max(initial=0.0) <= 0.9 and (g[st == 1] < -1e-2).all() and (g[st == 2] > 1e-2).all():
                break
        else:
            raise RuntimeError(f"no exact row of {m} bounds in 50 draws")
        q[b], state[b] = qb, st
    return q, lb, ub, state


@pytest.fixture(scope="module")
def sized():
    """One handle of the large-set family (tq = I: q = x0), predictor on, lock-step rounds; solve(sizes, seed) -> (on, off, state)."""
    from industrial_nnmpc_2021_amd.qp import BatchedBoxQP
    P = H.large_set_hessian(N_, PSEED)
    qp = BatchedBoxQP(P, np.eye(N_), NU, max_batch=128, seg_max=4096, method="asm", asm_tail_batch=-1, asm_predict_iters=0)

    def solve(monkeypatch, sizes, seed):
        q, lb, ub, state = _leading_rows(P, seed, sizes)
        out = {}
        for tag in ("on", "off"):
            _carry(monkeypatch, tag == "on")
            out[tag] = _call(qp, q, lb, ub)
        return out["on"], out["off"], state
    yield solve
    qp.close()


def test_side_stream_classes_carry(sized, monkeypatch):
    """145 .. 176 bounds only: asm_lambda_reg32b_k on the side stream is the only kernel that can stash."""
    sizes = [145, 150, 160, 161, 170, 176] * 4
    on, off, state = sized(monkeypatch, sizes, 51)
    print("CARRY 145..176: carried", on["stats"]["asm_carried"], "of", len(sizes), "rounds", on["stats"]["asm_rounds"])
    assert on["stats"]["asm_predict_launches"] == 1
    assert (on["status"] == 0).all() and np.array_equal(on["active"], H.state_to_active(state, NU))
    _assert_bit_equal(on, off)
    assert 0 < on["stats"]["asm_carried"] <= len(sizes) and off["stats"]["asm_carried"] == 0


@pytest.mark.parametrize("size,carries", [(144, True), (145, True), (176, True), (177, False)])
def test_class_edge_and_edge_of_the_carry(sized, monkeypatch, size, carries):
    """144 / 145: the last set of the main kernel and the first of the side-stream one; 176 / 177: the last set that is corrected
    in registers and the first that keeps the f32 -> fp64 ladder (nothing to carry)."""
    sizes = [size] * 6
    on, off, state = sized(monkeypatch, sizes, 60 + size)
    print(f"CARRY size {size}: carried", on["stats"]["asm_carried"], "of", len(sizes), "rounds", on["stats"]["asm_rounds"])
    assert (on["status"] == 0).all() and np.array_equal(on["active"], H.state_to_active(state, NU))
    _assert_bit_equal(on, off)
    assert off["stats"]["asm_carried"] == 0
    assert (on["stats"]["asm_carried"] > 0) == carries, on["stats"]["asm_carried"]


# ---- nothing leaks from call to call ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first", ["batch", "tail_only"])
def test_no_leak_between_calls(first):
    """Two different batches one after the other on one handle, then the second on a fresh handle.  tail_only: the first call has
    64 problems and goes to the device tail from the start (asm_tail_batch left at its default).  Both handles get the far-field
    factors of every window before their first call: a handle otherwise adds the factors of the windows a call met afterwards,
    and its next call's full-width pass takes the factored form where a fresh handle's takes the dense one -- a difference of
    1e-13 in u beyond the window that has nothing to do with the carry (NNMPC_CARRY=0 shows it just the same)."""
    kw = {} if first == "batch" else {"asm_tail_batch": 0}
    xa = _batch(3, 2.0) if first == "batch" else _batch(5, 2.0, 64)
    xb = _batch(8, 2.5)

    def handle():
        qp = _handle(**kw)
        qp.prepare_farfield_windows(hi=N_ - 128)
        return qp
    qp = handle()
    one = _call(qp, *xa)
    two = _call(qp, *xb)
    qp.close()
    qp = handle()
    fresh = _call(qp, *xb)
    qp.close()
    assert (one["stats"]["asm_carried"] > 0) == (first == "batch")
    assert two["stats"]["asm_carried"] > 0 and two["stats"]["asm_carried"] == fresh["stats"]["asm_carried"]
    _assert_bit_equal(two, fresh, first)


# ---- beside a full-width pass -----------------------------------------------------------------------------------------------------

def test_carry_beside_a_pass(monkeypatch):
    """NNMPC_OVERLAP on / off x carry on / off on one handle whose second row space holds the whole batch (the test-only variable,
    as in tests/test_overlap_gpu.py), so that a round with carried problems fits the second view."""
    monkeypatch.setenv("NNMPC_OVERLAP_ROWS", str(B))          # (read when the handle is created)
    x0, lb, ub = _batch()
    qp = _handle(asm_overlap=0)
    qp.prepare_farfield_windows(hi=640)
    out = {}
    for ovl in (True, False):
        for car in (True, False):
            _carry(monkeypatch, car)
            if ovl:
                monkeypatch.delenv("NNMPC_OVERLAP", raising=False)
            else:
                monkeypatch.setenv("NNMPC_OVERLAP", "0")
            out[ovl, car] = _call(qp, x0, lb, ub)
    qp.close()
    for k, o in out.items():
        print("CARRY overlap, carry", k, "overlapped passes", o["stats"]["asm_overlapped_passes"], "carried", o["stats"]["asm_carried"],
              "rounds", o["stats"]["asm_rounds"])
    ref = out[False, False]
    for k, o in out.items():
        for key in KEYS:
            assert np.array_equal(o[key], ref[key]), (k, key)
        assert (o["stats"]["asm_carried"] > 0) == k[1] and (o["stats"]["asm_overlapped_passes"] > 0) == k[0], k
    assert out[True, True]["stats"]["asm_carried"] == out[False, True]["stats"]["asm_carried"]
    assert out[True, True]["stats"]["asm_rounds"] == out[True, False]["stats"]["asm_rounds"]
    assert out[False, True]["stats"]["asm_rounds"] == out[False, False]["stats"]["asm_rounds"]


# ---- rejected corrections -------------------------------------------------------------------------------------------------------

def test_rejected_corrections_in_a_child_process(tmp_path):
    """NNMPC_REFINE_TOL=1e-16 (read once per process: a fresh child) rejects every correction, carried or recomputed: both fail
    the same residual test and take the same fp64 round."""
    path = str(tmp_path / "carry_reject.npz")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NNMPC_REFINE_TOL="1e-16")
    env.pop("NNMPC_CARRY", None)
    subprocess.run([sys.executable, "-m", "tests.carry_worker", path], cwd=root, env=env, check=True, timeout=300)
    with np.load(path) as f:
        got = {k: f[k] for k in f.files}
    print("CARRY rejected: carried", got["carried_on"], got["carried_off"], "rounds", got["rounds_on"], got["rounds_off"])
    assert (got["status_on"] == 0).all() and (got["status_off"] == 0).all()
    assert np.array_equal(got["active_on"], got["active_off"])
    assert np.array_equal(got["u_on"], got["u_off"])
    assert got["carried_on"] > 0 and got["carried_off"] == 0 and got["rounds_on"] == got["rounds_off"]
    ref = _on_off()["on"]                                     # (the accepted corrections' answers: the same sets)
    assert np.array_equal(got["active_on"], ref["active"])
