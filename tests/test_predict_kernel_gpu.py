"""The first-set predictor's kernels (csrc/qp_predict.h) alone, through nnmpc_qp_debug_predict, against an emulation in numpy.

No result of a solve depends on what the predictor computes -- every answer is an fp64 solve on its final set that passed the
certificate -- so the tests of the solves cannot see a predictor that is subtly wrong.  Here the bound states asm_predict_k writes
are compared ENTRY BY ENTRY with helpers.pred_reference (the kernel's storage roundings, fp64 arithmetic): on every entry whose w
lies further than PRED_TAU max(1, max|w| of the row) from a bound the states must be equal.  Cases a .. i (helpers.PRED_CASES) are
the smallest shapes that reach every instance and every path inside them; batches of 1, MR - 1, MR + 1 (special rows, a ragged
second group of clones), 2 MR + 2 (three groups of different difficulty) and 2 (tight boxes: the adaptive count above its floor);
1, 2, 3, 8, 24 and 64 iterations and the adaptive count.  Pairs listed in helpers.PRED_FALLBACK are ALSO (for "variants" / "rsum":
ONLY) compared by the quality of the sets they name; tests/test_cpu_predict_inputs.py holds the inputs and the list to their
conditions.  profiles/predict_coverage.md has the figures of one run and the seeded defects these tests catch.
"""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

WINDOWS = H.pred_windows()
_RUNS = {}


def _handle(c, **kw):
    from industrial_nnmpc_2021_amd.qp import BatchedBoxQP
    return BatchedBoxQP(c["P"], c["tq"], c["nu"], max_batch=128, seg_max=256, **kw)


def run(name, wide):
    """One handle per window: the kernel's states of every batch and count, and the reference of the same."""
    if (name, wide) not in _RUNS:
        c = H.pred_case(name)
        W, MR = H.pred_instance(c["nu"], wide)
        qp = _handle(c)
        got, info = {}, None
        for tag, (x0, lb, ub) in H.pred_batches(c, MR).items():
            for k in H.PRED_COUNTS:
                out = qp.debug_predict(x0, lb, ub, iters=k, wide=wide)
                got[(tag, k)] = out["state"]
                info = {a: out[a] for a in ("W", "MR", "count", "wide", "L")}
                assert info == dict(W=W, MR=MR, count=-1, wide=wide, L=info["L"])
        qp.close()
        L = info["L"]
        _RUNS[(name, wide)] = dict(c=c, W=W, MR=MR, L=L, got=got, r64=H.pred_references(c, wide, L),
                                   r32=H.pred_references(c, wide, L, "f32", batches=(H.PRED_QUALITY_BATCH,)))
    return _RUNS[(name, wide)]


@pytest.mark.parametrize("name,wide", WINDOWS)
def test_step_constant_is_lambda_max(name, wide):
    r = run(name, wide)
    lam = H.pred_lambda(r["c"]["Pinv"], r["W"])
    print(name, wide, "L / 1.05 / lambda_max - 1 =", r["L"] / 1.05 / lam - 1.0)
    assert abs(r["L"] / 1.05 - lam) <= 1e-5 * lam


@pytest.mark.parametrize("name,wide", WINDOWS)
def test_states_are_bytes_of_the_window(name, wide):
    r = run(name, wide)
    for (tag, k), s in r["got"].items():
        assert s.dtype == np.uint8 and s.shape == (r["r64"][tag][k]["state"].shape[0], r["c"]["n"])
        assert s.max() <= 2, (tag, k, "a byte that is no state (255: a row the kernel did not write)")
        assert (s[:, r["W"]:] == 0).all(), (tag, k, "columns beyond the window")
    st = H.PRED_SPECIAL["steady"]
    for k in H.PRED_COUNTS:                                      # x0 = 0: w = 0 exactly, on two bounds and inside the others
        assert (r["got"][("mr+1", k)][st] == 0).all()


@pytest.mark.parametrize("name,wide", WINDOWS)
def test_states_entry_by_entry(name, wide):
    r = run(name, wide)
    W = r["W"]
    for k in H.PRED_COUNTS:
        listed = H.PRED_FALLBACK.get((name, wide, k), ())
        und = mism_und = mism_dec = total = 0
        for tag, ref in r["r64"].items():
            got, dec = r["got"][(tag, k)][:, :W], ref[k]["margin"] > H.PRED_TAU
            diff = got != ref[k]["state"]
            und, mism_und, mism_dec, total = und + int((~dec).sum()), mism_und + int((diff & ~dec).sum()), mism_dec + int((diff & dec).sum()), total + dec.size
            if not ("variants" in listed or "rsum" in listed):
                rows = np.flatnonzero((diff & dec).any(axis=1))
                assert rows.size == 0, (name, wide, tag, k, "rows", rows[:8].tolist(), "entries", int((diff & dec).sum()),
                                        "first columns", np.flatnonzero((diff & dec)[rows[0]])[:8].tolist())
        print(f"case {name} wide {wide} count {k:2d}: {total} entries, {und} undecided, mismatches {mism_und} undecided / {mism_dec} decided"
              + (f"  (listed: {', '.join(listed)})" if listed else ""))


@pytest.mark.parametrize("name,wide", WINDOWS)
def test_listed_pairs_by_the_quality_of_their_sets(name, wide):
    r = run(name, wide)
    opt = H.pred_golden_states(name, wide)
    for k in H.PRED_COUNTS:
        if (name, wide, k) not in H.PRED_FALLBACK:
            continue
        q = [H.pred_quality(s, opt, r["MR"]) for s in (r["got"][(H.PRED_QUALITY_BATCH, k)], r["r64"][H.PRED_QUALITY_BATCH][k]["state"],
                                              r["r32"][H.PRED_QUALITY_BATCH][k]["state"])]
        print(f"case {name} wide {wide} count {k:2d}: mean Hamming distance from the optimum's sets: kernel {q[0]:.3f}, reference {q[1]:.3f} / {q[2]:.3f}")
        assert q[0] <= max(q[1], q[2]) + H.pred_quality_allowance(q[1], q[2]), (name, wide, k, q)


@pytest.mark.parametrize("name", ["a", "g", "i"])
def test_debug_call_leaves_the_handle_as_it_was(name):
    c = H.pred_case(name)
    MR = H.pred_instance(c["nu"], 0)[1]
    x0, lb, ub = H.pred_batches(c, MR)["mix"]
    xb, lbb, ubb = H.pred_batches(c, MR)["mr+1"]
    qp = _handle(c)
    before = qp.solve_batch(x0, lb, ub)
    first = qp.debug_predict(xb, lbb, ubb, iters=0, wide=0)
    if name == "i":
        qp.debug_predict(xb, lbb, ubb, iters=24, wide=1)
    again = qp.debug_predict(xb, lbb, ubb, iters=0, wide=0)
    after = qp.solve_batch(x0, lb, ub)
    qp.close()
    assert np.array_equal(first["state"], again["state"])
    assert (before["status"] == 0).all()
    for key in ("u", "active", "status", "ipm_iters", "factorizations"):
        assert np.array_equal(before[key], after[key]), key


def test_extent_kernel_picks_the_window():
    c = H.pred_case("i")
    qp = _handle(c)
    for tag, (x0, lb, ub) in H.pred_extent_batches(c).items():
        out = qp.debug_predict(x0, lb, ub, iters=8, wide=-1)
        count = H.pred_extent_count(c, x0, lb, ub)
        assert out["count"] == count and out["wide"] == int(count * 4 > x0.shape[0]) == int(tag == "wide"), (tag, out, count)
        assert (out["W"], out["MR"]) == H.pred_instance(c["nu"], out["wide"])
        forced = qp.debug_predict(x0, lb, ub, iters=8, wide=out["wide"])
        assert np.array_equal(out["state"], forced["state"]) and forced["count"] == -1
    qp.close()
    ca = H.pred_case("a")                                        # no 1024-column window: the extent kernel does not run
    qp = _handle(ca)
    x0, lb, ub = H.pred_batches(ca, 64)["b1"]
    out = qp.debug_predict(x0, lb, ub, iters=8, wide=-1)
    assert (out["count"], out["wide"], out["W"]) == (-1, 0, 512)
    qp.close()


@pytest.mark.parametrize("name,wide", [("a", 0), ("f", 0), ("i", 1)])
def test_nonfinite_and_out_of_range_x_unc(name, wide):
    """fminf(fmaxf(x, -60000), 60000) makes -60000 of a NaN (C's fmaxf returns the operand that is a number), so such a row behaves
    like one whose x_unc is -60000 everywhere; it is rejected elsewhere.  The ordinary rows of its group still match the reference."""
    c = H.pred_case(name)
    W, MR = H.pred_instance(c["nu"], wide)
    x0, lb, ub = H.pred_nonfinite_batch(c, MR)
    qp = _handle(c)
    got = {k: qp.debug_predict(x0, lb, ub, iters=k, wide=wide) for k in H.PRED_NONFINITE_COUNTS}
    qp.close()
    ref = H.pred_reference(c["Pinv"], x0 @ c["Kunc"].T, lb, ub, c["nu"], W, MR, got[1]["L"], counts=H.PRED_NONFINITE_COUNTS)
    ordinary = np.setdiff1d(np.arange(MR - 1), H.PRED_NONFINITE_ROWS)
    for k in H.PRED_NONFINITE_COUNTS:
        s = got[k]["state"]
        assert s.max() <= 2 and (s[:, W:] == 0).all()
        dec = ref[k]["margin"][ordinary] > H.PRED_TAU
        diff = s[ordinary, :W] != ref[k]["state"][ordinary]
        print(name, wide, k, "ordinary rows:", int((~dec).sum()), "undecided,", int((diff & ~dec).sum()), "/", int((diff & dec).sum()), "mismatches")
        assert not (diff & dec).any(), (name, wide, k)
    assert (got[1]["state"][H.PRED_NONFINITE_ROWS[0], :W] == 2).all()          # the NaN row: -60000, below every lower bound
    assert np.array_equal(got[1]["state"][H.PRED_NONFINITE_ROWS[1], :W], ref[1]["state"][H.PRED_NONFINITE_ROWS[1]])


def test_debug_entry_refuses_what_it_cannot_do():
    from industrial_nnmpc_2021_amd import _lib, synthetic
    from industrial_nnmpc_2021_amd.linearMPC_build import build_regulator_matrices
    from industrial_nnmpc_2021_amd.qp import BatchedBoxQP
    c = H.pred_case("a")
    x0, lb, ub = H.pred_batches(c, 64)["mr+1"]
    qp = _handle(c)
    with pytest.raises(_lib.NnmpcError, match="1024-column"):
        qp.debug_predict(x0, lb, ub, iters=8, wide=1)
    with pytest.raises(_lib.NnmpcError, match="bad arguments"):
        qp.debug_predict(x0, lb, ub, iters=65, wide=0)
    with pytest.raises(_lib.NnmpcError, match="bad arguments"):
        qp.debug_predict(np.tile(x0, (4, 1)), np.tile(lb, (4, 1)), np.tile(ub, (4, 1)), iters=8, wide=0)      # 260 > the segment size
    qp.close()
    qp = _handle(c, asm_predict_iters=-1)
    with pytest.raises(_lib.NnmpcError, match="no predictor window"):
        qp.debug_predict(x0, lb, ub, iters=8, wide=0)
    qp.close()
    pl = synthetic.plant("mini_cdu", 0)
    P, tq, nu = build_regulator_matrices(pl)
    qp = BatchedBoxQP(P, tq, nu, max_batch=128)
    s, x0, lb, ub = H.batch_inputs(pl, 4, 1, 2.0)
    with pytest.raises(_lib.NnmpcError, match="no predictor window"):
        qp.debug_predict(x0, lb, ub, iters=8, wide=0)
    qp.close()
    qp = BatchedBoxQP(P, tq, nu, max_batch=128, method="pdip")
    with pytest.raises(_lib.NnmpcError, match="set_inverse"):
        qp.debug_predict(x0, lb, ub, iters=8, wide=0)
    qp.close()


def test_production_launch_of_the_per_column_instance():
    """nu = 6, N = 121: n = 726 is past the one-wave path of small problems (n <= 724), so a call of 300 problems launches
    asm_predict_k<4, 2, false> -- the instance no other solve of the suite reaches.  Same status, sets and u as without the predictor
    (the bars of tests/test_predict_gpu.py), strictly fewer rounds, two rows against the oracle."""
    from industrial_nnmpc_2021_amd.linearMPC_build import build_regulator_matrices
    from industrial_nnmpc_2021_amd.qp import BatchedBoxQP
    pl = H.pred_plant(6, 121, 390)
    P, tq, nu = build_regulator_matrices(pl)
    N, n, B = pl["N"], P.shape[0], 300
    assert (nu, n) == (6, 726)
    s, x0, lb, ub = H.batch_inputs(pl, B, 3, 4.0)
    out = {}
    for tag, iters in (("off", -1), ("on", 0)):
        qp = BatchedBoxQP(P, tq, nu, max_batch=512, seg_max=512, asm_predict_iters=iters, asm_tail_batch=-1)
        qp.stats(reset=True)
        out[tag] = qp.solve_batch(x0, lb, ub)
        out[tag]["stats"] = qp.stats()
        qp.close()
    assert out["off"]["stats"]["asm_predict_launches"] == 0 and out["on"]["stats"]["asm_predict_launches"] == 1
    assert out["on"]["stats"]["asm_small_passes"] == 0
    assert (out["on"]["status"] == 0).all() and (out["off"]["status"] == 0).all()
    assert np.array_equal(out["on"]["active"], out["off"]["active"])
    assert np.abs(out["on"]["u"] - out["off"]["u"]).max() <= 1e-10 * max(1.0, np.abs(out["off"]["u"]).max())
    print("asm_rounds with / without the predictor:", out["on"]["stats"]["asm_rounds"], "/", out["off"]["stats"]["asm_rounds"])
    assert out["on"]["stats"]["asm_rounds"] < out["off"]["stats"]["asm_rounds"]
    Ps = np.tril(P) + np.tril(P, -1).T
    rows = [int(np.argmax(out["on"]["active"].sum(axis=1))), 17]
    for r, (xe, active) in zip(rows, H.oracle_box_rows(Ps, tq, nu, N, x0, lb, ub, rows)):
        ref = np.zeros(2 * n, bool)
        ref[active] = True
        assert np.abs(out["on"]["u"][r] - xe).max() <= 1e-8 * max(1.0, np.abs(xe).max()), r
        assert np.array_equal(out["on"]["active"][r], ref), r
