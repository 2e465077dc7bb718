"""The inputs and the reference of tests/test_predict_kernel_gpu.py, held to their conditions on the CPU (no GPU, no library).

  * build_predictor's power iteration, emulated step for step, gives L / 1.05 within 1e-5 of eigvalsh's lambda_max on every case's
    matrix (with the stop rule it had before -- a change of 1e-6 per step, 200 steps at most -- it missed that on cases b and g
    (1.0e-5 and 2.9e-5 short) and on case f (2.3e-3 short: the two largest eigenvalues are a factor 0.9988 apart));
  * every (case, window, count) either meets the caps of the entrywise comparison over the batches of its case -- at most 2 % of
    the entries undecided, at least 3 % of the decided ones non-free, both signs, a row with an empty set, every restart sum that
    decides a kb at least 1e-3 of the sum of its terms' absolute values, the two arithmetic variants of the reference equal on every
    decided entry -- or is listed in helpers.PRED_FALLBACK with exactly the caps it misses;
  * PRED_TAU_MEASURED is the smallest power of two at which the two variants agree on every decided entry of every pair that is not
    listed for "variants", and PRED_TAU is 4 x that;
  * the adaptive count reaches its floor of 8 in every case and at least 12 in every case but g; the special rows are what they are meant to be;
  * the reference alone is worth comparing against: on case i after 24 iterations its mean Hamming distance from the oracle's sets is
    below a quarter of the x_unc start's (rows at sx = 2, as the figures in csrc/qp_predict.h: 512-column window 10.5 -> 0.375,
    1024-column window 10.9 -> 0.75; mid_cdu gave 31.8 -> 2.1.  Rows at sx = 6 come down more slowly: 31.1 -> 9.9 after 24
    iterations, 1.6 after 64);
  * the fixture tests/golden/predict_oracle_sets.npz holds what oracle.qp.solve_exact_box says today.
"""
import numpy as np
import pytest

from tests import helpers as H

WINDOWS = H.pred_windows()
_REFS = {}


def refs(name, wide):
    """(case, L, reference by batch, f32 variant by batch), computed once per window."""
    if (name, wide) not in _REFS:
        c = H.pred_case(name)
        L = H.pred_power_iteration(c["Pinv"], H.pred_instance(c["nu"], wide)[0])
        _REFS[(name, wide)] = (c, L, H.pred_references(c, wide, L), H.pred_references(c, wide, L, "f32"))
    return _REFS[(name, wide)]


@pytest.mark.parametrize("name,wide", WINDOWS)
def test_power_iteration_finds_lambda_max(name, wide):
    c = H.pred_case(name)
    W = H.pred_instance(c["nu"], wide)[0]
    L, lam = H.pred_power_iteration(c["Pinv"], W), H.pred_lambda(c["Pinv"], W)
    print(name, wide, "L / 1.05 / lambda_max - 1 =", L / 1.05 / lam - 1.0)
    assert abs(L / 1.05 - lam) <= 1e-5 * lam


def test_cases_are_the_shapes_they_are_meant_to_be():
    for name, (nu, N) in H.PRED_CASES.items():
        c = H.pred_case(name)
        assert c["n"] == nu * N and c["P"].shape == (nu * N, nu * N) and c["tq"].shape == (nu * N, 12 + nu)
        assert np.abs(c["Ps"] @ c["Pinv"] - np.eye(c["n"])).max() < 1e-9
    n = {k: v[0] * v[1] for k, v in H.PRED_CASES.items()}
    assert (n["a"], n["b"], n["c"], n["d"], n["e"], n["f"], n["g"], n["h"], n["i"]) == (512, 512, 512, 516, 512, 516, 515, 518, 1024)
    assert n["g"] % 4 != 0 and all(H.PRED_CASES[k][0] % 4 for k in "fgh") and not any(H.PRED_CASES[k][0] % 4 for k in "abcdei")
    assert 32 % H.PRED_CASES["d"][0] != 0 and H.PRED_CASES["b"][0] + 4 == 36
    assert H.pred_instance(6, 0) == (512, 32) and H.pred_instance(8, 0) == (512, 64) and H.pred_instance(16, 1) == (1024, 32)
    for name, wide in WINDOWS:
        c = H.pred_case(name)
        MR = H.pred_instance(c["nu"], wide)[1]
        b = H.pred_batches(c, MR)
        assert [b[t][0].shape[0] for t in ("b1", "mr-1", "mr+1", "mix", "tight")] == [1, MR - 1, MR + 1, 2 * MR + 2, 2]


@pytest.mark.parametrize("name,wide", WINDOWS)
def test_every_pair_meets_the_caps_or_is_listed(name, wide):
    c, L, r64, r32 = refs(name, wide)
    for k in H.PRED_COUNTS:
        cond = H.pred_pair_conditions(r64, r32, k)
        failed = H.pred_failed_conditions(cond)
        print(name, wide, k, {a: (round(b, 5) if isinstance(b, float) else b) for a, b in cond.items()}, failed)
        assert tuple(failed) == H.PRED_FALLBACK.get((name, wide, k), ()), (name, wide, k, cond)
    for r in (r64, r32):
        assert all((r[t]["nit"] == r64[t]["nit"]).all() for t in r64)          # the adaptive count does not hang on the arithmetic


def test_tau_is_what_the_two_variants_need():
    need = 0.0
    for name, wide in WINDOWS:
        c, L, r64, r32 = refs(name, wide)
        for k in H.PRED_COUNTS:
            if "variants" not in H.PRED_FALLBACK.get((name, wide, k), ()):
                need = max(need, H.pred_pair_conditions(r64, r32, k)["need"])
    print("largest margin of an entry on which the variants differ:", need)
    assert need > 0.0 and 2.0 ** np.ceil(np.log2(need)) == H.PRED_TAU_MEASURED
    assert H.PRED_TAU == 4.0 * H.PRED_TAU_MEASURED
    # only the longest count ever needs the fallback for a reason that makes the entrywise comparison unsound
    assert all(k == 64 for (_, _, k), f in H.PRED_FALLBACK.items() if "variants" in f or "rsum" in f)


@pytest.mark.parametrize("name,wide", WINDOWS)
def test_adaptive_counts_and_special_rows(name, wide):
    c, L, r64, r32 = refs(name, wide)
    W, MR = H.pred_instance(c["nu"], wide)
    nits = np.concatenate([r64[t]["nit"] for t in r64])
    print(name, wide, {t: (r64[t]["nit"].tolist(), r64[t]["nviol"].tolist()) for t in r64})
    # (case g, nu = 5: x_unc leaves the box in 46 entries at most however tight the box -- 0.3 per bound stays below 12; its groups
    # are all at the floor, which still tells a floor of 8 from any other)
    assert nits.min() == 8 and r64["mix"]["nit"][0] == 8 and (nits.max() >= 12 or name == "g")
    assert r64["mix"]["nviol"][0] < r64["mix"]["nviol"][1]
    # the clones of a ragged last group count: without them the tight batch's two rows would stay at the floor whatever they are
    assert r64["tight"]["nit"][0] == nits.max()
    for k in H.PRED_COUNTS:
        s = r64["mr+1"][k]["state"]
        assert (s[H.PRED_SPECIAL["steady"]] == 0).all() and (s[H.PRED_SPECIAL["wide"]] == 0).all()
        # (the +-0.02 box holds every bound x_unc reaches; beyond the first stages x_unc is 0 on this plant and inside any box around 0)
        sizes = np.sort((s[:MR] != 0).sum(axis=1))
        assert (s[H.PRED_SPECIAL["tiny"]] != 0).sum() == sizes[-1] >= 1.5 * sizes[-2]
    x0, lb, ub = H.pred_batches(c, MR)["mr+1"]
    s = H.PRED_SPECIAL["steady"]
    assert (x0[s] == 0).all() and ub[s, 0] == 0 and lb[s, 1] == 0


def test_reference_names_the_oracles_sets_on_case_i():
    for wide in (0, 1):
        c, L, r64, r32 = refs("i", wide)
        opt = H.pred_golden_states("i", wide)
        q = {k: H.pred_quality(r64[H.PRED_QUALITY_BATCH][k]["state"], opt, H.pred_instance(c["nu"], wide)[1]) for k in H.PRED_COUNTS}
        print("case i, wide", wide, "mean Hamming distance from the oracle's sets by count:", q)
        assert q[24] < 0.25 * q[1]


def test_golden_sets_are_the_oracles():
    for name, wide in WINDOWS:
        c = H.pred_case(name)
        got = H.pred_golden_states(name, wide)
        assert got.dtype == np.uint8 and got.shape == (H.PRED_QUALITY_ROWS, H.pred_instance(c["nu"], wide)[0])
        assert np.array_equal(got, H.pred_oracle_states(c, wide)), (name, wide)


def test_extent_batches_sit_on_either_side_of_the_threshold():
    c = H.pred_case("i")
    b = H.pred_extent_batches(c)
    counts = {t: H.pred_extent_count(c, *b[t]) for t in b}
    assert counts == {"narrow": 2, "wide": 3} and b["narrow"][0].shape[0] == 8
    assert not counts["narrow"] * 4 > 8 and counts["wide"] * 4 > 8


@pytest.mark.parametrize("name,wide", [("a", 0), ("f", 0), ("i", 1)])
def test_nonfinite_batch_leaves_the_ordinary_rows_comparable(name, wide):
    c = H.pred_case(name)
    W, MR = H.pred_instance(c["nu"], wide)
    L = H.pred_power_iteration(c["Pinv"], W)
    x0, lb, ub = H.pred_nonfinite_batch(c, MR)
    xunc = x0 @ c["Kunc"].T
    nan_row, big_row = H.PRED_NONFINITE_ROWS
    assert np.isnan(xunc[nan_row, :W]).all() and np.abs(xunc[big_row, :W]).max() > 60000 and np.isfinite(np.delete(xunc, nan_row, 0)).all()
    assert (H.pred_xunc_f16(xunc[nan_row, :W]) == -60000).all() and np.abs(H.pred_xunc_f16(xunc[big_row, :W])).max() == 60000
    r = [H.pred_reference(c["Pinv"], xunc, lb, ub, c["nu"], W, MR, L, counts=H.PRED_NONFINITE_COUNTS, variant=v) for v in ("f64", "f32")]
    ordinary = np.setdiff1d(np.arange(MR - 1), H.PRED_NONFINITE_ROWS)
    assert (r[0][1]["state"][nan_row] == 2).all()              # x_unc = -60000 everywhere: below every lower bound
    for k in H.PRED_NONFINITE_COUNTS:
        assert min(H.pred_deciding_rsum(v, k) for v in r) >= H.PRED_MIN_RSUM_REL
        dec = r[0][k]["margin"][ordinary] > H.PRED_TAU_MEASURED
        assert np.array_equal(r[0][k]["state"][ordinary][dec], r[1][k]["state"][ordinary][dec])
