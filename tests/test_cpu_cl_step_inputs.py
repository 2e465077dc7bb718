"""The inputs and the reference of tests/test_cl_step_gpu.py and tests/test_chain_step_gpu.py, held to their conditions on the CPU.

  * every case of helpers.CL_STEP_CASES is SIMULATED with the step reference alone (helpers.cl_step_simulate: state carried, target
    optimum from the certified oracle, NN and MPC moves from oracle.nn / oracle.qp) and must give what the GPU tests rest on: every
    target row certified and feasible, at most 5 % of the (instance, step) rows dropped by ts_kept, us with an input on a bound in
    some kept rows and none in others over the case list, at most half of the SATDLQR entries on a bound within a case and some in
    at least three cases, |u - us| above 100 x the bar in every column of the NN and MPC instances, every record below 1e3;
  * the 513-step model of the event-block test stays bounded (spectral radius of the estimator matrix, and the simulation itself);
  * the step reference is validated against the reference project's own output: fed with closed_loop._model of the golden plant
    and the noise simulate_closed_loop_batch draws for seed 17, its simulated satdlqr and us trajectories reproduce
    tests/golden/closed_loop_baselines.npz at the bars of test_baselines_match_reference_fixture;
  * the derived bounds are what the module comment of helpers says (n from the shapes), and a seeded error of a few ulp beyond
    them is seen by helpers.cl_identity_ratios.
"""
import os

import numpy as np
import pytest

from tests import helpers as H

CASES = sorted(H.CL_STEP_CASES)


@pytest.fixture(scope="module")
def sims():
    out = {}
    for c in CASES:
        b = H.cl_step_batch(c)
        out[c] = (b, H.cl_step_simulate(b))            # a row the oracle cannot certify (infeasible) raises ArithmeticError here
    return out


def _kind(b):
    return np.array([("nn" if s["kind"] == "nn" else s["kind"]) for s in b["slots"]])[b["inst_slot"]]


@pytest.mark.parametrize("case", CASES)
def test_case_meets_the_conditions_of_the_gpu_tests(sims, case):
    b, r = sims[case]
    M = b["M"]
    nx, nu, ny, nd, nz = H.CL_STEP_CASES[case]
    assert (M["nx"], M["nu"], M["ny"], M["nd"], M["nz"]) == (nx, nu, ny, nd, nz)
    assert b["inst_slot"].size == 16 and set(b["scen"]) == {0, 1, 2} and b["SP"].shape == (3, H.CL_STEP_T, ny)
    assert abs(np.abs(np.linalg.eigvals(M["A"])).max() - 0.9) < 1e-9
    assert np.array_equal(M["Aaug"][:nx, :nx], M["A"]) and np.array_equal(M["Aaug"][nx:, nx:], np.eye(nd))
    assert np.array_equal(M["Caug"][:, :nx], M["C"]) and np.array_equal(M["Baug"][:nx], M["B"]) and not M["Baug"][nx:].any()
    assert (M["Bp"] is None) == (nd == 0) and (M["Cd"] is None) == (nd == 0) and (M["Eb"] is None) == (nz == 0)
    assert np.linalg.eigvalsh(M["Qaug"])[0] > -1e-12
    for k in ("y", "x", "xhat", "u", "xs", "us", "avg"):
        assert np.isfinite(r[k]).all() and np.abs(r[k]).max() < 1e3, (k, np.abs(r[k]).max())
    assert (r["us"] >= M["ulb"] - H.TS_SLACK).all() and (r["us"] <= M["uub"] + H.TS_SLACK).all()
    assert (~r["kept"]).mean() <= 0.05
    kind = _kind(b)
    sat = r["u"][:, kind == "satdlqr"]
    assert H.share_on_bound(sat.reshape(-1, nu), M["ulb"], M["uub"]) <= 0.5
    for k, tol in (("nn", H.CL_STEP_NN_TOL), ("mpc", H.cl_mpc_tol())):
        d = np.abs(r["u"] - r["us"])[:, kind == k]
        assert (d.max(axis=(0, 1)) > 100 * tol).all(), (k, d.max(axis=(0, 1)))


def test_shares_over_the_case_list(sims):
    """us: rows with an input on a bound and rows without, among the kept ones; SATDLQR: clipped entries in at least three cases."""
    on = np.concatenate([r["on_bound"][r["kept"]] for _, r in sims.values()])
    assert (on > 0).any() and (on == 0).any()
    clipped = [c for c, (b, r) in sims.items()
               if H.share_on_bound(r["u"][:, _kind(b) == "satdlqr"].reshape(-1, b["M"]["nu"]), b["M"]["ulb"], b["M"]["uub"]) > 0]
    assert len(clipped) >= 3, clipped
    for c, (b, r) in sims.items():
        sat = r["u"][:, _kind(b) == "satdlqr"].reshape(-1, b["M"]["nu"])
        print(f"case {c}: dropped {(~r['kept']).mean():.3f}, us rows on a bound {(r['on_bound'] > 0).mean():.2f}, SATDLQR entries clipped "
              f"{H.share_on_bound(sat, b['M']['ulb'], b['M']['uub']):.2f}, max |record| {max(np.abs(r[k]).max() for k in ('y', 'x', 'xhat', 'avg')):.3g}")


def test_long_run_model_stays_bounded():
    """Case b, US and SATDLQR slots, 513 steps (tests/test_cl_step_gpu.py crosses the 256-step event blocks with it)."""
    T = max(H.CL_STEP_LONG_T)
    b = H.cl_step_batch("b", kinds=("us", "satdlqr"), counts=(2, 2), T=T)
    M = b["M"]
    rho = np.abs(np.linalg.eigvals((np.eye(M["nx"] + M["nd"]) - M["L"] @ M["Caug"]) @ M["Aaug"])).max()
    assert rho < 0.97, rho
    r = H.cl_step_simulate(b)
    assert r["u"].shape == (T, 4, M["nu"])
    for k in ("y", "x", "xhat", "u", "xs", "us", "avg"):
        assert np.isfinite(r[k]).all() and np.abs(r[k]).max() < 1e3, k


def test_bounds_follow_the_shapes_and_see_a_seeded_error(sims):
    b, r = sims["c"]
    M = b["M"]
    nx, nu, ny, nd, nz = H.CL_STEP_CASES["c"]
    na = nx + nd
    assert H.cl_gamma(100) == 100 * H.TS_EPS / (1 - 100 * H.TS_EPS)
    xh = r["xhat"][3]
    ref, bnd = H.cl_ref_filter(M, xh, r["u"][2], r["y"][3])
    assert ref.dtype == np.longdouble and np.finfo(np.longdouble).eps < 1e-18
    A, Bm, Cm, L = (np.abs(M[k]) for k in ("Aaug", "Baug", "Caug", "L"))
    axp = np.abs(xh) @ A.T + np.abs(r["u"][2]) @ Bm.T
    mag = axp + (np.abs(r["y"][3]) + axp @ Cm.T) @ L.T
    n = na + nu + na + ny + 2
    assert np.allclose(np.asarray(bnd, float), 2 * n * H.TS_EPS / (1 - n * H.TS_EPS) * mag, rtol=1e-12)
    assert np.abs(np.asarray(ref, float) - r["xhat"][4]).max() <= float(bnd.max())       # the float64 simulation itself is inside
    # the whole set of identities on the simulated records: every ratio <= 1 (float64 roundings of the carried state), and a seeded
    # error of 1e-11 (avg: 1e-9) in one entry of one record is seen by exactly the identities that read or produce it
    rec = {k: r[k] for k in ("y", "x", "xhat", "u", "xs", "us", "avg")}
    base = H.cl_identity_ratios(H.cl_step_reference(b, rec, want=()))
    assert set(base) >= {"xhat", "us", "xs", "u_us", "u_satdlqr", "avg", "x", "y"} and max(base.values()) <= 1.0, base
    for key, row, hit in (("xhat", 5, {"xhat"}), ("xs", 4, {"xs"}), ("x", 7, {"x"}), ("y", 6, {"y"}), ("avg", 9, {"avg"})):
        eps = 1e-9 if key == "avg" else 1e-11          # (the cost is a sum of ~1e5 products of the order of 1: its bound is ~1e-10)
        bad = {k: v.copy() for k, v in rec.items()}
        bad[key][row, 4, ...] = bad[key][row, 4, ...] + eps
        got = H.cl_identity_ratios(H.cl_step_reference(b, bad, want=()))
        assert hit <= {k for k, v in got.items() if v > 1.0}, (key, got)


@pytest.mark.parametrize("nx,nu,nd", H.CHAIN_STEP_SHAPES)
def test_chain_cases_decide_something(nx, nu, nd):
    """The chains' first step: the move differs from us in every column by far more than the bar, and the state stays small."""
    c = H.chain_step_case(nx, nu, nd, 5)
    assert c["Bd"].shape == (nx, nd) and c["D"].shape == (H.CHAIN_STEP_T, 5, nd)
    z = np.concatenate((c["x0"] - c["Xs"][0], c["uprev0"] - c["Us"][0]), axis=1)
    first, vmax = H.cl_ref_mpc(c["spec"], z, c["Us"][0], c["ulb"], c["uub"])
    assert (np.abs(first).max(axis=0) > 100 * H.cl_mpc_tol()).all()
    ev = np.linalg.eigvalsh(c["spec"]["P"])
    assert ev[0] > 0 and ev[-1] / ev[0] <= H.CL_STEP_MPC_COND * (1 + 1e-9)


def test_step_reference_reproduces_the_reference_projects_baselines(golden_dir):
    """The identities of helpers are a reading of the kernels; here they are held to the reference project's own trajectories."""
    from industrial_nnmpc_2021_amd import closed_loop as cl, controller_evaluation as ce, linearMPC as lm, target as tg
    g = np.load(os.path.join(golden_dir, "closed_loop.npz"))
    f = np.load(os.path.join(golden_dir, "closed_loop_baselines.npz"))
    Nx, Nu = g["B"].shape
    Ny, Nd, Nsim = g["C"].shape[0], g["Bd"].shape[1], int(g["Nsim"])
    common = dict(A=g["A"], B=g["B"], C=g["C"], H=g["H"], Qwx=g["Qwx"], Qwd=g["Qwd"], Rv=g["Rv"], xprior=np.zeros((Nx, 1)),
                  dprior=np.zeros((Nd, 1)), Rs=g["Rs"], Qs=g["Qs"], Bd=g["Bd"], Cd=g["Cd"], usp=np.zeros((Nu, 1)),
                  uprev=np.zeros((Nu, 1)), Q=g["Q"], R=g["R"], S=g["S"], ulb=g["ulb"], uub=g["uub"])
    plant = lm.LinearPlantSimulator(A=g["A"], B=g["B"], C=g["C"], Bp=g["Bd"], Rv=g["Rv"], sample_time=1.0, x0=np.zeros((Nx, 1)))
    sat = ce.SatDlqrController(**common)
    M = cl._model(plant, sat)
    for k in ("ulb", "uub", "x0", "xhat0", "uprev0", "q0"):
        M[k] = np.ravel(M[k]).astype(np.float64)
    red = tg.ReducedTargetProblem(sat.A, sat.B, sat.C, sat.H, sat.Bd, sat.Cd, sat.Qs, sat.Rs, sat.usp)
    M.update(Pr=red.Pr, E=red.E)
    np.random.seed(17)                                   # simulate_closed_loop_batch's draws: the plant's first, then one per step
    V = np.random.randn(Nsim + 1, Ny)
    b = dict(M=M, slots=[dict(kind="satdlqr", Kaug=sat.Kaug), dict(kind="us")], inst_slot=np.array([0, 1], np.int32),
             scen=np.zeros(2, np.int32), SP=g["setpoints"][None, :Nsim], DS=g["disturbances"][None, :Nsim],
             V=np.stack((V, V), axis=1), sigma=np.sqrt(np.diag(g["Rv"])), T=Nsim)
    r = H.cl_step_simulate(b)
    for i, name in enumerate(("satdlqr", "us")):
        for k in ("y", "u", "x", "xhat"):
            assert r[k][:, i].shape == f[f"{name}_{k}"].shape, (name, k)
            assert np.abs(r[k][:, i] - f[f"{name}_{k}"]).max() < 1e-6, (name, k, np.abs(r[k][:, i] - f[f"{name}_{k}"]).max())
        assert np.abs(r["avg"][:, i] - f[f"{name}_avg_cost"]).max() < 1e-5, name
    assert np.abs(f["satdlqr_u"]).max() > 0.999          # the clip is exercised
