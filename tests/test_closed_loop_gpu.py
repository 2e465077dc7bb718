"""Lock-step closed-loop evaluation (nnmpc_cl_*, closed_loop.simulate_closed_loop_batch) against the reference's
online_simulation: the golden trajectories of tests/golden/closed_loop.npz and the host loop of this package, instance by
instance, on a small plant with every controller kind."""
import contextlib
import io
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _mini_problem():
    """mini_cstrs plant + integrating disturbances, target on the first two outputs, filter tuning."""
    from industrial_nnmpc_2021_amd import synthetic
    pl = synthetic.plant("mini_cstrs", seed=4, rho=0.9)
    rng = np.random.default_rng(11)
    Nx, Nu = pl["B"].shape
    Ny, Nd = pl["C"].shape[0], 2
    Bd = rng.standard_normal((Nx, Nd)) / np.sqrt(Nx)
    common = dict(A=pl["A"], B=pl["B"], C=pl["C"], H=np.eye(2, Ny), Qwx=1e-4 * np.eye(Nx), Qwd=1e-2 * np.eye(Nd),
                  Rv=1e-4 * np.eye(Ny), xprior=np.zeros((Nx, 1)), dprior=np.zeros((Nd, 1)), Rs=1e-3 * np.eye(Nu), Qs=np.eye(Ny),
                  Bd=Bd, Cd=np.zeros((Ny, Nd)), usp=np.zeros((Nu, 1)), uprev=np.zeros((Nu, 1)), Q=pl["Q"], R=pl["R"], S=pl["S"],
                  ulb=pl["ulb"], uub=pl["uub"])
    T = 100
    scen = []
    for s in range(2):
        sp = np.zeros((T, Ny))
        sp[:, :2] = np.repeat(rng.uniform(-0.05, 0.05, (4, 2)), T // 4, axis=0)      # reachable inside the input box
        ds = np.repeat(rng.uniform(-0.05, 0.05, (2, Nd)), T // 2, axis=0)
        scen.append((sp, ds))
    return pl, common, scen


def _weights(rng, din, width, nu, scale=0.3):
    dims = [din, width, width, nu]
    W = []
    for i in range(3):
        W.append(scale * rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i]))
        if i < 2:
            W.append(0.1 * rng.standard_normal(dims[i + 1]))
    return W


def _controllers(common, specs):
    """specs: ("mpc", N) | ("nn", width, withuprev, seed) | ("satdlqr",) | ("us",) -> fresh controllers."""
    from industrial_nnmpc_2021_amd import linearMPC as lm, controller_evaluation as ce
    Nx, Nu = common["B"].shape
    out = []
    for sp in specs:
        if sp[0] == "mpc":
            out.append(lm.LinearMPCController(N=sp[1], **common))
        elif sp[0] == "nn":
            rng = np.random.default_rng(sp[3])
            W = _weights(rng, 2 * Nx + (2 if sp[2] else 1) * Nu, sp[1], Nu)
            out.append(ce.NeuralNetworkController(regulator_weights=W, xscale=rng.uniform(0.5, 2.0, Nx), nnwithuprev=sp[2],
                                                  **common))
        elif sp[0] == "satdlqr":
            out.append(ce.SatDlqrController(**common))
        else:
            out.append(ce.SteadyStateController(**common))
    return out


def _host_loaded(plant, ctl, sp, ds, Nsim, seed):
    """The reference's evaluation scripts: an already built (unpickled) plant, np.random.seed(seed) afterwards
    (_simulate_scenarios, lib/controller_evaluation.py:353-360)."""
    import copy
    from industrial_nnmpc_2021_amd import linearMPC as lm
    plant = copy.deepcopy(plant)
    np.random.seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        lm.online_simulation(plant, ctl, setpoints=sp, disturbances=ds, Nsim=Nsim)
    return dict(y=np.array(plant.y)[:, :, 0], u=np.array(plant.u)[:, :, 0], avg=np.array(ctl.average_stage_costs).ravel())


def _host(pl_mats, ctl, sp, ds, Nsim, seed, x0):
    from industrial_nnmpc_2021_amd import linearMPC as lm
    np.random.seed(seed)
    plant = lm.LinearPlantSimulator(x0=x0, sample_time=1.0, **pl_mats)
    with contextlib.redirect_stdout(io.StringIO()):
        lm.online_simulation(plant, ctl, setpoints=sp, disturbances=ds, Nsim=Nsim)
    return dict(y=np.array(plant.y)[:, :, 0], u=np.array(plant.u)[:, :, 0], x=np.array(plant.x)[:, :, 0],
                xhat=np.array(ctl.filter.xhat)[:, :, 0], avg=np.array(ctl.average_stage_costs).ravel())


SPECS = [("nn", 16, True, 1), ("nn", 24, False, 2), ("nn", 40, True, 3), ("mpc", 25), ("mpc", 6), ("satdlqr",), ("us",)]


@pytest.fixture(scope="module")
def batch_run():
    from industrial_nnmpc_2021_amd import linearMPC as lm
    from industrial_nnmpc_2021_amd.closed_loop import simulate_closed_loop_batch
    pl, common, scen = _mini_problem()
    mats = dict(A=pl["A"], B=pl["B"], C=pl["C"], Bp=common["Bd"], Rv=common["Rv"])
    plant = lm.LinearPlantSimulator(x0=np.zeros((pl["A"].shape[0], 1)), sample_time=1.0, **mats)
    ctls = _controllers(common, SPECS)
    res = simulate_closed_loop_batch(plant, ctls, scenarios=scen, Nsim=100, seeds=[3, 5, 8, 13, 21])
    return dict(pl=pl, common=common, scen=scen, mats=mats, plant=plant, res=res)


def test_golden_mpc_and_nn_match_reference_online_simulation(golden_dir):
    from industrial_nnmpc_2021_amd import linearMPC as lm, controller_evaluation as ce
    from industrial_nnmpc_2021_amd.closed_loop import simulate_closed_loop_batch
    g = np.load(os.path.join(golden_dir, "closed_loop.npz"))
    Nx, Nu = g["B"].shape
    Ny, Nd, Nsim = g["C"].shape[0], g["Bd"].shape[1], int(g["Nsim"])
    common = dict(A=g["A"], B=g["B"], C=g["C"], H=g["H"], Qwx=g["Qwx"], Qwd=g["Qwd"], Rv=g["Rv"], xprior=np.zeros((Nx, 1)),
                  dprior=np.zeros((Nd, 1)), Rs=g["Rs"], Qs=g["Qs"], Bd=g["Bd"], Cd=g["Cd"], usp=np.zeros((Nu, 1)),
                  uprev=np.zeros((Nu, 1)), Q=g["Q"], R=g["R"], S=g["S"], ulb=g["ulb"], uub=g["uub"])
    W = [g[f"W{i}"] for i in range(int(g["nW"]))]
    plant = lm.LinearPlantSimulator(A=g["A"], B=g["B"], C=g["C"], Bp=g["Bd"], Rv=g["Rv"], sample_time=1.0, x0=np.zeros((Nx, 1)))
    ctls = [lm.LinearMPCController(N=int(g["N"]), **common),
            ce.NeuralNetworkController(regulator_weights=W, xscale=g["xscale"], nnwithuprev=True, **common)]
    res = simulate_closed_loop_batch(plant, ctls, scenarios=[(g["setpoints"], g["disturbances"])], Nsim=Nsim, seeds=[17],
                                     return_objects=True)
    for i, (name, tol) in enumerate((("mpc", 1e-6), ("nn", 2e-4))):
        for k in ("y", "u", "x", "xhat"):
            assert res[k][i].shape == g[f"{name}_{k}"].shape, (name, k)
            assert np.abs(res[k][i] - g[f"{name}_{k}"]).max() < tol, (name, k)
        assert np.abs(res["avg"][i] - g[f"{name}_avg_cost"]).max() < 10 * tol, name
        assert (res["ts_status"][i] == 0).all() and (res["reg_status"][i] == 0).all()
        c = res["controllers"][i]
        assert len(c.average_stage_costs) == Nsim + 1 and len(c.computation_times) == Nsim and len(res["plants"][i].y) == Nsim + 1
    assert np.abs(res["u"]).max() > 0.999                                        # the bounds are hit in closed loop


def test_batched_matches_host_online_simulation(batch_run):
    """Every instance (3 NN slots of different widths / input layouts, MPC at two horizons, satK, us; 2 scenarios x 5 seeds)
    against the host loop with the same seed."""
    b = batch_run
    res, common = b["res"], b["common"]
    assert len(res["instances"]) == 70
    assert (res["ts_status"] == 0).all() and (res["reg_status"] == 0).all()
    x0 = np.zeros((common["A"].shape[0], 1))
    worst = {}
    for i, (c, s, seed) in enumerate(res["instances"]):
        if seed not in (3, 21):                                                  # the host loop is slow: two seeds of five
            continue
        ctl = _controllers(common, [SPECS[c]])[0]
        h = _host(b["mats"], ctl, b["scen"][s][0], b["scen"][s][1], 100, seed, x0)
        tol = 2e-4 if SPECS[c][0] == "nn" else 1e-8
        for k in ("y", "u", "x", "xhat", "avg"):
            err = np.abs(res[k][i] - h[k]).max()
            worst[SPECS[c][0]] = max(worst.get(SPECS[c][0], 0.0), err)
            assert err < tol, (i, SPECS[c], k, err)
    assert set(worst) == {"nn", "mpc", "satdlqr", "us"}


def test_batch_independence(batch_run):
    """An instance alone gives the same trajectory as inside the 70-instance run: bit for bit (NN, satK, us), 1e-12 (MPC)."""
    from industrial_nnmpc_2021_amd.closed_loop import simulate_closed_loop_batch
    b = batch_run
    res = b["res"]
    ctls = _controllers(b["common"], SPECS)
    for c in range(len(SPECS)):
        i = [j for j, inst in enumerate(res["instances"]) if inst[0] == c and inst[1] == 1 and inst[2] == 13][0]
        one = simulate_closed_loop_batch(b["plant"], ctls, scenarios=b["scen"], Nsim=100, seeds=[13], instances=[(c, 1, 13)])
        if SPECS[c][0] == "mpc":
            assert np.abs(one["u"][0] - res["u"][i]).max() < 1e-12 and np.abs(one["avg"][0] - res["avg"][i]).max() < 1e-12
        else:
            assert np.array_equal(one["u"][0], res["u"][i]) and np.array_equal(one["avg"][0], res["avg"][i]), SPECS[c]


def test_chunked_runs_and_reset(batch_run):
    """run(40) + run(60) == run(100) bit for bit, and reset restores the initial state."""
    from industrial_nnmpc_2021_amd import closed_loop as cl
    b = batch_run
    ctls = _controllers(b["common"], [s for s in SPECS if s[0] != "mpc"] + [("mpc", 6)])
    slots = []
    for c in ctls:
        k = cl._kind(c)
        slots.append(dict(kind="mpc", qp=c.regulator._solver()) if k == "mpc" else
                     dict(kind="nn", weights=c.regulator_weights, with_uprev=c.nnwithuprev, xscale=np.ravel(c.xscale))
                     if k == "nn" else dict(kind="satdlqr", Kaug=c.Kaug) if k == "satdlqr" else dict(kind="us"))
    inst_slot = np.repeat(np.arange(len(slots)), 2).astype(np.int32)
    scen = np.tile([0, 1], len(slots)).astype(np.int32)
    nb, Ny = inst_slot.size, b["pl"]["C"].shape[0]
    np.random.seed(99)
    V = np.random.randn(101, nb, Ny)
    sig = np.sqrt(np.diag(b["common"]["Rv"]))
    SP = np.stack([s[0] for s in b["scen"]])
    DS = np.stack([s[1] for s in b["scen"]])
    dev = cl.DeviceClosedLoop(cl._model(b["plant"], ctls[0]), ctls[0].target_selector._device(), slots, inst_slot)
    full = dev.run(SP, DS, scen, V, sig)
    dev.reset()
    a = dev.run(SP[:, :40], DS[:, :40], scen, V[:41], sig)
    c = dev.run(SP[:, 40:], DS[:, 40:], scen, V[40:], sig)
    tot, phase, ss = dev.last_ms()
    dev.close()
    mpc = inst_slot == len(slots) - 1
    for k in ("y", "x", "xhat", "avg"):
        joined = np.concatenate((a[k], c[k][1:]), axis=0)
        assert np.array_equal(joined[:, ~mpc], full[k][:, ~mpc]), k
        assert np.abs(joined[:, mpc] - full[k][:, mpc]).max() < 1e-12, k
    for k in ("u", "xs", "us"):
        joined = np.concatenate((a[k], c[k]), axis=0)
        assert np.array_equal(joined[:, ~mpc], full[k][:, ~mpc]) and np.abs(joined - full[k]).max() < 1e-12, k
    assert (full["status"][0] == 0).all() and (full["status"][1] == 0).all()
    assert tot > 0 and ss.shape == (60, len(slots)) and phase["nn"] > 0 and phase["mpc"] > 0


def test_report_functions_match_host_losses(batch_run):
    from industrial_nnmpc_2021_amd import linearMPC as lm, controller_evaluation as ce
    b = batch_run
    common, Nsim = b["common"], 40
    Nx, Nu = common["B"].shape
    mpc = lm.LinearMPCController(N=25, **common)
    rng = np.random.default_rng(7)
    weights = [_weights(rng, 2 * Nx + 2 * Nu, w, Nu) for w in (16, 16, 24, 24)]
    xscale = rng.uniform(0.5, 2.0, Nx)
    scen = [(s[0][:Nsim], s[1][:Nsim]) for s in b["scen"]]
    out = ce.simulate_neural_networks(plant=b["plant"], mpc_controller=mpc, online_test_scenarios=scen,
                                      trained_regulator_weights=weights, num_architectures=2, num_samples=[100, 200],
                                      xscale=xscale, Nsim=Nsim, seed=4)
    loss = out["performance_loss"]
    assert loss.shape == (2, 2, 2) and out["average_speedups"].shape == (2, 2) and len(out["plants"]) == 10
    # the report functions follow the reference's scripts: y_0 = the given plant's y[0], the seed set afterwards
    mpc_h = [_host_loaded(b["plant"], lm.LinearMPCController(N=25, **common), *scen[s], Nsim, 4) for s in range(2)]
    mpc_ell = [h["avg"][-1] for h in mpc_h]
    assert all(np.array_equal(p.y[0], b["plant"].y[0]) for p in out["plants"])
    for a in range(2):
        for k in range(2):
            for s in range(2):
                ctl = ce._get_nn_controller(mpc, weights[2 * a + k], xscale, True)
                h = _host_loaded(b["plant"], ctl, *scen[s], Nsim, 4)
                j = (2 * a + k) * 2 + s
                assert np.abs(np.array(out["plants"][j].y)[:, :, 0] - h["y"]).max() < 2e-4, (a, k, s)
                ell = h["avg"][-1]
                ref = 100 * (ell - mpc_ell[s]) / mpc_ell[s]
                assert abs(loss[a, k, s] - ref) < 1e-3 * max(1.0, abs(ref)), (a, k, s, loss[a, k, s], ref)
    sc = ce.simulate_scenarios(plant=b["plant"], mpc_controller=mpc, controller=ce._get_satdlqr_controller(mpc),
                               online_test_scenarios=scen, Nsim=Nsim, seed=4)
    assert sc["performance_loss"].shape == (2,) and np.isfinite(sc["worst_case_speedups"]).all()
    for s in range(2):
        hs = _host_loaded(b["plant"], ce._get_satdlqr_controller(mpc), *scen[s], Nsim, 4)
        assert np.abs(np.array(sc["plants"][s].u)[:, :, 0] - hs["u"]).max() < 1e-8
        assert abs(sc["performance_loss"][s] - 100 * (hs["avg"][-1] - mpc_ell[s]) / mpc_ell[s]) < 1e-6 * max(1.0, abs(sc["performance_loss"][s]))


def test_validation_rejects_mismatched_controllers(batch_run):
    from industrial_nnmpc_2021_amd import controller_evaluation as ce
    from industrial_nnmpc_2021_amd.closed_loop import simulate_closed_loop_batch
    b = batch_run
    other = dict(b["common"], Qwx=2e-4 * np.eye(b["common"]["A"].shape[0]))
    with pytest.raises(ValueError):
        simulate_closed_loop_batch(b["plant"], [ce.SteadyStateController(**b["common"]), ce.SteadyStateController(**other)],
                                   scenarios=b["scen"], Nsim=10, seeds=[0])


def test_cdu_size_smoke():
    """8 networks of the CDU widths (without uprev, like cdu_train.py) and one MPC instance at the CDU size, 200 steps."""
    from industrial_nnmpc_2021_amd import linearMPC as lm, controller_evaluation as ce, synthetic
    from industrial_nnmpc_2021_amd.closed_loop import simulate_closed_loop_batch
    pl = synthetic.plant("cdu", seed=2)
    rng = np.random.default_rng(3)
    Nx, Nu = pl["B"].shape
    Ny, Nd = pl["C"].shape[0], 4
    Bd = rng.standard_normal((Nx, Nd)) / np.sqrt(Nx)
    H = np.zeros((4, Ny)); H[np.arange(4), Ny - 4 + np.arange(4)] = 1.0
    common = dict(A=pl["A"], B=pl["B"], C=pl["C"], H=H, Qwx=1e-4 * np.eye(Nx), Qwd=1e-2 * np.eye(Nd), Rv=1e-4 * np.eye(Ny),
                  xprior=np.zeros((Nx, 1)), dprior=np.zeros((Nd, 1)), Rs=1e-3 * np.eye(Nu), Qs=np.eye(Ny), Bd=Bd,
                  Cd=np.zeros((Ny, Nd)), usp=np.zeros((Nu, 1)), uprev=np.zeros((Nu, 1)), Q=pl["Q"], R=pl["R"], S=pl["S"],
                  ulb=pl["ulb"], uub=pl["uub"])
    T = 200
    sp = np.zeros((T, Ny)); sp[:, -4:] = np.repeat(rng.uniform(-0.1, 0.1, (2, 4)), T // 2, axis=0)
    ds = np.repeat(rng.uniform(-0.1, 0.1, (2, Nd)), T // 2, axis=0)
    mpc = lm.LinearMPCController(N=pl["N"], **common)
    nns = []
    from tests.helpers import cl_nn_weights
    for j, w in enumerate((832, 896, 960, 1024, 832, 896, 960, 1024)):
        # He-scaled hidden layers, head scaled down: u - us is far above the f32 tolerance of the one-step identity below (with
        # kernels of 0.05 / sqrt(fan-in) it was ~1e-5 and any forward, right or wrong, returned us)
        W = cl_nn_weights(30 + j, 2 * Nx + Nu, [w, w, w], Nu, head_scale=0.5)
        nns.append(ce._get_nn_controller(mpc, W, rng.uniform(0.5, 2.0, Nx), False))
    plant = lm.LinearPlantSimulator(A=pl["A"], B=pl["B"], C=pl["C"], Bp=Bd, Rv=common["Rv"], sample_time=1.0, x0=np.zeros((Nx, 1)))
    res = simulate_closed_loop_batch(plant, [mpc] + nns, scenarios=[(sp, ds)], Nsim=T, seeds=[1])
    for k in ("y", "u", "x", "xhat", "avg"):
        assert np.isfinite(res[k]).all(), k
    assert (res["ts_status"] == 0).all() and (res["reg_status"] == 0).all()
    h = _host(dict(A=pl["A"], B=pl["B"], C=pl["C"], Bp=Bd, Rv=common["Rv"]), lm.LinearMPCController(N=pl["N"], **common),
              sp[:20], ds[:20], 20, 1, np.zeros((Nx, 1)))
    assert np.abs(res["u"][0][:20] - h["u"]).max() < 1e-8 and np.abs(res["avg"][0][:21] - h["avg"]).max() < 1e-8
    # the eight networks: every step of every one against the fp64 oracle on the recorded inputs of that step (f32 tolerance)
    from tests.helpers import cl_assert_one_step_identity
    share, worst = cl_assert_one_step_identity(res, [mpc] + nns, common, 1e-4, "cdu size")
    print(f"cdu size: share on a bound {share:.4f}, worst column error {worst:.3e}")
    assert share <= 0.05, share


def test_baselines_match_reference_fixture(golden_dir):
    """closed_loop_baselines.npz (make_golden_baselines.py): the reference's SatDlqrController, SteadyStateController and a
    short-horizon LinearMPCController through its online_simulation, seed 17.  Pinned: the host classes of this package in the
    host loop, and the device slots of simulate_closed_loop_batch."""
    from industrial_nnmpc_2021_amd import linearMPC as lm, controller_evaluation as ce
    from industrial_nnmpc_2021_amd.closed_loop import simulate_closed_loop_batch
    g = np.load(os.path.join(golden_dir, "closed_loop.npz"))
    f = np.load(os.path.join(golden_dir, "closed_loop_baselines.npz"))
    Nx, Nu = g["B"].shape
    Nd, Nsim = g["Bd"].shape[1], int(g["Nsim"])
    common = dict(A=g["A"], B=g["B"], C=g["C"], H=g["H"], Qwx=g["Qwx"], Qwd=g["Qwd"], Rv=g["Rv"], xprior=np.zeros((Nx, 1)),
                  dprior=np.zeros((Nd, 1)), Rs=g["Rs"], Qs=g["Qs"], Bd=g["Bd"], Cd=g["Cd"], usp=np.zeros((Nu, 1)),
                  uprev=np.zeros((Nu, 1)), Q=g["Q"], R=g["R"], S=g["S"], ulb=g["ulb"], uub=g["uub"])
    mats = dict(A=g["A"], B=g["B"], C=g["C"], Bp=g["Bd"], Rv=g["Rv"])
    mk = dict(satdlqr=lambda: ce.SatDlqrController(**common), us=lambda: ce.SteadyStateController(**common),
              short=lambda: lm.LinearMPCController(N=int(f["short_N"]), **common))
    names = list(mk)
    tol = 1e-6
    for name in names:
        h = _host(mats, mk[name](), g["setpoints"], g["disturbances"], Nsim, 17, np.zeros((Nx, 1)))
        for k in ("y", "u", "x", "xhat"):
            assert np.abs(h[k] - f[f"{name}_{k}"]).max() < tol, ("host", name, k)
        assert np.abs(h["avg"] - f[f"{name}_avg_cost"]).max() < 10 * tol, ("host", name)
    plant = lm.LinearPlantSimulator(x0=np.zeros((Nx, 1)), sample_time=1.0, **mats)
    res = simulate_closed_loop_batch(plant, [mk[n]() for n in names], scenarios=[(g["setpoints"], g["disturbances"])],
                                     Nsim=Nsim, seeds=[17])
    for i, name in enumerate(names):
        for k in ("y", "u", "x", "xhat"):
            assert np.abs(res[k][i] - f[f"{name}_{k}"]).max() < tol, ("device", name, k)
        assert np.abs(res["avg"][i] - f[f"{name}_avg_cost"]).max() < 10 * tol, ("device", name)
    assert max(np.abs(f[f"{n}_u"]).max() for n in names) > 0.999                  # the clip / the bounds are exercised


def test_unreachable_target_stays_inside_its_instance():
    """nnmpc_cl_run calls ts_solve_k through nnmpc_ts_launch_internal (no active / lam_eq outputs, the loop's own stream).  One
    instance gets a setpoint no steady state inside the input box reaches from step t0 on: its ts_status is non-zero from t0, its
    records are non-finite from there (NaN moves are the documented behaviour, not a fault), and every other instance is bit
    for bit what it is in a run without the bad one."""
    from industrial_nnmpc_2021_amd import linearMPC as lm
    from industrial_nnmpc_2021_amd.closed_loop import simulate_closed_loop_batch
    pl, common, scen = _mini_problem()
    mats = dict(A=pl["A"], B=pl["B"], C=pl["C"], Bp=common["Bd"], Rv=common["Rv"])
    plant = lm.LinearPlantSimulator(x0=np.zeros((pl["A"].shape[0], 1)), sample_time=1.0, **mats)
    t0, T = 37, 60
    bad_sp = scen[1][0].copy()
    bad_sp[t0:, :2] = 50.0                                                       # as in test_chain_target_gpu.py: far outside what the box reaches
    scen3 = scen + [(bad_sp, scen[1][1])]
    others = [(c, s, 13) for c in (0, 1, 2, 4, 5, 6) for s in (0, 1)]            # NN x 3, MPC (N = 6), satK, us
    bad = (0, 2, 13)
    mixed = others[:5] + [bad] + others[5:]
    run = lambda inst: simulate_closed_loop_batch(plant, _controllers(common, SPECS), scenarios=scen3, Nsim=T, seeds=[13],
                                                  instances=inst, allow_uncertified=True)
    with_bad, without = run(mixed), run(others)
    j = mixed.index(bad)
    assert with_bad["instances"][j] == bad
    st = with_bad["ts_status"][j]
    assert (st[:t0] == 0).all() and (st[t0:] != 0).all()
    for k in ("us", "xs", "u"):
        assert np.isfinite(with_bad[k][j][:t0]).all() and not np.isfinite(with_bad[k][j][t0:]).any(), k
    for k in ("y", "x", "avg"):                                                  # every later row of the plant's records carries it
        a = with_bad[k][j].reshape(T + 1, -1)
        assert np.isfinite(a[:t0 + 1]).all() and (~np.isfinite(a[t0 + 1:])).any(axis=1).all(), k
    keep = [i for i in range(len(mixed)) if i != j]
    assert [with_bad["instances"][i] for i in keep] == without["instances"]
    assert (without["ts_status"] == 0).all() and (without["reg_status"] == 0).all()
    for k in ("y", "x", "xhat", "u", "xs", "us", "avg", "ts_status", "reg_status"):
        assert with_bad[k][keep].tobytes() == without[k].tobytes(), k
