"""The CSTRs-with-flash host model (cstrs_parameters.py, nonlinearMPC.py) against the reference's fixture; no GPU.

cstrs_model.npz holds the reference's _cstrs_ode / _cstrs_measurement on seeded operating-box samples, its rectified xs and
linearisation (DOP853 and differences in place of casadi), the MPC tuning and strided rows of its scenario signals
(tests/golden/make_golden_cstrs.py).
"""
import os

import numpy as np
import pytest
from scipy.integrate import solve_ivp

from industrial_nnmpc_2021_amd import cstrs_parameters as cp
from industrial_nnmpc_2021_amd.nonlinearMPC import SUBSTEPS, DiscreteSimulator, NonlinearPlantSimulator

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "cstrs_model.npz"))


@pytest.fixture(scope="module")
def rectified():
    par = cp._get_cstrs_parameters()
    par["xs"] = cp._get_cstrs_rectified_xs(parameters=par)
    return par


def _dop853(par, x, u, p, tol=1e-13):
    f = cp.CstrsOde(par)
    return solve_ivp(lambda t, z: f(z, u, p), (0.0, par["sample_time"]), x, method="DOP853", rtol=tol, atol=tol).y[:, -1]


def test_parameters_equal_fixture():
    par = cp._get_cstrs_parameters()
    for k in G.files:
        if not k.startswith("par_"):
            continue
        name = k[4:]
        if name in par:
            got = par[name]
        else:
            outer, inner = name.rsplit("_", 1)
            got = par[outer][inner]
        np.testing.assert_array_equal(np.asarray(got, dtype=float), G[k].astype(float), err_msg=name)
    np.testing.assert_array_equal(par["xs"], G["xs_nominal"])


def test_ode_and_measurement_match_fixture():
    par = cp._get_cstrs_parameters()
    for i in range(G["ode_x"].shape[0]):
        x, u, p = G["ode_x"][i], G["ode_u"][i], G["ode_p"][i]
        ref = G["ode_f"][i]
        scale = np.abs(ref).max()
        for got in (cp._cstrs_ode(x, u, p, par), cp._cstrs_ode(x[:, None], u[:, None], p[:, None], par).ravel(),
                    cp._cstrs_ode(x.astype(complex), u, p, par).real):
            assert np.abs(got - ref).max() <= 1e-13 * scale, i
        np.testing.assert_allclose(cp._cstrs_measurement(x, par), G["meas_y"][i], rtol=1e-15, atol=0)
    X, U, P = G["ode_x"][:7].T, G["ode_u"][:7].T, G["ode_p"][:7].T       # columns of several states at once
    assert np.abs(cp._cstrs_ode(X, U, P, par).T - G["ode_f"][:7]).max() <= 1e-13 * np.abs(G["ode_f"][:7]).max()


def test_non_positive_level_gives_nan():
    par = cp._get_cstrs_parameters()
    x = np.zeros(12)
    x[8] = -par["xs"][8] - 1.0                                             # flash level below zero
    assert np.isnan(cp._cstrs_ode(x, np.zeros(6), np.zeros(5), par)).any()
    assert np.isnan(cp._cstrs_ode(x[:, None], np.zeros(6), np.zeros(5), par)).any()


def test_rectified_xs(rectified):
    par = rectified
    f = cp._cstrs_ode(np.zeros(12), np.zeros(6), np.zeros(5), par)
    assert np.abs(f).max() <= 1e-10
    np.testing.assert_allclose(par["xs"], G["xs"], rtol=0, atol=1e-8)


def test_linearisation_matches_flow_map_differences(rectified):
    par = rectified
    A, B, Cm, Bp = cp._get_linearized_model(parameters=par)
    np.testing.assert_array_equal(Cm, np.diag(1 / par["yscale"]))
    z0 = np.zeros(23)
    J = np.empty((12, 23))
    for j in range(23):
        d = 1e-4
        zp, zm = z0.copy(), z0.copy()
        zp[j] += d
        zm[j] -= d
        J[:, j] = (_dop853(par, zp[:12], zp[12:18], zp[18:]) - _dop853(par, zm[:12], zm[12:18], zm[18:])) / (2 * d)
    for got, ref in ((A, J[:, :12]), (B, J[:, 12:18]), (Bp, J[:, 18:])):
        assert np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max()
    for k, v in (("A", A), ("B", B), ("Bp", Bp)):
        np.testing.assert_allclose(v, G[k], rtol=0, atol=1e-6 * np.abs(G[k]).max(), err_msg=k)
    assert np.abs(np.linalg.eigvals(A)).max() < 1.0


def test_host_integrator_against_dop853():
    par = cp._get_cstrs_parameters()
    sim = DiscreteSimulator(cp.CstrsOde(par), par["sample_time"], [12, 6, 5])
    assert sim.substeps == SUBSTEPS
    for i in range(50):
        x, u, p = G["ode_x"][i], G["ode_u"][i], G["ode_p"][i]
        ref = _dop853(par, x, u, p)
        got = sim.sim(x, u, p)
        assert np.abs(got - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max()), i
        # columns of states take the array path: the same numbers
        np.testing.assert_allclose(sim.sim(np.stack([x, x], 1), u[:, None], p[:, None])[:, 0], got, rtol=1e-14, atol=1e-14)


def test_plant_noise_order_and_records(rectified):
    par = rectified
    np.random.seed(3)
    pl = cp._get_cstrs_plant(linear=False, parameters=par)
    np.random.seed(3)
    v0 = np.random.randn(12, 1)
    np.testing.assert_array_equal(pl.y[0], pl.hx.C @ pl.x[0] + pl.measurement_noise_std * v0)
    u, p = 0.1 * np.ones((6, 1)), -0.2 * np.ones((5, 1))
    y1 = pl.step(u, p)
    v1 = np.random.RandomState(3).randn(24)[12:, None]
    np.testing.assert_allclose(y1, pl.hx.C @ pl.x[1] + pl.measurement_noise_std * v1, rtol=1e-15)
    assert len(pl.x) == len(pl.y) == 2 and len(pl.u) == len(pl.p) == 1 and pl.t == [0., 10.]
    np.testing.assert_array_equal(pl.x[1].ravel(), pl.fxup.sim(np.zeros(12), u, p))
    lin = cp._get_cstrs_plant(linear=True, parameters=par)
    np.testing.assert_array_equal(lin.C, pl.hx.C)


def test_controller_tuning_and_scenarios_match_fixture(rectified):
    par = rectified
    pl = cp._get_cstrs_plant(linear=False, parameters=par)
    mpc = cp._get_cstrs_mpc_controller(pl, par, cp.Z_INDICES, cp.EXP_DIST_INDICES)
    for k in ("Qwx", "Qwd", "Rv", "Rs", "Qs", "Cd", "R", "S", "ulb", "uub", "usp", "H"):
        np.testing.assert_array_equal(np.asarray(getattr(mpc, k)), G[k], err_msg=k)
    assert mpc.N == int(G["N"]) == 90 and mpc.H.shape == (0, 12)
    np.testing.assert_allclose(mpc.Q, G["Q"], rtol=1e-14)
    np.testing.assert_allclose(mpc.Bd, G["Bd"], rtol=0, atol=1e-6 * np.abs(G["Bd"]).max())
    scen = cp._get_cstrs_online_test_scenarios(Nsim=4320, z_indices=cp.Z_INDICES, unexp_z_indices=cp.UNEXP_Z_INDICES,
                                               parameters=par, exp_dist_indices=cp.EXP_DIST_INDICES, seed=50, tsteps_steady=5)
    r = G["scen_rows"]
    np.testing.assert_array_equal(scen[0][0][r], G["scen0_sp"])
    np.testing.assert_array_equal(scen[1][0][r], G["scen1_sp"])
    np.testing.assert_array_equal(scen[0][1][r], G["scen_ds"])
    np.testing.assert_array_equal(scen[1][1][r], G["scen_ds"])
    sp, ds = cp._offline_signals(par, cp.Z_INDICES, cp.UNEXP_Z_INDICES, cp.EXP_DIST_INDICES, 150000, 1.02, 1)
    assert sp.shape[0] == int(G["off_len"])
    np.testing.assert_array_equal(sp[G["off_rows"]], G["off_sp"])
    np.testing.assert_array_equal(ds[G["off_rows"]], G["off_ds"])


def test_parameter_dict_factory(rectified):
    d = cp.get_cstrs_parameters_dict(rectified_xs=rectified["xs"])
    assert set(d) == {"plant", "mpc", "us", "satdlqr", "short_horizon", "offline_simulator", "online_test_scenarios",
                      "cstrs_plant_parameters"}
    assert isinstance(d["plant"], NonlinearPlantSimulator) and d["short_horizon"].N == 10 and d["mpc"].N == 90
    assert len(d["online_test_scenarios"]) == 2 and d["online_test_scenarios"][0][0].shape == (4320, 12)
    par = d["cstrs_plant_parameters"]
    assert par["z_indices"] == cp.Z_INDICES and tuple(par["exp_dist_indices"]) == cp.EXP_DIST_INDICES
    blk = cp.device_parameter_block(par)
    assert blk.shape == (51,) and np.array_equal(blk[17:29], par["xs"])


def test_closed_loop_refuses_other_nonlinear_plants_before_device_work(rectified, monkeypatch):
    from industrial_nnmpc_2021_amd import closed_loop as cl
    par = rectified
    good = cp._get_cstrs_plant(linear=False, parameters=par)
    lin = cp._get_cstrs_plant(linear=True, parameters=par)
    A, B, Cm, Bp = lin.A, lin.B, lin.C, lin.Bp
    # a controller object is not needed for the plant checks: _validate looks at the plant first / at shapes only
    ctl = type("Ctl", (), {})()
    for k, v in dict(A=A, B=B, C=Cm, Bd=Bp, H=np.zeros((0, 12))).items():
        setattr(ctl, k, v)

    def no_device(*a, **k):
        raise AssertionError("device work started")
    monkeypatch.setattr(cl, "DeviceClosedLoop", no_device)
    monkeypatch.setattr(cl, "_kind", lambda c: "us")
    scen = [(np.zeros((5, 12)), np.zeros((5, 5)))]
    lam = NonlinearPlantSimulator(fxup=lambda x, u, p: -x, hx=lambda x: x, Rv=par["Rv"], Nx=12, Nu=6, Np=5, Ny=12,
                                  sample_time=10., x0=np.zeros((12, 1)))
    with pytest.raises(TypeError, match="CSTRs"):
        cl.simulate_closed_loop_batch(lam, [ctl], scenarios=scen, Nsim=5, seeds=[0])
    wrong_hx = NonlinearPlantSimulator(fxup=cp.CstrsOde(par), hx=lambda x: x, Rv=par["Rv"], Nx=12, Nu=6, Np=5, Ny=12,
                                       sample_time=10., x0=np.zeros((12, 1)))
    with pytest.raises(TypeError, match="CSTRs"):
        cl.simulate_closed_loop_batch(wrong_hx, [ctl], scenarios=scen, Nsim=5, seeds=[0])
    ctl4 = type("Ctl", (), {})()
    for k, v in dict(A=A, B=B, C=Cm, Bd=Bp[:, :4], H=np.zeros((0, 12))).items():
        setattr(ctl4, k, v)
    with pytest.raises(ValueError, match="Np"):                           # plant Np 5, filter Nd 4
        cl.simulate_closed_loop_batch(good, [ctl4], scenarios=[(np.zeros((5, 12)), np.zeros((5, 4)))], Nsim=5, seeds=[0])
