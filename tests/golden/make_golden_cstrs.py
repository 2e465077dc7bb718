#!/usr/bin/env python3
"""Regenerates cstrs_model.npz and cstrs_closed_loop.npz (run in the BUILD container only, next to make_golden.py).

Imports the reference's cstrs_parameters.py and lib/ with mpctools, cvxopt and h5py stubbed (make_golden.import_reference for
cvxopt / h5py; the QP seam is oracle.qp).  The mpctools stand-ins do not share the package's numerics:
  DiscreteSimulator    scipy DOP853 at rtol = atol = 1e-12 over each sample (not the package's fixed-step RK4);
  getLinearizedModel   central differences of the ODE, then the zero-order hold by scipy.linalg.expm;
  getCasadiFunc        the Python function itself.
Only data is stored:
  cstrs_model.npz        the parameter dict (arrays and scalars), _cstrs_ode / _cstrs_measurement on NODE seeded (x, u, p) of
                         the operating box, the rectified xs (7200 DOP853 samples), (A, B, C, Bp), the MPC's tuning
                         matrices, strided rows of both online test scenarios (Nsim 4320, seed 50) and of the offline
                         simulator's setpoints / disturbances (Nsim 150000, seed 1, conservative factor 1.02)
  cstrs_closed_loop.npz  the reference's online_simulation on its NonlinearPlantSimulator (np.random.seed(SEED) before the
                         plant is built), scenario 0, NSIM steps: MPC (N = 90), short-horizon MPC (N = 10), satK, u = us and
                         one seeded network of the CSTRs input layout (36 inputs, with uprev): y, u, x, xhat, average costs
"""
import os
import sys
import tempfile
import types

import numpy as np
import scipy.linalg
from scipy.integrate import solve_ivp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

REF_ROOT = "/root/reference"
NSIM, SEED, STRIDE_ONLINE, STRIDE_OFFLINE, NODE = 44, 7, 40, 1500, 170
NN_DIMS = [36, 16, 16, 6]


def _stub_mpctools():
    mpc = types.ModuleType("mpctools")

    class DiscreteSimulator:
        def __init__(self, f, Delta, sizes, names):
            self.f, self.Delta = f, float(Delta)

        def sim(self, x, u, p):
            u, p = np.ravel(u), np.ravel(p)
            sol = solve_ivp(lambda t, z: np.ravel(self.f(z, u, p)), (0.0, self.Delta), np.ravel(x).astype(float),
                            method="DOP853", rtol=1e-12, atol=1e-12)
            return sol.y[:, -1]

    def getCasadiFunc(f, sizes, names, funcname=None):
        return f

    def getLinearizedModel(f, args, names, Delta):
        z0 = [np.ravel(a).astype(float) for a in args]
        Nx = z0[0].size
        jac = []
        for k in range(len(z0)):
            J = np.empty((Nx, z0[k].size))
            for j in range(z0[k].size):
                step = 1e-6 * max(1.0, abs(z0[k][j]))
                zp = [a.copy() for a in z0]; zm = [a.copy() for a in z0]
                zp[k][j] += step; zm[k][j] -= step
                J[:, j] = (np.ravel(f(*zp)) - np.ravel(f(*zm))) / (2 * step)
            jac.append(J)
        out = {}
        n = sum(J.shape[1] for J in jac)
        M = np.zeros((n, n))
        M[:Nx, :] = np.hstack(jac)
        E = scipy.linalg.expm(M * Delta)
        out[names[0]] = E[:Nx, :Nx]
        c = Nx
        for name, J in zip(names[1:], jac[1:]):
            out[name] = E[:Nx, c:c + J.shape[1]]
            c += J.shape[1]
        return out

    mpc.DiscreteSimulator = DiscreteSimulator
    mpc.getCasadiFunc = getCasadiFunc
    mpc.util = types.SimpleNamespace(getLinearizedModel=getLinearizedModel)
    sys.modules["mpctools"] = mpc


def box_sample(rng, n):
    """(x, u, p) in the operating box: levels / temperatures around the steady state, fractions inside [0, 1]."""
    X = np.empty((n, 12)); U = rng.uniform(-1, 1, (n, 6)); P = rng.uniform(-1, 1, (n, 5))
    for b in range(3):
        X[:, 4 * b] = rng.uniform(-5, 5, n) if b < 2 else rng.uniform(-1, 1, n)
        xa = rng.uniform(0, 1, n)
        X[:, 4 * b + 1] = xa - 1.0
        X[:, 4 * b + 2] = rng.uniform(0, 1, n) * (1 - xa)
        X[:, 4 * b + 3] = rng.uniform(-10, 10, n)
    return X, U, P


def main():
    _stub_mpctools()
    ref, _ = import_reference()
    sys.path.insert(0, REF_ROOT)
    import cstrs_parameters as cp
    from controller_evaluation import (_get_nn_controller, _get_satdlqr_controller, _get_short_horizon_controller,
                                       _get_us_controller)

    z_indices, unexp_z_indices, exp_dist_indices = (0, 3, 4, 7, 8, 11), [4], (0, 1, 2, 3, 4)
    par = cp._get_cstrs_parameters()
    nominal = dict(par)
    rng = np.random.default_rng(5)
    X, U, P = box_sample(rng, NODE)
    f = np.array([cp._cstrs_ode(X[i], U[i], P[i], nominal) for i in range(NODE)])
    y = np.array([cp._cstrs_measurement(X[i], nominal) for i in range(NODE)])
    par["xs"] = cp._get_cstrs_rectified_xs(parameters=par)
    print("rectified xs - nominal:", par["xs"] - nominal["xs"])
    par["exp_dist_indices"], par["z_indices"], par["unexp_z_indices"] = exp_dist_indices, z_indices, unexp_z_indices
    (A, B, C, Bp) = cp._get_linearized_model(parameters=par)
    plant0 = cp._get_cstrs_plant(linear=False, parameters=par)
    mpc = cp._get_cstrs_mpc_controller(plant0, par, z_indices, exp_dist_indices)
    scen = cp._get_cstrs_online_test_scenarios(Nsim=4320, z_indices=z_indices, unexp_z_indices=unexp_z_indices,
                                               parameters=par, exp_dist_indices=exp_dist_indices, seed=50, tsteps_steady=5)
    off = cp._get_cstrs_offline_simulator(mpc, par, z_indices, unexp_z_indices, exp_dist_indices, Nsim=150000,
                                          num_data_gen_task=1, num_process_per_task=1, conservative_factor=1.02, seed=1)
    off_sp = np.concatenate([np.asarray(s) for s in off.setpoints[0]])
    off_ds = np.concatenate([np.asarray(d) for d in off.disturbances[0]])
    model = dict(ode_x=X, ode_u=U, ode_p=P, ode_f=f, meas_y=y, xs_nominal=nominal["xs"], xs=par["xs"], A=A, B=B, C=C, Bp=Bp,
                 Qwx=mpc.Qwx, Qwd=mpc.Qwd, Rv=mpc.Rv,
                 Rs=mpc.Rs, Qs=mpc.Qs, Bd=mpc.Bd, Cd=mpc.Cd, Q=mpc.Q, R=mpc.R, S=mpc.S, ulb=mpc.ulb, uub=mpc.uub, N=mpc.N,
                 H=mpc.H, usp=mpc.usp, Aaug=mpc.filter.A, Caug=mpc.filter.C, L=mpc.filter.L,
                 scen_rows=np.arange(0, 4320, STRIDE_ONLINE), scen0_sp=scen[0][0][::STRIDE_ONLINE],
                 scen1_sp=scen[1][0][::STRIDE_ONLINE], scen_ds=scen[0][1][::STRIDE_ONLINE],
                 off_rows=np.arange(0, off_sp.shape[0], STRIDE_OFFLINE), off_sp=off_sp[::STRIDE_OFFLINE],
                 off_ds=off_ds[::STRIDE_OFFLINE], off_len=off_sp.shape[0])
    for k, v in nominal.items():
        if isinstance(v, dict):
            for kk, vv in v.items():
                model[f"par_{k}_{kk}"] = vv
        elif k != "xs":
            model[f"par_{k}"] = v
    model = {k: v for k, v in model.items() if v is not None}
    np.savez_compressed(os.path.join(HERE, "cstrs_model.npz"), **model)

    # closed loop on the nonlinear plant, scenario 0
    nrng = np.random.default_rng(11)
    W = []
    for i in range(len(NN_DIMS) - 1):
        W.append(0.2 * nrng.standard_normal((NN_DIMS[i], NN_DIMS[i + 1])) / np.sqrt(NN_DIMS[i]))
        if i < len(NN_DIMS) - 2:
            W.append(0.1 * nrng.standard_normal(NN_DIMS[i + 1]))
    xscale = nrng.uniform(0.5, 2.0, 12)
    makers = dict(mpc=lambda pl: cp._get_cstrs_mpc_controller(pl, par, z_indices, exp_dist_indices),
                  sh=lambda pl: _get_short_horizon_controller(cp._get_cstrs_mpc_controller(pl, par, z_indices,
                                                                                           exp_dist_indices), N=10),
                  satdlqr=lambda pl: _get_satdlqr_controller(cp._get_cstrs_mpc_controller(pl, par, z_indices, exp_dist_indices)),
                  us=lambda pl: _get_us_controller(cp._get_cstrs_mpc_controller(pl, par, z_indices, exp_dist_indices)))
    def mk_nn(pl):
        m = cp._get_cstrs_mpc_controller(pl, par, z_indices, exp_dist_indices)
        return _get_nn_controller(m, W, xscale, True)
    makers["nn"] = mk_nn
    out = {}
    old = sys.stdout
    for name, mk in makers.items():
        np.random.seed(SEED)
        pl = cp._get_cstrs_plant(linear=False, parameters=par)
        ctl = mk(pl)
        with tempfile.NamedTemporaryFile("w") as tf:
            try:
                ref.online_simulation(pl, ctl, setpoints=scen[0][0][:NSIM], disturbances=scen[0][1][:NSIM], Nsim=NSIM,
                                      stdout_filename=tf.name)
            finally:
                sys.stdout.close(); sys.stdout = old
        out[f"{name}_y"] = np.array(pl.y)[:, :, 0]; out[f"{name}_u"] = np.array(pl.u)[:, :, 0]
        out[f"{name}_x"] = np.array(pl.x)[:, :, 0]
        out[f"{name}_xhat"] = np.array(ctl.filter.xhat)[:, :, 0]
        out[f"{name}_avg_cost"] = np.array(ctl.average_stage_costs).ravel()
        print("cstrs closed loop", name, "max |u|", np.abs(out[f"{name}_u"]).max(), "final avg cost", out[f"{name}_avg_cost"][-1])
    np.savez_compressed(os.path.join(HERE, "cstrs_closed_loop.npz"), Nsim=NSIM, seed=SEED, xscale=xscale, nW=len(W),
                        **{f"W{i}": w for i, w in enumerate(W)}, **out)


if __name__ == "__main__":
    main()
