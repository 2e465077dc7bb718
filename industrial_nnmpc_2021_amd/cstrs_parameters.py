"""The CSTRs-with-flash plant of the reference's study (cstrs_parameters.py there), rebuilt without casadi.

Two CSTRs in series and a flash drum; 12 states (level H, mass fractions xA / xB, temperature T of each unit), 6 inputs
(feed F0, heat Qr, feed F1, heat Qm, recycle D, heat Qb), 5 disturbances (feed fractions xA0 / xB0 / xA1 / xB1, feed
temperature T0), all in deviation variables about (xs, us, ps) and scaled by uscale / pscale; y = x / yscale.

casadi plays three roles in the reference, replaced here as follows:
  * integrator (mpctools.DiscreteSimulator): ``nonlinearMPC.DiscreteSimulator``, fixed-step fp64 RK4;
  * Jacobians (mpctools.util.getLinearizedModel): complex-step derivatives of ``_cstrs_ode``, then ``linearMPC.c2d`` (the
    zero-order hold by one matrix exponential) over [B, Bp];
  * rectified steady state: the same 7200-sample simulation from the nominal point, with the package's integrator.

``get_cstrs_parameters_dict`` returns what the reference's ``__main__`` pickles (cstrs_parameters.pickle).
"""
import math

import numpy as np

from .controller_evaluation import (_get_satdlqr_controller, _get_short_horizon_controller, _get_us_controller,
                                    sample_prbs_like)
from .linearMPC import LinearMPCController, LinearPlantSimulator, OfflineSimulator, c2d
from .nonlinearMPC import NonlinearPlantSimulator

Z_INDICES = (0, 3, 4, 7, 8, 11)
UNEXP_Z_INDICES = [4]
EXP_DIST_INDICES = (0, 1, 2, 3, 4)

# physical constants in the order of the device's parameter block (include/nnmpc.h, NNMPC_CL_PLANT_CSTRS_FLASH)
CONSTANTS = ("alphaA", "alphaB", "alphaC", "pho", "Cp", "Ar", "Am", "Ab", "kr", "km", "kb", "delH1", "delH2", "EbyR",
             "k1star", "k2star", "Td")


def _rhs(X, U, P, g, exp, sqrt):
    """The 12 right-hand sides from absolute states X (12), inputs U (6), disturbances P (5): floats or arrays."""
    Hr, xAr, xBr, Tr, Hm, xAm, xBm, Tm, Hb, xAb, xBb, Tb = X
    F0, Qr, F1, Qm, D, Qb = U
    xA0, xB0, xA1, xB1, T0 = P
    aA, aB, aC = g["alphaA"], g["alphaB"], g["alphaC"]
    rho, cp = g["pho"], g["Cp"]
    # relative volatility: vapour fractions of the flash
    vden = aA * xAb + aB * xBb + aC * (1 - xAb - xBb)
    xAd, xBd = aA * xAb / vden, aB * xBb / vden
    # outflows through the valves and the purge
    Fr, Fm, Fb = g["kr"] * sqrt(Hr), g["km"] * sqrt(Hm), g["kb"] * sqrt(Hb)
    Fp = 0.01 * D
    # Arrhenius factors, one exponential per reactor temperature
    er, em = exp(-g["EbyR"] / Tr), exp(-g["EbyR"] / Tm)
    k1r, k2r = g["k1star"] * er, g["k2star"] * er
    k1m, k2m = g["k1star"] * em, g["k2star"] * em
    dH1, dH2, Td = g["delH1"], g["delH2"], g["Td"]
    # reactor 1: fresh feed F0 and the recycle D
    mr = rho * g["Ar"] * Hr
    f = [(F0 + D - Fr) / (rho * g["Ar"]),
         (F0 * (xA0 - xAr) + D * (xAd - xAr)) / mr - k1r * xAr,
         (F0 * (xB0 - xBr) + D * (xBd - xBr)) / mr + k1r * xAr - k2r * xBr,
         (F0 * (T0 - Tr) + D * (Td - Tr)) / mr - (k1r * xAr * dH1 + k2r * xBr * dH2) / cp + Qr / (mr * cp)]
    # reactor 2: outflow of reactor 1 and the second feed F1
    mm = rho * g["Am"] * Hm
    f += [(Fr + F1 - Fm) / (rho * g["Am"]),
          (Fr * (xAr - xAm) + F1 * (xA1 - xAm)) / mm - k1m * xAm,
          (Fr * (xBr - xBm) + F1 * (xB1 - xBm)) / mm + k1m * xAm - k2m * xBm,
          (Fr * (Tr - Tm) + F1 * (T0 - Tm)) / mm - (k1m * xAm * dH1 + k2m * xBm * dH2) / cp + Qm / (mm * cp)]
    # flash: vapour (recycle + purge) leaves at the vapour fractions
    mb = rho * g["Ab"] * Hb
    f += [(Fm - Fb - D - Fp) / (rho * g["Ab"]),
          (Fm * (xAm - xAb) - (D + Fp) * (xAd - xAb)) / mb,
          (Fm * (xBm - xBb) - (D + Fp) * (xBd - xBb)) / mb,
          Fm * (Tm - Tb) / mb + Qb / (mb * cp)]
    return f


def _fsqrt(v):
    return math.sqrt(v) if v >= 0 else math.nan     # numpy's real sqrt: NaN below 0


def _fexp(v):
    try:
        return math.exp(v)
    except OverflowError:
        return math.inf


def _fdiv_safe(fn):
    try:
        return fn()
    except ZeroDivisionError:
        return None


def _cstrs_ode(x, u, p, parameters):
    """dx/dt of the deviation state.  x (12,), (12, 1) or (12, n) columns; u, p likewise (6 / 5 rows); real or complex.
    Returns the shape of x."""
    x = np.asarray(x)
    if x.size == 12 and not np.iscomplexobj(x) and not np.iscomplexobj(u) and not np.iscomplexobj(p):
        # one real state: plain floats (the host integrator's 7200-sample rectification is dominated by this call)
        xs, us_, ps = _deviation_offsets(parameters)
        X = [a + b for a, b in zip(x.ravel().tolist(), xs)]
        U = [a * s + b for a, s, b in zip(np.ravel(u).tolist(), us_[0], us_[1])]
        P = [a * s + b for a, s, b in zip(np.ravel(p).tolist(), ps[0], ps[1])]
        f = _fdiv_safe(lambda: _rhs(X, U, P, parameters, _fexp, _fsqrt))
        if f is not None:
            return np.array(f).reshape(x.shape)
    one_d = x.ndim == 1
    col = lambda a: np.asarray(a, dtype=float).reshape(-1, 1)
    X = x.reshape(12, -1) + col(parameters["xs"])
    U = np.asarray(u).reshape(6, -1) * col(parameters["uscale"]) + col(parameters["us"])
    P = np.asarray(p).reshape(5, -1) * col(parameters["pscale"]) + col(parameters["ps"])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        out = np.array(np.broadcast_arrays(*_rhs(X, U, P, parameters, np.exp, np.sqrt)))
    return out.ravel() if one_d else out.reshape(x.shape[0], -1) if x.ndim == 2 else out


def _deviation_offsets(parameters):
    """(xs, (uscale, us), (pscale, ps)) as float lists."""
    fl = lambda k: np.ravel(np.asarray(parameters[k], dtype=float)).tolist()
    return fl("xs"), (fl("uscale"), fl("us")), (fl("pscale"), fl("ps"))


def _cstrs_measurement(x, parameters):
    """y = diag(1 / yscale) C x."""
    Cm = np.diag(1 / np.ravel(parameters["yscale"])) @ parameters["C"]
    return Cm.dot(x)


class CstrsOde:
    """``fxup`` of the nonlinear CSTRs plant: _cstrs_ode with its parameters (the device recognises this type)."""

    def __init__(self, parameters):
        self.parameters = parameters

    def __call__(self, x, u, p):
        return _cstrs_ode(x, u, p, self.parameters)

    def rk4(self, x, u, p, sample_time, substeps):
        """The classical RK4 flow map of nonlinearMPC.DiscreteSimulator for ONE real state, on plain floats (the same
        arithmetic as the array path; the 7200-sample rectification spends its time here).  Returns (12,)."""
        g = self.parameters
        xs, us_, ps = _deviation_offsets(g)
        U = [a * s + b for a, s, b in zip(np.ravel(u).tolist(), us_[0], us_[1])]
        P = [a * s + b for a, s, b in zip(np.ravel(p).tolist(), ps[0], ps[1])]
        x = np.ravel(x).tolist()
        h = sample_time / substeps
        f = lambda z: _rhs([a + b for a, b in zip(z, xs)], U, P, g, _fexp, _fsqrt)
        try:
            for _ in range(substeps):
                k1 = f(x)
                k2 = f([a + (0.5 * h) * b for a, b in zip(x, k1)])
                k3 = f([a + (0.5 * h) * b for a, b in zip(x, k2)])
                k4 = f([a + h * b for a, b in zip(x, k3)])
                x = [a + (h / 6.0) * (((b + 2.0 * c) + 2.0 * d) + e) for a, b, c, d, e in zip(x, k1, k2, k3, k4)]
        except ZeroDivisionError:
            return None
        return np.array(x)


class CstrsMeasurement:
    """``hx`` of the nonlinear CSTRs plant: y = C x with C = diag(1 / yscale) (the device's measurement matrix)."""

    def __init__(self, parameters):
        self.parameters = parameters
        self.C = np.diag(1 / np.ravel(parameters["yscale"])) @ parameters["C"]

    def __call__(self, x):
        return self.C.dot(x)


def _get_cstrs_parameters():
    """Physical constants, nominal steady state, bounds and scalings; sample time in seconds."""
    Nx, Nu, Np, Ny = 12, 6, 5, 12
    par = dict(alphaA=3.5, alphaB=1.1, alphaC=0.5, pho=50., Cp=3., Ar=0.3, Am=2., Ab=4., kr=2.5, km=2.5, kb=1.5,
               delH1=-40, delH2=-50, EbyR=150, k1star=4e-4, k2star=1.8e-6, Td=313)
    par.update(Nx=Nx, Nu=Nu, Ny=Ny, Np=Np, sample_time=10.)
    par["xs"] = np.array([178.56, 1, 0, 313, 190.07, 1, 0, 313, 5.17, 1, 0, 313])
    par["us"] = np.array([2., 0., 1., 0., 30., 0.])
    par["ps"] = np.array([0.8, 0.1, 0.8, 0.1, 313])
    ulb, uub = np.tile([-0.5, -500.], 3), np.tile([0.5, 500.], 3)
    ylb = np.array([-5., 0., 0., -10., -5., 0., 0., -3., -1., 0., 0., -10.])
    yub = np.array([5., 1., 1., 10., 5., 1., 1., 3., 1., 1, 1., 10.])
    plb = np.array([-0.1, -0.1, -0.1, -0.1, -8.])
    pub = np.array([0.05, 0.05, 0.05, 0.05, 8.])
    par["uscale"], par["pscale"], par["yscale"] = 0.5 * (uub - ulb), 0.5 * (pub - plb), 0.5 * (yub - ylb)
    par["lb"] = dict(u=ulb / par["uscale"], y=ylb / par["yscale"], p=plb / par["pscale"])
    par["ub"] = dict(u=uub / par["uscale"], y=yub / par["yscale"], p=pub / par["pscale"])
    par["C"] = np.eye(Nx)
    H = np.zeros((6, Ny))
    H[np.arange(6), list(Z_INDICES)] = 1.
    par["H"] = H
    par["Rv"] = 1e-20 * np.diag(np.array([1e-4, 1e-6, 1e-6, 1e-4] * 3))
    return par


def _get_cstrs_rectified_xs(*, parameters, substeps=None):
    """Nominal xs + the state the plant reaches from it after 7200 samples at (us, ps)."""
    from .nonlinearMPC import SUBSTEPS, DiscreteSimulator
    sim = DiscreteSimulator(CstrsOde(parameters), parameters["sample_time"],
                            [parameters["Nx"], parameters["Nu"], parameters["Np"]], substeps=substeps or SUBSTEPS)
    x = np.zeros(parameters["Nx"])
    u, p = np.zeros(parameters["Nu"]), np.zeros(parameters["Np"])
    for _ in range(7200):
        x = sim.sim(x, u, p)
    return parameters["xs"] + x


def _continuous_jacobians(parameters, x=None, u=None, p=None):
    """(df/dx, df/du, df/dp) by complex-step differentiation (exact to rounding)."""
    Nx, Nu, Np = parameters["Nx"], parameters["Nu"], parameters["Np"]
    x0 = np.zeros(Nx) if x is None else np.ravel(x)
    u0 = np.zeros(Nu) if u is None else np.ravel(u)
    p0 = np.zeros(Np) if p is None else np.ravel(p)
    z0 = np.concatenate((x0, u0, p0)).astype(complex)
    h = 1e-30
    J = np.empty((Nx, z0.size))
    for j in range(z0.size):
        z = z0.copy()
        z[j] += 1j * h
        J[:, j] = np.imag(_cstrs_ode(z[:Nx], z[Nx:Nx + Nu], z[Nx + Nu:], parameters)) / h
    return J[:, :Nx], J[:, Nx:Nx + Nu], J[:, Nx + Nu:]


def _get_linearized_model(*, parameters):
    """(A, B, C, Bp) of the model linearised about (xs, us, ps), zero-order hold over one sample."""
    Ac, Bc, Bpc = _continuous_jacobians(parameters)
    Nu = Bc.shape[1]
    A, BB = c2d(Ac, np.hstack((Bc, Bpc)), parameters["sample_time"])
    Cm = np.diag(1 / np.ravel(parameters["yscale"])) @ parameters["C"]
    return (A, BB[:, :Nu], Cm, BB[:, Nu:])


def _get_cstrs_plant(*, linear, parameters):
    """The linearised (LinearPlantSimulator) or the nonlinear (NonlinearPlantSimulator) plant, x0 = 0."""
    Nx = parameters["Nx"]
    if linear:
        (A, B, Cm, Bp) = _get_linearized_model(parameters=parameters)
        return LinearPlantSimulator(A=A, B=B, C=Cm, Bp=Bp, Rv=parameters["Rv"], sample_time=parameters["sample_time"],
                                    x0=np.zeros((Nx, 1)))
    return NonlinearPlantSimulator(fxup=CstrsOde(parameters), hx=CstrsMeasurement(parameters), Rv=parameters["Rv"], Nx=Nx,
                                   Nu=parameters["Nu"], Np=parameters["Np"], Ny=parameters["Ny"],
                                   sample_time=parameters["sample_time"], x0=np.zeros((Nx, 1)))


def _get_cstrs_mpc_controller(plant, parameters, z_indices, exp_dist_indices, linear_model=None):
    """MPC on the linearised model: no target equalities (H has 0 rows), Rs = 0, Qs on the z outputs, N = 90."""
    (A, B, Cm, Bp) = linear_model if linear_model is not None else _get_linearized_model(parameters=parameters)
    (Nx, Nu), Ny = B.shape, Cm.shape[0]
    Nd = len(exp_dist_indices)
    Bd = Bp[:, list(exp_dist_indices)]
    Qs = np.zeros((Ny, Ny))
    Qs[list(z_indices), list(z_indices)] = 1.
    return LinearMPCController(A=A, B=B, C=Cm, H=np.zeros((0, Ny)),
                               Qwx=1e-16 * np.eye(Nx), Qwd=1e-2 * np.eye(Nd),
                               Rv=1e+20 * np.diag(np.ravel(plant.measurement_noise_std)) ** 2,
                               xprior=plant.x[-1], dprior=np.zeros((Nd, 1)),
                               Rs=np.zeros((Nu, Nu)), Qs=Qs, Bd=Bd, Cd=np.zeros((Ny, Nd)), usp=np.zeros((Nu, 1)),
                               uprev=np.zeros((Nu, 1)), Q=1e+3 * (Cm.T @ Cm), R=0.1 * np.eye(Nu), S=0.1 * np.eye(Nu), N=90,
                               ulb=parameters["lb"]["u"][:, np.newaxis], uub=parameters["ub"]["u"][:, np.newaxis])


def _offline_signals(parameters, z_indices, unexp_z_indices, exp_dist_indices, Nsim, conservative_factor, seed):
    """Setpoints (Nsim, Ny) and disturbances (Nsim, Nd) of the offline data generation."""
    sp = np.zeros((Nsim, parameters["Ny"]))
    ally = sample_prbs_like(num_change=1250, num_steps=Nsim, lb=parameters["lb"]["y"] * conservative_factor,
                            ub=parameters["ub"]["y"] * conservative_factor, mean_change=120, sigma_change=2, seed=seed)
    sp[:, list(z_indices)] = ally[:, list(z_indices)]
    sp[:, list(unexp_z_indices)] = 0.
    ds = sample_prbs_like(num_change=2500, num_steps=Nsim, lb=parameters["lb"]["p"] * conservative_factor,
                          ub=parameters["ub"]["p"] * conservative_factor, mean_change=60, sigma_change=5, seed=seed + 1)
    return sp, ds[:, list(exp_dist_indices)]


def _get_cstrs_offline_simulator(controller, parameters, z_indices, unexp_z_indices, exp_dist_indices, Nsim,
                                 num_data_gen_task, num_process_per_task, conservative_factor, seed):
    """OfflineSimulator on the controller's model and PRBS setpoints / disturbances widened by conservative_factor."""
    sp, ds = _offline_signals(parameters, z_indices, unexp_z_indices, exp_dist_indices, Nsim, conservative_factor, seed)
    c = controller
    return OfflineSimulator(A=c.A, B=c.B, C=c.C, H=c.H, Rs=c.Rs, Qs=c.Qs, Bd=c.Bd, Cd=c.Cd, usp=c.usp, uprev=c.usp,
                            Q=c.Q, R=c.R, S=c.S, ulb=c.ulb, uub=c.uub, N=c.N, xprior=c.xprior, setpoints=sp,
                            disturbances=ds, num_data_gen_task=num_data_gen_task,
                            num_process_per_task=num_process_per_task)


def _get_cstrs_online_test_scenarios(*, Nsim, z_indices, unexp_z_indices, parameters, exp_dist_indices, seed,
                                     tsteps_steady):
    """[(setpoints with the unexpected z zeroed, disturbances), (all z setpoints, disturbances)], steady for tsteps_steady."""
    Ny, Np = parameters["Ny"], parameters["Np"]
    sp = np.zeros((Nsim, Ny))
    ally = sample_prbs_like(num_change=24, num_steps=Nsim, lb=parameters["lb"]["y"], ub=parameters["ub"]["y"],
                            mean_change=180, sigma_change=2, seed=seed)
    sp[:, list(z_indices)] = ally[:, list(z_indices)]
    sp[:tsteps_steady] = 0.
    sp_exp = sp.copy()
    sp_exp[:, list(unexp_z_indices)] = 0.
    ds = sample_prbs_like(num_change=48, num_steps=Nsim, lb=parameters["lb"]["p"], ub=parameters["ub"]["p"],
                          mean_change=90, sigma_change=1, seed=seed + 1)
    ds[:tsteps_steady] = 0.
    return [(sp_exp, ds), (sp.copy(), ds)]


def get_cstrs_parameters_dict(*, rectified_xs=None, offline_Nsim=150000, online_Nsim=4320):
    """What the reference's cstrs_parameters.py pickles: plant (nonlinear), mpc, us, satdlqr, short_horizon (N = 10),
    offline_simulator, online_test_scenarios (seed 50, 5 steady steps), cstrs_plant_parameters.  ``rectified_xs``: a
    precomputed _get_cstrs_rectified_xs result (the 7200-sample simulation takes seconds on the host)."""
    par = _get_cstrs_parameters()
    par["xs"] = _get_cstrs_rectified_xs(parameters=par) if rectified_xs is None else np.array(rectified_xs, dtype=float)
    par["exp_dist_indices"] = EXP_DIST_INDICES
    par["z_indices"] = Z_INDICES
    par["unexp_z_indices"] = UNEXP_Z_INDICES
    plant = _get_cstrs_plant(linear=False, parameters=par)
    mpc = _get_cstrs_mpc_controller(plant, par, Z_INDICES, EXP_DIST_INDICES)
    scen = _get_cstrs_online_test_scenarios(Nsim=online_Nsim, z_indices=Z_INDICES, unexp_z_indices=UNEXP_Z_INDICES,
                                            parameters=par, exp_dist_indices=EXP_DIST_INDICES, seed=50, tsteps_steady=5)
    off = _get_cstrs_offline_simulator(mpc, par, Z_INDICES, UNEXP_Z_INDICES, EXP_DIST_INDICES, Nsim=offline_Nsim,
                                       num_data_gen_task=1, num_process_per_task=1, conservative_factor=1.02, seed=1)
    return dict(plant=plant, mpc=mpc, us=_get_us_controller(mpc), satdlqr=_get_satdlqr_controller(mpc),
                short_horizon=_get_short_horizon_controller(mpc, N=10), offline_simulator=off,
                online_test_scenarios=scen, cstrs_plant_parameters=par)


def device_parameter_block(parameters):
    """The fp64 block of nnmpc_cl_set_plant_cstrs (include/nnmpc.h): 17 constants (CONSTANTS order), xs (12), us (6),
    ps (5), uscale (6), pscale (5)."""
    return np.concatenate([np.array([float(parameters[k]) for k in CONSTANTS])] +
                          [np.ravel(np.asarray(parameters[k], dtype=float)) for k in ("xs", "us", "ps", "uscale", "pscale")])
