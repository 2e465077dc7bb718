"""Counterparts of the hot-path pieces of the reference's lib/controller_evaluation.py:
the NN controllers, structured and unstructured (forward on the GPU), and the PRBS sampler / training-data scaling
that sit either side of the offline data-generation path."""
import itertools
import time

import numpy as np

from .linearMPC import LinearMPCController, _save_training_data
from .linearMPC_build import dlqr
from .nn import StructuredNN, UnstructuredNN


def _sample_repeats(num_change, num_simulation_steps, mean_change, sigma_change):
    """(reference :21-29; the removed np.int alias is not used)"""
    repeat = sigma_change * np.random.randn(num_change - 1) + mean_change
    repeat = np.floor(repeat)
    repeat = np.where(repeat <= 0., 0., repeat)
    repeat = np.append(repeat, num_simulation_steps - int(np.sum(repeat)))
    return repeat.astype(int)


def sample_prbs_like(*, num_change, num_steps, lb, ub, mean_change, sigma_change, seed=1):
    """PRBS-like piecewise-constant signal, same stream of numpy draws as the reference (:31-47)."""
    signal_dimension = lb.shape[0]
    lb, ub = lb.squeeze(), ub.squeeze()
    np.random.seed(seed)
    values = (ub - lb) * np.random.rand(num_change, signal_dimension) + lb
    repeat = _sample_repeats(num_change, num_steps, mean_change, sigma_change)
    return np.repeat(values, repeat, axis=0)


def _get_data_for_training(*, data, num_samples, scale=True):
    """First num_samples rows of the generated data; with ``scale`` also xscale = (max - min)/2 of x, x and xs divided
    by it, returned as (data, xscale) -- without, the dict alone (reference :254-271, same return convention)."""
    out = {k: np.asarray(data[k])[0:num_samples, :] for k in ("x", "uprev", "xs", "us", "u")}
    if not scale:
        return out
    xscale = 0.5 * (np.max(out["x"], axis=0) - np.min(out["x"], axis=0))
    out["x"] = out["x"] / xscale
    out["xs"] = out["xs"] / xscale
    return (out, xscale)


get_data_for_training = _get_data_for_training


def _load_training_data(filename):
    """One array per key (reference lib/python_utils.py:44-51); .h5 when h5py wrote it, else the .npz stand-in."""
    try:
        import h5py
        with h5py.File(filename, "r") as f:
            return {k: np.asarray(f.get(k)) for k in f.keys()}
    except (ImportError, OSError):
        with np.load(filename if filename.endswith(".npz") else filename + ".npz") as f:
            return {k: f[k] for k in f.files}


def _post_process_data(*, data_filename, num_data_gen_task, num_process_per_task):
    """Concatenate the per-chain files '<task>-<proc>-<data_filename>' that generate_data wrote, task-major like the
    reference (:273-295): rows of x / uprev / xs / us / u (and the solver's status) stacked, data_gen_time averaged;
    the result is saved under data_filename and returned."""
    training_data = {}
    for (task, process) in itertools.product(range(num_data_gen_task), range(num_process_per_task)):
        sub = _load_training_data(str(task) + '-' + str(process) + '-' + data_filename)
        for key, value in sub.items():
            training_data.setdefault(key, []).append(value)
    for key in training_data:
        if key == 'data_gen_time':
            training_data[key] = np.mean(np.asarray(training_data[key]))
        else:
            training_data[key] = np.concatenate(training_data[key], axis=0)
    _save_training_data(training_data, data_filename)
    return training_data


def relu(x):
    return np.where(x < 0, 0., x)


class NeuralNetworkController(LinearMPCController):
    """Closed-loop NN controller (reference :780-892); the structured forward runs on the GPU."""

    def __init__(self, *, A, B, C, H, Qwx, Qwd, Rv, xprior, dprior, Rs, Qs, Bd, Cd, usp, uprev,
                 ulb, uub, regulator_weights, xscale, nnwithuprev, Q, R, S, build_forward=True):
        self.A, self.B, self.C, self.H = A, B, C, H
        self.Nx, self.Nu, self.Ny, self.Nd = A.shape[0], B.shape[1], C.shape[0], Bd.shape[1]
        self.Qwx, self.Qwd, self.Rv, self.xprior, self.dprior = Qwx, Qwd, Rv, xprior, dprior
        self.Qs, self.Rs, self.Bd, self.Cd, self.usp = Qs, Rs, Bd, Cd, usp
        self.uprev, self.ulb, self.uub, self.Q, self.R, self.S = uprev, ulb, uub, Q, R, S
        self.regulator_weights = regulator_weights
        self.xscale = xscale[:, np.newaxis]
        self.nnwithuprev = nnwithuprev
        self.filter = LinearMPCController.setup_filter(A=A, B=B, C=C, Bd=Bd, Cd=Cd, Qwx=Qwx, Qwd=Qwd, Rv=Rv,
                                                       xprior=xprior, dprior=dprior)
        self.target_selector = LinearMPCController.setup_target_selector(A=A, B=B, C=C, H=H, Bd=Bd, Cd=Cd, usp=usp,
                                                                         Qs=Qs, Rs=Rs, ulb=ulb, uub=uub)
        (_, _, self.Qaug, self.Raug, self.Maug) = LinearMPCController.get_augmented_matrices_for_regulator(A, B, Q, R, S)
        self.computation_times = []
        self.average_stage_costs = [np.zeros((1, 1))]
        # x, xs arrive already divided by xscale (control_law does it), so the kernel gets xscale = None.
        # build_forward=False defers the device handle of the host forward to its first use: a controller that only fills a slot
        # of the lock-step evaluation (closed_loop.py copies the weights itself) does not upload them twice
        self._net = self._make_net() if build_forward else None

    def _make_net(self):
        return StructuredNN(self.regulator_weights, self.Nx, self.Nu, nnwithuprev=self.nnwithuprev,
                            ulb=self.ulb, uub=self.uub, max_batch=1024)

    def control_law(self, ysp, y):
        (xhat, dhat) = LinearMPCController.get_state_estimates(self.filter, y, self.uprev, self.Nx)
        (xs, us) = LinearMPCController.get_target_pair(self.target_selector, ysp, dhat)
        tstart = time.time()
        (xhat_scaled, xs_scaled) = self._get_scaled_x_xs(xhat, xs)
        useq_nn = self._get_control_input(xhat_scaled, self.uprev, xs_scaled, us)
        tend = time.time()
        avg_ell = LinearMPCController.get_updated_average_stage_cost(
            xhat, self.uprev, xs, us, useq_nn[0:self.Nu, :], self.Qaug, self.Raug, self.Maug,
            self.average_stage_costs[-1], len(self.average_stage_costs))
        self.average_stage_costs.append(avg_ell)
        self.uprev = useq_nn[0:self.Nu, :]
        self.computation_times.append(tend - tstart)
        return self.uprev

    def _get_scaled_x_xs(self, x, xs):
        return (x / self.xscale, xs / self.xscale)

    def _get_control_input(self, x, uprev, xs, us):
        """(Nx,1),(Nu,1),(Nx,1),(Nu,1) -> (Nu,1)   (reference :868-875)."""
        return self._get_control_input_batch(x.T, uprev.T, xs.T, us.T).T

    def _get_control_input_batch(self, X, Uprev, Xs, Us):
        """Rows are samples: (B, Nx), (B, Nu), (B, Nx), (B, Nu) -> (B, Nu)."""
        if self._net is None:
            self._net = self._make_net()
        return self._net.forward(X, Uprev if self.nnwithuprev else None, Xs, Us)


class NeuralNetworkControllerUnstd(NeuralNetworkController):
    """The unstructured comparison controller (reference :895-916): u = clip(NN(x/xscale, (uprev), xs/xscale, us)), one pass,
    linear head with a bias; ``regulator_weights`` is the even-length Keras list [W1, b1, ..., WL, bL]."""

    def _make_net(self):
        return UnstructuredNN(self.regulator_weights, self.Nx, self.Nu, nnwithuprev=self.nnwithuprev,
                              ulb=self.ulb, uub=self.uub, max_batch=1024, head_relu=False)


class _BaselineController(LinearMPCController):
    """Filter + target selector + stage cost of LinearMPCController without a regulator: the common part of the reference's
    SatDlqrController and SteadyStateController (lib/controller_evaluation.py:918-1087)."""

    def __init__(self, *, A, B, C, H, Qwx, Qwd, Rv, xprior, dprior, Rs, Qs, Bd, Cd, usp, uprev, ulb, uub, Q, R, S):
        self.A, self.B, self.C, self.H = A, B, C, H
        self.Nx, self.Nu, self.Ny, self.Nd = A.shape[0], B.shape[1], C.shape[0], Bd.shape[1]
        self.Qwx, self.Qwd, self.Rv, self.xprior, self.dprior = Qwx, Qwd, Rv, xprior, dprior
        self.Qs, self.Rs, self.Bd, self.Cd, self.usp = Qs, Rs, Bd, Cd, usp
        self.uprev, self.ulb, self.uub, self.Q, self.R, self.S = uprev, ulb, uub, Q, R, S
        self.filter = LinearMPCController.setup_filter(A=A, B=B, C=C, Bd=Bd, Cd=Cd, Qwx=Qwx, Qwd=Qwd, Rv=Rv,
                                                       xprior=xprior, dprior=dprior)
        self.target_selector = LinearMPCController.setup_target_selector(A=A, B=B, C=C, H=H, Bd=Bd, Cd=Cd, usp=usp,
                                                                         Qs=Qs, Rs=Rs, ulb=ulb, uub=uub)
        (self._Aaug, self._Baug, self.Qaug, self.Raug, self.Maug) = \
            LinearMPCController.get_augmented_matrices_for_regulator(A, B, Q, R, S)
        self.computation_times = []
        self.average_stage_costs = [np.zeros((1, 1))]

    def _move(self, xhat, xs, us):
        raise NotImplementedError

    def control_law(self, ysp, y):
        (xhat, dhat) = LinearMPCController.get_state_estimates(self.filter, y, self.uprev, self.Nx)
        (xs, us) = LinearMPCController.get_target_pair(self.target_selector, ysp, dhat)
        tstart = time.time()
        u = self._move(xhat, xs, us)
        tend = time.time()
        avg_ell = LinearMPCController.get_updated_average_stage_cost(
            xhat, self.uprev, xs, us, u, self.Qaug, self.Raug, self.Maug, self.average_stage_costs[-1],
            len(self.average_stage_costs))
        self.average_stage_costs.append(avg_ell)
        self.uprev = u
        self.computation_times.append(tend - tstart)
        return self.uprev

    def _clip_control_input(self, u):
        u = np.where(u > self.uub, self.uub, u)
        return np.where(u < self.ulb, self.ulb, u)


class SatDlqrController(_BaselineController):
    """u = sat(Kaug [xhat - xs; uprev - us] + us), Kaug the infinite-horizon LQR gain of the augmented regulator
    (reference :918-1005)."""

    def __init__(self, **kw):
        super().__init__(**kw)
        (self.Kaug, _) = dlqr(self._Aaug, self._Baug, self.Qaug, self.Raug, self.Maug)

    def _move(self, xhat, xs, us):
        return self._clip_control_input(self.Kaug @ np.concatenate((xhat - xs, self.uprev - us), axis=0) + us)


class SteadyStateController(_BaselineController):
    """u = us (reference :1007-1087)."""

    def _move(self, xhat, xs, us):
        return us


def _shared(optimal_controller):
    c = optimal_controller
    return dict(A=c.A, B=c.B, C=c.C, H=c.H, Qwx=c.Qwx, Qwd=c.Qwd, Rv=c.Rv, xprior=c.xprior, dprior=c.dprior, Rs=c.Rs, Qs=c.Qs,
                Bd=c.Bd, Cd=c.Cd, usp=c.usp, uprev=c.uprev, ulb=c.ulb, uub=c.uub, Q=c.Q, R=c.R, S=c.S)


def _get_nn_controller(optimal_controller, regulator_weights, xscale, nnwithuprev):
    """(reference :656-682)"""
    return NeuralNetworkController(regulator_weights=regulator_weights, xscale=xscale, nnwithuprev=nnwithuprev,
                                   **_shared(optimal_controller))


def _get_nn_controller_unstd(optimal_controller, regulator_weights, xscale, nnwithuprev):
    """(reference :684-710)"""
    return NeuralNetworkControllerUnstd(regulator_weights=regulator_weights, xscale=xscale, nnwithuprev=nnwithuprev,
                                        **_shared(optimal_controller))


def _get_satdlqr_controller(optimal_controller):
    """(reference :712-731)"""
    return SatDlqrController(**_shared(optimal_controller))


def _get_short_horizon_controller(optimal_controller, N):
    """(reference :733-752)"""
    return LinearMPCController(N=N, **_shared(optimal_controller))


def _get_us_controller(optimal_controller):
    """(reference :754-775)"""
    return SteadyStateController(**_shared(optimal_controller))


def _speedups(mpc_times, ctl_times):
    return np.mean(mpc_times) / np.mean(ctl_times), np.min(mpc_times) / np.max(ctl_times)


def simulate_scenarios(*, plant, mpc_controller, online_test_scenarios, Nsim, controller=None, seed=0, **kw):
    """_simulate_scenarios (reference :322-419) for one controller and its MPC, every scenario in ONE device run
    (closed_loop.simulate_closed_loop_batch).  ``controller=None``: the MPC alone -> plants, controllers, average_comp_time,
    worst_case_comp_time; otherwise also the MPC's instances -> plants, controllers, performance_loss (num_scenarios,),
    average_speedups, worst_case_speedups.  Computation times are per-step device times of the whole lock-step batch.  Noise in
    the reference script's order: y_0 = plant.y[0], np.random.seed(seed) afterwards (simulate_closed_loop_batch, plant_y0=True)."""
    from .closed_loop import simulate_closed_loop_batch
    kw.setdefault("plant_y0", True)
    ctls = [mpc_controller] if controller is None else [controller, mpc_controller]
    ns = len(online_test_scenarios)
    res = simulate_closed_loop_batch(plant, ctls, scenarios=online_test_scenarios, Nsim=Nsim, seeds=[seed],
                                     return_objects=True, **kw)
    if controller is None:
        ct = res["computation_times"]
        return dict(plants=res["plants"], controllers=res["controllers"], average_comp_time=ct.mean(axis=1),
                    worst_case_comp_time=ct.max(axis=1))
    ell = res["avg"][:, -1]
    ctl_ell, mpc_ell = ell[:ns], ell[ns:]
    sp = np.array([_speedups(res["computation_times"][ns + s], res["computation_times"][s]) for s in range(ns)])
    performance_loss = 100 * (ctl_ell - mpc_ell) / mpc_ell
    return dict(plants=res["plants"][:ns], controllers=res["controllers"][:ns], performance_loss=performance_loss,
                average_speedups=sp[:, 0], worst_case_speedups=sp[:, 1], mpc_plants=res["plants"][ns:],
                mpc_controllers=res["controllers"][ns:])


def simulate_neural_networks(*, plant, mpc_controller, online_test_scenarios, trained_regulator_weights, num_architectures,
                             num_samples, xscale, Nsim, nnwithuprev=True, seed=0, **kw):
    """_simulate_neural_networks (reference :421-523): every trained network (architecture-major, like the reference's
    nn_weight_counter) on every scenario, with the MPC's instances in the SAME device run.  Returns performance_loss
    (num_architectures, num_nns_per_architecture, num_scenarios) = 100 (ell_nn - ell_mpc) / ell_mpc, average_comp_time,
    worst_case_comp_time, average_speedups, worst_case_speedups (num_architectures, num_scenarios; the networks that used
    the most samples), plants, controllers.  Computation times are per-step device times of the whole lock-step batch.  Noise
    in the reference script's order: y_0 = plant.y[0], np.random.seed(seed) afterwards (simulate_closed_loop_batch,
    plant_y0=True).  The network controllers are built without a host forward handle: the batch run uploads each network's
    weights once, itself."""
    from .closed_loop import simulate_closed_loop_batch
    kw.setdefault("plant_y0", True)
    nper = len(num_samples)
    ns = len(online_test_scenarios)
    nns = [NeuralNetworkController(regulator_weights=trained_regulator_weights[a * nper + s], xscale=xscale,
                                   nnwithuprev=nnwithuprev, build_forward=False, **_shared(mpc_controller))
           for a in range(num_architectures) for s in range(nper)]
    res = simulate_closed_loop_batch(plant, nns + [mpc_controller], scenarios=online_test_scenarios, Nsim=Nsim,
                                     seeds=[seed], return_objects=True, **kw)
    ell = res["avg"][:, -1].reshape(len(nns) + 1, ns)
    ct = res["computation_times"].reshape(len(nns) + 1, ns, -1)
    nn_metrics = ell[:-1].reshape(num_architectures, nper, ns)
    mpc_metrics = ell[-1][None, :]
    performance_loss = 100 * (nn_metrics - mpc_metrics) / mpc_metrics
    last = [a * nper + nper - 1 for a in range(num_architectures)]
    average_comp_time = np.array([[ct[j, s].mean() for s in range(ns)] for j in last])
    worst_case_comp_time = np.array([[ct[j, s].max() for s in range(ns)] for j in last])
    sp = np.array([[_speedups(ct[-1, s], ct[j, s]) for s in range(ns)] for j in last]).reshape(num_architectures, ns, 2)
    return dict(plants=res["plants"], controllers=res["controllers"], performance_loss=performance_loss,
                average_comp_time=average_comp_time, worst_case_comp_time=worst_case_comp_time,
                average_speedups=sp[..., 0], worst_case_speedups=sp[..., 1])


def simulate_neural_network_unstd(*, plant, mpc_controller, online_test_scenarios, regulator_weights, xscale, Nsim,
                                  nnwithuprev=True, seed=0, **kw):
    """_simulate_neural_network_unstd (reference :525-625): the ONE trained unstructured network on every scenario, with the
    MPC's instances in the same device run (the reference reads the MPC's costs from an earlier run's pickle).  Returns
    performance_loss = 100 (ell_nn - ell_mpc) / ell_mpc, average_comp_time, worst_case_comp_time, average_speedups,
    worst_case_speedups, each (1, num_scenarios) like the reference's arrays, and plants, controllers (the network's).
    Computation times are per-step device times of the whole lock-step batch; noise in the reference script's order
    (simulate_closed_loop_batch, plant_y0=True)."""
    from .closed_loop import simulate_closed_loop_batch
    kw.setdefault("plant_y0", True)
    ns = len(online_test_scenarios)
    nn = NeuralNetworkControllerUnstd(regulator_weights=regulator_weights, xscale=xscale, nnwithuprev=nnwithuprev,
                                      build_forward=False, **_shared(mpc_controller))
    res = simulate_closed_loop_batch(plant, [nn, mpc_controller], scenarios=online_test_scenarios, Nsim=Nsim, seeds=[seed],
                                     return_objects=True, **kw)
    ell = res["avg"][:, -1].reshape(2, ns)
    ct = res["computation_times"].reshape(2, ns, -1)
    performance_loss = 100 * (ell[:1] - ell[1:]) / ell[1:]
    sp = np.array([_speedups(ct[1, s], ct[0, s]) for s in range(ns)])
    return dict(plants=res["plants"][:ns], controllers=res["controllers"][:ns], performance_loss=performance_loss,
                average_comp_time=ct[0].mean(axis=1)[None, :], worst_case_comp_time=ct[0].max(axis=1)[None, :],
                average_speedups=sp[None, :, 0], worst_case_speedups=sp[None, :, 1],
                mpc_plants=res["plants"][ns:], mpc_controllers=res["controllers"][ns:])
