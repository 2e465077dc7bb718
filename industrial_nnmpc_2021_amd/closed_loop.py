"""Lock-step closed-loop evaluation on the device (host wrapper over nnmpc_cl_*).

The reference evaluates every controller by ``online_simulation`` (lib/linearMPC.py:703-718), one (controller, scenario,
noise seed) at a time: per step a host Kalman update, a target QP, a regulator QP or NN forward (_simulate_scenarios /
_simulate_neural_networks, lib/controller_evaluation.py:322-523).  ``simulate_closed_loop_batch`` advances ALL instances of an
evaluation together with plant, estimator, running costs and records in HBM (see include/nnmpc.h).  The measurement noise is
drawn on the host with the reference's stream, so the device run reproduces the reference's seeded trajectories, in either of
the reference's two orders: np.random.seed(seed) before the plant is built (its y_0 takes the first draw, then one draw per step;
the default, as make_golden.py runs online_simulation), or -- ``plant_y0=True``, what _simulate_scenarios /
_simulate_neural_networks do with a plant loaded from a pickle (lib/controller_evaluation.py:353-360, :455-460) -- y_0 is the
given plant's y[0] and the seed is set afterwards, so y_{t+1} takes draw t.
"""
import ctypes as C
import types

import numpy as np

from . import _lib

_SHARED = ("A", "B", "C", "H", "Qwx", "Qwd", "Rv", "xprior", "dprior", "Rs", "Qs", "Bd", "Cd", "usp", "uprev", "ulb", "uub",
           "Q", "R", "S")
RECORDS = ("y", "x", "xhat", "u", "xs", "us", "avg", "status")
PHASES = ("filter", "target", "expand", "nn", "mpc", "post")


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class DeviceClosedLoop:
    """Device handle of one evaluation.

    model: dict with nx, nu, ny, nd, nz and the matrices of nnmpc_cl_model (A, B, C, Bp, Aaug, Baug, Caug, L, tb, Qb, Qy,
    q0, Cd, Eb, Xb, Xu, Qaug, Raug, Maug, ulb, uub, x0, xhat0, uprev0); target: the ``target.BatchedTargetSelector`` whose
    handle solves the reduced target problems; slots: dicts with ``kind`` ("mpc" + ``qp`` (qp.BatchedBoxQP), "nn" + ``weights``,
    ``with_uprev``, ``xscale``, "nn_unstd" + the same with the even-length list [W1, b1, ..., WL, bL], "satdlqr" + ``Kaug``,
    "us"); inst_slot: slot of every instance, non-decreasing.  The QP and
    target handles are borrowed: they must outlive this object.
    """

    KINDS = {"mpc": _lib.CL_MPC, "nn": _lib.CL_NN, "satdlqr": _lib.CL_SATDLQR, "us": _lib.CL_US, "nn_unstd": _lib.CL_NN_UNSTD}

    def __init__(self, model, target, slots, inst_slot):
        lib = _lib.load()
        self._lib = lib
        keep = []
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p).value

        def arr(a):
            a = _f(a)
            keep.append(a)
            return p(a)
        m = _lib.ClModel()
        for k in ("nx", "nu", "ny", "nd", "nz"):
            setattr(m, k, int(model[k]))
        for k, _ in _lib.ClModel._fields_[5:]:
            setattr(m, k, arr(model[k]) if model.get(k) is not None else None)
        self.nx, self.nu, self.ny, self.nd, self.nz = (int(model[k]) for k in ("nx", "nu", "ny", "nd", "nz"))
        self.na = self.nx + self.nd
        cs = (_lib.ClSlot * len(slots))()
        for j, s in enumerate(slots):
            cs[j].kind = self.KINDS[s["kind"]]
            if s["kind"] == "mpc":
                cs[j].qp = s["qp"]._h.value
            elif s["kind"] == "satdlqr":
                cs[j].Kaug = arr(s["Kaug"])
            elif s["kind"] in ("nn", "nn_unstd"):
                w = s["weights"]
                if s["kind"] == "nn_unstd":                      # every layer has a bias; a missing one reaches the library as NULL
                    Ws = [_f(a) for a in w[0::2]]
                    bs = [None if a is None else _f(a).ravel() for a in w[1::2]]
                else:
                    Ws = [_f(a) for a in w[0:-1:2]] + [_f(w[-1])]
                    bs = [_f(a).ravel() for a in w[1::2]] + [None]
                L = len(Ws)
                dims = (C.c_int32 * (L + 1))(*([Ws[0].shape[0]] + [a.shape[1] for a in Ws]))
                Wp = (C.c_void_p * L)(*[a.ctypes.data for a in Ws])
                bp = (C.c_void_p * L)(*[None if a is None else a.ctypes.data for a in bs])
                keep += [Ws, bs, dims, Wp, bp]
                cs[j].nlayers, cs[j].dims = L, C.addressof(dims)
                cs[j].W, cs[j].b = C.addressof(Wp), C.addressof(bp)
                cs[j].with_uprev = int(bool(s["with_uprev"]))
                cs[j].xscale = arr(np.ravel(s["xscale"])) if s.get("xscale") is not None else None
        ins = np.ascontiguousarray(inst_slot, np.int32)
        self.nb, self.nslots = ins.size, len(slots)
        self._qps = [s["qp"] for s in slots if s["kind"] == "mpc"]
        self._target = target                                    # keeps the target handle alive
        self._h = C.c_void_p()
        _lib.check(lib.nnmpc_cl_create(C.byref(self._h), C.byref(m), target._h, len(slots), cs, self.nb,
                                       ins.ctypes.data_as(C.POINTER(C.c_int32))), "nnmpc_cl_create")
        self.T_last = 0

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.nnmpc_cl_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def reset(self):
        _lib.check(self._lib.nnmpc_cl_reset(self._h), "nnmpc_cl_reset")

    def run(self, setpoints, disturbances, scen, v, sigma, record=RECORDS, y0=None):
        """setpoints (S, T, Ny), disturbances (S, T, Nd), scen (nb,), v (T + 1, nb, Ny), sigma (Ny,), y0 (nb, Ny) or None (the
        first measurement after create / reset instead of C x0 + sigma o v[0]) -> dict of the records
        named in ``record``: y, x, xhat, avg (T + 1, nb, .) (row 0 = the state at the start of the call), u, xs, us (T, nb, .),
        status = (target status, regulator status) (T, nb) each."""
        sp = _f(setpoints)
        S, T = sp.shape[0], sp.shape[1]
        d = _f(disturbances).reshape(S, T, self.nd)
        v = _f(v).reshape(T + 1, self.nb, self.ny)
        sc = np.ascontiguousarray(scen, np.int32)
        sig = _f(sigma).ravel()
        nb = self.nb
        y0 = None if y0 is None else _f(y0).reshape(nb, self.ny)
        shapes = dict(y=(T + 1, nb, self.ny), x=(T + 1, nb, self.nx), xhat=(T + 1, nb, self.na), u=(T, nb, self.nu),
                      xs=(T, nb, self.nx), us=(T, nb, self.nu), avg=(T + 1, nb))
        out = {k: np.empty(shapes[k]) for k in shapes if k in record}
        st = (np.empty((T, nb), np.int32), np.empty((T, nb), np.int32)) if "status" in record else (None, None)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        _lib.check(self._lib.nnmpc_cl_run(self._h, T, S, p(sp), p(d), p(sc), p(v), p(sig), p(y0),
                                          *[p(out.get(k)) for k in ("y", "x", "xhat", "u", "xs", "us", "avg")],
                                          p(st[0]), p(st[1]), _lib.HOST), "nnmpc_cl_run")
        if st[0] is not None:
            out["status"] = st
        self.T_last = T
        for qp in self._qps:                                     # far-field windows the rounds met (chain.DeviceChains._after_run)
            fa = getattr(qp, "_farfield_auto", None)
            if fa is not None:
                fa()
        return out

    def set_plant_cstrs(self, parameters, sample_time, substeps):
        """Switch the plant to the CSTRs-with-flash ODE (nnmpc_cl_set_plant): ``parameters`` the plant's parameter dict."""
        from .cstrs_parameters import device_parameter_block
        blk = _f(device_parameter_block(parameters))
        _lib.check(self._lib.nnmpc_cl_set_plant(self._h, _lib.CL_PLANT_CSTRS_FLASH, blk.ctypes.data_as(C.c_void_p), blk.size,
                                                float(sample_time), int(substeps)), "nnmpc_cl_set_plant")

    def last_plant_ms(self):
        """Device ms of the nonlinear plant's step kernel summed over the last run (0 for the linear plant)."""
        v = C.c_double()
        _lib.check(self._lib.nnmpc_cl_last_plant_ms(self._h, C.byref(v)), "nnmpc_cl_last_plant_ms")
        return v.value

    def last_ms(self):
        """(total ms, {phase: ms summed over the steps}, slot_step_ms (T, nslots)) of the last run (hipEvent times)."""
        tot = C.c_double()
        ph = np.zeros(6)
        ss = np.zeros((max(self.T_last, 0), self.nslots))
        self._lib.nnmpc_cl_last_ms(self._h, C.byref(tot), ph.ctypes.data_as(C.c_void_p),
                                   ss.ctypes.data_as(C.c_void_p) if ss.size else None)
        return tot.value, dict(zip(PHASES, ph)), ss


def _kind(ctl):
    from .controller_evaluation import (NeuralNetworkController, NeuralNetworkControllerUnstd, SatDlqrController,
                                        SteadyStateController)
    from .linearMPC import LinearMPCController
    if isinstance(ctl, NeuralNetworkControllerUnstd):            # before its base class
        return "nn_unstd"
    if isinstance(ctl, NeuralNetworkController):
        return "nn"
    if isinstance(ctl, SatDlqrController):
        return "satdlqr"
    if isinstance(ctl, SteadyStateController):
        return "us"
    if isinstance(ctl, LinearMPCController) and hasattr(ctl, "regulator"):
        return "mpc"
    raise TypeError(f"simulate_closed_loop_batch: unsupported controller {type(ctl).__name__}")


def _nonlinear(plant):
    """True for a NonlinearPlantSimulator (only the CSTRs-with-flash model runs on the device: TypeError for any other)."""
    from .nonlinearMPC import NonlinearPlantSimulator
    if not isinstance(plant, NonlinearPlantSimulator):
        return False
    from .cstrs_parameters import CstrsMeasurement, CstrsOde
    if not isinstance(getattr(plant.fxup, "fxup", None), CstrsOde) or not isinstance(plant.hx, CstrsMeasurement):
        raise TypeError("simulate_closed_loop_batch: a NonlinearPlantSimulator runs on the device only with the CSTRs-with-flash "
                        "model (fxup = cstrs_parameters.CstrsOde, hx = cstrs_parameters.CstrsMeasurement)")
    return True


def _plant_dims(plant):
    """(Nu, Ny, Np) of a linear or nonlinear plant."""
    if _nonlinear(plant):
        return plant.Nu, plant.Ny, plant.Np
    return plant.B.shape[1], plant.C.shape[0], plant.Bp.shape[1]


def _validate(plant, controllers, scenarios, Nsim, seeds, instances, record):
    """Everything that can be checked without the device; returns (kinds, instances)."""
    if _nonlinear(plant) and (plant.Nx, plant.Nu, plant.Np, plant.Ny) != (12, 6, 5, 12):
        raise ValueError("simulate_closed_loop_batch: the CSTRs-with-flash plant has Nx=12 Nu=6 Np=5 Ny=12")
    if not isinstance(Nsim, (int, np.integer)) or Nsim <= 0:
        raise ValueError("simulate_closed_loop_batch: Nsim must be a positive integer")
    if not controllers:
        raise ValueError("simulate_closed_loop_batch: no controllers")
    kinds = [_kind(c) for c in controllers]
    ref = controllers[0]
    for j, c in enumerate(controllers[1:], 1):
        for k in _SHARED:
            a, b = getattr(ref, k, None), getattr(c, k, None)
            if a is None or b is None or np.shape(a) != np.shape(b) or not np.array_equal(np.asarray(a), np.asarray(b)):
                raise ValueError(f"simulate_closed_loop_batch: controller {j} differs from controller 0 in {k}; all controllers "
                                 "of one evaluation share the filter, target, cost and plant data")
    Nu, Ny, Nd = ref.B.shape[1], ref.C.shape[0], ref.Bd.shape[1]
    for j, (c, k) in enumerate(zip(controllers, kinds)):
        if k == "nn_unstd":
            _check_unstd_weights(j, c, ref.B.shape[0], Nu)
    if _plant_dims(plant) != (Nu, Ny, Nd):
        raise ValueError("simulate_closed_loop_batch: plant and controllers disagree on Nu / Ny / Nd (the plant's Np must "
                         "equal the filter's Nd)")
    if not scenarios:
        raise ValueError("simulate_closed_loop_batch: no scenarios")
    for s, sc in enumerate(scenarios):
        if len(sc) != 2:
            raise ValueError(f"simulate_closed_loop_batch: scenario {s} is not a (setpoints, disturbances) pair")
        sp, ds = np.asarray(sc[0]), np.asarray(sc[1])
        if sp.ndim != 2 or sp.shape[1] != Ny or sp.shape[0] < Nsim or ds.ndim != 2 or ds.shape[1] != Nd or ds.shape[0] < Nsim:
            raise ValueError(f"simulate_closed_loop_batch: scenario {s} needs setpoints (>= Nsim, {Ny}) and disturbances "
                             f"(>= Nsim, {Nd}), got {sp.shape} and {ds.shape}")
    seeds = list(seeds)
    if not seeds:
        raise ValueError("simulate_closed_loop_batch: no seeds")
    if instances is None:
        instances = [(c, s, r) for c in range(len(controllers)) for s in range(len(scenarios)) for r in seeds]
    instances = [tuple(int(a) for a in inst) for inst in instances]
    if not instances:
        raise ValueError("simulate_closed_loop_batch: no instances")
    for inst in instances:
        if len(inst) != 3 or not 0 <= inst[0] < len(controllers) or not 0 <= inst[1] < len(scenarios):
            raise ValueError(f"simulate_closed_loop_batch: instance {inst} is not (controller, scenario, seed) within range")
    bad = set(record) - set(RECORDS)
    if bad:
        raise ValueError(f"simulate_closed_loop_batch: unknown records {sorted(bad)} (known: {RECORDS})")
    return kinds, instances


def _check_unstd_weights(j, ctl, Nx, Nu):
    """The unstructured controller's list [W1, b1, ..., WL, bL]: even length, kernels that chain from the input width
    2 Nx + (2 | 1) Nu to Nu, a bias of its kernel's width on every layer."""
    from .nn import split_unstd_weights
    who = f"simulate_closed_loop_batch: controller {j} (unstructured NN)"
    try:
        Ws, _ = split_unstd_weights(ctl.regulator_weights)
    except ValueError as e:
        raise ValueError(f"{who}: {e}") from None
    din = 2 * Nx + (2 if ctl.nnwithuprev else 1) * Nu
    if Ws[0].shape[0] != din or Ws[-1].shape[1] != Nu:
        raise ValueError(f"{who}: the network maps {Ws[0].shape[0]} inputs to {Ws[-1].shape[1]} outputs, "
                         f"the plant needs {din} -> {Nu}")


def _model(plant, ctl):
    from .target import ReducedTargetProblem
    red = ReducedTargetProblem(ctl.A, ctl.B, ctl.C, ctl.H, ctl.Bd, ctl.Cd, ctl.Qs, ctl.Rs, ctl.usp)
    f = ctl.filter
    Nx, Nu = ctl.B.shape
    # nonlinear plant: the linearisation fills the plant matrices nnmpc_cl_create requires; the integration replaces the step
    A, B, Cm, Bp = (ctl.A, ctl.B, plant.hx.C, ctl.Bd) if _nonlinear(plant) else (plant.A, plant.B, plant.C, plant.Bp)
    return dict(nx=Nx, nu=Nu, ny=ctl.C.shape[0], nd=ctl.Bd.shape[1], nz=red.Nz, A=A, B=B, C=Cm, Bp=Bp,
                Aaug=f.A, Baug=f.B, Caug=f.C, L=f.L, tb=red.tb, Qb=red.Qb, Qy=red.Qy, q0=red.q0, Cd=ctl.Cd, Eb=red.Eb, Xb=red.Xb,
                Xu=red.Xu, Qaug=ctl.Qaug, Raug=np.atleast_2d(ctl.Raug), Maug=ctl.Maug, ulb=ctl.ulb, uub=ctl.uub,
                x0=plant.x[0], xhat0=f.xhat[0], uprev0=ctl.uprev)


def simulate_closed_loop_batch(plant, controllers, *, scenarios, Nsim, seeds, instances=None, record=RECORDS, chunk=None,
                               return_objects=False, allow_uncertified=False, plant_y0=False):
    """All (controller, scenario, seed) instances of an evaluation in one device run.

    plant: a ``LinearPlantSimulator`` (A, B, C, Bp, the noise std of Rv, x[0]; its own noise draws are not used) or a
    ``nonlinearMPC.NonlinearPlantSimulator`` of the CSTRs-with-flash model (``cstrs_parameters._get_cstrs_plant(linear=False)``:
    the ODE is integrated on the device with the host simulator's RK4 scheme, y = C x + noise with C = hx.C; any other
    nonlinear model raises ``TypeError``); controllers:
    ``LinearMPCController`` (any horizon), ``NeuralNetworkController``, ``NeuralNetworkControllerUnstd``, ``SatDlqrController``, ``SteadyStateController`` in
    their initial state, sharing the filter, target, cost and plant data (``ValueError`` otherwise, before any device work);
    scenarios: (setpoints (>= Nsim, Ny), disturbances (>= Nsim, Nd)) pairs; seeds: noise seeds.  ``instances`` defaults to
    controllers x scenarios x seeds as (controller, scenario, seed) triples.  ``chunk``: steps per device call (the state
    carries over; default all Nsim).  Noise: by default every instance's plant is as if built after np.random.seed(seed)
    (y_0 = C x0 + sigma o v_0 with the first draw, then one draw per step: make_golden.py's order); ``plant_y0=True`` keeps the
    given plant's y[0] and seeds afterwards, so y_{t+1} takes draw t -- the order of the reference's evaluation scripts, which
    load an already built plant from a pickle and then seed (lib/controller_evaluation.py:353-360, :455-460).

    Returns a dict: ``instances``, the records named in ``record`` as (n_instances, T(+1), .) arrays -- y, x, xhat, avg with
    Nsim + 1 rows like the reference's lists, u, xs, us, ts_status, reg_status with Nsim -- and ``computation_times``
    (n_instances, Nsim): the per-step device time of the instance's controller phase FOR THE WHOLE LOCK-STEP BATCH (MPC: its
    slot's batched regulator solve, NN: the grouped forward of all networks, satK / us: the expansion kernel).  These are
    not the per-instance batch-1 latencies the reference's time.time() pairs measure.  ``phase_ms``: device time per phase,
    ``plant_ms``: device time of the nonlinear plant's integration (0 for the linear plant), ``wall_s``.  With ``return_objects`` also ``plants`` / ``controllers``: objects with the reference's attributes
    (x, u, y lists; filter.xhat, average_stage_costs, computation_times) that its plotting code reads.
    """
    import time
    kinds, instances = _validate(plant, controllers, scenarios, Nsim, seeds, instances, record)
    rec = set(record)
    if return_objects:
        rec |= {"y", "x", "xhat", "u", "avg"}
    ctl0 = controllers[0]
    model = _model(plant, ctl0)
    target = ctl0.target_selector._device()
    order = sorted(range(len(instances)), key=lambda i: instances[i][0])        # instances of a slot contiguous
    inv = np.argsort(order)
    used = sorted({instances[i][0] for i in order})
    slot_of = {c: j for j, c in enumerate(used)}
    slots = []
    for c in used:
        ctl, k = controllers[c], kinds[c]
        if k == "mpc":
            slots.append(dict(kind="mpc", qp=ctl.regulator._solver()))
        elif k in ("nn", "nn_unstd"):
            slots.append(dict(kind=k, weights=ctl.regulator_weights, with_uprev=ctl.nnwithuprev, xscale=np.ravel(ctl.xscale)))
        elif k == "satdlqr":
            slots.append(dict(kind="satdlqr", Kaug=ctl.Kaug))
        else:
            slots.append(dict(kind="us"))
    inst_slot = np.array([slot_of[instances[i][0]] for i in order], np.int32)
    scen = np.array([instances[i][1] for i in order], np.int32)
    Ny = model["ny"]
    draws = {}
    for r in sorted({inst[2] for inst in instances}):
        np.random.seed(r)
        if plant_y0:                                             # y_0 given, one draw per step; row 0 unused
            draws[r] = np.concatenate((np.zeros((1, Ny)), np.random.randn(Nsim, Ny)))
        else:                                                    # the plant's first draw, then one per step (same stream)
            draws[r] = np.random.randn(Nsim + 1, Ny)
    V = np.stack([draws[instances[i][2]] for i in order], axis=1)                # (Nsim + 1, nb, Ny)
    Y0 = np.tile(np.ravel(plant.y[0]), (len(order), 1)) if plant_y0 else None
    sigma = np.ravel(plant.measurement_noise_std)                               # sqrt(diag(Rv))
    SP = np.stack([np.asarray(s[0], float)[:Nsim] for s in scenarios])
    DS = np.stack([np.asarray(s[1], float)[:Nsim] for s in scenarios]).reshape(len(scenarios), Nsim, -1)
    t0 = time.time()
    dev = DeviceClosedLoop(model, target, slots, inst_slot)
    if _nonlinear(plant):
        try:
            dev.set_plant_cstrs(plant.fxup.fxup.parameters, plant.sample_time, plant.fxup.substeps)
        except Exception:
            dev.close()
            raise
    step = int(chunk or Nsim)
    plant_ms = 0.0
    parts, slot_ms, phase = [], [], dict.fromkeys(("filter", "target", "expand", "nn", "mpc", "post"), 0.0)
    total_ms = 0.0
    try:
        for a in range(0, Nsim, step):
            b = min(Nsim, a + step)
            parts.append(dev.run(SP[:, a:b], DS[:, a:b], scen, V[a:b + 1], sigma, record=rec, y0=Y0 if a == 0 else None))
            tot, ph, ss = dev.last_ms()
            total_ms += tot
            plant_ms += dev.last_plant_ms()
            for k in phase:
                phase[k] += ph[k]
            slot_ms.append(ss)
    finally:
        dev.close()
    wall = time.time() - t0
    out = dict(instances=instances, wall_s=wall, device_ms=total_ms, phase_ms=phase, plant_ms=plant_ms)
    for k in ("y", "x", "xhat", "avg"):
        if k in rec:
            arr = np.concatenate([parts[0][k]] + [p_[k][1:] for p_ in parts[1:]], axis=0)
            out[k] = np.ascontiguousarray(np.swapaxes(arr, 0, 1)[inv])
    for k in ("u", "xs", "us"):
        if k in rec:
            out[k] = np.ascontiguousarray(np.swapaxes(np.concatenate([p_[k] for p_ in parts], axis=0), 0, 1)[inv])
    if "status" in rec:
        for j, name in enumerate(("ts_status", "reg_status")):
            out[name] = np.ascontiguousarray(np.concatenate([p_["status"][j] for p_ in parts], axis=0).T[inv])
    sm = np.concatenate(slot_ms, axis=0)                                         # (Nsim, nslots)
    out["computation_times"] = np.ascontiguousarray(sm[:, inst_slot].T[inv]) * 1e-3
    if "status" in rec and not allow_uncertified:
        for name in ("ts_status", "reg_status"):
            if (out[name] != 0).any():
                i, t = np.argwhere(out[name] != 0)[0]
                raise RuntimeError(f"simulate_closed_loop_batch: {int((out[name] != 0).sum())} {name} entries not 0 (first: "
                                   f"instance {i} {instances[i]}, step {t}); pass allow_uncertified=True to get the records anyway")
    if return_objects:
        out["plants"], out["controllers"] = _objects(out, plant, controllers, instances)
    return out


def _objects(out, plant, controllers, instances):
    """Reference-shaped plant / controller records: lists of column vectors, as online_simulation leaves them."""
    col = lambda a: [r[:, None] for r in a]
    plants, ctls = [], []
    nonlinear = _nonlinear(plant)
    for i, (c, _, _) in enumerate(instances):
        t = list(plant.sample_time * np.arange(out["x"].shape[1]))
        if nonlinear:                                            # NonlinearPlantSimulator's attributes (lib/nonlinearMPC.py:11-48)
            plants.append(types.SimpleNamespace(x=col(out["x"][i]), u=col(out["u"][i]), y=col(out["y"][i]), fxup=plant.fxup,
                                                hx=plant.hx, Nx=plant.Nx, Nu=plant.Nu, Ny=plant.Ny, Np=plant.Np,
                                                measurement_noise_std=plant.measurement_noise_std,
                                                sample_time=plant.sample_time, t=t))
        else:
            plants.append(types.SimpleNamespace(x=col(out["x"][i]), u=col(out["u"][i]), y=col(out["y"][i]), A=plant.A,
                                                B=plant.B, C=plant.C, Bp=plant.Bp, sample_time=plant.sample_time, t=t))
        ctls.append(types.SimpleNamespace(filter=types.SimpleNamespace(xhat=col(out["xhat"][i])),
                                          average_stage_costs=[np.array([[v]]) for v in out["avg"][i]],
                                          computation_times=list(out["computation_times"][i]),
                                          uprev=out["u"][i][-1][:, None], kind=_kind(controllers[c])))
    return plants, ctls


def cstrs_flow(parameters, X, U, P, substeps=None):
    """Device flow map of the CSTRs-with-flash plant (nnmpc_cstrs_flow): rows X (nb, 12), U (nb, 6), P (nb, 5) -> (nb, 12),
    the host nonlinearMPC.DiscreteSimulator's RK4 with the same substeps (default nonlinearMPC.SUBSTEPS)."""
    from .cstrs_parameters import device_parameter_block
    from .nonlinearMPC import SUBSTEPS
    lib = _lib.load()
    X = _f(X).reshape(-1, 12)
    nb = X.shape[0]
    U, P = _f(U).reshape(nb, 6), _f(P).reshape(nb, 5)
    blk = _f(device_parameter_block(parameters))
    out = np.empty_like(X)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(lib.nnmpc_cstrs_flow(nb, p(blk), blk.size, float(parameters["sample_time"]), int(substeps or SUBSTEPS), p(X), p(U),
                                    p(P), p(out), _lib.HOST), "nnmpc_cstrs_flow")
    return out
