#!/usr/bin/env python3
"""Timing and report of the lock-step closed-loop evaluation (closed_loop.simulate_closed_loop_batch).

The reference's evaluation: 4 architectures x 13 training-set sizes = 52 networks (cdu_train.py / cstrs_train.py), each run
in closed loop for 2880 steps (cdu_parameters.py:218), plus the MPC, short-horizon MPC, satK and u = us baselines.  Here
random weights of the reference's widths on a synthetic plant of the reference's size (synthetic.py), one scenario,
``--seeds R`` noise seeds (Monte Carlo).  Prints wall time, per-phase device times per step, the grouped NN forward against
its HBM bound (every step streams all f32 weights: more than the 256 MiB Infinity Cache holds at the CDU size), and the host
online_simulation on a few instances for comparison.  One JSON line per size at the end.

    python scripts/closed_loop_eval.py --size both --steps 2880 --seeds 1

``--unstd K`` adds K unstructured networks (controller_evaluation.NeuralNetworkControllerUnstd: one pass, a bias on the head)
of the same widths to the batch; they share the grouped forward's launches with the structured ones.

``--size cstrs-flash`` is the reference's real CSTRs study instead: its linearised model and controllers, both online test
scenarios for 4320 steps, 48 random networks of its widths, the nonlinear plant integrated on the device (run_cstrs_flash).
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBPS = 6.3                      # measured stream bandwidth
WIDTHS = {"cdu": (832, 896, 960, 1024), "cstrs": (224, 240, 256, 272)}
WITH_UPREV = {"cdu": False, "cstrs": True}       # input widths 536 / 72 of the reference's architectures
SHORT_N = {"cdu": 20, "cstrs": 15}


def problem(size, steps, seed=0):
    from industrial_nnmpc_2021_amd import linearMPC as lm, synthetic
    pl = synthetic.plant(size, seed=seed)
    rng = np.random.default_rng(seed + 1)
    Nx, Nu = pl["B"].shape
    Ny, Nd = pl["C"].shape[0], 4
    Bd = rng.standard_normal((Nx, Nd)) / np.sqrt(Nx)
    H = np.zeros((4, Ny)); H[np.arange(4), Ny - 4 + np.arange(4)] = 1.0
    common = dict(A=pl["A"], B=pl["B"], C=pl["C"], H=H, Qwx=1e-4 * np.eye(Nx), Qwd=1e-2 * np.eye(Nd), Rv=1e-4 * np.eye(Ny),
                  xprior=np.zeros((Nx, 1)), dprior=np.zeros((Nd, 1)), Rs=1e-3 * np.eye(Nu), Qs=np.eye(Ny), Bd=Bd,
                  Cd=np.zeros((Ny, Nd)), usp=np.zeros((Nu, 1)), uprev=np.zeros((Nu, 1)), Q=pl["Q"], R=pl["R"], S=pl["S"],
                  ulb=pl["ulb"], uub=pl["uub"])
    nchg = max(1, steps // 240)
    sp = np.zeros((steps, Ny))
    sp[:, -4:] = np.repeat(rng.uniform(-0.1, 0.1, (nchg, 4)), -(-steps // nchg), axis=0)[:steps]
    ds = np.repeat(rng.uniform(-0.1, 0.1, (nchg, Nd)), -(-steps // nchg), axis=0)[:steps]
    plant = lm.LinearPlantSimulator(A=pl["A"], B=pl["B"], C=pl["C"], Bp=Bd, Rv=common["Rv"], sample_time=1.0, x0=np.zeros((Nx, 1)))
    return pl, common, plant, [(sp, ds)]


def networks(size, Nx, Nu, nets, rng):
    din = 2 * Nx + (2 if WITH_UPREV[size] else 1) * Nu
    out = []
    for j in range(nets):
        w = WIDTHS[size][j * 4 // nets if nets >= 4 else j % 4]
        dims = [din, w, w, w, Nu]
        W = []
        for i in range(4):
            W.append((0.05 * rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float64))
            if i < 3:
                W.append(0.01 * rng.standard_normal(dims[i + 1]))
        out.append(W)
    return out


def unstd_networks(size, Nx, Nu, nets, rng):
    """``networks`` with a head bias: the even-length list [W1, b1, ..., WL, bL] of the unstructured controller."""
    return [W + [0.1 * rng.standard_normal(Nu)] for W in networks(size, Nx, Nu, nets, rng)]


def run(size, args):
    from industrial_nnmpc_2021_amd import linearMPC as lm, controller_evaluation as ce
    from industrial_nnmpc_2021_amd.closed_loop import simulate_closed_loop_batch
    t_setup = time.time()
    pl, common, plant, scen = problem(size, args.steps)
    Nx, Nu = pl["B"].shape
    mpc = lm.LinearMPCController(N=pl["N"], **common)
    rng = np.random.default_rng(5)
    Ws = networks(size, Nx, Nu, args.nets, rng)
    xscale = rng.uniform(0.5, 2.0, Nx)
    nns = [ce.NeuralNetworkController(regulator_weights=W, xscale=xscale, nnwithuprev=WITH_UPREV[size], build_forward=False,
                                      **ce._shared(mpc)) for W in Ws]          # the batch run uploads the weights itself
    base = [mpc, ce._get_short_horizon_controller(mpc, SHORT_N[size]), ce._get_satdlqr_controller(mpc), ce._get_us_controller(mpc)]
    ctls = nns + base
    uns = []
    if args.unstd:                                          # after the baselines: the instance order of the rest is unchanged
        Wu = unstd_networks(size, Nx, Nu, args.unstd, np.random.default_rng(6))
        uns = [ce.NeuralNetworkControllerUnstd(regulator_weights=W, xscale=xscale, nnwithuprev=WITH_UPREV[size],
                                               build_forward=False, **ce._shared(mpc)) for W in Wu]
        ctls = ctls + uns
        Ws = Ws + Wu
    nn_bytes = sum(4 * sum(np.asarray(a).size for a in W) for W in Ws)
    # one short run first: the regulators' one-time setup (inverse, far-field factors) and the kernels' first launches
    simulate_closed_loop_batch(plant, ctls, scenarios=scen, Nsim=4, seeds=[0], record=("avg",))
    setup_s = time.time() - t_setup
    res = simulate_closed_loop_batch(plant, ctls, scenarios=scen, Nsim=args.steps, seeds=list(range(args.seeds)),
                                     record=("u", "avg", "status"), chunk=args.chunk)
    T, nb = args.steps, len(res["instances"])
    ph = {k: v / T for k, v in res["phase_ms"].items()}
    nn_bound_ms = nn_bytes / (HBM_TBPS * 1e12) * 1e3
    frac = nn_bound_ms / ph["nn"] if ph["nn"] > 0 else float("nan")
    if uns:
        print(f"[{size}] of the networks below, {len(uns)} are unstructured (one pass, one row per instance)")
    print(f"[{size}] {len(nns) + len(uns)} networks ({nn_bytes / 1e6:.1f} MB f32) + 4 baselines, {len(scen)} scenario x {args.seeds} seed(s) = "
          f"{nb} instances, {T} steps (setup {setup_s:.1f} s)")
    print(f"[{size}] wall {res['wall_s']:.3f} s, device {res['device_ms'] / 1e3:.3f} s, {1e3 * res['wall_s'] / T:.3f} ms per step")
    print(f"[{size}] per step (ms): " + ", ".join(f"{k} {v:.4f}" for k, v in ph.items()))
    print(f"[{size}] grouped NN forward: {ph['nn'] * 1e3:.1f} us per step vs HBM bound {nn_bound_ms * 1e3:.1f} us -> {frac:.2f} of the bound")
    # host online_simulation on a few instances (one network, the MPC) for comparison
    host = {}
    for name, mk in (("nn", lambda: ce._get_nn_controller(mpc, Ws[len(nns) - 1], xscale, WITH_UPREV[size])),
                     ("mpc", lambda: lm.LinearMPCController(N=pl["N"], **common))):
        ctl = mk()
        np.random.seed(0)
        hp = lm.LinearPlantSimulator(A=pl["A"], B=pl["B"], C=pl["C"], Bp=common["Bd"], Rv=common["Rv"], sample_time=1.0,
                                     x0=np.zeros((Nx, 1)))
        t0 = time.time()
        with contextlib.redirect_stdout(io.StringIO()):
            lm.online_simulation(hp, ctl, setpoints=scen[0][0][:args.host_steps], disturbances=scen[0][1][:args.host_steps],
                                 Nsim=args.host_steps)
        host[name] = (time.time() - t0) / args.host_steps
    host_est = ((len(nns) + len(uns)) * args.seeds * host["nn"] + 2 * args.seeds * host["mpc"] + 2 * args.seeds * host["nn"]) * T
    print(f"[{size}] host online_simulation: {1e3 * host['nn']:.2f} ms per NN step, {1e3 * host['mpc']:.2f} ms per MPC step "
          f"-> ~{host_est:.1f} s for the same instances (estimate; baselines priced as NN steps), speed-up {host_est / res['wall_s']:.1f}x")
    loss = 100 * (res["avg"][:len(nns) * args.seeds, -1] - res["avg"][len(nns) * args.seeds, -1]) / res["avg"][len(nns) * args.seeds, -1]
    print(f"[{size}] performance loss of the (random) networks vs MPC: median {np.median(loss):.1f} %")
    extra = {}
    if uns:
        k0 = (len(nns) + len(base)) * args.seeds
        uloss = 100 * (res["avg"][k0:, -1] - res["avg"][len(nns) * args.seeds, -1]) / res["avg"][len(nns) * args.seeds, -1]
        print(f"[{size}] performance loss of the (random) unstructured networks vs MPC: median {np.median(uloss):.1f} %")
        extra = dict(unstd_networks=len(uns))
    return dict(extra, size=size, networks=len(nns), instances=nb, steps=T, wall_s=res["wall_s"], device_s=res["device_ms"] / 1e3,
                phase_ms_per_step=ph, nn_bytes=nn_bytes, nn_bound_us=nn_bound_ms * 1e3, nn_fraction_of_bound=frac,
                host_ms_per_step=dict((k, 1e3 * v) for k, v in host.items()), host_estimate_s=host_est,
                speedup=host_est / res["wall_s"], setup_s=setup_s)


def run_cstrs_flash(args):
    """The reference's CSTRs study end to end (cstrs_parameters.py, cstrs_mpc.py / cstrs_neural_network.py): the real
    linearised model and controllers, both online test scenarios for 4320 steps, the nonlinear CSTRs-with-flash plant
    integrated on the device.  Instances: MPC (N = 90), short-horizon MPC (N = 10), satK, us and 48 random networks of the
    widths of cstrs_train.py (4 architectures x 12 training-set sizes, with uprev), on both scenarios."""
    from industrial_nnmpc_2021_amd import controller_evaluation as ce, cstrs_parameters as cp
    from industrial_nnmpc_2021_amd.closed_loop import simulate_closed_loop_batch
    t0 = time.time()
    par = cp._get_cstrs_parameters()
    par["xs"] = cp._get_cstrs_rectified_xs(parameters=par)
    rect_s = time.time() - t0
    steps = 4320
    plant = cp._get_cstrs_plant(linear=False, parameters=par)
    mpc = cp._get_cstrs_mpc_controller(plant, par, cp.Z_INDICES, cp.EXP_DIST_INDICES)
    scen = cp._get_cstrs_online_test_scenarios(Nsim=steps, z_indices=cp.Z_INDICES, unexp_z_indices=cp.UNEXP_Z_INDICES,
                                               parameters=par, exp_dist_indices=cp.EXP_DIST_INDICES, seed=50, tsteps_steady=5)
    rng = np.random.default_rng(5)
    Ws = networks("cstrs", 12, 6, 48, rng)
    xscale = rng.uniform(0.5, 2.0, 12)
    nns = [ce.NeuralNetworkController(regulator_weights=W, xscale=xscale, nnwithuprev=True, build_forward=False,
                                      **ce._shared(mpc)) for W in Ws]
    base = [mpc, ce._get_short_horizon_controller(mpc, 10), ce._get_satdlqr_controller(mpc), ce._get_us_controller(mpc)]
    ctls = nns + base
    simulate_closed_loop_batch(plant, ctls, scenarios=scen, Nsim=4, seeds=[0], record=("avg",), plant_y0=True)
    setup_s = time.time() - t0
    res = simulate_closed_loop_batch(plant, ctls, scenarios=scen, Nsim=steps, seeds=[0], record=("x", "u", "avg", "status"),
                                     chunk=args.chunk, plant_y0=True, allow_uncertified=True)
    nb = len(res["instances"])
    ph = {k: v / steps for k, v in res["phase_ms"].items()}
    plant_us = 1e3 * res["plant_ms"] / steps
    ok = bool((res["ts_status"] == 0).all() and (res["reg_status"] == 0).all())
    finite = bool(all(np.isfinite(res[k]).all() for k in ("x", "u", "avg")))
    ell = res["avg"][:, -1].reshape(len(ctls), len(scen))
    mpc_ell = ell[len(nns)]
    loss = {name: 100 * (ell[len(nns) + j] - mpc_ell) / mpc_ell for j, name in ((1, "sh"), (2, "satdlqr"), (3, "us"))}
    print(f"[cstrs-flash] {len(nns)} networks + 4 baselines x {len(scen)} scenarios = {nb} instances, {steps} steps, nonlinear "
          f"plant (RK4, {plant.fxup.substeps} substeps of {plant.sample_time / plant.fxup.substeps:g} s); rectified xs "
          f"{rect_s:.1f} s, setup {setup_s:.1f} s")
    print(f"[cstrs-flash] wall {res['wall_s']:.3f} s, device {res['device_ms'] / 1e3:.3f} s, "
          f"{1e3 * res['wall_s'] / steps:.3f} ms per step; all statuses 0: {ok}; finite records: {finite}")
    print("[cstrs-flash] per step (ms): " + ", ".join(f"{k} {v:.4f}" for k, v in ph.items()) + f", plant {plant_us / 1e3:.4f}")
    for name, v in loss.items():
        print(f"[cstrs-flash] performance loss {name} vs MPC: " + ", ".join(f"scenario {s} {x:.2f} %" for s, x in enumerate(v)))
    return dict(size="cstrs-flash", networks=len(nns), instances=nb, steps=steps, wall_s=res["wall_s"],
                device_s=res["device_ms"] / 1e3, phase_ms_per_step=ph, plant_us_per_step=plant_us,
                substeps=plant.fxup.substeps, all_status_zero=ok, finite=finite,
                loss_sh_vs_mpc=list(loss["sh"]), loss_satdlqr_vs_mpc=list(loss["satdlqr"]), loss_us_vs_mpc=list(loss["us"]),
                rectify_s=rect_s, setup_s=setup_s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", choices=("cstrs", "cdu", "both", "cstrs-flash"), default="both")
    ap.add_argument("--steps", type=int, default=2880)
    ap.add_argument("--seeds", type=int, default=1)
    ap.add_argument("--nets", type=int, default=52)
    ap.add_argument("--unstd", type=int, default=0, help="unstructured networks added to the batch (sizes cstrs / cdu)")
    ap.add_argument("--chunk", type=int, default=None, help="steps per device call (records stream back per chunk)")
    ap.add_argument("--host-steps", type=int, default=30)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.size == "cstrs-flash":
        out = [run_cstrs_flash(args)]
    else:
        out = [run(s, args) for s in (("cstrs", "cdu") if args.size == "both" else (args.size,))]
    for o in out:
        print(json.dumps(o))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
