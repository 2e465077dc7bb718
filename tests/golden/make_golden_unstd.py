#!/usr/bin/env python3
"""Regenerates the fixtures of the unstructured NN controller (run in the BUILD container only, like make_golden.py, whose
import of the read-only reference and small plant it reuses).  Only data is stored -- no reference source travels.

  nn_unstd_<case>.npz      the reference's NeuralNetworkControllerUnstd._get_control_input (lib/controller_evaluation.py:
                           895-916) on 64 seeded rows: weights [W1, b1, ..., WL, bL] with a head bias of magnitude >= 0.1 in
                           every column, inputs, xscale, bounds, outputs
  closed_loop_unstd.npz    the reference's online_simulation (lib/linearMPC.py:703-718) with NeuralNetworkControllerUnstd on
                           make_golden.py's closed-loop plant, same seed, setpoints and disturbances

Weight scales are chosen so that the reference alone leaves at most 5 % of the recorded moves on a bound (asserted here and
in tests/test_cpu_unstd.py): a clipped entry says nothing about the arithmetic that produced it.
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

MAX_SHARE = 0.05


def unstd_weights(rng, dims, head_scale):
    """He-scaled hidden kernels, small hidden biases, the head's kernel scaled by head_scale, head bias 0.1 .. 0.3 either sign."""
    W = []
    L = len(dims) - 1
    for i in range(L):
        k = rng.standard_normal((dims[i], dims[i + 1])) * np.sqrt(2.0 / dims[i])
        W.append(head_scale * k if i == L - 1 else k)
        if i < L - 1:
            W.append(0.1 * rng.standard_normal(dims[i + 1]))
    W.append(rng.uniform(0.1, 0.3, dims[-1]) * rng.choice([-1.0, 1.0], dims[-1]))
    return W


def share_on_bound(u, ulb, uub):
    return float(((u == np.ravel(ulb)) | (u == np.ravel(uub))).mean())


def make_forward(ce):
    for name, (nx, nu, hid, withu) in {"with_uprev": (5, 3, 16, True), "without_uprev": (6, 2, 24, False)}.items():
        rng = np.random.default_rng(211 + withu)
        din = 2 * nx + (2 if withu else 1) * nu
        W = unstd_weights(rng, [din, hid, hid, nu], head_scale=0.2)
        xscale = rng.uniform(0.5, 3.0, nx)
        ulb, uub = -np.ones((nu, 1)), np.ones((nu, 1))
        stub = types.SimpleNamespace(regulator_weights=W, nnwithuprev=withu, xscale=xscale[:, None], ulb=ulb, uub=uub)
        for meth in ("_get_regulator_nn_output", "_clip_control_input", "_get_control_input", "_get_scaled_x_xs"):
            setattr(stub, meth, types.MethodType(getattr(ce.NeuralNetworkControllerUnstd, meth), stub))
        nb = 64
        x = 2 * rng.standard_normal((nb, nx)); xs = rng.standard_normal((nb, nx))
        us = rng.uniform(-.8, .8, (nb, nu)); uprev = us + rng.uniform(-.5, .5, (nb, nu))
        u = []
        for b in range(nb):
            xsc, xssc = stub._get_scaled_x_xs(x[b][:, None], xs[b][:, None])
            u.append(stub._get_control_input(xsc, uprev[b][:, None], xssc, us[b][:, None]).ravel())
        u = np.array(u)
        share = share_on_bound(u, ulb, uub)
        assert share <= MAX_SHARE and (np.abs(W[-1]) >= 0.1).all(), (name, share)
        np.savez_compressed(os.path.join(HERE, f"nn_unstd_{name}.npz"), nx=nx, nu=nu, withuprev=withu, xscale=xscale,
                            ulb=ulb, uub=uub, x=x, xs=xs, us=us, uprev=uprev, u=u,
                            **{f"W{i}": w for i, w in enumerate(W)}, nW=len(W))
        print("nn_unstd", name, u.shape, "share on a bound", share, "max |u|", np.abs(u).max())


def make_closed_loop(ref, ce):
    """make_golden.make_closed_loop's plant, tuning, scenario and noise seed (the same generator, drawn in the same order)."""
    rng = np.random.default_rng(31)
    Nx, Nu, Ny, Nd, Nsim, seed = 6, 2, 3, 2, 30, 17
    A, B, C = mg.plant(rng, Nx, Nu, Ny, 0.9)
    Bd = rng.standard_normal((Nx, Nd)) / np.sqrt(Nx); Cd = np.zeros((Ny, Nd))
    H = np.eye(1, Ny)
    Q, R, S = 2.0 * C.T @ C, 0.1 * np.eye(Nu), 0.05 * np.eye(Nu)
    Rs, Qs = 1e-3 * np.eye(Nu), np.eye(Ny)
    Qwx, Qwd, Rv = 1e-4 * np.eye(Nx), 1e-2 * np.eye(Nd), 1e-4 * np.eye(Ny)
    ulb, uub = -np.ones((Nu, 1)), np.ones((Nu, 1))
    setpoints = np.repeat(rng.uniform(-0.4, 0.4, (3, Ny)), Nsim // 3 + 1, axis=0)[:Nsim]
    disturbances = np.repeat(rng.uniform(-0.5, 0.5, (2, Nd)), Nsim // 2 + 1, axis=0)[:Nsim]
    common = dict(A=A, B=B, C=C, H=H, Qwx=Qwx, Qwd=Qwd, Rv=Rv, xprior=np.zeros((Nx, 1)), dprior=np.zeros((Nd, 1)),
                  Rs=Rs, Qs=Qs, Bd=Bd, Cd=Cd, usp=np.zeros((Nu, 1)), uprev=np.zeros((Nu, 1)), Q=Q, R=R, S=S, ulb=ulb, uub=uub)
    wrng = np.random.default_rng(231)
    W = unstd_weights(wrng, [2 * Nx + 2 * Nu, 16, 16, Nu], head_scale=0.3)
    xscale = wrng.uniform(0.5, 2.0, Nx)
    old = sys.stdout
    np.random.seed(seed)
    pl = ref.LinearPlantSimulator(A=A, B=B, C=C, Bp=Bd, Rv=Rv, sample_time=1.0, x0=np.zeros((Nx, 1)))
    ctl = ce.NeuralNetworkControllerUnstd(regulator_weights=W, xscale=xscale, nnwithuprev=True, **common)
    with tempfile.NamedTemporaryFile("w") as tf:
        try:
            ref.online_simulation(pl, ctl, setpoints=setpoints, disturbances=disturbances, Nsim=Nsim, stdout_filename=tf.name)
        finally:
            sys.stdout.close(); sys.stdout = old
    out = dict(y=np.array(pl.y)[:, :, 0], u=np.array(pl.u)[:, :, 0], x=np.array(pl.x)[:, :, 0],
               xhat=np.array(ctl.filter.xhat)[:, :, 0], avg_cost=np.array(ctl.average_stage_costs).ravel())
    share = share_on_bound(out["u"], ulb, uub)
    assert share <= MAX_SHARE, share
    np.savez_compressed(os.path.join(HERE, "closed_loop_unstd.npz"), A=A, B=B, C=C, H=H, Bd=Bd, Cd=Cd, Q=Q, R=R, S=S, Rs=Rs, Qs=Qs,
                        Qwx=Qwx, Qwd=Qwd, Rv=Rv, ulb=ulb, uub=uub, Nsim=Nsim, seed=seed, withuprev=True, setpoints=setpoints,
                        disturbances=disturbances, xscale=xscale, nW=len(W), **{f"W{i}": w for i, w in enumerate(W)}, **out)
    print("closed_loop_unstd: share on a bound", share, "max |u|", np.abs(out["u"]).max(), "final avg cost", out["avg_cost"][-1])


def main():
    ref, ce = mg.import_reference()
    make_forward(ce)
    make_closed_loop(ref, ce)


if __name__ == "__main__":
    main()
