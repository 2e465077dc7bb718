#!/usr/bin/env python3
"""Regenerates closed_loop_baselines.npz (run in the BUILD container only, next to make_golden.py).

The reference's online_simulation (lib/linearMPC.py:703-718) on the plant of closed_loop.npz with the baseline controllers
of the closed-loop evaluation: SatDlqrController and SteadyStateController (lib/controller_evaluation.py:918-1087) and a
short-horizon LinearMPCController (_get_short_horizon_controller, :733-752; the oracle solves its QPs at the cvxopt seam).
np.random.seed(17) before the plant is built, as in closed_loop.npz.  Only data is stored: y, u, x, xhat and the average
stage costs of each run.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

SHORT_N = 3


def main():
    ref, ce = import_reference()
    g = np.load(os.path.join(HERE, "closed_loop.npz"))
    Nx, Nu = g["B"].shape
    Nd, Nsim = g["Bd"].shape[1], int(g["Nsim"])
    common = dict(A=g["A"], B=g["B"], C=g["C"], H=g["H"], Qwx=g["Qwx"], Qwd=g["Qwd"], Rv=g["Rv"], xprior=np.zeros((Nx, 1)),
                  dprior=np.zeros((Nd, 1)), Rs=g["Rs"], Qs=g["Qs"], Bd=g["Bd"], Cd=g["Cd"], usp=np.zeros((Nu, 1)),
                  uprev=np.zeros((Nu, 1)), Q=g["Q"], R=g["R"], S=g["S"], ulb=g["ulb"], uub=g["uub"])
    makers = dict(satdlqr=lambda: ce.SatDlqrController(**common), us=lambda: ce.SteadyStateController(**common),
                  short=lambda: ref.LinearMPCController(N=SHORT_N, **common))
    out = {}
    old = sys.stdout
    for name, mk in makers.items():
        np.random.seed(17)
        pl = ref.LinearPlantSimulator(A=g["A"], B=g["B"], C=g["C"], Bp=g["Bd"], Rv=g["Rv"], sample_time=1.0, x0=np.zeros((Nx, 1)))
        ctl = mk()
        with tempfile.NamedTemporaryFile("w") as tf:
            try:
                ref.online_simulation(pl, ctl, setpoints=g["setpoints"], disturbances=g["disturbances"], Nsim=Nsim,
                                      stdout_filename=tf.name)
            finally:
                sys.stdout.close(); sys.stdout = old
        out[f"{name}_y"] = np.array(pl.y)[:, :, 0]; out[f"{name}_u"] = np.array(pl.u)[:, :, 0]; out[f"{name}_x"] = np.array(pl.x)[:, :, 0]
        out[f"{name}_xhat"] = np.array(ctl.filter.xhat)[:, :, 0]
        out[f"{name}_avg_cost"] = np.array(ctl.average_stage_costs).ravel()
        if name == "satdlqr":
            out["satdlqr_Kaug"] = ctl.Kaug
        print("baseline", name, "max |u|", np.abs(out[f"{name}_u"]).max(), "final avg cost", out[f"{name}_avg_cost"][-1])
    np.savez_compressed(os.path.join(HERE, "closed_loop_baselines.npz"), short_N=SHORT_N, **out)


if __name__ == "__main__":
    main()
