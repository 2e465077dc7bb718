"""ms per optimiser step and per epoch of the native training step WITH the tangent loss (train_nn_controller(backend="hip",
tan_weight=w): L = mse + w tan_mse, three stacked row blocks, csrc/nn_train.hip) beside the plain step (w = 0) of the same
build, in the style of scripts/train_bench.py and with its helpers:

  shapes   [536, 832, 832, 832, 32] without uprev and [36, 224, 224, 224, 6] with uprev, batch 2048, --rows synthetic rows,
           validation_split 0.05; synthetic standard-normal directions and targets (the time does not depend on their values)
  clock    train_nn_controller's own (the window opens once the dataset is on the device), one warm-up epoch, then the median
           (min, max) of --repeats runs of --epochs epochs; an epoch is its optimiser steps plus the validation pass
  device   hipEvent times of nnmpc_train_last_ms over the epoch calls of a HipTrainer(tangents=True)

The row count alone predicts 1.5 x the plain step (3 Bp stacked rows for 2 Bp); the launches per step are the plain step's
(6 per layer).  One JSON line per (shape, w).

    python scripts/tan_train_bench.py [--rows 100000] [--batch 2048] [--epochs 5] [--repeats 5] [--shapes cdu,small] [--weight 0.5]
    python scripts/tan_train_bench.py --one-step small     # a single tangent step and nothing else: what a kernel trace counts
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from train_bench import SHAPES, geometry, spread, synthetic   # noqa: E402


def with_tangents(data, nx, nu, seed=1):
    rng = np.random.default_rng(seed)
    n = data["x"].shape[0]
    return dict(data, dx=rng.standard_normal((n, nx)), duprev=rng.standard_normal((n, nu)), du=0.5 * rng.standard_normal((n, nu)))


def run_wall(dims, uprev, data, batch, epochs, repeats, w, vs):
    """ms per epoch over train_nn_controller's own clock, as train_bench.run_wall."""
    import torch
    from industrial_nnmpc_2021_amd.train import RegulatorModel, train_nn_controller
    nx, nu = geometry(dims, uprev)
    kw = dict(backend="hip", batch_size=batch, validation_split=vs, tan_weight=w)
    m, _, _ = train_nn_controller(RegulatorModel(nx, nu, dims, nnwithuprev=uprev), data, epochs=1, **kw)   # warm-up
    per_epoch = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        m, ttime, hist = train_nn_controller(m, data, epochs=epochs, **kw)
        per_epoch.append(1e3 * ttime / epochs)
    return dict(epoch_ms=spread(per_epoch), loss=hist[-1][0])


def trainer(dims, uprev, data, batch, w):
    from industrial_nnmpc_2021_amd.train import HipTrainer, RegulatorModel
    nx, nu = geometry(dims, uprev)
    tr = HipTrainer(RegulatorModel(nx, nu, dims, nnwithuprev=uprev).get_weights(), nx, nu, nnwithuprev=uprev, max_batch=batch,
                    tangents=True)
    tr.set_data(data)
    tr.set_tangents(data)
    tr.set_tan_weight(w)
    return tr


def run_hip_events(dims, uprev, data, batch, epochs, repeats, w, vs):
    """hipEvent times of the epoch calls (device time, no host in it), as train_bench.run_hip_events."""
    n = data["x"].shape[0]
    ntr = n - int(n * vs)
    tr = trainer(dims, uprev, data, batch, w)
    rng = np.random.default_rng(1)
    tr.epoch(rng.permutation(ntr), batch)                                                     # warm-up
    tot, gemm = [], []
    for _ in range(repeats):
        t = g = 0.0
        for _ep in range(epochs):
            tr.epoch(rng.permutation(ntr), batch)
            ge, te = tr.last_ms()
            t += te
            g += ge
        tot.append(t / epochs)
        gemm.append(g / epochs)
    tr.step(np.arange(batch))
    slices = tr.dw_slices()                                                                   # of a full batch
    tr.close()
    return dict(epoch_event_ms=spread(tot), epoch_gemm_event_ms=spread(gemm), dw_slices=slices)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="cdu,small")
    ap.add_argument("--weight", type=float, default=0.5)
    ap.add_argument("--validation-split", type=float, default=0.05)
    ap.add_argument("--one-step", default="", help="shape: one tangent step of a full batch and nothing else (for a kernel trace)")
    a = ap.parse_args()
    if a.one_step:
        dims, uprev = SHAPES[a.one_step]
        nx, nu = geometry(dims, uprev)
        tr = trainer(dims, uprev, with_tangents(synthetic(a.batch, nx, nu), nx, nu), a.batch, a.weight)
        print(json.dumps(dict(shape=a.one_step, one_step_loss=tr.step(np.arange(a.batch)), layers=len(dims) - 1)), flush=True)
        tr.close()
        return
    for sname in a.shapes.split(","):
        dims, uprev = SHAPES[sname]
        nx, nu = geometry(dims, uprev)
        data = with_tangents(synthetic(a.rows, nx, nu), nx, nu)
        vs = a.validation_split
        steps = -(-(a.rows - int(a.rows * vs)) // a.batch)
        out = []
        for w in (a.weight, 0.0):
            r = run_wall(dims, uprev, data, a.batch, a.epochs, a.repeats, w, vs)
            r.update(run_hip_events(dims, uprev, data, a.batch, a.epochs, a.repeats, w, vs))
            r.update(shape=sname, dims=dims, tan_weight=w, rows=a.rows, batch=a.batch, validation_split=vs, steps_per_epoch=steps,
                     step_ms=r["epoch_ms"]["median"] / steps, step_event_ms=r["epoch_event_ms"]["median"] / steps,
                     epochs=a.epochs, repeats=a.repeats)
            out.append(r)
        out[0]["step_event_ratio_to_plain"] = out[0]["step_event_ms"] / out[1]["step_event_ms"]
        out[0]["epoch_ratio_to_plain"] = out[0]["epoch_ms"]["median"] / out[1]["epoch_ms"]["median"]
        for r in out:
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
