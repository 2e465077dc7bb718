"""ms per optimiser step and per epoch of the structured network's training, three paths on one GPU:

  torch64  train_nn_controller as it stands: stock PyTorch ops in float64 on the device
  torch32  the same with a float32 model
  hip      backend="hip": the native f32 step (csrc/nn_train.hip)

Shapes: the reference sweep's widest network [536, 832, 832, 832, 32] without uprev and [36, 224, 224, 224, 6] with uprev,
batch 2048, synthetic rows, validation_split 0.05, one warm-up epoch and then --repeats timed runs of --epochs epochs each
(min / median / max over the runs are reported).  An epoch is its optimiser steps plus the validation pass, as fit() runs
it.  Every path is timed by train_nn_controller's own clock, which starts once the dataset is on the device, so the
three windows hold the same work.  The hip path also reports the hipEvent times of nnmpc_train_last_ms and the step's
fraction of the 157.3 TF f32 MFMA peak on its own flop count
2 (2B) (3 sum_{l>=1} d_l d_{l+1} + 2 d_0 d_1).  One JSON line per (shape, path).

    python scripts/train_bench.py [--rows 100000] [--batch 2048] [--epochs 5] [--repeats 5] [--paths torch64,torch32,hip] [--shapes cdu,small]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_MFMA = 157.3e12
SHAPES = {"cdu": ([536, 832, 832, 832, 32], False), "small": ([36, 224, 224, 224, 6], True)}


def geometry(dims, uprev):
    nu = dims[-1]
    nx = (dims[0] - (2 if uprev else 1) * nu) // 2
    assert 2 * nx + (2 if uprev else 1) * nu == dims[0]
    return nx, nu


def step_flop(dims, B):
    inner = sum(dims[l] * dims[l + 1] for l in range(1, len(dims) - 1))
    return 2.0 * (2 * B) * (3 * inner + 2 * dims[0] * dims[1])


def synthetic(n, nx, nu, seed=0):
    rng = np.random.default_rng(seed)
    x, xs = rng.standard_normal((n, nx)), 0.3 * rng.standard_normal((n, nx))
    us = rng.uniform(-.5, .5, (n, nu))
    return dict(x=x, xs=xs, us=us, uprev=us + rng.uniform(-.3, .3, (n, nu)),
                u=np.clip(us + 0.5 * rng.standard_normal((n, nu)), -1, 1))


def spread(v):
    v = sorted(v)
    return dict(min=v[0], median=v[len(v) // 2], max=v[-1])


def run_wall(dims, uprev, data, batch, epochs, repeats, path):
    """ms per epoch of train_nn_controller for any path, over ITS OWN clock (the returned training_time): the window opens
    after the dataset is on the device and the optimiser / handle exists and closes after the last epoch and the restore
    of the best weights -- the same window for the three paths, and no part of it depends on --epochs."""
    import torch
    from industrial_nnmpc_2021_amd.train import RegulatorModel, train_nn_controller
    nx, nu = geometry(dims, uprev)
    kw = dict(backend="hip") if path == "hip" else dict(device="cuda")
    m = RegulatorModel(nx, nu, dims, nnwithuprev=uprev, dtype=torch.float32 if path == "torch32" else torch.float64)
    m, _, _ = train_nn_controller(m, data, epochs=1, batch_size=batch, **kw)                  # warm-up
    per_epoch = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        m, ttime, hist = train_nn_controller(m, data, epochs=epochs, batch_size=batch, **kw)   # every epoch ends in a host read of its validation loss
        per_epoch.append(1e3 * ttime / epochs)
    return dict(epoch_ms=spread(per_epoch), loss=hist[-1][0])


def run_hip_events(dims, uprev, data, batch, epochs, repeats):
    """hipEvent times of the epoch calls of a HipTrainer (device time, no host in it)."""
    from industrial_nnmpc_2021_amd.train import HipTrainer, RegulatorModel
    nx, nu = geometry(dims, uprev)
    n = data["x"].shape[0]
    ntr = n - int(n * 0.05)
    tr = HipTrainer(RegulatorModel(nx, nu, dims, nnwithuprev=uprev).get_weights(), nx, nu, nnwithuprev=uprev, max_batch=batch)
    tr.set_data(data)
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
    ap.add_argument("--paths", default="torch64,torch32,hip")
    ap.add_argument("--shapes", default="cdu,small")
    a = ap.parse_args()
    for sname in a.shapes.split(","):
        dims, uprev = SHAPES[sname]
        nx, nu = geometry(dims, uprev)
        data = synthetic(a.rows, nx, nu)
        ntr = a.rows - int(a.rows * 0.05)
        steps = -(-ntr // a.batch)
        for path in a.paths.split(","):
            r = run_wall(dims, uprev, data, a.batch, a.epochs, a.repeats, path)
            if path == "hip":
                r.update(run_hip_events(dims, uprev, data, a.batch, a.epochs, a.repeats))
                # the epoch's flop: full batches and the short one
                flop = (ntr // a.batch) * step_flop(dims, a.batch) + (step_flop(dims, ntr % a.batch) if ntr % a.batch else 0.0)
                r["step_event_ms"] = r["epoch_event_ms"]["median"] / steps
                r["f32_mfma_peak_fraction"] = flop / (r["epoch_event_ms"]["median"] * 1e-3) / PEAK_F32_MFMA
            r.update(shape=sname, dims=dims, path=path, rows=a.rows, batch=a.batch, steps_per_epoch=steps,
                     step_ms=r["epoch_ms"]["median"] / steps, epochs=a.epochs, repeats=a.repeats)
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
