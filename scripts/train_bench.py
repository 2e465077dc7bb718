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
                                  [--validation-split 0.05] [--unstd [--head linear|relu]]

--unstd times the same shapes with the unstructured comparison network (UnstdRegulatorModel, one pass, a bias on the head;
--head relu, the Keras layer as written, is the default) through the same three paths, each in turn: torch64 / torch32 are
train_unstd_nn_controller(backend="torch"), hip is its native one-pass step; the flop count is then 2 B (...), one stacked
pass.  The reference trains it with batch 1024 and validation_split 0.1 (cstrs_train_unstd.py):

    python scripts/train_bench.py --unstd --shapes small --batch 1024 --validation-split 0.1

--sweep cstrs|cdu times a whole sweep of the reference (cstrs_train.py: [36, w, w, w, 6], w in 224 .. 272, 40 000 .. 150 000
rows, batch 1024, validation_split 0.1: 48 networks; cdu_train.py: [536, w, w, w, 32], w in 832 .. 1024, 20 000 .. 357 600
rows, batch 2048, validation_split 0.05: 52 networks) two ways with the same protocol and clock convention:

  loop   the networks one after another, each a HipTrainer: epoch + eval per epoch
  group  one HipGroupTrainer (csrc/nn_train_group.hip): one grouped epoch + one grouped eval per epoch

and prints one JSON line per way: ms per sweep epoch (min / median / max over the runs), and for the group the hipEvent
time, the launches per lock-step step and the fraction of the f32 MFMA peak on the sweep's own flop count.

    python scripts/train_bench.py --sweep cstrs [--epochs 5] [--repeats 5] [--ways loop,group]

--sweep cstrs --unstd [--head linear|relu] times the same 48-member grid with the unstructured comparison network
(UnstdRegulatorModel [36, w, w, w, 6], one pass, a bias on the head): "loop" is 48 HipTrainer(form=...), "group" one
HipGroupTrainer(form=...); the flop count is the one-pass one.
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


def step_flop(dims, B, passes=2):
    inner = sum(dims[l] * dims[l + 1] for l in range(1, len(dims) - 1))
    return 2.0 * (passes * B) * (3 * inner + 2 * dims[0] * dims[1])


def synthetic(n, nx, nu, seed=0):
    rng = np.random.default_rng(seed)
    x, xs = rng.standard_normal((n, nx)), 0.3 * rng.standard_normal((n, nx))
    us = rng.uniform(-.5, .5, (n, nu))
    return dict(x=x, xs=xs, us=us, uprev=us + rng.uniform(-.3, .3, (n, nu)),
                u=np.clip(us + 0.5 * rng.standard_normal((n, nu)), -1, 1))


def spread(v):
    v = sorted(v)
    return dict(min=v[0], median=v[len(v) // 2], max=v[-1])


def run_wall(dims, uprev, data, batch, epochs, repeats, path, vs=0.05, unstd=None):
    """ms per epoch of train_nn_controller (unstd = "linear" | "relu": of train_unstd_nn_controller) for any path, over ITS
    OWN clock (the returned training_time): the window opens after the dataset is on the device and the optimiser / handle
    exists and closes after the last epoch and the restore of the best weights -- the same window for the three paths, and
    no part of it depends on --epochs."""
    import torch
    from industrial_nnmpc_2021_amd.train import (RegulatorModel, UnstdRegulatorModel, train_nn_controller,
                                                 train_unstd_nn_controller)
    nx, nu = geometry(dims, uprev)
    dt = torch.float32 if path == "torch32" else torch.float64
    kw = dict(backend="hip") if path == "hip" else dict(device="cuda", backend="torch")
    kw.update(batch_size=batch, validation_split=vs)
    if unstd:
        m, fit = UnstdRegulatorModel(nx, nu, dims, nnwithuprev=uprev, head_relu=unstd == "relu", dtype=dt), train_unstd_nn_controller
    else:
        m, fit = RegulatorModel(nx, nu, dims, nnwithuprev=uprev, dtype=dt), train_nn_controller
    m, _, _ = fit(m, data, epochs=1, **kw)                                                    # warm-up
    per_epoch = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        m, ttime, hist = fit(m, data, epochs=epochs, **kw)                                    # every epoch ends in a host read of its validation loss
        per_epoch.append(1e3 * ttime / epochs)
    return dict(epoch_ms=spread(per_epoch), loss=hist[-1][0])


def run_hip_events(dims, uprev, data, batch, epochs, repeats, vs=0.05, unstd=None):
    """hipEvent times of the epoch calls of a HipTrainer (device time, no host in it)."""
    from industrial_nnmpc_2021_amd import _lib
    from industrial_nnmpc_2021_amd.train import HipTrainer, RegulatorModel, UnstdRegulatorModel
    nx, nu = geometry(dims, uprev)
    n = data["x"].shape[0]
    ntr = n - int(n * vs)
    if unstd:
        w, form = UnstdRegulatorModel(nx, nu, dims, nnwithuprev=uprev).get_weights(), (_lib.NN_UNSTD_RELU if unstd == "relu" else _lib.NN_UNSTD)
    else:
        w, form = RegulatorModel(nx, nu, dims, nnwithuprev=uprev).get_weights(), _lib.NN_STRUCTURED
    tr = HipTrainer(w, nx, nu, nnwithuprev=uprev, max_batch=batch, form=form)
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


SWEEPS = {
    "cstrs": dict(dims=[[36, w, w, w, 6] for w in (224, 240, 256, 272)], uprev=True, rows=list(range(40000, 150001, 10000)),
                  batch=1024, validation_split=0.1),
    "cdu": dict(dims=[[536, w, w, w, 32] for w in (832, 896, 960, 1024)], uprev=False,
                rows=[20000] + list(range(30000, 330001, 30000)) + [357600], batch=2048, validation_split=0.05),
}


def run_sweep(name, epochs, repeats, ways, unstd=None):
    """unstd = "linear" | "relu": the sweep's grid with the unstructured network of that head, through form=."""
    import itertools
    import time
    from industrial_nnmpc_2021_amd import _lib
    from industrial_nnmpc_2021_amd.train import HipGroupTrainer, HipTrainer, RegulatorModel, UnstdRegulatorModel, group_schedule
    sw = SWEEPS[name]
    uprev, batch, vs = sw["uprev"], sw["batch"], sw["validation_split"]
    members = list(itertools.product(sw["dims"], sw["rows"]))                 # the reference's loop order
    nx, nu = geometry(members[0][0], uprev)
    data = synthetic(max(sw["rows"]), nx, nu)
    if unstd:
        form, passes = (_lib.NN_UNSTD_RELU if unstd == "relu" else _lib.NN_UNSTD), 1
        weights = [UnstdRegulatorModel(nx, nu, d, nnwithuprev=uprev, head_relu=unstd == "relu").get_weights() for d, _ in members]
    else:
        form, passes = _lib.NN_STRUCTURED, 2
        weights = [RegulatorModel(nx, nu, d, nnwithuprev=uprev).get_weights() for d, _ in members]
    nval = [int(n * vs) for _, n in members]
    ntr = [n - v for (_, n), v in zip(members, nval)]
    sched = group_schedule(ntr, batch)
    flop = sum(step_flop(d, B, passes) for (d, _), s in zip(members, sched) for B in s)
    common = dict(sweep=name, form=("unstd_" + unstd) if unstd else "structured", members=len(members), batch=batch, epochs=epochs, repeats=repeats,
                  member_steps_per_epoch=sum(len(s) for s in sched), lockstep_steps_per_epoch=max(len(s) for s in sched))
    if "loop" in ways:
        runs = [0.0] * repeats
        for (d, n), w, a, v in zip(members, weights, ntr, nval):
            tr = HipTrainer(w, nx, nu, nnwithuprev=uprev, max_batch=batch, form=form)
            tr.set_data({k: x[:n] for k, x in data.items()})
            rng = np.random.default_rng(1)
            tr.epoch(rng.permutation(a), batch)                               # warm-up
            tr.eval(a, v)
            for r in range(repeats):
                t0 = time.time()
                for _ep in range(epochs):
                    tr.epoch(rng.permutation(a), batch)
                    tr.eval(a, v)
                runs[r] += time.time() - t0
            tr.close()
        print(json.dumps(dict(common, way="loop", epoch_ms=spread([1e3 * t / epochs for t in runs]))), flush=True)
    if "group" in ways:
        tr = HipGroupTrainer(weights, nx, nu, nnwithuprev=uprev, max_batch=batch, form=form)
        tr.set_data(data)
        rngs = [np.random.default_rng(1) for _ in members]
        tr.epoch([g.permutation(a) for g, a in zip(rngs, ntr)], batch)        # warm-up
        tr.eval(ntr, nval)
        runs, ev, gemm = [], [], []
        for r in range(repeats):
            t0, e, ge = time.time(), 0.0, 0.0
            for _ep in range(epochs):
                tr.epoch([g.permutation(a) for g, a in zip(rngs, ntr)], batch)
                launches = tr.last_launches()
                g_ms, t_ms = tr.last_ms()
                e += t_ms
                ge += g_ms
                tr.eval(ntr, nval)
            runs.append(1e3 * (time.time() - t0) / epochs)
            ev.append(e / epochs)
            gemm.append(ge / epochs)
        tr.close()
        steps = common["lockstep_steps_per_epoch"]
        print(json.dumps(dict(common, way="group", epoch_ms=spread(runs), epoch_event_ms=spread(ev),
                              epoch_gemm_event_ms=spread(gemm), launches_per_lockstep_step=launches / steps,
                              f32_mfma_peak_fraction=flop / (spread(ev)["median"] * 1e-3) / PEAK_F32_MFMA)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--paths", default="torch64,torch32,hip")
    ap.add_argument("--shapes", default="cdu,small")
    ap.add_argument("--validation-split", type=float, default=0.05)
    ap.add_argument("--unstd", action="store_true", help="the unstructured network through the same three paths (with --sweep: both ways)")
    ap.add_argument("--head", default="relu", choices=("linear", "relu"), help="with --unstd: the head's form")
    ap.add_argument("--sweep", default="", help="cstrs or cdu: time the whole sweep, looped and grouped, instead of the shapes")
    ap.add_argument("--ways", default="loop,group")
    a = ap.parse_args()
    if a.sweep:
        for name in a.sweep.split(","):
            run_sweep(name, a.epochs, a.repeats, a.ways.split(","), a.head if a.unstd else None)
        return
    for sname in a.shapes.split(","):
        dims, uprev = SHAPES[sname]
        nx, nu = geometry(dims, uprev)
        data = synthetic(a.rows, nx, nu)
        vs, unstd, passes = a.validation_split, (a.head if a.unstd else None), (1 if a.unstd else 2)
        ntr = a.rows - int(a.rows * vs)
        steps = -(-ntr // a.batch)
        for path in a.paths.split(","):
            r = run_wall(dims, uprev, data, a.batch, a.epochs, a.repeats, path, vs, unstd)
            if path == "hip":
                r.update(run_hip_events(dims, uprev, data, a.batch, a.epochs, a.repeats, vs, unstd))
                # the epoch's flop: full batches and the short one
                flop = (ntr // a.batch) * step_flop(dims, a.batch, passes) + (step_flop(dims, ntr % a.batch, passes) if ntr % a.batch else 0.0)
                r["step_event_ms"] = r["epoch_event_ms"]["median"] / steps
                r["f32_mfma_peak_fraction"] = flop / (r["epoch_event_ms"]["median"] * 1e-3) / PEAK_F32_MFMA
            r.update(shape=sname, dims=dims, path=path, form=("unstd_" + a.head) if a.unstd else "structured", validation_split=vs, rows=a.rows, batch=a.batch, steps_per_epoch=steps,
                     step_ms=r["epoch_ms"]["median"] / steps, epochs=a.epochs, repeats=a.repeats)
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
