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

--sweep cstrs|cdu times a whole sweep WITH the tangent loss, on the grid of scripts/train_bench.py --sweep (its SWEEPS: 48
networks [36, w, w, w, 6] on 40 000 .. 150 000 rows, or 52 networks [536, w, w, w, 32]) at --batch and the grid's
validation_split, every member at --weight, with that script's protocol (one warm-up epoch, --repeats runs of --epochs sweep
epochs, the epoch loop's own clock around epoch + eval):

  loop    the networks one after another, each a HipTrainer(tangents=True)
  group   one HipGroupTrainer(tangents=True) (csrc/nn_train_group.hip): one grouped epoch + one grouped eval per sweep epoch
  plain   the plain HipGroupTrainer on the same grid and batch: what 3-over-2 stacked row blocks are measured against

One JSON line per way, printed and appended to --out (profiles/tan_train_bench.jsonl); the grouped ways also carry the
hipEvent time of the epoch calls (last_ms) and the launches per lock-step step (last_launches).

    python scripts/tan_train_bench.py --sweep cstrs [--batch 2048] [--weight 0.5] [--ways loop,group] [--epochs 5] [--repeats 5]

--fan times the step with several directions per row and whole-input directions (nnmpc_train_create_tan_ex) beside what it
replaces, per shape of --shapes at --batch, hipEvent ms per optimiser step (nnmpc_train_last_ms over epoch calls of --fan-rows
rows, one warm-up epoch, the median (min, max) of --repeats runs of --epochs epochs).  Legs (--legs):

  plain   the tangent handle at w = 0: the plain step          d1    one direction in [dx, (duprev)]: the pair launch
  rep4    the d1 handle on a dataset that repeats each row four times: ms per FOUR steps, the work d4 does in one
  d4      four directions per row in one step, partial input   w1, w2, w4   whole-input directions, D = 1, 2, 4

The stacked rows give d4 / rep4 = (2 + 4) / (3 x 4) = 0.5.  --root runs the legs on the package of another checkout (an
older build knows plain, d1 and rep4 only), so two builds can be alternated in one session.  One JSON line per (shape, leg),
printed and appended to --out.

    python scripts/tan_train_bench.py --fan [--legs plain,d1,rep4,d4,w1,w2,w4] [--fan-rows 40960] [--root PATH] [--tag NAME]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:                                                      # the package of another checkout, before ours
    sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--root") + 1]))
else:
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


def run_sweep(name, batch, w, epochs, repeats, ways, out):
    import itertools
    import time
    from industrial_nnmpc_2021_amd.train import HipGroupTrainer, HipTrainer, RegulatorModel, group_schedule
    from train_bench import SWEEPS
    sw = SWEEPS[name]
    uprev, vs = sw["uprev"], sw["validation_split"]
    members = list(itertools.product(sw["dims"], sw["rows"]))                 # the reference's loop order
    nx, nu = geometry(members[0][0], uprev)
    data = with_tangents(synthetic(max(sw["rows"]), nx, nu), nx, nu)
    weights = [RegulatorModel(nx, nu, d, nnwithuprev=uprev).get_weights() for d, _ in members]
    nval = [int(n * vs) for _, n in members]
    ntr = [n - v for (_, n), v in zip(members, nval)]
    sched = group_schedule(ntr, batch)
    steps = max(len(s) for s in sched)
    common = dict(sweep=name, members=len(members), batch=batch, validation_split=vs, tan_weight=w, epochs=epochs, repeats=repeats,
                  member_steps_per_epoch=sum(len(s) for s in sched), lockstep_steps_per_epoch=steps)

    def emit(r):
        line = json.dumps(dict(common, **r))
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")

    if "loop" in ways:
        runs, ev = [0.0] * repeats, [0.0] * repeats
        for (d, n), wk, a, v in zip(members, weights, ntr, nval):
            tr = HipTrainer(wk, nx, nu, nnwithuprev=uprev, max_batch=batch, tangents=True)
            part = {k: x[:n] for k, x in data.items()}
            tr.set_data(part)
            tr.set_tangents(part)
            tr.set_tan_weight(w)
            rng = np.random.default_rng(1)
            tr.epoch(rng.permutation(a), batch)                               # warm-up
            tr.eval(a, v)
            for r in range(repeats):
                t0 = time.time()
                for _ep in range(epochs):
                    tr.epoch(rng.permutation(a), batch)
                    ev[r] += tr.last_ms()[1]
                    tr.eval(a, v)
                runs[r] += time.time() - t0
            tr.close()
        emit(dict(way="loop", epoch_ms=spread([1e3 * t / epochs for t in runs]), epoch_event_ms=spread([e / epochs for e in ev])))
    for way in ("group", "plain"):
        if way not in ways:
            continue
        tr = HipGroupTrainer(weights, nx, nu, nnwithuprev=uprev, max_batch=batch, **({"tangents": True} if way == "group" else {}))
        tr.set_data(data)
        if way == "group":
            tr.set_tangents(data)
            tr.set_tan_weights([w] * len(members))
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
        emit(dict(way=way, epoch_ms=spread(runs), epoch_event_ms=spread(ev), epoch_gemm_event_ms=spread(gemm),
                  last_launches=launches, launches_per_lockstep_step=launches / steps))


FAN_LEGS = {"plain": (1, False, 1, 0.0), "d1": (1, False, 1, None), "rep4": (1, False, 4, None), "d4": (4, False, 1, None),
            "w1": (1, True, 1, None), "w2": (2, True, 1, None), "w4": (4, True, 1, None)}   # D, whole input, row repeats, weight


def run_fan(shapes, legs, batch, rows, w, epochs, repeats, tag, out):
    from industrial_nnmpc_2021_amd.train import HipTrainer, RegulatorModel
    for sname in shapes:
        dims, uprev = SHAPES[sname]
        nx, nu = geometry(dims, uprev)
        base = synthetic(rows, nx, nu)
        weights = RegulatorModel(nx, nu, dims, nnwithuprev=uprev).get_weights()
        for leg in legs:
            D, whole, reps, wl = FAN_LEGS[leg]
            rng = np.random.default_rng(1)
            data = {k: np.repeat(v, reps, axis=0) for k, v in base.items()}
            n = rows * reps
            shape = (lambda k: (n, D, k)) if (D > 1 or whole) else (lambda k: (n, k))
            data.update(dx=rng.standard_normal(shape(nx)), duprev=rng.standard_normal(shape(nu)), du=0.5 * rng.standard_normal(shape(nu)))
            more = {}
            if D > 1 or whole:
                more = dict(tan_dirs=D, tan_whole_input=whole)
            if whole:
                data.update(dxs=rng.standard_normal(shape(nx)), dus=rng.standard_normal(shape(nu)))
            tr = HipTrainer(weights, nx, nu, nnwithuprev=uprev, max_batch=batch, tangents=True, **more)
            tr.set_data(data)
            tr.set_tangents(data)
            tr.set_tan_weight(w if wl is None else wl)
            steps = -(-n // batch)
            tr.epoch(rng.permutation(n), batch)                                                   # warm-up
            tot, gemm = [], []
            for _ in range(repeats):
                t = g = 0.0
                for _ep in range(epochs):
                    tr.epoch(rng.permutation(n), batch)
                    ge, te = tr.last_ms()
                    t += te
                    g += ge
                tot.append(reps * t / epochs / steps)
                gemm.append(reps * g / epochs / steps)
            tr.close()
            line = json.dumps(dict(fan_leg=leg, build=tag, shape=sname, dims=dims, batch=batch, rows=rows, dirs=D, whole_input=whole,
                                   row_repeats=reps, tan_weight=w if wl is None else wl, steps_counted_as_one=reps,
                                   step_event_ms=spread(tot), step_gemm_event_ms=spread(gemm), epochs=epochs, repeats=repeats))
            print(line, flush=True)
            if out:
                with open(out, "a") as f:
                    f.write(line + "\n")


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
    ap.add_argument("--sweep", default="", help="cstrs or cdu: time the whole sweep with the tangent loss instead of the shapes")
    ap.add_argument("--ways", default="loop,group", help="with --sweep: loop, group, plain")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tan_train_bench.jsonl"),
                    help="with --sweep: the file the JSON lines are appended to ('' for none)")
    ap.add_argument("--fan", action="store_true", help="time the step with several directions per row / whole-input directions")
    ap.add_argument("--legs", default="plain,d1,rep4,d4,w1,w2,w4", help="with --fan")
    ap.add_argument("--fan-rows", type=int, default=40960, help="with --fan: dataset rows (rep4 repeats each four times)")
    ap.add_argument("--root", default="", help="with --fan: the checkout whose package is measured (default: this one)")
    ap.add_argument("--tag", default="this", help="with --fan: the name of the build in the JSON lines")
    a = ap.parse_args()
    if a.fan:
        run_fan(a.shapes.split(","), a.legs.split(","), a.batch, a.fan_rows, a.weight, a.epochs, a.repeats, a.tag, a.out)
        return
    if a.sweep:
        for name in a.sweep.split(","):
            run_sweep(name, a.batch, a.weight, a.epochs, a.repeats, a.ways.split(","), a.out)
        return
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
