"""What the directional derivatives cost: a solve with multipliers, then nnmpc_qp_sensitivity on its result, on HBM-resident buffers.

  cdu    the CDU-size synthetic plant of bench.py (n = 4480), 100 000 problems, sx = 2
  cstrs  the CSTRs-size plant (n = 540), 10 000 problems

Protocol of scripts/mult_bench.py: far-field windows prepared as bench.py does, `--warmup` untimed rounds, then `--repeats` (5) timed
rounds, each on a fresh seeded batch already resident in HBM.  A round is one solve_batch_device with `mult` and then, on its active
words and status, one sensitivity call per (D, output): D in --directions (1, 8), first moves and the whole sequence with dmult.
Times are hipEvent times from the library's own records (nnmpc_qp_set_profiling): total_ms of the solve, sens_total_ms of a
sensitivity call (the whole call on the handle's stream, the host's sorting of each segment included) and sens_ms (the sens_k launches
alone).  Median, minimum and maximum of the repeats; the set sizes and the instances the problems ran in are reported beside them.
One JSON line per workload.

    python scripts/sens_bench.py [--workloads cdu,cstrs] [--batch 0] [--repeats 5] [--warmup 1] [--sx 2.0] [--directions 1,8]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(workload, B, repeats, warmup, sx, dirs):
    from industrial_nnmpc_2021_amd import _lib, synthetic
    from industrial_nnmpc_2021_amd.linearMPC_build import build_regulator_matrices
    from industrial_nnmpc_2021_amd.qp import BatchedBoxQP
    pl = synthetic.plant(workload, seed=0)
    P, tq, nu = build_regulator_matrices(pl)
    n, n_aug = P.shape[0], tq.shape[1]
    qp = BatchedBoxQP(P, tq, nu, max_batch=min(1024 if workload == "cdu" else 8192, B))
    if workload == "cdu":
        qp.prepare_farfield_windows()
    D = _lib.DeviceArray
    nsets = warmup + repeats
    sets = []
    for i in range(nsets):
        s = synthetic.samples(pl, B, seed=1000 + 7919 * i, sx=sx)
        x0 = np.concatenate((s["x"] - s["xs"], s["uprev"] - s["us"]), axis=1)
        sets.append(tuple(D.from_host(a) for a in (x0, pl["ulb"].T - s["us"], pl["uub"].T - s["us"])))
    u, act, st, it = D((B, n), np.float64), D((B, qp.words), np.uint32), D((B,), np.int32), D((B, 2), np.int32)
    mult, flag = D((B, n), np.float64), D((B,), np.int32)
    rng = np.random.default_rng(5)
    dmax = max(dirs)
    # one set of directions (their values do not change the work); a call with D directions reads the leading B D rows
    dx0 = D.from_host(rng.standard_normal((B * dmax, n_aug)))
    dlb, dub = D.from_host(0.1 * rng.standard_normal((B * dmax, nu))), D.from_host(0.1 * rng.standard_normal((B * dmax, nu)))
    du, dm = D((B * dmax, n), np.float64), D((B * dmax, n), np.float64)
    q = lambda a: None if a is None else C.c_void_p(a.data_ptr())
    qp.set_profiling(True)

    def sens(nd, first):
        qp.stats(reset=True)
        _lib.check(qp._lib.nnmpc_qp_sensitivity(qp._h, B, nd, q(act), q(st), q(dx0), q(dlb), q(dub), q(du), None if first else q(dm), q(flag),
                                                _lib.DEVICE, _lib.OUT_FIRST_MOVE if first else _lib.OUT_SEQUENCE), "nnmpc_qp_sensitivity")
        s = qp.stats()
        return s["sens_total_ms"], s["sens_ms"], s["sens_lds_problems"], s["sens_slab_problems"]

    keys = [(nd, first) for nd in dirs for first in (True, False)]
    solve, total, kern, sizes, flags, inst = [], {k: [] for k in keys}, {k: [] for k in keys}, [], np.zeros(4, int), np.zeros(2, int)
    for i in range(nsets):
        x0, lb, ub = sets[i]
        qp.stats(reset=True)
        qp.solve_batch_device(B, x0, lb, ub, u, act, st, it, mult=mult)
        t_solve = qp.stats()["total_ms"]
        res = {k: sens(*k) for k in keys}
        if i < warmup:
            continue
        solve.append(t_solve)
        for k in keys:
            total[k].append(res[k][0])
            kern[k].append(res[k][1])
        inst += np.array(res[keys[0]][2:4])
        flags += np.bincount(flag.to_host(), minlength=4)[:4]
        sizes.append(np.unpackbits(act.to_host().view(np.uint8), axis=1).sum(axis=1))
    qp.set_profiling(False)
    sizes = np.concatenate(sizes)
    stat = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))
    out = dict(workload=workload, n=n, n_aug=n_aug, problems=B, sx=sx, repeats=repeats, solve_with_mult_ms=stat(solve),
               set_size=dict(median=float(np.median(sizes)), max=int(sizes.max()), over_160=int((sizes > 160).sum())),
               lds_problems=int(inst[0]), slab_problems=int(inst[1]), flag_hist=flags.tolist())
    for nd, first in keys:
        tag = f"D{nd}_{'first_move' if first else 'sequence_dmult'}"
        out[tag + "_ms"] = stat(total[(nd, first)])
        out[tag + "_kernel_ms"] = stat(kern[(nd, first)])
    for d in [a for s in sets for a in s] + [u, act, st, it, mult, flag, dx0, dlb, dub, du, dm]:
        d.free()
    qp.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="cdu,cstrs")
    ap.add_argument("--batch", type=int, default=0, help="problems per call (0: 100 000 cdu, 10 000 cstrs)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sx", type=float, default=2.0)
    ap.add_argument("--directions", default="1,8")
    a = ap.parse_args()
    dirs = [int(d) for d in a.directions.split(",")]
    for w in a.workloads.split(","):
        print(json.dumps(run(w, a.batch or (100000 if w == "cdu" else 10000), a.repeats, a.warmup, a.sx, dirs)), flush=True)


if __name__ == "__main__":
    main()
