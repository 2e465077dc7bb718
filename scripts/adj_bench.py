"""What the adjoint products cost beside the forward ones: a solve with multipliers, then nnmpc_qp_sensitivity and nnmpc_qp_adjoint on its
result, on HBM-resident buffers.

  cdu    the CDU-size synthetic plant of bench.py (n = 4480), 100 000 problems, sx = 2
  cstrs  the CSTRs-size plant (n = 540), 10 000 problems

Protocol of scripts/sens_bench.py: far-field windows prepared as bench.py does, `--warmup` untimed rounds, then `--repeats` (5) timed
rounds, each on a fresh seeded batch already resident in HBM.  A round is one solve_batch_device with `mult` and then, on its active
words and status: the forward for D in {1, 8}, first moves and the whole sequence (without dmult); the adjoint of the first move for
D = 1 and D = nu (the gain matrix: the nu unit cotangents) and of the sequence for D = 1 and D = 8, each with glb and gub and without
gbound.  The sequence cotangents are the du the forward's D = 8 call left on the device (finite wherever that call's flag is 0).
Times are hipEvent times from the library's own records (nnmpc_qp_set_profiling): sens_total_ms / adj_total_ms of a call (the whole
call on the handle's stream, the host's sorting of each segment included) and sens_ms / adj_ms (the sens_k / adj_k launches alone).
Median, minimum and maximum of the repeats.  One JSON line per workload.

    python scripts/adj_bench.py [--workloads cdu,cstrs] [--batch 0] [--repeats 5] [--warmup 1] [--sx 2.0]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(workload, B, repeats, warmup, sx):
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
    dseq, dgain = 8, nu
    dx0 = D.from_host(rng.standard_normal((B * dseq, n_aug)))
    dlb, dub = D.from_host(0.1 * rng.standard_normal((B * dseq, nu))), D.from_host(0.1 * rng.standard_normal((B * dseq, nu)))
    du = D((B * dseq, n), np.float64)                                           # the forward's output, then the sequence cotangents
    v0 = D.from_host(np.ascontiguousarray(np.broadcast_to(np.eye(nu), (B, nu, nu))).reshape(B * nu, nu))
    gx0 = D((B * max(dseq, dgain), n_aug), np.float64)
    glb, gub = D((B * max(dseq, dgain), nu), np.float64), D((B * max(dseq, dgain), nu), np.float64)
    q = lambda a: None if a is None else C.c_void_p(a.data_ptr())
    qp.set_profiling(True)

    def fwd(nd, first):
        qp.stats(reset=True)
        _lib.check(qp._lib.nnmpc_qp_sensitivity(qp._h, B, nd, q(act), q(st), q(dx0), q(dlb), q(dub), q(du), None, q(flag),
                                                _lib.DEVICE, _lib.OUT_FIRST_MOVE if first else _lib.OUT_SEQUENCE), "nnmpc_qp_sensitivity")
        s = qp.stats()
        return s["sens_total_ms"], s["sens_ms"]

    def adj(nd, first):
        qp.stats(reset=True)
        _lib.check(qp._lib.nnmpc_qp_adjoint(qp._h, B, nd, q(act), q(st), q(v0 if first else du), q(gx0), q(glb), q(gub), None, q(flag),
                                            _lib.DEVICE, _lib.OUT_FIRST_MOVE if first else _lib.OUT_SEQUENCE), "nnmpc_qp_adjoint")
        s = qp.stats()
        return s["adj_total_ms"], s["adj_ms"], s["adj_lds_problems"], s["adj_slab_problems"]

    # the forward's D = 8 sequence call comes last among the forward calls: its du is what the sequence adjoints read
    fkeys = [(1, True), (8, True), (1, False), (8, False)]
    akeys = [(1, True), (dgain, True), (1, False), (dseq, False)]
    solve, sizes, flags, inst = [], [], np.zeros(4, int), np.zeros(2, int)
    ft, fk, at, ak = ({k: [] for k in keys} for keys in (fkeys, fkeys, akeys, akeys))
    for i in range(nsets):
        x0, lb, ub = sets[i]
        qp.stats(reset=True)
        qp.solve_batch_device(B, x0, lb, ub, u, act, st, it, mult=mult)
        t_solve = qp.stats()["total_ms"]
        rf = {k: fwd(*k) for k in fkeys}
        ra = {k: adj(*k) for k in akeys}
        if i < warmup:
            continue
        solve.append(t_solve)
        for k in fkeys:
            ft[k].append(rf[k][0])
            fk[k].append(rf[k][1])
        for k in akeys:
            at[k].append(ra[k][0])
            ak[k].append(ra[k][1])
        inst += np.array(ra[akeys[0]][2:4])
        flags += np.bincount(flag.to_host(), minlength=4)[:4]                   # (of the last call: the sequence adjoint, D = 8)
        sizes.append(np.unpackbits(act.to_host().view(np.uint8), axis=1).sum(axis=1))
    qp.set_profiling(False)
    sizes = np.concatenate(sizes)
    stat = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))
    out = dict(workload=workload, n=n, nu=nu, n_aug=n_aug, problems=B, sx=sx, repeats=repeats, solve_with_mult_ms=stat(solve),
               set_size=dict(median=float(np.median(sizes)), max=int(sizes.max()), over_160=int((sizes > 160).sum())),
               lds_problems=int(inst[0]), slab_problems=int(inst[1]), flag_hist=flags.tolist())
    name = lambda first: "first_move" if first else "sequence"
    for nd, first in fkeys:
        out[f"forward_D{nd}_{name(first)}_ms"] = stat(ft[(nd, first)])
        out[f"forward_D{nd}_{name(first)}_kernel_ms"] = stat(fk[(nd, first)])
    for nd, first in akeys:
        out[f"adjoint_D{nd}_{name(first)}_ms"] = stat(at[(nd, first)])
        out[f"adjoint_D{nd}_{name(first)}_kernel_ms"] = stat(ak[(nd, first)])
    for d in [a for s in sets for a in s] + [u, act, st, it, mult, flag, dx0, dlb, dub, du, v0, gx0, glb, gub]:
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
    a = ap.parse_args()
    for w in a.workloads.split(","):
        print(json.dumps(run(w, a.batch or (100000 if w == "cdu" else 10000), a.repeats, a.warmup, a.sx)), flush=True)


if __name__ == "__main__":
    main()
