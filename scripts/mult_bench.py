"""What the bound multipliers cost: solve_batch_device on HBM-resident buffers with and without `mult`, on one GPU.

  cdu    the CDU-size synthetic plant of bench.py (n = 4480), 100 000 problems, sx = 2
  cstrs  the CSTRs-size plant (n = 540), 10 000 problems

Per workload: far-field windows prepared as bench.py does, `--warmup` untimed calls, then `--repeats` (5) timed calls EACH way, every
call on a fresh seeded batch already resident in HBM (the two ways see the same batches and take turns at going first on one).  Times are hipEvent times from the library's
own records (nnmpc_qp_set_profiling: total_ms = the whole call on the handle's stream, mult_ms = asm_mult_k alone); the median,
minimum and maximum of the repeats are reported.  The bytes of P and tq rows the kernel gathers follow from the delivered active
words: active bounds x (np + ka) x 8.  One JSON line per workload.

    python scripts/mult_bench.py [--workloads cdu,cstrs] [--batch 0] [--repeats 5] [--warmup 1] [--sx 2.0]
"""
import argparse
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
    mult = D((B, n), np.float64)
    qp.set_profiling(True)

    def timed(i, m):
        x0, lb, ub = sets[i]
        qp.stats(reset=True)
        qp.solve_batch_device(B, x0, lb, ub, u, act, st, it, mult=m)
        s = qp.stats()
        return s["total_ms"], s["mult_ms"]

    for i in range(warmup):
        timed(i, None)
        timed(i, mult)
    plain, dual, kern, nact, status = [], [], [], [], np.zeros(3, int)
    for i in range(warmup, nsets):
        # the second call on a batch finds x0 and the bounds in the caches: the two ways take turns at going first
        if (i - warmup) % 2 == 0:
            plain.append(timed(i, None)[0])
            t, k = timed(i, mult)
        else:
            t, k = timed(i, mult)
            plain.append(timed(i, None)[0])
        dual.append(t)
        kern.append(k)
        nact.append(int(np.unpackbits(act.to_host().view(np.uint8), axis=1).sum()))
        status += np.bincount(st.to_host(), minlength=3)[:3]
    qp.set_profiling(False)
    np_, ka = qp._np, -(-n_aug // 32) * 32
    stat = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))
    gathered = float(np.median(nact)) * (np_ + ka) * 8
    out = dict(workload=workload, n=n, n_aug=n_aug, problems=B, sx=sx, repeats=repeats, status_hist=status.tolist(),
               solve_ms=stat(plain), solve_with_mult_ms=stat(dual), mult_kernel_ms=stat(kern),
               active_bounds_per_problem=float(np.median(nact)) / B, gathered_row_bytes=gathered,
               gathered_TB_per_s=gathered / (np.median(kern) * 1e-3) / 1e12,
               mult_share_of_call=float(np.median(kern) / np.median(dual)))
    for d in [a for s in sets for a in s] + [u, act, st, it, mult]:
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
