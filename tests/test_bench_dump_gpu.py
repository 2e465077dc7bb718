"""bench.py --dump-outputs: what the timed path returned in its LAST timed step, as float .npy files within 64 MB, the same on
every run with the same arguments (the inputs are seeded) -- once through the plain single-process path, once through the
rank code with a communicator (NNMPC_FORCE_DIST=1: the first moves come back through the gather).  The dumped rows are
checked against the inputs of the last timed step, rebuilt here from the seeds: fp64 KKT conditions and the first moves."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, STEPS, WARMUP = 2048, 2, 1


def _run(out_dir, extra_env):
    env = dict(os.environ, **extra_env)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--batch", str(B), "--steps", str(STEPS), "--warmup", str(WARMUP),
                        "--dump-outputs", str(out_dir)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    return line, {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_dump_outputs_are_the_last_timed_step_and_reproducible(tmp_path):
    import bench
    la, a = _run(tmp_path / "plain", {})
    lb, b = _run(tmp_path / "comm", {"NNMPC_FORCE_DIST": "1"})
    for line in (la, lb):
        assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["ms_per_step"] > 0 and line["value"] > 0
        assert "parity" not in line and "cpu_baseline" not in line and "configs" not in line
    assert set(a) == set(b) == {"u", "active", "u_rows", "status", "ipm_iters", "factorizations", "first_moves"}
    for d in (a, b):
        assert all(v.dtype in (np.float32, np.float64) for v in d.values())
        assert sum(v.nbytes for v in d.values()) <= bench.DUMP_LIMIT
    # the same arguments, the same inputs: the same outputs (certified optima: active sets and status exactly)
    for k in ("active", "u_rows", "status"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("u", "first_moves"):
        assert np.abs(a[k] - b[k]).max() <= 1e-10 * max(1.0, np.abs(a[k]).max()), k

    pl, P, tq, nu = bench.make_problem("cdu")
    n, N = P.shape[0], pl["N"]
    rows = a["u_rows"].astype(np.int64)
    assert a["u"].shape == (rows.size, n) and a["active"].shape == (rows.size, 2 * n) and rows.size == 256
    assert a["first_moves"].shape == (B, nu) and a["status"].shape == (B,) and (a["status"] == 0).all()
    # the inputs of the last timed step: bench_qp's seed stream, last of its min(NSETS_MAX, 1 + W + K) sets
    nsets = min(bench.NSETS_MAX, 1 + WARMUP + STEPS)
    x0, lb, ub, us = bench.make_samples(pl, B, 1000 + 7919 * (nsets - 1), 2.0)
    U, bits = a["u"], a["active"].astype(bool)
    assert np.array_equal(a["first_moves"][rows], U[:, :nu] + us[rows])
    Ps = np.tril(P) + np.tril(P, -1).T
    G = U @ Ps + x0[rows] @ tq.T
    LB, UB = np.tile(lb[rows], (1, N)), np.tile(ub[rows], (1, N))
    k, c = np.arange(n) // nu, np.arange(n) % nu
    au, al = bits[:, k * 2 * nu + c], bits[:, k * 2 * nu + nu + c]
    scale = np.maximum(1.0, np.abs(x0[rows] @ tq.T).max(axis=1, keepdims=True))
    assert (U <= UB + 1e-9).all() and (U >= LB - 1e-9).all()
    assert np.array_equal(U[au], UB[au]) and np.array_equal(U[al], LB[al])
    assert (np.abs(np.where(~(au | al), G, 0)) <= 1e-8 * scale).all()
    assert (np.where(au, -G, 1) > 0).all() and (np.where(al, G, 1) > 0).all()
