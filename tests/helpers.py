"""Shared builders for the parity tests (oracle side)."""
import numpy as np

from industrial_nnmpc_2021_amd import condense as pc, synthetic
from oracle import condense as oc, qp as oqp


def regulator_problem(name, seed=0, rho=0.97):
    """(plant dict, oracle DenseRegulator) for a synthetic plant."""
    pl = synthetic.plant(name, seed, rho)
    reg = oc.setup_regulator(pl["A"], pl["B"], pl["Q"], pl["R"], pl["S"], pl["N"], pl["ulb"], pl["uub"])
    return pl, reg


def batch_inputs(pl, B, seed=1, sx=1.0):
    """x0 (B, n_aug), lb, ub (B, nu) exactly as get_control_sequence forms them
    (reference lib/linearMPC.py:682-689)."""
    s = synthetic.samples(pl, B, seed, sx)
    x0 = np.concatenate((s["x"] - s["xs"], s["uprev"] - s["us"]), axis=1)
    lb = pl["ulb"].T - s["us"]
    ub = pl["uub"].T - s["us"]
    return s, x0, lb, ub


def oracle_solve(reg, x0, lb, ub):
    """Exact optimum + active rows (reference G row order) for every sample."""
    B = x0.shape[0]
    n = reg.N * reg.nu
    U = np.empty((B, n))
    act = np.zeros((B, 2 * n), bool)
    Ps = np.tril(reg.P) + np.tril(reg.P, -1).T
    for b in range(B):
        G, h = oqp.box_as_Gh(reg.nu, reg.N, lb[b], ub[b])
        info = {}
        U[b] = oqp.solve_exact(Ps, reg.tq @ x0[b], G, h, info=info)
        act[b, info["active"]] = True
        assert info["kkt"][0] < 1e-6 * max(1.0, np.abs(reg.tq @ x0[b]).max()) and info["kkt"][1] < 1e-9
    return U, act


def oracle_box_rows(Ps, tq, nu, N, x0, lb, ub, rows):
    """[(u*, active rows of G)] of the listed problems by oracle.qp.solve_exact_box.  At the CDU size a solve takes seconds, so
    the rows are shared out over worker PROCESSES -- started as fresh interpreters (`python -m tests.oracle_worker`), never
    forked: a child forked from a process that has touched the GPU inherits the KFD descriptors and objects whose __del__ calls
    into the runtime (undefined behaviour on ROCm).  Matrices and results travel as .npz files under /dev/shm."""
    import os
    import shutil
    import subprocess
    import sys
    import tempfile
    rows = [int(r) for r in rows]
    nw = max(1, min(16, len(rows), (os.cpu_count() or 1) // 4))
    if nw == 1 or Ps.shape[0] < 1024:
        out = []
        for r in rows:
            info = {"nu": nu}
            xe = oqp.solve_exact_box(Ps, tq @ x0[r], np.tile(lb[r], N), np.tile(ub[r], N), info=info)
            out.append((xe, info["active"]))
        return out
    keep = np.array(sorted(set(rows)), dtype=int)           # only the listed rows travel (the batch can be hundreds of MB)
    sub = {int(r): i for i, r in enumerate(keep)}
    d = tempfile.mkdtemp(prefix="nnmpc_test_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        np.savez(os.path.join(d, "job.npz"), Ps=Ps, tq=tq, nu=nu, N=N, x0=x0[keep], lb=lb[keep], ub=ub[keep])
        threads = max(1, (os.cpu_count() or 1) // (2 * nw))
        env = dict(os.environ, OMP_NUM_THREADS=str(threads), OPENBLAS_NUM_THREADS=str(threads), MKL_NUM_THREADS=str(threads))
        procs = [subprocess.Popen([sys.executable, "-m", "tests.oracle_worker", d, str(w), str(nw)], cwd=root, env=env) for w in range(nw)]
        codes = [p.wait() for p in procs]
        if any(codes):
            raise RuntimeError(f"oracle worker exit codes {codes}")
        res = {}
        for w in range(nw):
            with np.load(os.path.join(d, f"out{w}.npz"), allow_pickle=False) as f:
                for i in f["rows"]:
                    res[int(i)] = (f[f"x{i}"], f[f"a{i}"])
        return [res[sub[r]] for r in rows]
    finally:
        shutil.rmtree(d, ignore_errors=True)


# ---- structured-NN forward: inputs, references and the error measure shared by the NN parity tests ----------------------------

def bf16_round(a):
    """Round to nearest-even bf16 (returned as float32), like v_cvt_pk_bf16_f32 / the library's weight upload.  Inf stays Inf,
    a finite value beyond the largest bf16 becomes Inf, NaN stays NaN (the carry of the rounding must not run into the sign)."""
    f = np.ascontiguousarray(a, dtype=np.float32)
    u = f.view(np.uint32).astype(np.uint64)
    r = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16) & 0xFFFFFFFF
    r = np.where(np.isnan(f), (u & 0x80000000) | 0x7FC00000, r)
    return r.astype(np.uint32).view(np.float32).reshape(f.shape)


def bf16_forward(W, x, uprev, xs, us, xscale):
    """The structured forward (lib/controller_evaluation.py:863-886) with the bf16 path's roundings: inputs, weights
    and hidden activations in bf16, sums and biases wider, head output unrounded.  ``W`` is any Keras-ordered list
    [W1, b1, ..., Wout]: one matrix alone, or hidden layers of different widths."""
    sc = (1.0 / np.asarray(xscale)).astype(np.float32) if xscale is not None else np.ones(x.shape[1], np.float32)

    def mlp(a, b):
        z = [a.astype(np.float32) * sc] + ([b.astype(np.float32)] if b is not None else []) + [xs.astype(np.float32) * sc, us.astype(np.float32)]
        h = bf16_round(np.concatenate(z, axis=1)).astype(np.float64)
        nl = (len(W) + 1) // 2
        for l in range(nl - 1):
            h = h @ bf16_round(W[2 * l]).astype(np.float64) + W[2 * l + 1].astype(np.float32).astype(np.float64)
            h = bf16_round(np.maximum(h, 0.0)).astype(np.float64)
        return (h @ bf16_round(W[-1]).astype(np.float64)).astype(np.float32).astype(np.float64)
    return us + (mlp(x, uprev) - mlp(xs, us if uprev is not None else None))


def nn_weights(rng, dims, wscale=1.0, bscale=0.05):
    """Keras-ordered weights of an MLP with the layer widths ``dims`` = [din, h1, ..., nu]: He-scaled kernels (activations keep
    their size from layer to layer whatever the depth), small biases on the hidden layers, none on the head."""
    W = []
    for i in range(len(dims) - 1):
        W.append(wscale * rng.standard_normal((dims[i], dims[i + 1])) * np.sqrt(2.0 / dims[i]))
        if i < len(dims) - 2:
            W.append(bscale * rng.standard_normal(dims[i + 1]))
    return W


def share_on_bound(u, ulb, uub):
    """Share of the entries of a clipped oracle output that sit exactly on a bound."""
    return float(((u == np.ravel(ulb)) | (u == np.ravel(uub))).mean())


def nn_case(seed, hidden, nx, nu, withu, B, *, eps=1.0, xscale=True, ulb=None, uub=None, steady_row=None):
    """Weights and inputs of one structured-NN case from a seed, and what the fp64 oracle makes of them.

    x = xs + eps N(0, 1), uprev = us + eps U(-1, 1), xs ~ 0.3 N(0, 1), us ~ U(-.5, .5): ``eps`` is the distance from the steady
    state, i.e. the size of u - us.  Returns a dict with W, dims, the inputs, ``ref`` (the oracle's UNCLIPPED u), ``ref_clip``
    (clipped to ulb / uub when given, else ref) and ``share`` (entries of ref_clip on a bound; 0 without bounds).
    ``steady_row``: that row gets x = xs, uprev = us (u = clip(us) exactly, whatever the weights)."""
    from oracle import nn as onn
    rng = np.random.default_rng(seed)
    dims = [2 * nx + (2 if withu else 1) * nu] + list(hidden) + [nu]
    W = nn_weights(rng, dims)
    xs = 0.3 * rng.standard_normal((B, nx))
    us = rng.uniform(-0.5, 0.5, (B, nu))
    x = xs + eps * rng.standard_normal((B, nx))
    up = us + eps * rng.uniform(-1.0, 1.0, (B, nu)) if withu else None
    xsc = rng.uniform(0.5, 2.0, nx) if xscale else None
    if steady_row is not None and B > steady_row:
        x[steady_row] = xs[steady_row]
        if withu:
            up[steady_row] = us[steady_row]
    ref = onn.control_input(W, x, up, xs, us, xsc, None, None, withu)
    c = dict(W=W, dims=dims, nx=nx, nu=nu, withu=withu, x=x, uprev=up, xs=xs, us=us, xscale=xsc, ulb=ulb, uub=uub, ref=ref,
             ref_clip=ref, share=0.0)
    if ulb is not None:
        c["ref_clip"] = onn.control_input(W, x, up, xs, us, xsc, ulb, uub, withu)
        c["share"] = share_on_bound(c["ref_clip"], ulb, uub)
    return c


def col_err(u, ref):
    """Per output column: max over rows of |u - ref|, in units of max(1, max over rows of |ref[:, col]|)."""
    return np.abs(u - ref).max(axis=0) / np.maximum(1.0, np.abs(ref).max(axis=0))


def assert_cols_close(u, ref, tol, what=""):
    """max_rows |u - ref| <= tol max(1, max_rows |ref[:, col]|) for EVERY column: a wrong low-magnitude column cannot hide
    behind a large one."""
    assert u.shape == ref.shape, (what, u.shape, ref.shape)
    assert np.isfinite(u).all(), (what, "non-finite entries", int((~np.isfinite(u)).sum()))
    e = col_err(u, ref)
    assert (e <= tol).all(), (what, "worst column", int(e.argmax()), float(e.max()), "tol", tol)


# The shape matrix of tests/test_nn_paths_gpu.py (every case runs in all three precisions), kept here so that
# tests/test_cpu_nn_inputs.py can judge the same inputs with the oracle alone.  A sparse product: every value of every axis
# appears at least once --
#   depth: one matrix, one hidden layer, three, five;  hidden widths at and around every dispatch threshold of nnmpc_nn_create /
#   nnmpc_nn_forward (64-tile <= 64 < 128-tile; bf16: wide tile from a padded width of 416, i.e. widths >= 385);  ragged nets;
#   nu in {1, 5, 6, 16, 32, 64, 65, 80};  din a multiple of 64 (64, 192, 512) and not;  with / without uprev and xscale;
#   batch 1, 127, 128, 129, max_batch - 1, max_batch, max_batch + 1, 3 max_batch + 7 for max_batch 128 and 256;  two cases
#   through forward_device.
# (name, hidden widths, nx, nu, with uprev, xscale given, B, max_batch, through forward_device)
NN_SHAPE_CASES = [
    ("linear_b1", [], 12, 6, True, True, 1, 128, False),
    ("linear_din512", [], 240, 32, False, False, 127, 128, False),
    ("h1", [1], 12, 6, True, True, 128, 128, False),
    ("h63_nu5", [63], 7, 5, False, True, 129, 128, False),
    ("h64_din64", [64], 16, 16, True, False, 127, 128, False),
    ("h65", [65], 12, 6, False, True, 128, 128, False),
    ("h127_nu1", [127], 5, 1, True, True, 129, 128, False),
    ("h128_3mb7", [128], 12, 6, True, False, 3 * 128 + 7, 128, False),
    ("h129_nu64_din192", [129], 32, 64, True, True, 255, 256, False),
    ("h130", [130], 12, 6, False, True, 256, 256, False),
    ("h200", [200], 12, 6, True, True, 257, 256, False),
    ("h384_385", [384, 385], 12, 6, True, True, 130, 128, False),
    ("h415_3mb7_dev", [415], 252, 32, False, True, 3 * 256 + 7, 256, True),
    ("h416_b1", [416], 12, 6, True, False, 1, 256, False),
    ("h417", [417], 12, 6, False, True, 127, 256, False),
    ("h831", [831], 252, 32, True, True, 128, 128, False),
    ("cdu_832x3_dev", [832, 832, 832], 252, 32, False, True, 129, 128, True),
    ("h833", [833], 12, 6, True, False, 128, 256, False),
    ("h1024_din512", [1024], 240, 32, False, True, 130, 128, False),
    ("five_hidden", [128, 64, 416, 130, 65], 12, 6, True, True, 200, 128, False),
    ("taper_832_416_64", [832, 416, 64], 252, 32, False, True, 300, 128, False),
    ("grow_64_832", [64, 832], 12, 6, True, True, 129, 128, False),
    ("ragged_130_417_200", [130, 417, 200], 7, 5, False, False, 131, 128, False),
    ("nu65", [128], 10, 65, False, True, 129, 128, False),
    ("nu80_taper", [416, 64], 24, 80, True, True, 257, 256, False),
]


def nn_shape_case(i, **kw):
    """nn_case of NN_SHAPE_CASES[i] (seed = 100 + i)."""
    name, hidden, nx, nu, withu, xsc, B, mb, dev = NN_SHAPE_CASES[i]
    return nn_case(100 + i, hidden, nx, nu, withu, B, xscale=xsc, **kw)


# Architectures of the property tests (exactness, stale state, non-finite inputs, clip): one per GEMM kernel family --
# 64-wide tiles; 128-wide tiles with a partial last column tile; the wide tile followed by the 128- and the 64-wide one.
NN_PROPERTY_NETS = [("n64", [64, 64], 12, 6, True), ("n130_200", [130, 200], 7, 5, False), ("taper", [832, 416, 64], 40, 32, False)]
# distance from the steady state at which the oracle alone leaves at most 5 % of the entries on the bounds -1 / +1
NN_BOUNDED_EPS = 0.1


# ---- grouped closed-loop NN forward (cl_nn_layer_k): the network mix of tests/test_closed_loop_nn_gpu.py ------------------------
# (name, hidden widths, with uprev, instances) on the mini_cstrs plant (Nx = 6, Nu = 3: first-layer K = 18 / 15, neither a multiple
# of the kernel's 4 K slices).  Side by side in ONE batch: 1, 2, 3 and 5 weight matrices (the shallow nets end at an earlier layer
# index while the others go on using the ping-pong buffers); widths 40, 64, 65, 130, 832, 1024 and NN_MAXK = 2048; with and
# without uprev; 1, 3, 8 and 9 instances (two rows each, walked in blocks of NN_RB = 8 rows).
CL_NN_MIX = [
    ("w40", [40], True, 1),
    ("linear", [], False, 3),
    ("w64_65", [64, 65], True, 8),
    ("deep_130_832_1024_65", [130, 832, 1024, 65], False, 9),
    ("w2048", [2048], True, 1),
]
CL_NN_HEAD_SCALE = 1.0            # gain of u - us on [xhat - xs; uprev - us]: |u - us| stays > 100 x the f32 tolerance, the loop inside the box (share asserted)


def cl_nn_weights(seed, din, hidden, nu, head_scale=CL_NN_HEAD_SCALE):
    """He-scaled hidden layers (the difference of the two passes keeps its size through any depth), head scaled down."""
    W = nn_weights(np.random.default_rng(seed), [din] + list(hidden) + [nu], bscale=0.1)
    W[-1] = head_scale * W[-1]
    return W


def cl_one_step_reference(W, xscale, withu, ulb, uub, rec_u, rec_xhat, rec_xs, rec_us, uprev0, nx):
    """What the oracle makes of the recorded inputs of every step of one instance: (unclipped u, clipped u), rows = steps.
    The estimate a step's controller sees is row t + 1 of the xhat record: cl_filter_k overwrites xhat with the corrected estimate
    before cl_expand_k reads it, and cl_post_k records it as row t + 1; uprev of step t is u[t - 1] (step 0: the initial uprev)."""
    from oracle import nn as onn
    xh = rec_xhat[1:, :nx]
    up = np.concatenate((np.ravel(uprev0)[None, :], rec_u[:-1]), axis=0)
    free = onn.control_input(W, xh, up, rec_xs, rec_us, np.ravel(xscale), None, None, withu)
    clipped = onn.control_input(W, xh, up, rec_xs, rec_us, np.ravel(xscale), np.ravel(ulb), np.ravel(uub), withu)
    return free, clipped


def cl_assert_one_step_identity(res, ctls, common, tol, what):
    """The one-step identity u[t] == clip(oracle(recorded inputs of step t)) for every NN instance of a
    simulate_closed_loop_batch result, per column within tol max(1, |ref|); every column must carry a signal (|u - us| well above
    the tolerance at some step).  Returns (share of the oracle's entries on a bound, worst column error)."""
    Nx = common["A"].shape[0]
    on, total, worst = 0, 0, 0.0
    for i, (c, s, seed) in enumerate(res["instances"]):
        ctl = ctls[c]
        if not hasattr(ctl, "regulator_weights"):
            continue
        free, ref = cl_one_step_reference(ctl.regulator_weights, ctl.xscale, ctl.nnwithuprev, common["ulb"], common["uub"],
                                          res["u"][i], res["xhat"][i], res["xs"][i], res["us"][i], common["uprev"], Nx)
        assert (np.abs(free - res["us"][i]).max(axis=0) > 100 * tol).all(), (what, i, "u - us too small to test anything")
        on += int(((ref == np.ravel(common["ulb"])) | (ref == np.ravel(common["uub"]))).sum())
        total += ref.size
        assert_cols_close(res["u"][i], ref, tol, (what, "instance", i, (c, s, seed)))
        worst = max(worst, float(col_err(res["u"][i], ref).max()))
    assert total > 0
    return on / total, worst


# ---- target-selector QP kernel (ts_solve_k) straight through the C ABI: tests/test_target_kernel_gpu.py ------------------------

TS_EPS = float(np.finfo(np.float64).eps)
TS_ERR_FACTOR = 64.0              # |us - ref| <= 64 eps cond_2(K_A) max(1, |ref|): one fp64 solve of the final KKT system, order <= 64
TS_KKT_TOL = 64.0 * 64.0 * TS_EPS  # row-wise backward error of GEPP: order <= 64 times a growth allowance of 64
TS_MARGIN = 1e-6                  # a case is compared when the certified reference is this far from a change of bound state
TS_SLACK = 1e-9                   # feasibility slack of the kernel, as include/nnmpc.h documents it
TS_SHAPES = [(1, 0), (2, 1), (5, 2), (6, 0), (7, 2), (17, 3), (32, 4), (33, 16), (48, 16), (60, 4), (63, 1), (64, 0)]
TS_CONDS = [1e1, 1e4, 1e7]
TS_BATCHES = (1, 63, 65, 257)


def ts_amax(a):
    """max |a|, 0 for an empty array (lam_eq of a problem without equalities)."""
    a = np.asarray(a)
    return float(np.abs(a).max()) if a.size else 0.0


def ts_matrices(seed, nu, nz, cond):
    """Pr = Q diag(logspace(0, log10 cond)) Q' (symmetric, eigenvalues 1 .. cond), Gaussian E, asymmetric bounds
    lb_i in -[0.2, 1.5], ub_i in [0.2, 1.5]."""
    rng = np.random.default_rng(seed)
    Qm = np.linalg.qr(rng.standard_normal((nu, nu)))[0]
    d = rng.permutation(np.logspace(0.0, np.log10(cond), nu)) if nu > 1 else np.array([cond])
    Pr = (Qm * d) @ Qm.T
    Pr = 0.5 * (Pr + Pr.T)
    E = rng.standard_normal((nz, nu))
    lb, ub = -rng.uniform(0.2, 1.5, nu), rng.uniform(0.2, 1.5, nu)
    return Pr, E, lb, ub


def ts_rhs(seed, Pr, E, lb, ub, B):
    """q (B, nu), e (B, nz) of B feasible problems: e = E u0 with u0 inside the box.  One row in three has q = -Pr w with the
    unconstrained optimum w next to u0 (0.005 / 0.01 N(0, 1) away: the optimum stays inside the box); the others a Gaussian q whose size
    runs through 12 log-spaced steps from 1e-2 to 30 max|Pr| (from "the equalities decide" to "every bound that can be active
    is": nu - nz of them)."""
    rng = np.random.default_rng(seed)
    nu = Pr.shape[0]
    u0 = lb + rng.uniform(0.1, 0.9, (B, nu)) * (ub - lb)
    k = np.arange(B)
    near = np.array([0.005, 0.01])[(k // 3) % 2]
    q = -(u0 + near[:, None] * rng.standard_normal((B, nu))) @ Pr.T
    mags = np.logspace(-2.0, np.log10(30.0 * np.abs(Pr).max()), 12)[(k // 3 + 5 * (k % 3)) % 12]
    far = k % 3 != 0
    q[far] = (mags[:, None] * rng.standard_normal((B, nu)))[far]
    return q, u0 @ E.T


class TsHandle:
    """nnmpc_ts_create / nnmpc_ts_solve_batch bound through _lib, nothing in between (no de-duplication, every output kept)."""
    SENTINEL = -7.25

    def __init__(self, Pr, E, lb, ub):
        import ctypes as C
        from industrial_nnmpc_2021_amd import _lib
        self._C, self._lib_mod, self._lib = C, _lib, _lib.load()
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        self.nu = int(np.asarray(Pr).shape[0])
        self.nz = 0 if E is None else int(np.asarray(E).reshape(-1, self.nu).shape[0])
        self._keep = (f(Pr), f(E if self.nz else np.zeros((1, self.nu))), f(lb).ravel(), f(ub).ravel())
        self._h = C.c_void_p()
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(self._lib.nnmpc_ts_create(C.byref(self._h), self.nu, self.nz, *[p(a) for a in self._keep]), "nnmpc_ts_create")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.nnmpc_ts_destroy(self._h)
            self._h = self._C.c_void_p()

    __del__ = close

    def solve(self, q, e=None, kind="host", lam=True, active=True):
        """q (B, nu), e (B, nz) -> (us, lam_eq or None, active or None, status), through NNMPC_HOST or NNMPC_DEVICE pointers.
        Outputs start out filled with a sentinel, so what the library did not write shows."""
        C, _lib = self._C, self._lib_mod
        q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, self.nu)
        B = q.shape[0]
        e = np.ascontiguousarray(e if self.nz else np.zeros((B, 0)), dtype=np.float64).reshape(B, self.nz)
        us = np.full((B, self.nu), self.SENTINEL)
        lm = np.full((B, self.nz), self.SENTINEL) if lam and self.nz else None
        ac = np.full((B, self.nu), 77, np.uint8) if active else None
        st = np.full(B, -5, np.int32)
        if B == 0:                                       # no storage behind the pointers: the library may not touch them
            dummy = np.full(8, self.SENTINEL)
            p = dummy.ctypes.data_as(C.c_void_p)
            _lib.check(self._lib.nnmpc_ts_solve_batch(self._h, 0, p, p, p, p if lam else None, p if active else None, p,
                                                      _lib.HOST if kind == "host" else _lib.DEVICE), "nnmpc_ts_solve_batch")
            assert (dummy == self.SENTINEL).all()
            return us, lm, ac, st
        if kind == "host":
            p = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(C.c_void_p)
            _lib.check(self._lib.nnmpc_ts_solve_batch(self._h, B, p(q), p(e), p(us), p(lm), p(ac), p(st), _lib.HOST),
                       "nnmpc_ts_solve_batch")
            return us, lm, ac, st
        up = lambda a: None if a is None or a.size == 0 else _lib.DeviceArray.from_host(a)
        d = [up(a) for a in (q, e, us, lm, ac, st)]
        p = lambda a: None if a is None else C.c_void_p(a.data_ptr())
        _lib.check(self._lib.nnmpc_ts_solve_batch(self._h, B, *[p(a) for a in d], _lib.DEVICE), "nnmpc_ts_solve_batch")
        out = [None if a is None else a.to_host() for a in d[2:]]
        for a in d:
            if a is not None:
                a.free()
        return out[0], out[1], out[2], out[3]


def ts_kkt_certificate(Pr, E, lb, ub, q, e, us, lam, act):
    """KKT certificate of ONE returned (us, lam_eq, active) alone, every row normalised by the size of its own terms:
    stationarity |g_i| on free rows and the wrong-signed part of g_i on held rows (g = Pr us + q + E' lam_eq: <= 0 at ub, >= 0 at
    lb), over (|Pr| |us| + |q| + |E'| |lam_eq|)_i; equalities |E us - e| over |E| |us| + |e|.  Returns the largest ratio."""
    nz = E.shape[0]
    lam = np.zeros(0) if lam is None or nz == 0 else lam
    g = Pr @ us + q + E.T @ lam
    den = np.abs(Pr) @ np.abs(us) + np.abs(q) + np.abs(E.T) @ np.abs(lam)
    bad = np.where(act == 0, np.abs(g), np.where(act == 1, np.maximum(g, 0.0), np.maximum(-g, 0.0)))
    worst = float(np.max(np.where(bad > 0.0, bad / np.where(den > 0, den, 1e-300), 0.0)))
    if nz:
        r = np.abs(E @ us - e)
        den = np.abs(E) @ np.abs(us) + np.abs(e)
        worst = max(worst, float(np.max(np.where(r > 0.0, r / np.where(den > 0, den, 1e-300), 0.0))))
    return worst


def ts_reference(Pr, E, lb, ub, Q, Ee):
    """Certified fp64 reference of every row: the enumeration of all bound states for nu <= 7, oracle.target.solve (the
    active-set proposer, the interior-point oracle when that one is refused, + certify) above.  Returns a list of dicts (us, lam_eq, state, primal_margin, dual_margin, cond)."""
    from oracle import target as ot
    if Pr.shape[0] <= 7:
        return [ot.pick_state(f) for f in ot.enumerate_states(Pr, Q, E, Ee, lb, ub)]
    return [ot.solve(Pr, Q[i], E, Ee[i], lb, ub, propose="active_set") for i in range(Q.shape[0])]


def ts_kept(ref, q):
    """The margin rule: primal and dual margin of the certified reference > 1e-6 (dual: relative to max(1, |q|inf))."""
    return ref["primal_margin"] > TS_MARGIN and ref["dual_margin"] > TS_MARGIN * max(1.0, float(np.abs(q).max()))


# ---- box QPs with an active set of a chosen size: tests/test_large_sets_gpu.py, tests/test_cpu_large_set_inputs.py ------------

def kkt_check(P, tq, nu, N, x0, lb, ub, out, stat_tol):
    """Independent fp64 check of every returned solution."""
    Ps = np.tril(P) + np.tril(P, -1).T
    U = out["u"]
    G = U @ Ps + x0 @ tq.T                     # gradient rows
    LB, UB = np.tile(lb, (1, N)), np.tile(ub, (1, N))
    n = P.shape[0]
    k, c = np.arange(n) // nu, np.arange(n) % nu
    au, al = out["active"][:, k * 2 * nu + c], out["active"][:, k * 2 * nu + nu + c]
    assert not (au & al).any()
    assert (U <= UB + 1e-9).all() and (U >= LB - 1e-9).all()                 # primal feasibility
    assert np.abs(np.where(au, U - UB, 0)).max() == 0 and np.abs(np.where(al, U - LB, 0)).max() == 0
    scale = np.maximum(1.0, np.abs(x0 @ tq.T).max(axis=1, keepdims=True))
    free = ~(au | al)
    assert (np.abs(np.where(free, G, 0)) <= stat_tol * scale).all()            # stationarity on the free set
    assert (np.where(au, -G, 1) > 0).all() and (np.where(al, G, 1) > 0).all()  # multiplier signs


def kkt_stationarity(P, q, nu, out):
    """Per row: max |gradient| over the free variables in units of max(1, |q|inf) -- the figure kkt_check bounds (tq = I)."""
    n = P.shape[0]
    k, c = np.arange(n) // nu, np.arange(n) % nu
    free = ~(out["active"][:, k * 2 * nu + c] | out["active"][:, k * 2 * nu + nu + c])
    G = out["u"] @ (np.tril(P) + np.tril(P, -1).T) + q
    return np.abs(np.where(free, G, 0)).max(axis=1) / np.maximum(1.0, np.abs(q).max(axis=1))


def state_to_active(state, nu):
    """(B, n) uint8 bound states (0 free, 1 upper, 2 lower: the `guess` format) -> (B, 2n) bool rows of the reference's G."""
    B, n = state.shape
    k, c = np.arange(n) // nu, np.arange(n) % nu
    act = np.zeros((B, 2 * n), bool)
    act[:, k * 2 * nu + c] = state == 1
    act[:, k * 2 * nu + nu + c] = state == 2
    return act


def active_to_state(active, nu):
    """The inverse of state_to_active."""
    n = active.shape[1] // 2
    k, c = np.arange(n) // nu, np.arange(n) % nu
    return active[:, k * 2 * nu + c].astype(np.uint8) + 2 * active[:, k * 2 * nu + nu + c].astype(np.uint8)


def spd_logspectrum(n, seed, cond):
    """Dense Q diag(exp(U(0, log cond))) Q' (the Hessian of tests/test_asm_gpu.py)."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = np.exp(rng.uniform(0.0, np.log(cond), n))
    return (Q * ev) @ Q.T


def large_set_hessian(n, seed):
    """P = diag(U(1, 4)) + 0.15 (G + G'), G = N(0, 1) / sqrt(n): diagonally dominated, cond ~ 5 at n = 1024."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n)) / np.sqrt(n)
    return np.diag(rng.uniform(1.0, 4.0, n)) + 0.15 * (G + G.T)


def pushed_rows(P, nu, seed, sizes, lo, hi, exact=False):
    """One problem per entry of ``sizes`` (tq = I, so q = x0; bounds -1 / +1 on every input): the unconstrained optimum x_unc is
    0.05 N(0, 1), except on m indices drawn without replacement over the whole horizon, which sit at +-U(lo, hi) -- beyond a
    bound -- and q = -P x_unc.  Returns q (B, n), lb, ub (nu,), the pushed bound states (B, n) uint8 (1 upper, 2 lower) and, with
    ``exact``, the optimum x (B, n) in fp64.

    exact: every row is CERTIFIED to have the pushed set as its optimal set -- the fp64 solve on that set (solve_on_set) keeps
    every free variable within 0.9 of the origin and every multiplier above 1e-2 with the right sign, which for a positive definite
    P makes it the optimum.  The couplings of hundreds of active bounds do now and then carry a pushed variable back inside the box
    (seen at 768 bounds: x_unc = 1.64, optimum 0.84); such a row is drawn again (from the same generator: still a function of the
    seed alone)."""
    n = P.shape[0]
    rng = np.random.default_rng(seed)
    B = len(sizes)
    Ps = np.tril(P) + np.tril(P, -1).T
    lb, ub = -np.ones(nu), np.ones(nu)
    xunc = 0.05 * rng.standard_normal((B, n))
    q = np.empty((B, n))
    state = np.zeros((B, n), np.uint8)
    xref = np.empty((B, n)) if exact else None
    for b, m in enumerate(sizes):
        for attempt in range(50):
            xu, st = xunc[b].copy(), np.zeros(n, np.uint8)
            idx = rng.choice(n, int(m), replace=False)
            sgn = rng.choice([-1.0, 1.0], int(m))
            xu[idx] = sgn * rng.uniform(lo, hi, int(m))
            st[idx] = np.where(sgn > 0, 1, 2)
            qb = -Ps @ xu
            if not exact:
                break
            x = solve_on_set(Ps, qb, lb, ub, st)
            g = Ps @ x + qb
            if np.abs(x[st == 0]).max(initial=0.0) <= 0.9 and (g[st == 1] < -1e-2).all() and (g[st == 2] > 1e-2).all():
                xref[b] = x
                break
        else:
            raise RuntimeError(f"no exact row of {m} bounds in 50 draws")
        q[b], state[b] = qb, st
    return q, lb, ub, state, xref


def large_set_problem(n, nu, seed, sizes):
    """Problems whose optimal active set has EXACTLY the sizes asked for: large_set_hessian with pushes of +-U(1.5, 3), rows
    certified (pushed_rows, exact).  The optimum's set is the pushed set with the pushed signs, and so is the first set (the bounds
    x_unc violates): a solver's f32 round and its fp64 solve both run at size m (tests/test_cpu_large_set_inputs.py holds the
    oracle to this).  Returns P, q (B, n), lb, ub (nu,), expected bound states (B, n) uint8, the optimum x (B, n)."""
    P = large_set_hessian(n, seed)
    return (P,) + pushed_rows(P, nu, seed + 1, sizes, 1.5, 3.0, exact=True)


# Numerical strain: the dense log-spectrum Hessian at cond 1e4 (below the 5e4 up to which method "auto" must solve everything),
# pushes of +-U(1.2, 2): the couplings add bounds to the pushed ones, the free-block systems are ill conditioned.  The push counts
# were chosen with the oracle so that its sets cover both large classes (tests/test_cpu_large_set_inputs.py asserts the shares).
STRAIN_COND = 1e4
STRAIN_SEED = 31
STRAIN_PUSHES = [230, 250, 270, 300, 350, 400, 450, 500]        # oracle's sets: 264, 297, 335, 386, 429, 430, 479, 546 bounds


def strain_problem(n=1024, nu=8):
    """P, q, lb, ub of the strain family (the final sets are the oracle's to say)."""
    P = spd_logspectrum(n, STRAIN_SEED, STRAIN_COND)
    return (P,) + pushed_rows(P, nu, STRAIN_SEED + 1, STRAIN_PUSHES, 1.2, 2.0)[:3]


def solve_on_set(Ps, q, lb, ub, state):
    """fp64 optimum of ONE problem given its bound states (Ps: the full symmetric Hessian): x_A on the bounds,
    P_FF x_F = -(q_F + P_FA x_A).  With a state that passes kkt_check this is the optimum itself (P is positive definite)."""
    n = q.size
    N = n // np.size(lb)
    x = np.where(state == 1, np.tile(ub, N), np.where(state == 2, np.tile(lb, N), 0.0))
    fr, ac = np.flatnonzero(state == 0), np.flatnonzero(state != 0)
    if fr.size:
        x[fr] = np.linalg.solve(Ps[np.ix_(fr, fr)], -(q[fr] + Ps[np.ix_(fr, ac)] @ x[ac]))
    return x


def oracle_rows(P, q, lb, ub, nu, rows):
    """[(u*, active (2n,) bool)] of the listed rows by oracle.qp.solve_exact_box (tq = I)."""
    n = P.shape[0]
    out = []
    for r in rows:
        info = {"nu": nu}
        x = oqp.solve_exact_box(P, q[r], np.tile(lb, n // nu), np.tile(ub, n // nu), info=info)
        act = np.zeros(2 * n, bool)
        act[info["active"]] = True
        out.append((x, act))
    return out


# ---- PDIP path: tests/test_pdip_factor_gpu.py, tests/test_pdip_paths_gpu.py, tests/test_cpu_pdip_inputs.py --------------------

PDIP_FACTOR_COND = 1e2
# (n, nb): every n sits on a tile or a 32-row sub-block edge of chol_diag_k / chol_panel_k / trsv_k
PDIP_FACTOR_SHAPES = ([(n, 64) for n in (2, 31, 33, 64)] + [(n, nb) for n in (65, 127, 128, 129) for nb in (64, 128)]
                      + [(449, 64), (449, 128)])
PDIP_FACTOR_ROWS = 6
PDIP_PIVOT_SHAPE = (129, 64)
PDIP_PIVOT_AT = (5, 40, 70)       # sub-block 0 of tile 0, sub-block 1 of tile 0, tile 1 (nb = 64)
PDIP_PIVOT_ROW = 2


def pdip_unit_spd(n, seed, cond=PDIP_FACTOR_COND):
    """Dense SPD matrix with random orthogonal eigenvectors (every tile couples with every other) and log-uniform eigenvalues
    whose extremes are 1 and ``cond`` exactly, then rescaled to a unit diagonal (D^-1/2 P D^-1/2, diagonal set to exactly 1): the
    library's normalisation by the upper median of the diagonal is then exactly 1.  Returns (P, the matrix before rescaling)."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = np.exp(rng.uniform(0.0, np.log(cond), n))
    ev[0], ev[-1] = 1.0, cond
    P0 = (Q * ev) @ Q.T
    P0 = 0.5 * (P0 + P0.T)
    s = 1.0 / np.sqrt(np.diag(P0))
    P = P0 * s[:, None] * s[None, :]
    P = np.tril(P) + np.tril(P, -1).T
    np.fill_diagonal(P, 1.0)
    return P, P0


def pdip_factor_case(n, seed=None):
    """P (unit diagonal), tq (n x 1, unused by the factor hook) and the six rows of a factor / solve case: dvec, mask, rhs (f32).
    Row 0: dvec = 0, mask all ones.  Row 1: dvec = 1e-6.  Row 2: IPM-like, dvec = exp(U(-3, 3)).  Row 3: polish-like, a random
    30 % of the variables masked, dvec = 1 there and 1e-6 elsewhere.  Row 4: all but three variables masked (same dvec rule).
    Row 5: one whole tile masked (rows 64 .. 127) when n >= 128, otherwise another draw of row 3."""
    seed = 7000 + n if seed is None else seed
    P, _ = pdip_unit_spd(n, seed)
    rng = np.random.default_rng(seed + 1)
    B = PDIP_FACTOR_ROWS
    dvec = np.zeros((B, n), np.float32)
    mask = np.ones((B, n), np.float32)
    dvec[1] = 1e-6
    dvec[2] = np.exp(rng.uniform(-3.0, 3.0, n))

    def masked(r, off):
        mask[r, off] = 0.0
        dvec[r] = np.where(off, 1.0, 1e-6)
    masked(3, rng.random(n) < 0.3)
    off = np.ones(n, bool)
    off[rng.choice(n, min(3, n), replace=False)] = False
    masked(4, off)
    draw = rng.random(n) < 0.3
    masked(5, (np.arange(n) // 64 == 1) if n >= 128 else draw)
    rhs = rng.standard_normal((B, n)).astype(np.float32)
    return dict(P=P, tq=np.ones((n, 1)), dvec=dvec, mask=mask, rhs=rhs)


def pdip_second_call(case, seed=99):
    """Another (dvec, mask, rhs) for the same P: what the second call on one handle factors (the Dacc invariant)."""
    n = case["P"].shape[0]
    rng = np.random.default_rng(seed)
    B = PDIP_FACTOR_ROWS
    off = rng.random((B, n)) < 0.2
    mask = np.where(off, 0.0, 1.0).astype(np.float32)
    dvec = np.where(off, 1.0, np.exp(rng.uniform(-4.0, 1.0, (B, n)))).astype(np.float32)
    return dvec, mask, rng.standard_normal((B, n)).astype(np.float32)


def pdip_K(P, dvec_row, mask_row):
    """K = mask mask' o P32 + diag(dvec) in float64 from the f32-rounded P: the matrix the kernels factor."""
    P32 = P.astype(np.float32).astype(np.float64)
    m = mask_row.astype(np.float64)
    return m[:, None] * m[None, :] * P32 + np.diag(dvec_row.astype(np.float64))


def pdip_solve_errors(P, dvec, mask, rhs, sol):
    """Per row (e, e32): max|sol - ref| / max|ref| of the kernels' solution and of LAPACK's f32 Cholesky (cho_factor / cho_solve
    on the float32 K), both against np.linalg.solve on the float64 K."""
    import scipy.linalg as sla
    out = []
    for b in range(dvec.shape[0]):
        K = pdip_K(P, dvec[b], mask[b])
        ref = np.linalg.solve(K, rhs[b].astype(np.float64))
        s32 = sla.cho_solve(sla.cho_factor(K.astype(np.float32), lower=True), rhs[b])
        assert s32.dtype == np.float32
        rm = np.abs(ref).max()
        out.append((float(np.abs(sol[b].astype(np.float64) - ref).max() / rm), float(np.abs(s32.astype(np.float64) - ref).max() / rm)))
    return out


def pdip_pivot_rows(case, at):
    """The case's rows with row PDIP_PIVOT_ROW replaced by one whose K has a negative diagonal entry at index ``at``
    (dvec = -3 against P_ii = 1): a non-positive pivot whatever came before it."""
    dvec, mask = case["dvec"].copy(), case["mask"].copy()
    dvec[PDIP_PIVOT_ROW] = 0.0
    mask[PDIP_PIVOT_ROW] = 1.0
    dvec[PDIP_PIVOT_ROW, at] = -3.0
    return dvec, mask


# The family of tests/test_pdip_paths_gpu.py: the generic SPD construction of tests/test_random_shapes_gpu.py at n = 130 (nu = 2,
# N = 65: T = 3 tiles of 64 with 62 pad rows), cond(P) = 1e3, 24 problems; PDIP_FAMILY_SCALE was chosen with the oracle so that
# every row's set holds 10 - 50 % of the variables (tests/test_cpu_pdip_inputs.py asserts it); row 1 is the empty set.
PDIP_FAMILY_SEED = 4100
PDIP_FAMILY_SCALE = 0.3
PDIP_FAMILY_B = 24


def pdip_family(seed=PDIP_FAMILY_SEED, scale=PDIP_FAMILY_SCALE, n=130, nu=2, cond=1e3, B=PDIP_FAMILY_B, n_aug=6):
    rng = np.random.default_rng(seed)
    P = spd_logspectrum(n, seed + 1, cond)
    tq = rng.standard_normal((n, n_aug)) * np.sqrt(np.diag(P))[:, None] * scale
    x0 = rng.standard_normal((B, n_aug))
    x0[1] = 0.0
    lb = -rng.uniform(0.2, 2.0, (B, nu))
    ub = rng.uniform(0.2, 2.0, (B, nu))
    return dict(P=P, tq=tq, nu=nu, N=n // nu, n=n, x0=x0, lb=lb, ub=ub, cond=cond)


def pdip_family_oracle(fam):
    """(U* (B, n), active (B, 2n) bool) of the family by oracle.qp.solve_exact_box."""
    B, n = fam["x0"].shape[0], fam["n"]
    U, act = np.empty((B, n)), np.zeros((B, 2 * n), bool)
    for b in range(B):
        info = {"nu": fam["nu"]}
        U[b] = oqp.solve_exact_box(fam["P"], fam["tq"] @ fam["x0"][b], np.tile(fam["lb"][b], fam["N"]), np.tile(fam["ub"][b], fam["N"]),
                                   info=info)
        act[b, info["active"]] = True
    return U, act


def pdip_flipped_guess(state, seed=5):
    """The bound states with a random 10 % of every row's variables flipped: a free one put on a random bound, a held one freed."""
    rng = np.random.default_rng(seed)
    g = state.copy()
    B, n = g.shape
    for b in range(B):
        idx = rng.choice(n, max(1, n // 10), replace=False)
        g[b, idx] = np.where(g[b, idx] == 0, rng.integers(1, 3, idx.size), 0)
    return g


def pdip_indefinite(n=64, seed=11):
    """Unit diagonal, eigenvalues in [1, 10] but one negative: the diagonal is positive (the handle is created), no Cholesky exists."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = rng.uniform(1.0, 10.0, n)
    ev[0] = -5.0
    P0 = (Q * ev) @ Q.T
    P0 = 0.5 * (P0 + P0.T)
    s = 1.0 / np.sqrt(np.diag(P0))
    P = P0 * s[:, None] * s[None, :]
    P = np.tril(P) + np.tril(P, -1).T
    np.fill_diagonal(P, 1.0)
    return P


# ---- closed-loop and chain step kernels (csrc/closed_loop.hip, chain half of csrc/chain.hip): tests/test_cl_step_gpu.py,
# tests/test_chain_step_gpu.py, tests/test_cpu_cl_step_inputs.py ------------------------------------------------------------------
# Nothing below imports the package: the model is a bag of matrices in the fields of nnmpc_cl_model (include/nnmpc.h), the
# reference is numpy in np.longdouble on the RECORDED inputs of a step, and every fp64 identity comes with its own bound
#     |kernel - reference| <= 2 gamma_n (the identity with every matrix and vector replaced by its absolute value and every
#                                        subtraction by an addition),       gamma_n = n eps / (1 - n eps),
# n = the additions along the longest path through the identity: the forward bound of a dot product in any summation order
# (Higham, Accuracy and Stability, section 3.5); the factor 2 covers nesting and FMA contraction.

# case -> (nx, nu, ny, nd, nz); the boundary each one puts into play (all loops of the kernels stride by 256 threads):
CL_STEP_CASES = {
    "a": (1, 1, 1, 0, 0),        # every dimension 1, nd = 0, nz = 0: Bp / Cd / Eb NULL
    "b": (3, 2, 2, 1, 1),        # smallest with every term present
    "c": (254, 3, 7, 5, 1),      # nx < 256 < na = 259: bin[ny + k - nx] on a second trip; nx + nu = 257; nbv = 255
    "d": (255, 2, 5, 1, 1),      # na = nbv = 256 exactly; nx + nu = 257
    "e": (257, 5, 12, 0, 2),     # nx on a second trip with nd = 0; nbv = 259
    "f": (300, 4, 257, 3, 2),    # ny > 256 (r, bin, y); nx, na, nbv all on a second trip
    "g": (40, 6, 300, 2, 3),     # ny >> nx
    "h": (520, 2, 3, 2, 1),      # three trips
}
CL_STEP_T = 12
CL_STEP_N = 4                    # horizon of the MPC slot
CL_STEP_MPC_COND = 1e2
CL_STEP_HIDDEN = [64, 70]        # one full and one ragged column tile of cl_nn_layer_k
CL_STEP_KINDS = ("us", "satdlqr", "nn_u", "nn", "mpc")
CL_STEP_COUNTS = (3, 4, 2, 3, 4)  # instances per slot: nb = 16
CL_STEP_NSCEN = 3
CL_STEP_NN_TOL = 1e-4            # the bar of cl_assert_one_step_identity (f32 sums)
# Gaussian scales on top of 1 / sqrt(fan-in).  L: with a gain of the order of 1 the estimator matrix (I - L Caug) Aaug of a
# random draw has a norm of the order of sqrt(na) + sqrt(ny) and the estimate leaves every bound within 12 steps; entries of
# 0.3 / (sqrt(na) + sqrt(ny)) keep |L|_2 near 0.3 (tests/test_cpu_cl_step_inputs.py holds the records below 1e3).
# Qaug: G with entries 0.5 / sqrt(nx + nu) keeps the running cost of the largest case below 1e3.
CL_STEP_SCALES = dict(Qb=0.8, Qy=0.8, Eb=0.05, Kaug=0.3, L=0.3, Qaug=0.5, q0=0.1, x0=0.3, sigma=0.05, p=0.5)
# Seeds: 9000 + 10 * (index of the case).  Aaug has nd eigenvalues 1 and a small random L moves them either way; case b also
# carries the 513-step runs across the event blocks, so its seed was chosen with the reference alone among 9010 .. 9019 for an
# estimator matrix (I - L Caug) Aaug of spectral radius 0.954 (asserted on the CPU, like every share figure).
CL_STEP_SEEDS = dict({c: 9000 + 10 * i for i, c in enumerate(sorted(CL_STEP_CASES))}, b=9012)
CL_STEP_LONG_T = (257, 513)      # one and two crossings of the 256-step event block


def cl_step_model(seed, nx, nu, ny, nd, nz, scales=CL_STEP_SCALES):
    """A synthetic model in the fields of nnmpc_cl_model (plus Pr, E of the target handle, Kaug of a SATDLQR slot and sigma): A
    with spectral radius 0.9, Gaussian B, Bp, C, Cd, L, tb, Qb, Qy, Xb, Xu, Maug, Kaug scaled by 1 / sqrt(fan-in), Qaug = G G',
    Raug SPD, Pr / E / ulb / uub from ts_matrices(seed, nu, nz, 10), Eb small enough that E u = e stays feasible inside the
    box.  Aaug, Baug, Caug: the augmented matrices of A, B, Bp, C, Cd (constant disturbance model).  No Riccati equation, no
    reduction of a target problem: the kernels are linear maps and are tested as such.  Bp / Cd are None for nd = 0, Eb for
    nz = 0 (the NULL pointers nnmpc_cl_create allows)."""
    rng = np.random.default_rng(seed)
    g = lambda r, c, s=1.0: s * rng.standard_normal((r, c)) / np.sqrt(max(c, 1))
    na, nbv, nzz = nx + nd, nx + nz, nx + nu
    W = rng.standard_normal((nx, nx))
    A = 0.9 * W / np.abs(np.linalg.eigvals(W)).max()
    B, Bp, C, Cd = g(nx, nu), g(nx, nd), g(ny, nx), g(ny, nd)
    L = g(na, ny, scales["L"] * np.sqrt(ny) / (np.sqrt(na) + np.sqrt(ny)))
    tb, Qb, Qy = g(nbv, ny + nd), g(nu, nbv, scales["Qb"]), g(nu, ny, scales["Qy"])
    Eb, Xb, Xu = g(nz, nbv, scales["Eb"]), g(nx, nbv), g(nx, nu)
    Maug, Kaug = g(nzz, nu), g(nu, nzz, scales["Kaug"])
    G = g(nzz, nzz, scales["Qaug"])
    Gr = g(nu, nu)
    q0 = scales["q0"] * rng.standard_normal(nu)
    x0, xhat0 = scales["x0"] * rng.standard_normal(nx), scales["x0"] * rng.standard_normal(na)
    sigma = scales["sigma"] * rng.uniform(0.5, 1.5, ny)
    Pr, E, ulb, uub = ts_matrices(seed, nu, nz, 10.0)
    uprev0 = 0.5 * (ulb + rng.uniform(0.0, 1.0, nu) * (uub - ulb))
    Aaug = np.block([[A, Bp], [np.zeros((nd, nx)), np.eye(nd)]])
    Baug = np.vstack((B, np.zeros((nd, nu))))
    Caug = np.hstack((C, Cd))
    return dict(nx=nx, nu=nu, ny=ny, nd=nd, nz=nz, A=A, B=B, C=C, Bp=Bp if nd else None, Aaug=Aaug, Baug=Baug, Caug=Caug, L=L,
                tb=tb, Qb=Qb, Qy=Qy, q0=q0, Cd=Cd if nd else None, Eb=Eb if nz else None, Xb=Xb, Xu=Xu, Qaug=G @ G.T,
                Raug=Gr @ Gr.T + 0.1 * np.eye(nu), Maug=Maug, ulb=ulb, uub=uub, x0=x0, xhat0=xhat0, uprev0=uprev0,
                Pr=Pr, E=E, Kaug=Kaug, sigma=sigma)


def cl_step_batch(case, seed=None, kinds=CL_STEP_KINDS, counts=CL_STEP_COUNTS, T=CL_STEP_T):
    """Everything one run of a case needs but the device: the model, one slot spec per kind (dicts in the form DeviceClosedLoop
    takes; the MPC spec carries P, tq, nu, N in place of a solver), the slot and scenario of every instance, setpoints in +-1
    and disturbances in +-0.5 of three scenarios (a fresh draw at every step: every step is its own test vector), the noise."""
    nx, nu, ny, nd, nz = CL_STEP_CASES[case]
    seed = CL_STEP_SEEDS[case] if seed is None else seed
    M = cl_step_model(seed, nx, nu, ny, nd, nz)
    rng = np.random.default_rng(seed + 1)
    slots = []
    for k in kinds:
        if k == "us":
            slots.append(dict(kind="us"))
        elif k == "satdlqr":
            slots.append(dict(kind="satdlqr", Kaug=M["Kaug"]))
        elif k in ("nn_u", "nn"):
            wu = k == "nn_u"
            slots.append(dict(kind="nn", weights=cl_nn_weights(seed + (2 if wu else 3), 2 * nx + (2 if wu else 1) * nu, CL_STEP_HIDDEN, nu),
                              with_uprev=wu, xscale=np.random.default_rng(seed + 4).uniform(0.5, 2.0, nx)))
        else:
            n = CL_STEP_N * nu
            slots.append(dict(kind="mpc", P=spd_logspectrum(n, seed + 5, CL_STEP_MPC_COND), nu=nu, N=CL_STEP_N,
                              tq=np.random.default_rng(seed + 6).standard_normal((n, nx + nu)) / np.sqrt(nx + nu)))
    inst_slot = np.repeat(np.arange(len(kinds)), counts[:len(kinds)]).astype(np.int32)
    nb = inst_slot.size
    scen = ((np.arange(nb) + 1) % CL_STEP_NSCEN).astype(np.int32)
    SP = rng.uniform(-1.0, 1.0, (CL_STEP_NSCEN, T, ny))
    DS = CL_STEP_SCALES["p"] * rng.uniform(-1.0, 1.0, (CL_STEP_NSCEN, T, nd))
    V = rng.standard_normal((T + 1, nb, ny))
    return dict(case=case, M=M, slots=slots, inst_slot=inst_slot, scen=scen, SP=SP, DS=DS, V=V, sigma=M["sigma"], T=T)


def cl_gamma(n):
    return n * TS_EPS / (1.0 - n * TS_EPS)


def _cl_ld(M):
    """np.longdouble copies of the model's matrices and their absolute values (cached in the dict)."""
    if "_ld" not in M:
        nx, nu, ny, nd, nz = (M[k] for k in ("nx", "nu", "ny", "nd", "nz"))
        shape = dict(Bp=(nx, nd), Cd=(ny, nd), Eb=(nz, nx + nz), E=(nz, nu))
        ld, ab = {}, {}
        for k in ("A", "B", "C", "Bp", "Aaug", "Baug", "Caug", "L", "tb", "Qb", "Qy", "q0", "Cd", "Eb", "Xb", "Xu", "Qaug", "Raug",
                  "Maug", "ulb", "uub"):
            a = np.zeros(shape[k]) if M.get(k) is None else np.asarray(M[k], np.float64)
            ld[k] = a.astype(np.longdouble)
            ab[k] = np.abs(ld[k])
        M["_ld"] = (ld, ab)
    return M["_ld"]


def _ld(a):
    return np.asarray(a, np.longdouble)


def cl_ref_filter(M, xhat, uprev, y):
    """xp = Aaug xhat + Baug uprev, xhat' = xp + L (y - Caug xp); rows.  -> (xhat', bound)."""
    m, a = _cl_ld(M)
    xhat, uprev, y = _ld(xhat), _ld(uprev), _ld(y)
    xp = xhat @ m["Aaug"].T + uprev @ m["Baug"].T
    axp = np.abs(xhat) @ a["Aaug"].T + np.abs(uprev) @ a["Baug"].T
    out = xp + (y - xp @ m["Caug"].T) @ m["L"].T
    mag = axp + (np.abs(y) + axp @ a["Caug"].T) @ a["L"].T
    na = M["nx"] + M["nd"]
    return out, 2.0 * cl_gamma(na + M["nu"] + na + M["ny"] + 2) * mag


def cl_ref_reduce(M, xhat1, ysp):
    """dhat = xhat'[nx:], b = tb [ysp; dhat], q = Qb b + Qy (ysp - Cd dhat) + q0, e = Eb b.  -> (b, |b| bound form, q, e)."""
    m, a = _cl_ld(M)
    xhat1, ysp = _ld(xhat1), _ld(ysp)
    dhat = xhat1[:, M["nx"]:]
    bin_ = np.concatenate((ysp, dhat), axis=1)
    b = bin_ @ m["tb"].T
    q = b @ m["Qb"].T + (ysp - dhat @ m["Cd"].T) @ m["Qy"].T + m["q0"]
    return b, np.abs(bin_) @ a["tb"].T, q, b @ m["Eb"].T


def cl_ref_expand(M, b, babs, us):
    """xs = Xb b + Xu us.  -> (xs, bound)."""
    m, a = _cl_ld(M)
    us = _ld(us)
    n = M["ny"] + M["nd"] + M["nx"] + M["nz"] + M["nu"] + 2
    return b @ m["Xb"].T + us @ m["Xu"].T, 2.0 * cl_gamma(n) * (babs @ a["Xb"].T + np.abs(us) @ a["Xu"].T)


def cl_ref_z(xhat1, xs, uprev, us, nx):
    """z = [xhat'[:nx] - xs; uprev - us] and its absolute-value form."""
    xh, xs, uprev, us = _ld(xhat1)[:, :nx], _ld(xs), _ld(uprev), _ld(us)
    return (np.concatenate((xh - xs, uprev - us), axis=1),
            np.concatenate((np.abs(xh) + np.abs(xs), np.abs(uprev) + np.abs(us)), axis=1))


def cl_ref_satdlqr(M, Kaug, z, zabs, us):
    """clip(Kaug z + us).  -> (u, bound): the clip is 1-Lipschitz, so the bound of the unclipped value holds."""
    m, a = _cl_ld(M)
    K, us = _ld(Kaug), _ld(us)
    u = np.minimum(np.maximum(z @ K.T + us, m["ulb"]), m["uub"])
    return u, 2.0 * cl_gamma(M["nx"] + M["nu"] + 3) * (zabs @ np.abs(K).T + np.abs(us))


def cl_ref_cost(M, z, zabs, u, us, avg0, tg):
    """ell = z'Qaug z + w'Raug w + z'Maug w + w'Maug'z with w = u - us; avg' = (avg tg + ell) / (tg + 1).  -> (ell, avg', bound of avg')."""
    m, a = _cl_ld(M)
    u, us, avg0, tg = _ld(u), _ld(us), _ld(avg0), _ld(tg)
    w, wabs = u - us, np.abs(u) + np.abs(us)
    zM = z @ m["Maug"]
    ell = ((z @ m["Qaug"].T) * z).sum(axis=1) + ((w @ m["Raug"].T) * w).sum(axis=1) + 2.0 * (zM * w).sum(axis=1)
    mag = ((zabs @ a["Qaug"].T) * zabs).sum(axis=1) + ((wabs @ a["Raug"].T) * wabs).sum(axis=1) + 2.0 * ((zabs @ a["Maug"]) * wabs).sum(axis=1)
    n = 2 * (M["nx"] + M["nu"]) + M["nu"] + 8 + 4
    return ell, (avg0 * tg + ell) / (tg + 1.0), 2.0 * cl_gamma(n) * (np.abs(avg0) * tg + mag) / (tg + 1.0)


def cl_ref_plant(M, x, u, p):
    """x' = A x + B u + Bp p.  -> (x', bound)."""
    m, a = _cl_ld(M)
    x, u, p = _ld(x), _ld(u), _ld(p)
    x1 = x @ m["A"].T + u @ m["B"].T + p @ m["Bp"].T
    return x1, 2.0 * cl_gamma(M["nx"] + M["nu"] + M["nd"] + 2) * (np.abs(x) @ a["A"].T + np.abs(u) @ a["B"].T + np.abs(p) @ a["Bp"].T)


def cl_ref_measure(M, x1, v1, sigma):
    """y = C x + sigma o v.  -> (y, bound)."""
    m, a = _cl_ld(M)
    x1, v1, sigma = _ld(x1), _ld(v1), _ld(sigma)
    return x1 @ m["C"].T + sigma * v1, 2.0 * cl_gamma(M["nx"] + 2) * (np.abs(x1) @ a["C"].T + sigma * np.abs(v1))


def cl_ref_targets(M, q, e):
    """The certified target optimum of every row (ts_reference: the enumeration of all bound states, nu <= 7).
    -> (us (R, nu) float64, kept (R,) bool under ts_kept, cond (R,), number of inputs on a bound (R,))."""
    q = np.asarray(q, np.float64)
    e = np.asarray(e, np.float64).reshape(q.shape[0], M["nz"])
    refs = ts_reference(M["Pr"], M["E"], M["ulb"], M["uub"], q, e)
    return (np.array([r["us"] for r in refs]), np.array([ts_kept(r, q[i]) for i, r in enumerate(refs)]),
            np.array([r["cond"] for r in refs]), np.array([int((r["state"] != 0).sum()) for r in refs]))


def cl_ref_mpc(spec, z, us, ulb, uub):
    """First move of v* = argmin 1/2 v'P v + (tq z)'v, ulb - us <= v <= uub - us (every stage), by oracle.qp.solve_exact_box.
    -> (v*[:nu] (R, nu), max |v*| (R,))."""
    nu, N = spec["nu"], spec["N"]
    z, us = np.asarray(z, np.float64), np.asarray(us, np.float64)
    first, vmax = np.empty((z.shape[0], nu)), np.empty(z.shape[0])
    for r in range(z.shape[0]):
        v = oqp.solve_exact_box(spec["P"], spec["tq"] @ z[r], np.tile(ulb - us[r], N), np.tile(uub - us[r], N))
        first[r], vmax[r] = v[:nu], np.abs(v).max()
    return first, vmax


def cl_mpc_tol(cond=CL_STEP_MPC_COND):
    """The bar of tests/test_random_shapes_gpu.py for status-0 rows."""
    return 1e-7 * max(1.0, cond / 1e3)


def cl_step_reference(b, rec, tg0=0, uprev_in=None, want=None):
    """Every identity of one step, for every instance and step of a run, each from the RECORDED inputs of that step (errors do
    not compound).  ``b``: a cl_step_batch (its SP / DS / V are this call's tables), ``rec``: the records of the run (T + 1 rows
    of y, x, xhat, avg; T rows of u, xs, us), ``tg0``: steps since create / reset before this call, ``uprev_in``: (nb, nu) the
    previous input of every instance at the start of the call (default: the model's uprev0).
    Returns {identity: dict(got, ref, bound, mask)} with (T, nb, .) arrays; fp64 identities carry the derived ``bound``, "us" the
    TS_ERR_FACTOR bar (mask: ts_kept), "u_mpc" the bar of test_random_shapes_gpu.py, "u_us" must be equal bit for bit (bound 0); the NN
    moves are judged by cl_one_step_reference (not here)."""
    M = b["M"]
    nx, nu, ny, nd, nz = (M[k] for k in ("nx", "nu", "ny", "nd", "nz"))
    T, nb = rec["u"].shape[0], rec["u"].shape[1]
    fl = lambda a: np.ascontiguousarray(a).reshape(T * nb, a.shape[2] if a.ndim == 3 else 1)
    up = np.concatenate(((np.tile(M["uprev0"], (nb, 1)) if uprev_in is None else uprev_in)[None], rec["u"][:-1]), axis=0)
    ysp = np.swapaxes(b["SP"][b["scen"]], 0, 1)
    p = np.swapaxes(b["DS"][b["scen"]], 0, 1)
    tg = np.repeat(tg0 + np.arange(T), nb).astype(np.float64)
    out = {}
    put = lambda name, got, ref, bound, mask=None: out.__setitem__(name, dict(
        got=np.asarray(got).reshape(T, nb, -1), ref=np.asarray(ref).reshape(T, nb, -1), bound=np.asarray(bound).reshape(T, nb, -1),
        mask=np.ones((T, nb), bool) if mask is None else np.asarray(mask).reshape(T, nb)))
    xh1, bnd = cl_ref_filter(M, fl(rec["xhat"][:-1]), fl(up), fl(rec["y"][:-1]))
    put("xhat", rec["xhat"][1:], xh1, bnd)
    bb, babs, q, e = cl_ref_reduce(M, fl(rec["xhat"][1:]), fl(ysp))
    us, kept, cond, nact = cl_ref_targets(M, q, e)
    put("us", rec["us"], us, (TS_ERR_FACTOR * TS_EPS * cond * np.maximum(1.0, np.abs(us).max(axis=1)))[:, None] * np.ones((1, nu)), kept)
    out["us"]["on_bound"] = nact.reshape(T, nb)
    xs, bnd = cl_ref_expand(M, bb, babs, fl(rec["us"]))
    put("xs", rec["xs"], xs, bnd)
    z, zabs = cl_ref_z(fl(rec["xhat"][1:]), fl(rec["xs"]), fl(up), fl(rec["us"]), nx)
    for s, spec in enumerate(b["slots"]):
        rows = np.flatnonzero(np.tile(b["inst_slot"] == s, T))
        m = np.tile(b["inst_slot"] == s, T).reshape(T, nb)
        if spec["kind"] == "us":
            put("u_us", rec["u"], rec["us"], np.zeros((T * nb, nu)), m)
        elif spec["kind"] == "satdlqr":
            u, bnd = cl_ref_satdlqr(M, spec["Kaug"], z, zabs, fl(rec["us"]))
            put("u_satdlqr", rec["u"], u, bnd, m)
        elif spec["kind"] == "mpc" and (want is None or "u_mpc" in want):
            first = np.zeros((T * nb, nu))
            vmax = np.ones(T * nb)
            first[rows], vmax[rows] = cl_ref_mpc(spec, z[rows], fl(rec["us"])[rows], M["ulb"], M["uub"])
            put("u_mpc", rec["u"], first + fl(rec["us"]), (cl_mpc_tol() * np.maximum(1.0, vmax))[:, None] * np.ones((1, nu)), m)
            out["u_mpc"]["first"] = first.reshape(T, nb, nu)
    ell, avg1, bnd = cl_ref_cost(M, z, zabs, fl(rec["u"]), fl(rec["us"]), fl(rec["avg"][:-1])[:, 0], tg)
    put("avg", rec["avg"][1:], avg1, bnd)
    x1, bnd = cl_ref_plant(M, fl(rec["x"][:-1]), fl(rec["u"]), fl(p))
    put("x", rec["x"][1:], x1, bnd)
    y1, bnd = cl_ref_measure(M, fl(rec["x"][1:]), fl(b["V"][1:]), b["sigma"])
    put("y", rec["y"][1:], y1, bnd)
    return out


def cl_identity_ratios(idn):
    """Largest |got - ref| / bound of every identity over its masked rows (0 / 0 = 0; anything over a zero bound = inf)."""
    out = {}
    for name, d in idn.items():
        err = np.abs(_ld(d["got"]) - _ld(d["ref"]))[d["mask"]]
        bnd = _ld(d["bound"])[d["mask"]]
        if err.size == 0:
            out[name] = 0.0
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / bnd)
        out[name] = float(np.nanmax(np.where(np.isnan(r), np.inf, r)))
    return out


def cl_step_simulate(b, T=None):
    """The reference ALONE, state carried in float64 from step to step (us from the certified target oracle, NN moves from
    oracle.nn, MPC moves from oracle.qp): the records a faultless device run would give, up to rounding.  What
    tests/test_cpu_cl_step_inputs.py judges the inputs of the GPU tests with.  Also returns ``kept`` / ``on_bound`` (T, nb)."""
    from oracle import nn as onn
    M = b["M"]
    nx, nu = M["nx"], M["nu"]
    T = b["T"] if T is None else T
    nb = b["inst_slot"].size
    f8 = lambda a: np.asarray(a, np.float64)
    x, xhat, up = np.tile(M["x0"], (nb, 1)), np.tile(M["xhat0"], (nb, 1)), np.tile(M["uprev0"], (nb, 1))
    y = f8(cl_ref_measure(M, x, b["V"][0], b["sigma"])[0])
    avg = np.zeros(nb)
    rec = dict(y=[y], x=[x], xhat=[xhat], avg=[avg], u=[], xs=[], us=[], kept=[], on_bound=[])
    for t in range(T):
        xhat = f8(cl_ref_filter(M, xhat, up, y)[0])
        bb, babs, q, e = cl_ref_reduce(M, xhat, b["SP"][b["scen"], t])
        us, kept, _, nact = cl_ref_targets(M, q, e)
        xs = f8(cl_ref_expand(M, bb, babs, us)[0])
        z, zabs = cl_ref_z(xhat, xs, up, us, nx)
        u = np.empty((nb, nu))
        for s, spec in enumerate(b["slots"]):
            r = np.flatnonzero(b["inst_slot"] == s)
            if spec["kind"] == "us":
                u[r] = us[r]
            elif spec["kind"] == "satdlqr":
                u[r] = f8(cl_ref_satdlqr(M, spec["Kaug"], z[r], zabs[r], us[r])[0])
            elif spec["kind"] == "nn":
                u[r] = onn.control_input(spec["weights"], xhat[r, :nx], up[r], xs[r], us[r], spec["xscale"], M["ulb"], M["uub"], spec["with_uprev"])
            else:
                u[r] = cl_ref_mpc(spec, f8(z[r]), us[r], M["ulb"], M["uub"])[0] + us[r]
        avg = f8(cl_ref_cost(M, z, zabs, u, us, avg, np.full(nb, float(t)))[1])
        x = f8(cl_ref_plant(M, x, u, b["DS"][b["scen"], t])[0])
        y = f8(cl_ref_measure(M, x, b["V"][t + 1], b["sigma"])[0])
        up = u
        for k, v in (("y", y), ("x", x), ("xhat", xhat), ("avg", avg), ("u", u), ("xs", xs), ("us", us), ("kept", kept), ("on_bound", nact)):
            rec[k].append(v)
    return {k: np.array(v) for k, v in rec.items()}


# ---- chains (chain_pre_k / chain_post_k) and nnmpc_qp_first_moves -----------------------------------------------------------------
CHAIN_STEP_SHAPES = [(1, 1, 0), (3, 2, 1), (255, 2, 3), (257, 3, 0), (300, 5, 3), (520, 2, 2)]     # (nx, nu, nd); the last: nx + nu + nd > 512
CHAIN_STEP_T = 8
FIRST_MOVES_CASES = [(1, 1, 1, True), (7, 3, 11, False), (7, 3, 11, True), (70000, 16, 20, True)]  # (B, nu, ldu, us given); the last: 1 120 000 elements


def chain_step_case(nx, nu, nd, nc, seed=None, T=CHAIN_STEP_T):
    """A, B, Bd as in cl_step_model, the regulator's P / tq as in cl_step_batch's MPC slot, asymmetric bounds, and the target
    pairs / disturbances of T steps of nc chains (xs small beside x, us well inside the box)."""
    seed = 9500 + nx if seed is None else seed
    rng = np.random.default_rng(seed)
    g = lambda r, c: rng.standard_normal((r, c)) / np.sqrt(max(c, 1))
    W = rng.standard_normal((nx, nx))
    A = 0.9 * W / np.abs(np.linalg.eigvals(W)).max()
    B, Bd = g(nx, nu), g(nx, nd)
    ulb, uub = -rng.uniform(0.2, 1.5, nu), rng.uniform(0.2, 1.5, nu)
    n = CL_STEP_N * nu
    spec = dict(P=spd_logspectrum(n, seed + 5, CL_STEP_MPC_COND), nu=nu, N=CL_STEP_N, tq=rng.standard_normal((n, nx + nu)) / np.sqrt(nx + nu))
    return dict(nx=nx, nu=nu, nd=nd, nc=nc, A=A, B=B, Bd=Bd, ulb=ulb, uub=uub, spec=spec, x0=0.5 * rng.standard_normal(nx),
                uprev0=0.5 * (ulb + rng.uniform(0, 1, nu) * (uub - ulb)), Xs=0.3 * rng.standard_normal((T, nc, nx)),
                Us=0.5 * (ulb + rng.uniform(0, 1, (T, nc, nu)) * (uub - ulb)), D=0.5 * rng.uniform(-1, 1, (T, nc, nd)), T=T)


def chain_step_reference(c, rec, Xs, Us, D):
    """The chain identities from the recorded x, uprev, u of a call: u[t] = v*[:nu] + us[t] with z = [x[t] - xs[t]; uprev[t] - us[t]]
    (bar of test_random_shapes_gpu.py), x[t + 1] = A x[t] + B u[t] + Bd d[t] (derived bound, rows t < T - 1), uprev[t + 1] = u[t]
    (bit for bit).  -> {identity: dict(got, ref, bound, mask)}."""
    nx, nu, nd, nc = c["nx"], c["nu"], c["nd"], c["nc"]
    T = rec["u"].shape[0]
    fl = lambda a: np.ascontiguousarray(a).reshape(-1, a.shape[-1])
    z = np.concatenate((fl(rec["x"]) - fl(Xs), fl(rec["uprev"]) - fl(Us)), axis=1)
    first, vmax = cl_ref_mpc(c["spec"], z, fl(Us), c["ulb"], c["uub"])
    one = np.ones((T, nc), bool)
    out = dict(u=dict(got=rec["u"], ref=(first + fl(Us)).reshape(T, nc, nu), first=first.reshape(T, nc, nu), mask=one,
                      bound=((cl_mpc_tol() * np.maximum(1.0, vmax))[:, None] * np.ones((1, nu))).reshape(T, nc, nu)))
    A, B, Bd = _ld(c["A"]), _ld(c["B"]), _ld(c["Bd"])
    x, u, d = _ld(fl(rec["x"][:-1])), _ld(fl(rec["u"][:-1])), _ld(np.asarray(D[:T - 1]).reshape((T - 1) * nc, nd))
    x1 = x @ A.T + u @ B.T + d @ Bd.T
    bnd = 2.0 * cl_gamma(nx + nu + nd + 2) * (np.abs(x) @ np.abs(A).T + np.abs(u) @ np.abs(B).T + np.abs(d) @ np.abs(Bd).T)
    out["x"] = dict(got=rec["x"][1:], ref=x1.reshape(T - 1, nc, nx), bound=bnd.reshape(T - 1, nc, nx), mask=one[1:])
    out["uprev"] = dict(got=rec["uprev"][1:], ref=rec["u"][:-1], bound=np.zeros((T - 1, nc, nu)), mask=one[1:])
    return out


# ---- first-set predictor (csrc/qp_predict.h) through nnmpc_qp_debug_predict: tests/test_predict_kernel_gpu.py,
# tests/test_cpu_predict_inputs.py ------------------------------------------------------------------------------------------------
# pred_reference reproduces what asm_predict_k STORES (bf16 H', f16 x_unc, f32 bounds, bf16 y and nu between iterations, the restart
# and the adaptive count by group of MR rows) and nothing of how it computes; it imports nothing from the package.

PRED_COUNTS = (1, 2, 3, 8, 24, 64, 0)          # iterations: fixed, and 0 = adaptive
PRED_FAC10 = 3
# case -> (nu, N); n = nu N.  Plants of the form synthetic.plant returns: Nx = 12, Ny = 6, rho 0.97, the CDU tuning (Q = 2 C'C, R = 0.1 I, S = 0)
PRED_CASES = {
    "a": (8, 64),       # <4,4>: n = W exactly; per32 bound reuse
    "b": (32, 16),      # <4,4>: ldb = 36; one stage per 32 columns
    "c": (4, 128),      # <4,4>: the smallest nu; every lane one whole stage
    "d": (12, 43),      # <4,4>: NU4 but 32 % nu != 0 (no reuse across column tiles); n = 516 > W: columns 512 .. 515 stay 0
    "e": (64, 8),       # <4,4>: the largest nu; the largest LDS image
    "f": (6, 86),       # <4,2,false>: the per-column bound lookup with its wrap; MR = 32
    "g": (5, 103),      # <4,2,false>: n = 515 is no multiple of 4: the byte-store path of the states
    "h": (7, 74),       # <4,2,false>: wrap at an odd nu
    "i": (16, 64),      # n = 1024: <8,2> (wide = 1) and <4,4>
}
# plant seeds 300 + index; cases e and i moved on by 10: chosen with the reference alone so that no restart sum that decides a kb within
# the first 24 iterations is smaller than 1e-3 of its terms and the two arithmetic variants agree at every count but 64
PRED_SEEDS = dict({c: 300 + k for k, c in enumerate(sorted(PRED_CASES))}, e=314, i=318)
PRED_MIX_SX = (0.5, 2.0, 4.0)                  # state spread of the three groups of the 2 MR + 2 batch
PRED_SX = 6.0                                  # state spread of the B = 1, MR - 1, MR + 1 batches
PRED_TIGHT_B = 2
PRED_TIGHT = 0.05                              # box scale of the "tight" batch
PRED_SPECIAL = dict(tiny=3, wide=5, steady=7)  # rows of the MR + 1 batch: a box of +-0.02, one of +-50, x0 = 0 with two inputs exactly on a bound


def pred_instance(nu, wide):
    """(W, MR) of the instance the library launches."""
    return (1024, 32) if wide else (512, 64 if nu % 4 == 0 else 32)


def pred_plant(nu, N, seed, rho=0.97):
    """synthetic.plant's construction at Nx = 12, Ny = 6 with the CDU tuning."""
    rng = np.random.default_rng(seed)
    Nx, Ny = 12, 6
    W = rng.standard_normal((Nx, Nx)) / np.sqrt(Nx)
    A = rho * W / np.max(np.abs(np.linalg.eigvals(W)))
    B = rng.standard_normal((Nx, nu)) / np.sqrt(Nx)
    Cm = rng.standard_normal((Ny, Nx)) / np.sqrt(Nx)
    return dict(A=A, B=B, C=Cm, Q=2.0 * Cm.T @ Cm, R=0.1 * np.eye(nu), S=0.0 * np.eye(nu), N=N, ulb=-np.ones((nu, 1)), uub=np.ones((nu, 1)))


_PRED_CASE_CACHE = {}


def pred_case(name):
    """Plant, (P, tq, nu) of build_regulator_matrices and Pinv, Kunc exactly as BatchedBoxQP forms them for Kunc="auto"."""
    if name not in _PRED_CASE_CACHE:
        import scipy.linalg as sla
        from industrial_nnmpc_2021_amd.linearMPC_build import build_regulator_matrices
        nu, N = PRED_CASES[name]
        pl = pred_plant(nu, N, PRED_SEEDS[name])
        P, tq, nu2 = build_regulator_matrices(pl)
        assert nu2 == nu and P.shape[0] == nu * N
        P = np.ascontiguousarray(P, dtype=np.float64)
        tq = np.ascontiguousarray(tq, dtype=np.float64)
        Ps = np.tril(P) + np.tril(P, -1).T
        cf = sla.cho_factor(Ps, lower=True)
        Kunc = -sla.cho_solve(cf, tq)
        Pinv = sla.cho_solve(cf, np.eye(nu * N))
        _PRED_CASE_CACHE[name] = dict(name=name, pl=pl, P=P, Ps=Ps, tq=tq, nu=nu, N=N, n=nu * N, Kunc=Kunc, Pinv=Pinv)
    return _PRED_CASE_CACHE[name]


def pred_batches(c, MR):
    """name -> (x0, lb, ub): B = 1, MR - 1, MR + 1 (with the PRED_SPECIAL rows; its second group is one real row and MR - 1 clones)
    at sx = PRED_SX, 2 MR + 2 with sx = 0.5 / 2 / 4 by group, and B = 2 at sx = 4 with both boxes scaled by PRED_TIGHT: on this small
    plant the bounds x_unc violates stay within the first stages whatever sx is (at most ~40 per problem at sx = 4), so that the adaptive
    count of every group of the other batches is at or near its floor of 8; the tight boxes take it well above (the one group of that batch is two problems and MR - 2 clones of the second,
    which count like problems; only two rows, because next to a tight box most of a row's w lies within PRED_TAU max|w| of a bound)."""
    pl, seed = c["pl"], 10 * PRED_SEEDS[c["name"]]
    out = {}
    for k, (tag, B) in enumerate((("b1", 1), ("mr-1", MR - 1), ("mr+1", MR + 1))):
        _, x0, lb, ub = batch_inputs(pl, B, seed + k, PRED_SX)
        if tag == "mr+1":
            t, w, s = PRED_SPECIAL["tiny"], PRED_SPECIAL["wide"], PRED_SPECIAL["steady"]
            lb[t], ub[t] = -0.02, 0.02
            lb[w], ub[w] = -50.0, 50.0
            x0[s] = 0.0
            ub[s, 0] = 0.0                     # us on its upper bound for input 0, on its lower bound for input 1
            lb[s, 1] = 0.0
        out[tag] = (x0, lb, ub)
    parts = [batch_inputs(pl, b, seed + 3 + g, sx)[1:] for g, (b, sx) in enumerate(zip((MR, MR, 2), PRED_MIX_SX))]
    out["mix"] = tuple(np.ascontiguousarray(np.concatenate([p[i] for p in parts], axis=0)) for i in range(3))
    _, x0, lb, ub = batch_inputs(pl, PRED_TIGHT_B, seed + 6, PRED_MIX_SX[2])
    out["tight"] = (x0, PRED_TIGHT * lb, PRED_TIGHT * ub)
    return out


def pred_beta(iters=64):
    """beta[k] of the t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2 recursion, as floats."""
    beta, t = np.zeros(64, np.float32), 1.0
    for k in range(iters):
        tn = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
        beta[k] = np.float32((t - 1.0) / tn)
        t = tn
    return beta


def pred_hprime(Pinv, W, L):
    """H'[j][k] = bf16_rne(float(Pinv[j][k] / (L dg[k]))) over the window, as float32 (Pinv symmetrised as nnmpc_qp_set_inverse does)."""
    hh = 0.5 * (Pinv[:W, :W] + Pinv[:W, :W].T)
    return bf16_round((hh / (L * np.diag(hh))[None, :]).astype(np.float32))


def pred_xunc_f16(xunc):
    """x_unc as the kernel keeps it: f32, clamped to +-60000 by fminf(fmaxf(x, -60000), 60000) -- C's fmaxf returns the other operand
    for a NaN, so a NaN becomes -60000 --, then f16.  Returned as float32."""
    x = np.asarray(xunc, np.float64).astype(np.float32)
    x = np.fmin(np.fmax(x, np.float32(-60000.0)), np.float32(60000.0))
    return x.astype(np.float16).astype(np.float32)


def pred_reference(Pinv, xunc, lb, ub, nu, W, MR, L, counts=PRED_COUNTS, fac10=PRED_FAC10, variant="f64"):
    """The iteration of asm_predict_k on B problems with its storage roundings; xunc (B, >= W) = Kunc x0 in fp64, lb / ub (B, nu).

    Per iteration  w = y + (x_unc - H' y),  nu+ = w - clip(w, lb, ub),  y+ = nu+ + beta[kb] (nu+ - nu),  y and nu rounded to bf16
    where the kernel stores them.  By group of MR consecutive rows (the last group filled with clones of the last problem, which
    count like problems): kb goes back to 0 at iteration it when sum (y - nu+)(nu+ - nu) of iteration it - 1 was positive; the
    adaptive count is min(64, max(8, fac10 nviol / (10 MR))) with nviol the non-zeros of the bf16 nu after iteration 0.
    A fixed count of k iterations is the first k of the same trajectory (the beta table does not depend on the count).

    variant "f64": H' y and the elementwise part in fp64 (the reference); "f32": H' y accumulated in f32 in ascending k-steps of
    32, elementwise part in f32 (only measures how much arithmetic freedom the comparison must tolerate).

    Returns {count: dict(state (B, W) uint8, margin (B, W))} -- margin = min(|w - lb|, |w - ub|) / max(1, max_j |w_pj|) of the
    last iteration -- plus "nit" (groups,), "nviol" (groups,), "rsum_rel" (groups, 64): restart sum of every iteration over the sum
    of its terms' absolute values (1 where every term is zero; NaN beyond the 64 iterations run)."""
    B = xunc.shape[0]
    ft = np.float64 if variant == "f64" else np.float32
    Hp = pred_hprime(Pinv, W, L)
    HpT = np.ascontiguousarray(Hp.T.astype(ft))
    cols = np.arange(W) % nu
    xu_all = pred_xunc_f16(xunc[:, :W]).astype(ft)
    lb_all = np.asarray(lb, np.float64).astype(np.float32)[:, cols].astype(ft)
    ub_all = np.asarray(ub, np.float64).astype(np.float32)[:, cols].astype(ft)
    beta = pred_beta(64).astype(ft)
    ng = -(-B // MR)
    fixed = sorted(k for k in counts if k > 0)
    out = {k: dict(state=np.zeros((B, W), np.uint8), margin=np.zeros((B, W))) for k in counts}
    nits, nviols, rrel = np.zeros(ng, int), np.zeros(ng, int), np.full((ng, 64), np.nan)
    for g in range(ng):
        rows = np.minimum(np.arange(g * MR, (g + 1) * MR), B - 1)           # min(p0 + r, nseg - 1)
        real = np.arange(g * MR, min((g + 1) * MR, B)) - g * MR
        xu, lbg, ubg = xu_all[rows], lb_all[rows], ub_all[rows]
        y = np.zeros((MR, W), ft)
        nuv = np.zeros((MR, W), ft)
        kb, rprev, nit = 0, 0.0, 64
        for it in range(64):
            if it > 0:
                if variant == "f64":
                    acc = y @ HpT
                else:
                    acc = np.zeros((MR, W), np.float32)
                    for ks in range(0, W, 32):
                        acc += y[:, ks:ks + 32] @ HpT[ks:ks + 32]
                kb = 0 if rprev > 0.0 else kb + 1
            else:
                acc = np.zeros((MR, W), ft)
            w = y + (xu - acc)
            nun = w - np.minimum(np.maximum(w, lbg), ubg)
            dn = nun - nuv
            yn = beta[kb] * dn + nun
            terms = ((y - nun) * dn).astype(np.float64)
            rprev = float(terms.sum())
            den = float(np.abs(terms).sum())
            rrel[g, it] = rprev / den if den > 0 else 1.0
            y = bf16_round(yn).astype(ft)
            nuv = bf16_round(nun).astype(ft)
            if it == 0:
                nviols[g] = int((nuv != 0).sum())
                nit = min(64, max(8, (fac10 * nviols[g]) // (10 * MR)))
                nits[g] = nit
            for k in ([it + 1] if it + 1 in fixed else []) + ([0] if 0 in counts and it + 1 == nit else []):
                st = np.where(nuv > 0, 1, np.where(nuv < 0, 2, 0)).astype(np.uint8)
                wd = w.astype(np.float64)
                mg = np.minimum(np.abs(wd - lbg), np.abs(wd - ubg)) / np.maximum(1.0, np.abs(wd).max(axis=1, keepdims=True))
                out[k]["state"][g * MR + real] = st[real]
                out[k]["margin"][g * MR + real] = mg[real]
    out["nit"], out["nviol"], out["rsum_rel"] = nits, nviols, rrel
    return out


# The entrywise comparison: an entry is DECIDED when the reference's margin exceeds PRED_TAU; on every decided entry the kernel's
# state equals the reference's.  PRED_TAU_MEASURED is the smallest power of two at which the reference's two arithmetic variants
# name the same state on every decided entry of every case, batch and count (tests/test_cpu_predict_inputs.py measures it again and
# asserts it has not grown); the factor 4 is for the MFMA's internal summation order, a third variant nobody has observed.
PRED_TAU_MEASURED = 2.0 ** -12
PRED_TAU_FACTOR = 4.0
PRED_TAU = PRED_TAU_FACTOR * PRED_TAU_MEASURED
PRED_MAX_UNDECIDED = 0.02           # caps on the inputs, asserted on the reference alone
PRED_MIN_NONFREE = 0.03
PRED_MIN_RSUM_REL = 1e-3


# (case, wide, count) -> the caps of the entrywise comparison the pair misses on the reference alone (pred_failed_conditions), whatever
# the seed: on this small plant the bounds that matter sit in the first few stages, so that fewer than 3 % of a window are non-free
# in the first iterations ("nonfree"), and the iterates of rows far from the origin come to rest within PRED_TAU max|w| of many bounds
# ("und").  Those pairs are compared entry by entry all the same AND by the quality of their sets.  At 64 iterations the two
# arithmetic variants of the reference differ on decided entries ("variants") or a restart sum is too close to zero ("rsum"): those are
# compared by quality alone.  tests/test_cpu_predict_inputs.py asserts the list entry for entry.
PRED_FALLBACK = {
    ('a', 0, 64): ('variants', 'rsum', 'und'),
    ('b', 0, 1): ('nonfree',),
    ('b', 0, 2): ('nonfree',),
    ('b', 0, 64): ('variants', 'rsum'),
    ('c', 0, 1): ('nonfree',),
    ('c', 0, 2): ('nonfree',),
    ('c', 0, 3): ('nonfree',),
    ('c', 0, 64): ('variants', 'und'),
    ('d', 0, 64): ('variants', 'und'),
    ('e', 0, 1): ('nonfree',),
    ('e', 0, 2): ('nonfree',),
    ('e', 0, 3): ('nonfree',),
    ('e', 0, 8): ('nonfree',),
    ('e', 0, 0): ('nonfree',),
    ('f', 0, 1): ('nonfree',),
    ('f', 0, 2): ('nonfree',),
    ('f', 0, 3): ('nonfree',),
    ('f', 0, 24): ('und',),
    ('f', 0, 64): ('und',),
    ('f', 0, 0): ('und',),
    ('g', 0, 1): ('nonfree',),
    ('g', 0, 2): ('nonfree',),
    ('g', 0, 3): ('nonfree',),
    ('g', 0, 8): ('und', 'nonfree'),
    ('g', 0, 24): ('und',),
    ('g', 0, 64): ('und',),
    ('g', 0, 0): ('und', 'nonfree'),
    ('h', 0, 24): ('und',),
    ('h', 0, 64): ('variants', 'und'),
    ('h', 0, 0): ('und',),
    ('i', 0, 1): ('nonfree',),
    ('i', 0, 64): ('variants', 'rsum', 'und'),
    ('i', 1, 1): ('nonfree',),
    ('i', 1, 2): ('nonfree',),
    ('i', 1, 3): ('nonfree',),
    ('i', 1, 8): ('nonfree',),
    ('i', 1, 24): ('und', 'nonfree'),
    ('i', 1, 64): ('variants', 'und'),
    ('i', 1, 0): ('und', 'nonfree'),
}


def pred_hamming(state, ref_state):
    """Per row: entries in which two sets of bound states differ."""
    return (np.asarray(state) != np.asarray(ref_state)).sum(axis=1)


def pred_windows():
    """[(case name, wide)] of every instance the tests launch."""
    return [(name, w) for name in sorted(PRED_CASES) for w in ((0, 1) if name == "i" else (0,))]


def pred_lambda(Pinv, W):
    """lambda_max(D^-1/2 Pinv_WW D^-1/2) by eigvalsh."""
    hh = 0.5 * (Pinv[:W, :W] + Pinv[:W, :W].T)
    isd = 1.0 / np.sqrt(np.diag(hh))
    return float(np.linalg.eigvalsh(hh * isd[:, None] * isd[None, :]).max())


def pred_power_iteration(Pinv, W):
    """build_predictor's loop, step for step: L = 1.05 lam."""
    hh = 0.5 * (Pinv[:W, :W] + Pinv[:W, :W].T)
    isd = 1.0 / np.sqrt(np.diag(hh))
    v, lam = np.ones(W), 0.0
    for itp in range(5000):
        v = v * isd / np.sqrt((v * v).sum())
        u = (hh @ v) * isd
        num = float((u * v / isd).sum())
        conv = abs(num - lam) <= 1e-9 * abs(num)
        lam, v = num, u
        if conv and itp > 8:
            break
    return 1.05 * lam


def pred_references(c, wide, L, variant="f64", batches=None):
    """{batch: pred_reference of it} of one case and window."""
    W, MR = pred_instance(c["nu"], wide)
    out = {}
    for tag, (x0, lb, ub) in pred_batches(c, MR).items():
        if batches is None or tag in batches:
            out[tag] = pred_reference(c["Pinv"], x0 @ c["Kunc"].T, lb, ub, c["nu"], W, MR, L, variant=variant)
    return out


def pred_deciding_rsum(ref, k):
    """Smallest |restart sum| / sum |terms| among the sums that decide a kb when k iterations run (0: each group's adaptive count):
    the sums of the iterations 0 .. k - 2."""
    return min(float(np.abs(ref["rsum_rel"][g, :max((k if k else ref["nit"][g]) - 1, 0)]).min(initial=1.0)) for g in range(len(ref["nit"])))


def pred_pair_conditions(r64, r32, k, tau=None, tau_measured=None):
    """The conditions of one (case, window, count) over all batches of the case, on the reference alone.  r64 / r32: pred_references
    of the two variants.  Returns dict(und, nonfree, up, lo, empty, rsum, need, vdiff): undecided share; non-free share, upper / lower
    counts of the decided entries; rows with an empty set; smallest deciding restart sum of either variant; largest margin of an
    entry on which the variants differ; entries decided under tau_measured on which they differ."""
    tau = PRED_TAU if tau is None else tau
    tau_measured = PRED_TAU_MEASURED if tau_measured is None else tau_measured
    cat = lambda r, key: np.concatenate([r[t][k][key] for t in r64])
    s, m, s2 = cat(r64, "state"), cat(r64, "margin"), cat(r32, "state")
    dec, diff = m > tau, s != s2
    return dict(und=float(1.0 - dec.mean()), nonfree=float((s[dec] != 0).mean()), up=int((s[dec] == 1).sum()), lo=int((s[dec] == 2).sum()),
                empty=int(((s != 0).sum(axis=1) == 0).sum()),
                rsum=min(min(pred_deciding_rsum(r[t], k) for t in r64) for r in (r64, r32)),
                need=float(m[diff].max()) if diff.any() else 0.0, vdiff=int((diff & (m > tau_measured)).sum()))


def pred_failed_conditions(cond):
    """Names of the conditions a pair misses: "variants" and "rsum" make the entrywise comparison itself unsound (the pair is compared
    by quality alone); "und", "nonfree", "signs", "empty" only thin it out (the pair is compared entry by entry AND by quality)."""
    f = []
    if cond["vdiff"]:
        f.append("variants")
    if cond["rsum"] < PRED_MIN_RSUM_REL:
        f.append("rsum")
    if cond["und"] > PRED_MAX_UNDECIDED:
        f.append("und")
    if cond["nonfree"] < PRED_MIN_NONFREE:
        f.append("nonfree")
    if not (cond["up"] and cond["lo"]):
        f.append("signs")
    if not cond["empty"]:
        f.append("empty")
    return f


PRED_QUALITY_BATCH = "mix"          # the fallback rule's eight rows: the first eight of this batch's second group (sx = 2: what the figures of
                                    # csrc/qp_predict.h were measured at; from sx = 6 the iteration takes 64 steps to come as close)
PRED_QUALITY_ROWS = 8
PRED_GOLDEN = "predict_oracle_sets.npz"


def pred_oracle_states(c, wide):
    """(8, W) uint8 bound states of the optimum inside the window for the fallback rule's rows, by oracle.qp.solve_exact_box."""
    W, MR = pred_instance(c["nu"], wide)
    x0, lb, ub = pred_batches(c, MR)[PRED_QUALITY_BATCH]
    n = c["n"]
    act = np.zeros((PRED_QUALITY_ROWS, 2 * n), bool)
    for r, (_, a) in enumerate(oracle_box_rows(c["Ps"], c["tq"], c["nu"], c["N"], x0, lb, ub, range(MR, MR + PRED_QUALITY_ROWS))):
        act[r, a] = True
    return active_to_state(act, c["nu"])[:, :W]


def pred_golden_states(name, wide):
    """The same states from tests/golden (tests/test_cpu_predict_inputs.py holds the file to the oracle)."""
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", PRED_GOLDEN)) as f:
        return f[f"{name}{wide}"]


def pred_quality(state, opt, MR):
    """Mean Hamming distance of predicted sets from the optimum's sets inside the window over the fallback rule's rows."""
    return float(pred_hamming(state[MR:MR + PRED_QUALITY_ROWS, :opt.shape[1]], opt).mean())


def pred_quality_allowance(q64, q32):
    """What the kernel's figure may exceed the worse variant's by: twice the variants' own difference, one bound per four problems at least."""
    return max(2.0 * abs(q64 - q32), 0.25)


def pred_nonfinite_batch(c, MR):
    """The MR - 1 batch (one group) with row 2 given a NaN in x0 and row 4 scaled so that |x_unc| passes 60000."""
    x0, lb, ub = (a.copy() for a in pred_batches(c, MR)["mr-1"])
    x0[2, 1] = np.nan
    x0[4] *= 2.0e5 / np.abs(x0[4] @ c["Kunc"].T).max()
    return x0, lb, ub


PRED_NONFINITE_COUNTS = (1, 3, 8)
PRED_NONFINITE_ROWS = (2, 4)


def pred_extent_batches(c):
    """Case i: two batches of 8 rows on either side of asm_extent_k's threshold count 4 > B.  On this plant no ordinary row violates a
    bound in the columns [384, 512) -- x_unc is 0 that far out --; a row whose box [-2, -0.5] does not hold 0 does in every column.
    -> {"narrow": 2 such rows, "wide": 3}."""
    out = {}
    for tag, k in (("narrow", 2), ("wide", 3)):
        _, x0, lb, ub = batch_inputs(c["pl"], 8, 10 * PRED_SEEDS[c["name"]] + 8, 2.0)
        lb[1:1 + k], ub[1:1 + k] = -2.0, -0.5
        out[tag] = (x0, lb, ub)
    return out


def pred_extent_count(c, x0, lb, ub):
    """Rows with a violated bound in the columns [384, 512) of x_unc (fp64)."""
    cols = np.arange(384, 512)
    xu = (x0 @ c["Kunc"].T)[:, cols]
    return int(((xu > ub[:, cols % c["nu"]]) | (xu < lb[:, cols % c["nu"]])).any(axis=1).sum())


# ---- the GEMM kernels of the active-set path alone (csrc/gemm64.h, csrc/gemm_kernels.h) through nnmpc_qp_debug_gemm:
# ---- tests/test_gemm_kernel_gpu.py, tests/test_cpu_gemm_inputs.py ---------------------------------------------------------------
GEMM_SENTINEL = -777.25                          # no integer: an entry a kernel left alone is told from every exact product
GEMM_TILE = {1: 128, 2: 64, 3: 128, 4: 64}       # kind of nnmpc_qp_debug_gemm -> tile edge T
GEMM_CHUNK = {1: 16, 2: 16, 3: 32, 4: 32}        # -> K chunk c
GEMM_NAMES = {1: "gemm_nt_f64_t128_k", 2: "gemm_nt_f64_k", 3: "gemm_nt_f32_kdyn_k<128>", 4: "gemm_nt_f32_kdyn_k<64>"}
GEMM_WANT = 3                                    # the tag of the rowphase cases (not 0: rows tagged 0 sit in the tiles that must stay)


def gemm_dtype(kind):
    return np.float32 if kind in (3, 4) else np.float64


def gemm_unit(dtype):
    return 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53


def gemm_gamma(K, dtype):
    u = gemm_unit(dtype)
    return K * u / (1.0 - K * u)


def gemm_highprec():
    """The accumulation type of the rounded-data reference: np.longdouble where it has a 64-bit significand, else exact rationals."""
    if np.finfo(np.longdouble).eps <= 2.0 ** -63:
        return np.longdouble
    return object


def _gemm_cast(a, acc):
    if acc is np.int64:
        return np.nan_to_num(np.asarray(a, np.float64), nan=0.0).astype(np.int64)
    if acc is object:
        from fractions import Fraction
        return np.vectorize(lambda v: Fraction(float(v)), otypes=[object])(np.nan_to_num(np.asarray(a, np.float64), nan=0.0))
    return np.nan_to_num(np.asarray(a, np.float64), nan=0.0).astype(acc)


def gemm_reference(A, B, M, N, K, T, c, c_rows=None, rowphase=None, want=0, kdyn=None, kper=0, mdyn=None, rowmap=None, acc=np.int64):
    """What nnmpc_qp_debug_gemm's contract (include/nnmpc.h) says of C = A B' for tile edge T and chunk c, from the arguments alone:
    A (rows x >= K), B (>= N x >= K); row tiles of T rows; a tile is LEFT ALONE when its first row is >= mdyn or (rowphase given) none
    of its rows has tag `want`, else all its T rows are written; with kdyn the tile's bound is kdyn[0] (kper = 0) or the largest of its
    kper entries and the product runs over k < min(K, (bound // c + 1) c); with rowmap row i of A and of C is row rowmap[i] of the
    arrays, an entry < 0 or a row >= mdyn stores nothing.
    -> dict(val, absval: (c_rows, N) arrays of type acc -- the product and sum |a| |b| where written --, written: bool (c_rows, N),
    tiles / left: the row tiles written / left alone, kk: tile -> columns of K summed, poison: rows of C whose summed part of A holds a NaN)."""
    A, B = np.asarray(A), np.asarray(B)
    ntm = -(-M // T)
    if c_rows is None:
        c_rows = ntm * T
    mlim = 2 ** 31 - 1 if mdyn is None else int(np.asarray(mdyn).reshape(-1)[0])
    zero = acc(0) if acc is not object else 0
    val = np.full((c_rows, N), zero, dtype=acc)
    absval = np.full((c_rows, N), zero, dtype=acc)
    written = np.zeros((c_rows, N), bool)
    Bk = _gemm_cast(B[:N, :K], acc)
    tiles, left, kks, poison = [], [], {}, []
    for tm in range(ntm):
        r0 = tm * T
        if r0 >= mlim or (rowphase is not None and not (np.asarray(rowphase)[r0:r0 + T] == want).any()):
            left.append(tm)
            continue
        kk = K
        if kdyn is not None:
            kl = int(kdyn[0]) if kper == 0 else int(max(kdyn[kper * tm:kper * tm + kper]))
            kk = min(K, (kl // c + 1) * c)
        tiles.append(tm)
        kks[tm] = kk
        if rowmap is None:
            rows = np.arange(r0, r0 + T)
        else:
            idx = np.arange(r0, min(r0 + T, M))
            idx = idx[idx < mlim]
            rows = np.asarray(rowmap)[idx]
            rows = rows[rows >= 0]
        if rows.size == 0:
            continue
        At = A[rows, :kk]
        poison.extend(rows[np.isnan(np.asarray(At, np.float64)).any(axis=1)].tolist())
        Ai = _gemm_cast(At, acc)
        val[rows] = Ai @ Bk[:, :kk].T
        absval[rows] = np.abs(Ai) @ np.abs(Bk[:, :kk]).T
        written[rows] = True
    return dict(val=val, absval=absval, written=written, tiles=tiles, left=left, kk=kks, poison=sorted(poison))


def gemm_expected(ref, C0):
    """C after the call, for exact data: C0 (the view the kernel was given) with the written entries replaced."""
    out = np.array(C0, copy=True)
    out[ref["written"]] = ref["val"][ref["written"]].astype(C0.dtype)
    if ref["poison"]:
        out[ref["poison"]] = np.nan
    return out


def _gemm_case(cid, group, kind, M, N, K, **kw):
    T, c = GEMM_TILE[kind], GEMM_CHUNK[kind]
    d = dict(id=cid, group=group, kind=kind, M=M, N=N, K=K, T=T, c=c, data_id=kw.pop("data_id", cid), rounded=False, pa=0, pb=0, c0=0, cpad=8,
             spare=2, a_rows=None, rowphase=None, kdyn=None, kblocks=False, mdyn=None, rowmap=None, variant=None, nan=None, twin=None)
    d.update(kw)
    return d


def gemm_kdyn_orders(c, K):
    """Bounds per 64-row block, all from {-1, 0, c - 2, c - 1, c, 2 c - 1, K - 1, K + 5}.  o1: every value once; neighbouring blocks and
    neighbouring pairs of blocks run a different number of chunks; the larger entry of a pair stands first in three pairs and second
    in one.  o2: the values a pair of o1 hides behind a larger one as the LARGER entry (else a 128-row tile never runs them)."""
    return dict(o1=[-1, 0, K - 1, c - 2, c, c - 1, K + 5, 2 * c - 1], o2=[-1, -1, c - 2, -1, 0, 2 * c - 1, -1, c - 1])


def gemm_rowphase_tags(T):
    """Six row tiles: none / first row / last row / a middle row / every row / none tagged GEMM_WANT; the others 0, 1, 2 or 4."""
    rng = np.random.default_rng(4242 + T)
    tags = rng.choice([0, 1, 2, 4], size=6 * T).astype(np.int32)
    tags[0] = 0
    tags[5 * T:] = 0
    tags[T] = tags[3 * T - 1] = tags[3 * T + T // 2 - 3] = GEMM_WANT
    tags[4 * T:5 * T] = GEMM_WANT
    return tags


_GEMM_CASES = None


def gemm_cases():
    """The case table of tests/test_gemm_kernel_gpu.py (the dispatch cases of kind 0 apart: gemm_dispatch_inputs)."""
    global _GEMM_CASES
    if _GEMM_CASES is not None:
        return _GEMM_CASES
    cs = []

    def both(cid, group, M, N, K, **kw):                 # an fp64 case on the 128-grid: the 128 x 128 kernel and, same arguments, the 64 x 64 one
        cs.append(_gemm_case(cid + "-t128", group, 1, M, N, K, data_id=cid, twin=cid + "-k64", **kw))
        cs.append(_gemm_case(cid + "-k64", group, 2, M, N, K, data_id=cid, **kw))

    for ntm in (1, 7, 8, 9, 32, 33):                     # tile deal of the 128 x 128 kernel
        for ntn in (1, 3):
            both(f"deal-{ntm}x{ntn}", "deal", 128 * ntm, 128 * ntn, 48)
    for K in (16, 32, 48, 80):                           # the two-stage ring; padded rows, B and C inside wider arrays
        both(f"ring-K{K}", "ring", 256, 256, K, pa=6, pb=10, c0=128, cpad=64, rounded=True)
    for M in (64, 192, 320):                             # the same for the 64 x 64 kernel
        for N in (64, 192, 320):
            for K in (16, 32, 48):
                cs.append(_gemm_case(f"k64-{M}x{N}x{K}", "k64", 2, M, N, K, pa=6, pb=10, c0=64, cpad=64, rounded=True))
    for kind in (1, 2, 3, 4):                            # kdyn
        T, c = GEMM_TILE[kind], GEMM_CHUNK[kind]
        K = 4 * c
        tag = {1: "t128", 2: "k64", 3: "f32x128", 4: "f32x64"}[kind]
        for oname, order in gemm_kdyn_orders(c, K).items():
            for v in "ab":
                cs.append(_gemm_case(f"kdyn-{tag}-{oname}{v}", "kdyn", kind, 512, 128, K, pa=8, pb=12, kdyn=order, kblocks=True, variant=v))
        if kind in (1, 2):                               # (the f32 kernels are only ever launched with one bound per 64 rows)
            for kl in sorted(set(gemm_kdyn_orders(c, K)["o1"])):
                for v in "ab":
                    cs.append(_gemm_case(f"kdyn-{tag}-one{kl}{v}", "kdyn", kind, 2 * T, 128, K, pa=8, pb=12, kdyn=[kl], variant=v))
        o1 = gemm_kdyn_orders(c, K)["o1"]                # block 4: bound c, k < 2 c -- a NaN in column 2 c is outside, in column 2 c - 1 inside
        cs.append(_gemm_case(f"kdyn-{tag}-nan-out", "kdyn", kind, 512, 128, K, pa=8, pb=12, kdyn=o1, kblocks=True, variant="b", nan=(4 * 64 + 5, 2 * c)))
        cs.append(_gemm_case(f"kdyn-{tag}-nan-in", "kdyn", kind, 512, 128, K, pa=8, pb=12, kdyn=o1, kblocks=True, variant="b", nan=(4 * 64 + 5, 2 * c - 1)))
    for kind in (3, 4):                                  # tile map of the f32 kernels; <128>: the last tile has its first 64 rows in use
        T = GEMM_TILE[kind]
        for ntm in (1, 7, 8, 9, 17):
            for ntn in (1, 2, 3):
                M = T * ntm - (64 if kind == 3 else 0)
                nblk = ntm * (T // 64)
                kd = [[95, 31, 63][b % 3] if b * 64 < M else -1 for b in range(nblk)]
                cs.append(_gemm_case(f"f32map-{T}-{ntm}x{ntn}", "f32map", kind, M, T * ntn, 96, pa=4, pb=8, c0=32, cpad=16, kdyn=kd, kblocks=True,
                                     variant="b", rounded=ntm <= 7))
    for T, kinds in ((128, (1, 2)), (64, (2,))):         # rowphase
        for kind in kinds:
            tag = {1: "t128", 2: "k64"}[kind]
            cs.append(_gemm_case(f"rowphase-{tag}-T{T}", "rowphase", kind, 6 * T, 128, 32, data_id=f"rowphase-T{T}", rowphase=gemm_rowphase_tags(T),
                                 twin=f"rowphase-k64-T{T}" if kind == 1 else None))
    for kind in (1, 2):                                  # mdyn
        T = GEMM_TILE[kind]
        tag = {1: "t128", 2: "k64"}[kind]
        for md in (0, 1, T - 1, T, T + 1, 3 * T):
            cs.append(_gemm_case(f"mdyn-{tag}-{md}", "mdyn", kind, 3 * T, 128, 32, data_id=f"mdyn-{tag}", mdyn=md))
    rng = np.random.default_rng(777)                     # rowmap: a partial permutation of 500 rows, twelve entries "no row"
    rm = rng.permutation(500)[:384].astype(np.int32)
    rm[[0, 127, 128, 200, 383] + rng.choice(np.arange(1, 383), 7, replace=False).tolist()] = -1
    cs.append(_gemm_case("rowmap-plain", "rowmap", 1, 384, 256, 48, pa=6, pb=10, a_rows=500, rowmap=rm))
    cs.append(_gemm_case("rowmap-mdyn185", "rowmap", 1, 384, 256, 48, pa=6, pb=10, a_rows=500, rowmap=rm, mdyn=185))
    for c in list(cs):                                   # every other case of the 128 x 128 kernel without a rowmap: the same arguments
        if c["kind"] == 1 and c["rowmap"] is None and c["twin"] is None:      # through the 64 x 64 kernel (tiles of 64, one bound per tile)
            c["twin"] = c["id"] + "~k64"
            cs.append(dict(c, id=c["twin"], kind=2, T=64, c=16, twin=None))
    _GEMM_CASES = cs
    return cs


def gemm_case(cid):
    return next(c for c in gemm_cases() if c["id"] == cid)


def gemm_data(shape, rng, dtype, rounded, nonzero=False):
    """Exact data: integers in -3 .. 3 (nonzero: without 0).  Rounded data: standard normals scaled per row and per column by
    10^U(-3, 3) each (+-6 decades together)."""
    if not rounded:
        a = rng.integers(-3, 4, size=shape)
        if nonzero:
            a = np.where(a == 0, rng.choice([-3, -2, -1, 1, 2, 3], size=shape), a)
        return a.astype(dtype)
    a = rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, (shape[0], 1)) * 10.0 ** rng.uniform(-3, 3, (1, shape[1]))
    return a.astype(dtype)


def gemm_inputs(case, rounded=False):
    """The arrays of one call: full allocations (Af, Bf, Cf: Cf filled with the sentinel), the views the call gets (A, B, C), the
    keyword arguments of BatchedBoxQP.debug_gemm and of gemm_reference."""
    import zlib
    c = case
    rng = np.random.default_rng(zlib.crc32((c["data_id"] + ("/r" if rounded else "/e")).encode()))
    dt = gemm_dtype(c["kind"])
    M, N, K, T = c["M"], c["N"], c["K"], c["T"]
    mr = -(-M // T) * T
    a_rows = c["a_rows"] or mr
    c_rows = (c["a_rows"] or mr) + c["spare"]
    Af = gemm_data((a_rows, K + c["pa"]), rng, dt, rounded, nonzero=c["variant"] == "b")
    Bf = gemm_data((c["c0"] + N + 3, K + c["pb"]), rng, dt, rounded)
    kd = None if c["kdyn"] is None else np.asarray(c["kdyn"], np.int32)
    if c["variant"] == "a":                              # zeros beyond each 64-row block's own bound (one bound: beyond it)
        for b in range(mr // 64):
            Af[64 * b:64 * b + 64, max(int(kd[b] if c["kblocks"] else kd[0]) + 1, 0):] = 0
    if M < mr:
        Af[M:] = 0                                       # rows not in use (the f32 round's last tile): zero, as LAM32 keeps them
    if c["nan"]:
        Af[c["nan"]] = np.nan
    Cf = np.full((c_rows, c["c0"] + N + c["cpad"]), GEMM_SENTINEL, dt)
    kper = (T // 64) if (kd is not None and c["kblocks"]) else 0
    call = dict(rowphase=c["rowphase"], want=GEMM_WANT if c["rowphase"] is not None else 0, kdyn=kd, kblocks=c["kblocks"], mdyn=c["mdyn"],
                rowmap=c["rowmap"])
    ref = dict(c_rows=c_rows, rowphase=c["rowphase"], want=call["want"], kdyn=kd, kper=kper, mdyn=c["mdyn"], rowmap=c["rowmap"])
    return dict(Af=Af, Bf=Bf, Cf=Cf, A=Af[:, :K], B=Bf[c["c0"]:c["c0"] + N, :K], C=Cf[:, c["c0"]:c["c0"] + N], call=call, ref=ref)


def gemm_case_reference(case, inp, rounded=False):
    return gemm_reference(inp["A"], inp["B"], case["M"], case["N"], case["K"], case["T"], case["c"],
                          acc=gemm_highprec() if rounded else np.int64, **inp["ref"])


def gemm_bar(case, ref):
    """2 gamma_K |A| |B|' entrywise (any order of summation, one rounding per product and per add; the factor 2: cl_step_reference's)."""
    return 2.0 * gemm_gamma(case["K"], gemm_dtype(case["kind"])) * ref["absval"].astype(np.float64)


GEMM_DISPATCH = dict(t128=(3200, 1024, 16), k64=(3072, 1024, 16), offM=(3264, 1024, 16), offN=(3200, 1088, 16), offK=(3200, 1024, 24))


def gemm_dispatch_inputs():
    """One A (3264 rows), B (1088 rows), 24 columns each, exact data: every shape of GEMM_DISPATCH is a corner of them."""
    rng = np.random.default_rng(20250)
    return gemm_data((3264, 24), rng, np.float64, False), gemm_data((1088, 24), rng, np.float64, False)


# ---- certificates under inexact inverses and far-field factors: tests/test_certificate_gpu.py, tests/test_cpu_certificate_inputs.py

CERT_STAT_TOL = 1e-8       # csrc/qp_solver.hip, asm_args (the AsmDev setup of a segment): a.stat_tol = 1e-8; nnmpc_qp_create: d.stat_tol = 1e-8
CERT_BOUND_TOL = 1e-9      # csrc/qp_solver.hip, nnmpc_qp_create: opts.bound_tol <= 0 -> 1e-9 (BatchedBoxQP passes 0)
CERT_ROUND = 1e-14         # the rounding term of the bound (asm_update_k, asm_wide_k, asm_tail_k, asm_small_k)
CERT_GATE_E2 = 1e-6        # nnmpc_qp_set_inverse refuses |P Pinv - I|_max >= 1e-6
CERT_GATE_FAR = 1e-9       # nnmpc_qp_set_farfield refuses max |U V' - M| >= 1e-9
CERT_GATE_BAND = 1e-3      # numpy's figure and the device's differ by the rounding of an n-term product, n eps |P|_inf max |Pinv| ~ 2e-10 on
                           # entries the gate compares with 1e-6: inputs are held this far, relatively, from either gate
CERT_ST_REJECTED = 1       # NNMPC_ST_MAXITER: what a method-"asm" handle reports for a row its pass marked 3, "not solved here" (pdip_fallback)
CERT_PDIP_TOL = 1e-8       # |u - u*| <= 1e-8 max(1, |u*|inf): "certified exact" of tests/test_pdip_paths_gpu.py
CERT_MARGIN_FLOOR = 10.0 * CERT_STAT_TOL   # a kept row's margins are ten stationarity bars at least: a multiplier below the bar cannot be told from zero at that bar
CERT_MARGIN_SIGMA = 6.0    # ... and twice as far as entrywise relative errors of 6 sigma of the plant's REFUSED rung can move it, to first
                           # order (cert_shift): no accepted handle of the ladders is further from the exact inverse than that
CERT_MIN_CLASS = 8
CERT_MAX_LOST = 0.20

CERT_PLANTS = dict(mini_cdu=dict(seed=5, B=96, sample_seed=6, sx=2.5),
                   cstrs=dict(seed=0, B=128, sample_seed=1, sx=2.0),
                   mid_cdu=dict(seed=3, B=320, sample_seed=11, sx=2.0))
# relative-noise ladder: accepted rungs, then the rung just above the e2 < 1e-6 gate (tests/test_cpu_certificate_inputs.py holds every
# accepted rung below 0.9e-6 and the refused one above 1.1e-6 with e2 computed in numpy: the device's figure differs by rounding only)
CERT_LADDER = dict(mini_cdu=((0.0, 1e-13, 1e-12, 1e-11, 1e-10, 2e-10, 3e-8), 5e-8),
                   cstrs=((0.0, 1e-13), 5e-12),
                   mid_cdu=((0.0, 1e-13, 1e-12, 5e-11, 1e-10, 2e-10, 8e-9), 2e-8))
CERT_SITES = dict(small=dict(plant="mini_cdu", env={}, opts={}),
                  small_ill=dict(plant="cstrs", env={}, opts=dict(nb=64)),
                  update=dict(plant="mini_cdu", env={"NNMPC_NO_SMALL": "1"}, opts=dict(asm_tail_batch=-1)),
                  tail=dict(plant="mini_cdu", env={"NNMPC_NO_SMALL": "1"}, opts={}),
                  wide=dict(plant="mid_cdu", env={}, opts={}))
CERT_FAR_W = 256           # the column window of the mid_cdu batch's rounds: past its last active bound (index 191) plus one stage, on the 128 grid
CERT_FAR_SETTINGS = dict(exact=0.0, small=1e-11, aligned=8e-10, refused=2e-9)    # max |U V' - M| asked for
_CERT_CASES = {}


def cert_ld_eps():
    return float(np.finfo(np.longdouble).eps)


def cert_oracle_row(H, xunc, lbn, ubn):
    """Optimal bound states of one problem by a primal-dual active-set iteration on the exact inverse (all infeasible indices change
    sides while their number keeps falling, then the smallest one only): x = x_unc - H[:, A] lam, lam = H_AA^-1 (x_unc_A - b_A).
    What comes back is a candidate; cert_case certifies every row with P itself in np.longdouble (cert_property_a)."""
    n = xunc.size
    state = np.where(xunc > ubn, 1, np.where(xunc < lbn, 2, 0)).astype(np.uint8)
    best, grace = n + 1, 3
    for _ in range(2000):
        x, A, lam = cert_solve_on_set_inv(H, xunc, lbn, ubn, state)
        new = np.full(n, 255, np.uint8)
        fr = state == 0
        new[fr & (x > ubn)] = 1
        new[fr & (x < lbn)] = 2
        new[A[np.where(state[A] == 1, lam <= 0.0, lam >= 0.0)]] = 0
        inf = np.flatnonzero(new != 255)
        if inf.size == 0:
            return state, x, lam
        if inf.size < best:
            best, grace = inf.size, 3
        elif grace > 0:
            grace -= 1
        else:
            inf = inf[:1]
        state[inf] = new[inf]
    raise RuntimeError("cert_oracle_row: no settled set")


def cert_solve_on_set_inv(H, xunc, lbn, ubn, state):
    """(x, A, lam) on the set `state` through an inverse H, as the solver forms them: lam = H_AA^-1 (x_unc_A - b_A) (positive on
    upper bounds, negative on lower ones at an optimum), x = x_unc - H[:, A] lam with x_A = b_A exactly."""
    A = np.flatnonzero(state)
    if A.size == 0:
        return xunc.copy(), A, np.zeros(0)
    b = np.where(state[A] == 1, ubn[A], lbn[A])
    lam = np.linalg.solve(H[np.ix_(A, A)], xunc[A] - b)
    x = xunc - H[:, A] @ lam
    x[A] = b
    return x, A, lam


def cert_shift(H, K, x0, state, lam, eps):
    """First-order bound on how far entrywise relative errors of at most e = eps in H and K move the solution on a fixed set:
    with S = H_AA,  |d lam| <= |S^-1| e (|K_A| |x0| + |S| |lam|)  and  |d x_F| <= e (|K| |x0| + |H_:A| |lam|) + |H_:A| |d lam|.
    -> (max |d lam|, max |d x| over the free variables)."""
    e = eps
    A = np.flatnonzero(state)
    kx = np.abs(K) @ np.abs(x0)
    if A.size == 0:
        return 0.0, float(e * kx.max())
    S = H[np.ix_(A, A)]
    dl = np.abs(np.linalg.inv(S)) @ (e * (kx[A] + np.abs(S) @ np.abs(lam)))
    HA = np.abs(H[:, A])
    dx = e * (kx + HA @ np.abs(lam)) + HA @ dl
    fr = state == 0
    return float(dl.max()), float(dx[fr].max(initial=0.0))


def cert_case(plant):
    """Everything of one plant that is computed once: P (symmetric), tq, the exact inverse, the batch, the oracle's sets and optima
    (certified with P in np.longdouble), margins and the kept rows."""
    if plant in _CERT_CASES:
        return _CERT_CASES[plant]
    import scipy.linalg as sla
    from industrial_nnmpc_2021_amd.linearMPC_build import build_regulator_matrices
    spec = CERT_PLANTS[plant]
    pl = synthetic.plant(plant, spec["seed"])
    P, tq, nu = build_regulator_matrices(pl)
    Ps = np.tril(P) + np.tril(P, -1).T
    n = Ps.shape[0]
    N = n // nu
    cf = sla.cho_factor(Ps, lower=True)
    H = sla.cho_solve(cf, np.eye(n))
    H = np.ascontiguousarray(0.5 * (H + H.T))
    K = np.ascontiguousarray(-sla.cho_solve(cf, tq))
    _, x0, lb, ub = batch_inputs(pl, spec["B"], spec["sample_seed"], spec["sx"])
    x0, lb, ub = np.ascontiguousarray(x0), np.ascontiguousarray(lb), np.ascontiguousarray(ub)
    B = spec["B"]
    c = dict(plant=plant, pl=pl, P=P, Ps=Ps, tq=tq, nu=nu, N=N, n=n, B=B, H=H, K=K, x0=x0, lb=lb, ub=ub,
             pscale=float(np.sort(np.diag(Ps))[n // 2]), tqmax=float(np.abs(tq).max()), p_inf=float(np.abs(Ps).sum(axis=1).max()),
             LB=np.tile(lb, (1, N)), UB=np.tile(ub, (1, N)), q=x0 @ tq.T)
    c["scale"] = np.maximum(c["pscale"], np.abs(c["q"]).max(axis=1))
    c["bar"] = CERT_STAT_TOL * c["scale"]
    c["x1"] = np.abs(x0).sum(axis=1)
    state = np.zeros((B, n), np.uint8)
    xs = np.empty((B, n))
    lam = np.zeros((B, n))                                         # signed multipliers on the active bounds, 0 elsewhere
    lam_margin, slack_margin = np.empty(B), np.empty(B)
    dlam, dx = np.empty(B), np.empty(B)
    xunc = x0 @ K.T
    for b in range(B):
        state[b], xs[b], lm = cert_oracle_row(H, xunc[b], c["LB"][b], c["UB"][b])
        A = np.flatnonzero(state[b])
        lam[b, A] = lm
        fr = state[b] == 0
        lam_margin[b] = np.abs(lm).min(initial=np.inf) / c["scale"][b]
        slack_margin[b] = (np.minimum(c["UB"][b] - xs[b], xs[b] - c["LB"][b]) / (c["UB"][b] - c["LB"][b]))[fr].min(initial=np.inf)
        dl, dxf = cert_shift(H, K, x0[b], state[b], lm, CERT_MARGIN_SIGMA * CERT_LADDER[plant][1])
        dlam[b], dx[b] = dl / c["scale"][b], dxf / (c["UB"][b] - c["LB"][b]).min()
    c.update(state=state, xs=xs, lam=lam, active=state_to_active(state, nu), lam_margin=lam_margin, slack_margin=slack_margin,
             shift_lam=dlam, shift_x=dx)
    # kept: both margins above the floor and above twice what the largest inverse error of the plant's ladder can move (cert_shift)
    c["kept"] = (lam_margin > np.maximum(CERT_MARGIN_FLOOR, 2.0 * dlam)) & (slack_margin > np.maximum(CERT_MARGIN_FLOOR, 2.0 * dx))
    ref = cert_property_a(c, dict(u=xs, active=c["active"], status=np.zeros(B, np.int32)), precise=True)
    if not ref["ok"].all() or ref["ratio"].max() > 1e-3:
        raise RuntimeError(f"cert_case({plant}): the oracle's optimum is not certified: {ref['why'][:3]}, ratio {ref['ratio'].max():.2e}")
    c["oracle_ratio"] = ref["ratio"]
    _CERT_CASES[plant] = c
    return c


def cert_property_a(c, out, rows=None, precise=False):
    """The solver's own claim about every row with status 0, evaluated with the original P, q = tq x0 and the bounds: active entries
    equal their bounds bit for bit, no variable active on both sides, lb - bound_tol <= u <= ub + bound_tol, g = P u + q < 0 on
    upper-active and > 0 on lower-active entries, |g|inf over the free entries <= 1e-8 max(pscale, |q|inf).  g is evaluated in
    np.longdouble, and the only slack is the rounding of that evaluation, gamma(n + n_aug + 2) (|P| |u| + |tq| |x0|), on the
    stationarity bar.  (A longdouble product of the mid_cdu batch takes seconds: a row whose every comparison an fp64 evaluation
    with ITS rounding bound already decides, either way, keeps that verdict -- the longdouble one cannot differ; `precise` turns the
    short cut off.)  rows: the rows of the case the result holds (default: all, in order).
    -> dict(ok (B,) bool -- True for rows with status != 0, which may hold anything --, ratio (B,) free-set gradient / bar (0 for
    rows not checked), slack (largest longdouble rounding slack / bar), ld_rows (rows evaluated in longdouble), why [(row, reason)])."""
    u, act, status = np.asarray(out["u"]), np.asarray(out["active"]), np.asarray(out["status"])
    B, n = u.shape
    nu, na = c["nu"], c["tq"].shape[1]
    rows = np.arange(c["B"]) if rows is None else np.asarray(rows)
    k, cc = np.arange(n) // nu, np.arange(n) % nu
    ok = np.ones(B, bool)
    ratio = np.zeros(B)
    why = []
    chk = np.flatnonzero(status == 0)
    if chk.size == 0:
        return dict(ok=ok, ratio=ratio, slack=0.0, ld_rows=0, why=why)
    LB, UB = c["LB"][rows][chk], c["UB"][rows][chk]
    a_u, a_l = act[chk][:, k * 2 * nu + cc], act[chk][:, k * 2 * nu + nu + cc]
    fr = ~(a_u | a_l)
    finite = np.isfinite(u[chk]).all(axis=1)
    U = np.where(np.isfinite(u[chk]), u[chk], 0.0)
    x0 = c["x0"][rows][chk]
    Pa, ta = np.abs(c["Ps"]), np.abs(c["tq"])
    q = x0 @ c["tq"].T
    G = U @ c["Ps"] + q
    mag = np.abs(U) @ Pa + np.abs(x0) @ ta.T
    slack = cl_gamma(n + na + 2) * mag * (1.0 + 1e-12)
    bar = CERT_STAT_TOL * np.maximum(c["pscale"], np.abs(q).max(axis=1))
    ld = np.longdouble
    gam_ld = float((n + na + 2) * np.finfo(ld).eps)
    open_ = (fr & (np.abs(np.abs(G) - bar[:, None]) <= slack + 1e-12 * bar[:, None])).any(axis=1) | (~fr & (np.abs(G) <= slack)).any(axis=1)
    need = np.flatnonzero(open_ | precise)
    if need.size:
        if "_ld" not in c:
            c["_ld"] = (c["Ps"].astype(ld), c["tq"].astype(ld))
        Pl, tl = c["_ld"]
        ql = x0[need].astype(ld) @ tl.T
        Gl = U[need].astype(ld) @ Pl + ql
        # these rows' gradients, from longdouble (rounding them to fp64 moves them by 1e-16 |g|, far inside the slack below; a sign
        # is never lost: no gradient here is near the underflow threshold)
        G[need] = Gl.astype(np.float64)
        slack[need] = gam_ld * mag[need] + 2.0 * TS_EPS * np.abs(G[need])
    tol = CERT_BOUND_TOL
    # (u - ub and lb - u are exact or correctly rounded differences of fp64 numbers; 1e-9 is compared as the library compares it)
    tests = (("not finite", ~finite),
             ("active on both sides", (a_u & a_l).any(axis=1)),
             ("active entry off its bound", (a_u & (u[chk] != UB)).any(axis=1) | (a_l & (u[chk] != LB)).any(axis=1)),
             ("beyond a bound", ((U > UB + tol) | (U < LB - tol)).any(axis=1)),
             ("multiplier sign", (a_u & ~(G < 0)).any(axis=1) | (a_l & ~(G > 0)).any(axis=1)),
             ("free-set gradient", (fr & (np.abs(G) > bar[:, None] + slack)).any(axis=1)))
    for name, bad in tests:
        for i in np.flatnonzero(bad):
            why.append((int(chk[i]), name))
        ok[chk[bad]] = False
    ratio[chk] = np.where(fr, np.abs(G), 0).max(axis=1) / bar
    return dict(ok=ok, ratio=ratio, slack=float((gam_ld * mag.max(axis=1) / bar).max()), ld_rows=int(need.size), why=why)


def cert_perturb(c, eps, seed=1):
    """Relative noise: (Hinv (1 + eps N) symmetrised, Kunc (1 + eps N')); eps = 0: the exact pair."""
    rng = np.random.default_rng(seed)
    Nh, Nk = rng.standard_normal(c["H"].shape), rng.standard_normal(c["K"].shape)
    Hp = c["H"] * (1.0 + eps * Nh)
    return np.ascontiguousarray(0.5 * (Hp + Hp.T)), np.ascontiguousarray(c["K"] * (1.0 + eps * Nk))


def cert_perturb_rowcol(c, j, rel=1e-7):
    """Row and column j of Hinv scaled by 1 + rel (the diagonal entry twice), Kunc exact."""
    Hp = c["H"].copy()
    Hp[j, :] *= 1.0 + rel
    Hp[:, j] *= 1.0 + rel
    return np.ascontiguousarray(Hp), c["K"]


def cert_rowcol_index(c):
    """The first-stage variable whose scaled row and column leave the smallest |P Pinv - I|_max (~ rel (1 + P_jj Hinv_jj): most of them
    miss the gate at rel = 1e-7)."""
    if "rowcol" not in c:
        c["rowcol"] = int(np.argmin([cert_errors(c, *cert_perturb_rowcol(c, j))[1] for j in range(c["nu"])]))
    return c["rowcol"]


def cert_perturb_kunc(c, rel=1e-3, seed=2):
    """Kunc alone off by rel N', Hinv exact."""
    rng = np.random.default_rng(seed)
    return c["H"], np.ascontiguousarray(c["K"] * (1.0 + rel * rng.standard_normal(c["K"].shape)))


def cert_errors(c, Hp, Kp):
    """(e1max, e2max) as nnmpc_qp_set_inverse measures them, in numpy."""
    return float(np.abs(c["Ps"] @ Kp + c["tq"]).max()), float(np.abs(c["Ps"] @ Hp - np.eye(c["n"])).max())


def cert_errors_rounding(c, Hp, Kp):
    """How far two fp64 evaluations of (e1max, e2max) can differ: 2 gamma(n) max(|P| |Kunc| + |tq|), 2 gamma(n) max(|P| |Pinv| + I)."""
    g = 2.0 * cl_gamma(c["n"] + 2)
    Pa = np.abs(c["Ps"])
    return float(g * (Pa @ np.abs(Kp) + np.abs(c["tq"])).max()), float(g * ((Pa @ np.abs(Hp)).max() + 1.0))


def cert_emulate(c, Hp, Kp, e1max, e2max, ff_err=0.0, precise=False):
    """What the solver computes from the pair (Hp, Kp) on the oracle's sets, and the certificate it then forms:
    bnd = 2 (e1max |x0|_1 + e2max |lam|_1) + 1e-14 (tqmax |x0|_1 + |lam|_1) + ff_err (|x0|_1 + |lam|_1),
    sure = bnd <= stat_tol pscale and min |lam_a| > bnd.  -> dict of (B,) arrays: bnd, sure, undetermined (bnd within a factor 2 of
    either comparison), gfree (max |P x + q| over the free set; precise: every row in np.longdouble), ratio = gfree / bar, setok (the emulated
    solution keeps the oracle's set: feasible within bound_tol, multiplier signs right), and x (B, n), l1, lmin."""
    B, n = c["B"], c["n"]
    xunc = c["x0"] @ Kp.T
    x = np.empty((B, n))
    l1, lmin, setok = np.zeros(B), np.full(B, 1e300), np.ones(B, bool)
    for b in range(B):
        x[b], A, lm = cert_solve_on_set_inv(Hp, xunc[b], c["LB"][b], c["UB"][b], c["state"][b])
        if A.size:
            l1[b], lmin[b] = np.abs(lm).sum(), np.abs(lm).min()
            setok[b] = not np.where(c["state"][b][A] == 1, lm <= 0.0, lm >= 0.0).any()
        setok[b] &= bool(((x[b] <= c["UB"][b] + CERT_BOUND_TOL) & (x[b] >= c["LB"][b] - CERT_BOUND_TOL)).all())
    ev = cert_property_a(c, dict(u=x, active=c["active"], status=np.zeros(B, np.int32)), precise=precise)
    x1 = c["x1"]
    bnd = 2.0 * (e1max * x1 + e2max * l1) + CERT_ROUND * (c["tqmax"] * x1 + l1) + ff_err * (x1 + l1)
    lim = CERT_STAT_TOL * c["pscale"]
    sure = (bnd <= lim) & (lmin > bnd)
    und = ((bnd > 0.5 * lim) & (bnd < 2.0 * lim)) | ((bnd <= lim) & (lmin > 0.5 * bnd) & (lmin < 2.0 * bnd))
    return dict(x=x, l1=l1, lmin=lmin, bnd=bnd, sure=sure, undetermined=und, ratio=ev["ratio"], gfree=ev["ratio"] * c["bar"], setok=setok)


def cert_classes(c, em):
    """Kept, determined rows by class: 'sure'; 'accepted' (not sure, free-set gradient below a quarter of the bar: the check with P
    passes); 'rejected' (above four times the bar: it fails).  Rows in between, undetermined rows and rows that are not kept are in
    'lost'."""
    det = c["kept"] & ~em["undetermined"] & em["setok"]
    sure = det & em["sure"]
    acc = det & ~em["sure"] & (em["ratio"] < 0.25)
    rej = det & ~em["sure"] & (em["ratio"] > 4.0)
    return dict(sure=sure, accepted=acc, rejected=rej, lost=~(sure | acc | rej))


def cert_full_check_range(c, em):
    """[lo, hi] of asm_full_checks under method 'asm': the kept, determined rows that are not sure, plus at most the rest."""
    det = c["kept"] & ~em["undetermined"] & em["setok"]
    lo = int((det & ~em["sure"]).sum())
    return lo, lo + int((~det).sum())


def cert_u_tol(c, b):
    """1e-8 max(1, |u*|inf) + |P_FF^-1|inf bar: an accepted row's distance from the oracle's optimum (P_FF (u - u*)_F = g_F)."""
    tol = c.setdefault("_utol", {})
    if b not in tol:
        fr, A = c["state"][b] == 0, np.flatnonzero(c["state"][b])
        # the inverse of a principal block from the inverse of the whole: P_FF^-1 = H_FF - H_FA H_AA^-1 H_AF (n^2 |A| flops, not n^3)
        inv = c["H"][np.ix_(fr, fr)]
        if A.size:
            HFA = c["H"][np.ix_(fr, A)]
            inv = inv - HFA @ np.linalg.solve(c["H"][np.ix_(A, A)], HFA.T)
        norm = np.abs(inv).sum(axis=1).max() if fr.any() else 0.0
        tol[b] = 1e-8 * max(1.0, np.abs(c["xs"][b]).max()) + norm * c["bar"][b]
    return tol[b]


def cert_farfield_factors(c, W=CERT_FAR_W, rtol=1e-13):
    """U, Vx, Vl of M = [Kunc[W:] | -Hinv[W:, 0:W]] as BatchedBoxQP.prepare_farfield builds them (truncated SVD, staircase basis)."""
    import scipy.linalg as sla
    from industrial_nnmpc_2021_amd.qp import _staircase
    key = ("far", W)
    if key not in c:
        M = np.hstack((c["K"][W:], -c["H"][W:, :W]))
        U, s, Vt = sla.svd(M, full_matrices=False, lapack_driver="gesdd")
        r = max(1, int((s > rtol * s[0]).sum()))
        Uf, G = _staircase(U[:, :r] * s[:r], rtol * s[0])
        V = G @ Vt[:G.shape[1]]
        c[key] = (Uf, np.ascontiguousarray(V), M)
    return c[key]


CERT_FAR_ALIGNED = 8       # rows the 'aligned' factors are built for, one after the other: which rows of a batch settle in the rounds -- and go
                           # through the full-width pass -- and which are finished by the device tail, from Pinv itself, is the solver's to say


def cert_far_aligned_rows(c, W=CERT_FAR_W, k=CERT_FAR_ALIGNED):
    """[(row, ratio)]: the k kept rows whose z = [x0; lam[0:W]] has the largest |V z|^2 / max |V' V z| -- the rows 'aligned' factors
    move furthest --, each with the free-set gradient / bar of its optimum with the far columns moved by its factors (what a pass
    that delivered the factored product uncertified would hand out)."""
    Uf, V, _ = cert_farfield_factors(c, W)
    cand = []
    for b in np.flatnonzero(c["kept"]):
        if np.flatnonzero(c["state"][b]).max(initial=-1) >= W:
            continue
        Vz = V @ np.concatenate((c["x0"][b], c["lam"][b][:W]))
        cand.append((float(Vz @ Vz / np.abs(Vz @ V).max()), int(b)))
    out = []
    for _, row in sorted(cand, reverse=True)[:k]:
        Up = cert_farfield_perturbed(c, "aligned", row=row, W=W)[0]
        x = c["xs"][row].copy()
        x[W:] += (Up - Uf) @ (V @ np.concatenate((c["x0"][row], c["lam"][row][:W])))
        ev = cert_property_a(c, dict(u=x[None], active=c["active"][row][None], status=np.zeros(1, np.int32)), rows=[row])
        out.append((row, float(ev["ratio"][0])))
    return out


def cert_farfield_perturbed(c, setting, row=None, W=CERT_FAR_W, seed=3):
    """(U', Vx, Vl, efar): U perturbed so that max |U' V - M| is about CERT_FAR_SETTINGS[setting] (on top of the factors' own ~1e-13).
    'small', 'refused': dU = a N.  'aligned': rank one, dU = a w (V z)', z = [x0; lam[0:W]] of `row`: the row's far columns move by
    a |V z|^2 w, as far as max |dU V| = a max |V' V z| allows, with the signs w of the far row of P whose absolute sum is largest."""
    Uf, V, M = cert_farfield_factors(c, W)
    na = c["tq"].shape[1]
    target = CERT_FAR_SETTINGS[setting]
    rng = np.random.default_rng(seed)
    if setting == "exact":
        dU = np.zeros_like(Uf)
    elif setting == "aligned":
        z = np.concatenate((c["x0"][row], c["lam"][row][:W]))
        far = np.abs(c["Ps"][W:, W:]).sum(axis=1)
        w = np.sign(c["Ps"][W + int(np.argmax(far)), W:])           # ... and the moves add up in one far entry of P du
        w[w == 0] = 1.0
        dU = np.outer(w, V @ z)
    else:
        dU = rng.standard_normal(Uf.shape)
    if target > 0.0:
        dU *= target / np.abs(dU @ V).max()
    Up = np.ascontiguousarray(Uf + dU)
    efar = float(np.abs(Up @ V - M).max())
    return Up, np.ascontiguousarray(V[:, :na]), np.ascontiguousarray(V[:, na:]), efar
