"""The argument staging and the call epilogue of the QP entry points (csrc/dev_res.h Staging, csrc/qp_solver.hip CallScope), through
the C ABI: nnmpc_qp_solve_batch_ex, nnmpc_qp_solve_batch_dual, nnmpc_qp_multipliers, nnmpc_qp_sensitivity and nnmpc_ts_solve_batch.

One plant (helpers.pred_plant: n = 16, nu = 2, n_aug = 14) on a handle with max_batch = seg_max = 128, the smallest segment a handle
allows, and B = 300 problems: two full segments and one of 44.  No reference but the library itself -- every check is an equality of bytes:
  * host pointers against device pointers on the same handle;
  * one call over the 300 rows against three calls over rows 0:128, 128:256, 256:300 (the same launches per segment);
  * every combination of optional arguments left out against the call that passes them all (a null dlb / dub / status against zeros,
    which is what null means), in the outputs that remain;
  * every output buffer, host or device, is eight rows longer than B and keeps its sentinel there;
  * with profiling on, a call refused with NNMPC_EINVAL leaves nnmpc_qp_get_stats as it was and the next good call adds one call.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import helpers as H
from tests import sens_helpers as S

pytestmark = pytest.mark.gpu

B, PAD = 300, 8
SEGMENTS = [(0, 128), (128, 256), (256, 300)]
F64 = lambda *shape: (shape, np.float64, S.SENTINEL)
I32 = lambda *shape: (shape, np.int32, -9)
U32 = lambda *shape: (shape, np.uint32, 0xA5A5A5A5)


@pytest.fixture(scope="module")
def case():
    from industrial_nnmpc_2021_amd.linearMPC_build import build_regulator_matrices
    from industrial_nnmpc_2021_amd.qp import BatchedBoxQP
    pl = H.pred_plant(2, 8, seed=41)
    P, tq, nu = build_regulator_matrices(pl)
    qp = BatchedBoxQP(P, tq, nu, max_batch=128, seg_max=128)
    assert (qp.n, qp.nu, qp.n_aug) == (16, 2, 14) and qp.have_inverse
    _, x0, lb, ub = H.batch_inputs(pl, B, seed=42, sx=3.0)
    x0 = x0 * np.linspace(0.0, 1.0, B)[:, None]                                 # row 0: x0 = 0, the optimum u = 0 lies strictly inside its box
    c = dict(qp=qp, x0=x0, lb=lb, ub=ub)
    # the base solve every other call starts from: sequence, active words, status, iterations, multipliers
    u, words, st, it, mult = call(c, "dual", (0, B), [x0, lb, ub, None], dual_outs(qp), False, out_kind=0)
    u, words, st, mult = u[:B], words[:B], st[:B], mult[:B]
    bits = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :2 * qp.n].astype(bool)
    print("status", np.bincount(st, minlength=3).tolist(), "active bounds per problem", np.bincount(bits.sum(axis=1)).tolist())
    assert (st == 0).all() and 0 < bits.sum() and (bits.sum(axis=1) == 0).any()       # a null status means this; bounded and free rows
    rng = np.random.default_rng(43)
    c.update(u=u, words=words, status=st, mult=mult, guess=np.ascontiguousarray(qp.active_to_state(bits)),
             dx0=rng.standard_normal((B, 3, qp.n_aug)), dlb=0.1 * rng.standard_normal((B, 3, nu)), dub=0.1 * rng.standard_normal((B, 3, nu)))
    yield c
    qp.close()


def ex_outs(qp, first=False):
    return [F64(qp.nu if first else qp.n), U32(qp.words), I32(), I32(2)]


def dual_outs(qp):
    return ex_outs(qp) + [F64(qp.n)]


def sens_outs(qp, D, first):
    return [F64(D, qp.nu if first else qp.n), None if first else F64(D, qp.n), I32()]


def call(c, name, rows, ins, outs, device, D=None, out_kind=None, want=0):
    """One call of nnmpc_qp_<name> over rows lo:hi of `ins` (None: a null pointer).  outs: (shape of a row, dtype, fill) or None per
    output; every buffer is PAD rows longer than the call and starts out filled.  Returns the buffers as they came back."""
    from industrial_nnmpc_2021_amd import _lib
    qp = c["qp"]
    lo, hi = rows
    ins = [None if a is None else np.ascontiguousarray(a[lo:hi]) for a in ins]
    bufs = [None if o is None else np.full((hi - lo + PAD,) + o[0], o[2], o[1]) for o in outs]
    fn = getattr(qp._lib, {"ex": "nnmpc_qp_solve_batch_ex", "dual": "nnmpc_qp_solve_batch_dual", "mult": "nnmpc_qp_multipliers",
                           "sens": "nnmpc_qp_sensitivity"}[name])
    head = [qp._h, hi - lo] + ([] if D is None else [D])
    tail = [_lib.DEVICE if device else _lib.HOST] + ([] if out_kind is None else [out_kind])
    if not device:
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        rc = fn(*head, *(p(a) for a in ins + bufs), *tail)
        got = bufs
    else:
        dev = [None if a is None else _lib.DeviceArray.from_host(a) for a in ins + bufs]
        p = lambda a: None if a is None else C.c_void_p(a.data_ptr())
        rc = fn(*head, *(p(a) for a in dev), *tail)
        got = [None if a is None else a.to_host() for a in dev[len(ins):]]
        for a in dev:
            if a is not None:
                a.free()
    assert rc == want, qp._lib.nnmpc_last_error()
    for o, g in zip(outs, got):                                                 # no write past the call's rows, whatever else holds
        if o is not None:
            assert (g[hi - lo:] == np.full(1, o[2], o[1])).all(), (name, rows, device)
    return got


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_entry_point(c, name, ins, outs, optional_outs, **kw):
    """Host against device, one call against per-segment calls, and every subset of the optional outputs left out."""
    host = call(c, name, (0, B), ins, outs, False, **kw)
    dev = call(c, name, (0, B), ins, outs, True, **kw)
    for k, (a, b) in enumerate(zip(host, dev)):
        assert same_bits(a, b), (name, "host against device, output", k)
    parts = [call(c, name, seg, ins, outs, False, **kw) for seg in SEGMENTS]
    for k, a in enumerate(host):
        if a is not None:
            joined = np.concatenate([p[k][:hi - lo] for p, (lo, hi) in zip(parts, SEGMENTS)])
            assert same_bits(joined, a[:B]), (name, "one call against per-segment calls, output", k)
    for r in range(1, len(optional_outs) + 1):
        for leave in itertools.combinations(optional_outs, r):
            fewer = [None if k in leave else o for k, o in enumerate(outs)]
            for device in (False, True):
                got = call(c, name, (0, B), ins, fewer, device, **kw)
                for k, o in enumerate(fewer):
                    assert (got[k] is None) if o is None else same_bits(got[k], host[k]), (name, "left out", leave, "device" if device else "host", k)
    return host


@pytest.mark.parametrize("first", [False, True], ids=["sequence", "first_move"])
@pytest.mark.parametrize("guess", [False, True], ids=["cold", "guess"])
def test_solve_batch_ex(case, guess, first):
    c, qp = case, case["qp"]
    ins = [c["x0"], c["lb"], c["ub"], c["guess"] if guess else None]
    got = check_entry_point(c, "ex", ins, ex_outs(qp, first), (1, 2, 3), out_kind=1 if first else 0)
    assert same_bits(got[1][:B], c["words"]) and (got[2][:B] == 0).all()
    if not guess:
        assert same_bits(got[0][:B], np.ascontiguousarray(c["u"][:, :qp.nu if first else qp.n]))   # the base solve was cold


@pytest.mark.parametrize("guess", [False, True], ids=["cold", "guess"])
def test_solve_batch_dual(case, guess):
    c, qp = case, case["qp"]
    ins = [c["x0"], c["lb"], c["ub"], c["guess"] if guess else None]
    got = check_entry_point(c, "dual", ins, dual_outs(qp), (1, 2, 3), out_kind=0)   # (active and status left out: the handle keeps them for the kernel)
    assert same_bits(got[1][:B], c["words"]) and (guess or same_bits(got[4][:B], c["mult"]))   # the base solve was cold


def test_multipliers(case):
    c, qp = case, case["qp"]
    got = check_entry_point(c, "mult", [c["x0"], c["u"], c["words"], c["status"]], [F64(qp.n)], ())
    assert same_bits(got[0][:B], c["mult"])                                     # what the solve delivered with them
    for device in (False, True):                                                # the optional input: a null status means all zero
        none = call(c, "mult", (0, B), [c["x0"], c["u"], c["words"], None], [F64(qp.n)], device)
        assert same_bits(none[0], got[0])


@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("first", [False, True], ids=["sequence", "first_move"])
def test_sensitivity(case, first, D):
    c, qp = case, case["qp"]
    dx0, dlb, dub = (np.ascontiguousarray(c[k][:, :D]) for k in ("dx0", "dlb", "dub"))
    outs = sens_outs(qp, D, first)
    kw = dict(D=D, out_kind=1 if first else 0)
    optional_outs = (2,) if first else (1, 2)
    full = check_entry_point(c, "sens", [c["words"], c["status"], dx0, dlb, dub], outs, optional_outs, **kw)
    assert (full[2][:B] == 0).all() and np.isfinite(full[0][:B]).all()
    # the optional inputs, with every subset of the optional outputs: null dlb / dub are zeros, a null status is all zero
    for no_lb, no_ub in itertools.product((False, True), repeat=2):
        zeros = call(c, "sens", (0, B), [c["words"], c["status"], dx0, np.zeros_like(dlb) if no_lb else dlb, np.zeros_like(dub) if no_ub else dub], outs, False, **kw)
        for no_st in (False, True):
            if not (no_lb or no_ub or no_st):
                continue
            ins = [c["words"], None if no_st else c["status"], dx0, None if no_lb else dlb, None if no_ub else dub]
            for r in range(len(optional_outs) + 1):
                for leave in itertools.combinations(optional_outs, r):
                    fewer = [None if k in leave else o for k, o in enumerate(outs)]
                    for device in (False, True):
                        got = call(c, "sens", (0, B), ins, fewer, device, **kw)
                        for k, o in enumerate(fewer):
                            assert o is None or same_bits(got[k], zeros[k]), ("left out", no_st, no_lb, no_ub, leave, device, k)


def test_a_refused_call_leaves_the_statistics_alone(case):
    """dmult with first-move output is refused (NNMPC_EINVAL) -- and mult with first-move output by nnmpc_qp_solve_batch_dual.  The
    handle's statistics stay as they were, and the good call after it adds one call: the launch counts of one call exactly, and a
    total time below twice the longest of five good calls before it."""
    from industrial_nnmpc_2021_amd import _lib
    c, qp = case, case["qp"]
    dx0 = np.ascontiguousarray(c["dx0"][:, :1])
    sens_ins = [c["words"], c["status"], dx0, None, None]
    solve_ins = [c["x0"], c["lb"], c["ub"], None]
    good = {"sens": lambda: call(c, "sens", (0, B), sens_ins, sens_outs(qp, 1, False), False, D=1, out_kind=0),
            "ex": lambda: call(c, "ex", (0, B), solve_ins, ex_outs(qp), False, out_kind=0)}
    bad = {"sens": lambda: call(c, "sens", (0, B), sens_ins, [F64(1, qp.nu), F64(1, qp.n), I32()], False, D=1, out_kind=1, want=_lib.EINVAL),
           "ex": lambda: call(c, "dual", (0, B), solve_ins, ex_outs(qp, True) + [F64(qp.n)], False, out_kind=1, want=_lib.EINVAL)}
    total = {"sens": "sens_total_ms", "ex": "total_ms"}
    qp.set_profiling(True)
    try:
        for name in ("sens", "ex"):
            good[name]()                                                        # (the staging exists from here on)
            before, deltas = qp.stats(), []
            for _ in range(5):
                good[name]()
                after = qp.stats()
                deltas.append({k: after[k] - before[k] for k in after})
                before = after
            counts = [k for k in before if k.endswith("_launches") or k.endswith("_problems") or k == "problems"]
            for d in deltas[1:]:
                assert all(d[k] == deltas[0][k] for k in counts)                # one call is one call
            assert deltas[0][total[name]] > 0
            bad[name]()
            assert qp.stats() == before                                         # every field, bit for bit
            good[name]()
            after = qp.stats()
            d = {k: after[k] - before[k] for k in after}
            print(name, "total ms of five good calls", [x[total[name]] for x in deltas], "of the call after the refused one", d[total[name]])
            assert all(d[k] == deltas[0][k] for k in counts)
            assert 0 < d[total[name]] < 2 * max(x[total[name]] for x in deltas)
    finally:
        qp.set_profiling(False)


@pytest.mark.parametrize("nz", [1, 0])
def test_target_selector(nz):
    """nnmpc_ts_solve_batch at nu = 2, B = 5, with one equality and with none: host against device pointers, and lam_eq / active
    left out."""
    Pr, E, lb, ub = H.ts_matrices(5, 2, nz, 1e2)
    q, e = H.ts_rhs(6, Pr, E, lb, ub, 5)
    ts = H.TsHandle(Pr, E if nz else None, lb, ub)
    try:
        full = ts.solve(q, e, kind="host")
        assert (full[3] == 0).all() and not (full[0] == ts.SENTINEL).any() and (full[2] <= 2).all()
        assert (full[1] is None) if nz == 0 else not (full[1] == ts.SENTINEL).any()
        for kind in ("host", "device"):
            for lam, active in itertools.product((True, False), repeat=2):
                got = ts.solve(q, e, kind=kind, lam=lam, active=active)
                assert same_bits(got[0], full[0]) and same_bits(got[3], full[3]), (kind, lam, active)
                assert same_bits(got[1], full[1]) if lam else got[1] is None
                assert same_bits(got[2], full[2]) if active else got[2] is None
    finally:
        ts.close()
