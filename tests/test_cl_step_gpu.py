"""The step kernels of the lock-step closed loop (csrc/closed_loop.hip: cl_reset_k, cl_begin_k, cl_filter_k, cl_expand_k, cl_post_k)
beyond one 256-thread trip, step by step against a plain np.longdouble reference (tests/helpers.py: cl_step_reference).

One-step identities instead of trajectories: with the records of a run, every step of every instance is its own test vector --
the filter update, the target optimum, xs, the move of every controller kind, the running cost, the plant step and the
measurement are each recomputed from the RECORDED inputs of that step.  The fp64 identities carry a derived bound (2 gamma_n
times the identity in absolute values), us the bar of tests/test_target_kernel_gpu.py, the MPC move the bar of
tests/test_random_shapes_gpu.py, the NN move the 1e-4 of tests/test_closed_loop_nn_gpu.py.  The models are synthetic linear
maps (helpers.cl_step_model) at the shapes of helpers.CL_STEP_CASES; tests/test_cpu_cl_step_inputs.py holds them and the
reference to their conditions without a device.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

REC = ("y", "x", "xhat", "u", "xs", "us", "avg")


class _Dev:
    """DeviceClosedLoop of a helpers.cl_step_batch, built directly from the model dict, with the handles it borrows."""

    def __init__(self, b):
        from industrial_nnmpc_2021_amd import closed_loop as cl
        from industrial_nnmpc_2021_amd.qp import BatchedBoxQP
        M = b["M"]
        self.b = b
        self.ts = H.TsHandle(M["Pr"], M["E"] if M["nz"] else None, M["ulb"], M["uub"])
        self.qps, slots = [], []
        for s in b["slots"]:
            if s["kind"] == "mpc":
                self.qps.append(BatchedBoxQP(s["P"], s["tq"], s["nu"], max_batch=64))
                slots.append(dict(kind="mpc", qp=self.qps[-1]))
            else:
                slots.append(s)
        self.dev = cl.DeviceClosedLoop(M, self.ts, slots, b["inst_slot"])

    def run(self, t0=0, t1=None, V=None, **kw):
        b = self.b
        t1 = b["T"] if t1 is None else t1
        V = b["V"] if V is None else V
        return self.dev.run(b["SP"][:, t0:t1], b["DS"][:, t0:t1], b["scen"], V[t0:t1 + 1], b["sigma"], **kw)

    def close(self):
        self.dev.close()
        for q in self.qps:
            q.close()
        self.ts.close()


def _sub(b, idx):
    """The batch restricted to the instances ``idx`` (slots without an instance dropped)."""
    idx = np.asarray(idx)
    used = sorted(set(b["inst_slot"][idx]))
    return dict(b, slots=[b["slots"][s] for s in used], inst_slot=np.array([used.index(s) for s in b["inst_slot"][idx]], np.int32),
                scen=b["scen"][idx], V=np.ascontiguousarray(b["V"][:, idx]))


def _window(b, t0, t1):
    """The batch as a call over the steps [t0, t1) sees it."""
    return dict(b, SP=b["SP"][:, t0:t1], DS=b["DS"][:, t0:t1], V=b["V"][t0:t1 + 1], T=t1 - t0)


def _mpc(b):
    return np.array([b["slots"][s]["kind"] == "mpc" for s in b["inst_slot"]])


def _same(a, c, mpc, what):
    """Records equal bit for bit on the non-MPC instances and within 1e-12 on the MPC ones (tests/test_closed_loop_gpu.py)."""
    for k in a:
        if k == "status":
            assert np.array_equal(a[k][0], c[k][0]) and np.array_equal(a[k][1], c[k][1]), (what, k)
            continue
        assert a[k].shape == c[k].shape, (what, k)
        assert a[k][:, ~mpc].tobytes() == c[k][:, ~mpc].tobytes(), (what, k)
        if mpc.any():
            assert np.abs(a[k][:, mpc] - c[k][:, mpc]).max() < 1e-12, (what, k)


def _join(a, c):
    out = {k: np.concatenate((a[k], c[k][1:] if k in ("y", "x", "xhat", "avg") else c[k]), axis=0) for k in REC}
    out["status"] = tuple(np.concatenate((a["status"][j], c["status"][j]), axis=0) for j in range(2))
    return out


@functools.lru_cache(maxsize=None)
def _full(case):
    """One full-record run of all five slots of a case from a fresh handle (shared by the tests; never modified)."""
    b = H.cl_step_batch(case)
    d = _Dev(b)
    try:
        rec = d.run()
    finally:
        d.close()
    for v in rec.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            a.setflags(write=False)
    return b, rec


def _assert_identities(b, rec, what, tg0=0, uprev_in=None, want=None):
    idn = H.cl_step_reference(b, rec, tg0=tg0, uprev_in=uprev_in, want=want)
    ratios = H.cl_identity_ratios(idn)
    print(f"\n{what}: error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(ratios.items())))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (what, bad)
    return idn, ratios


@pytest.mark.parametrize("case", sorted(H.CL_STEP_CASES))
def test_one_step_identities(case):
    """One slot of each kind (US, SATDLQR, NN with and without uprev, MPC) in one batch of 16 instances, 12 steps, three
    scenarios: every identity on every instance and step."""
    b, rec = _full(case)
    M = b["M"]
    nx, nu = M["nx"], M["nu"]
    T, nb = b["T"], b["inst_slot"].size
    assert (rec["status"][0] == 0).all() and (rec["status"][1] == 0).all()
    for k in REC:
        assert np.isfinite(rec[k]).all(), k
    # row 0: the state after create, and the first measurement y_0 = C x0 + sigma o v_0
    assert np.array_equal(rec["x"][0], np.tile(M["x0"], (nb, 1))) and np.array_equal(rec["xhat"][0], np.tile(M["xhat0"], (nb, 1)))
    assert not rec["avg"][0].any()
    y0, bnd = H.cl_ref_measure(M, rec["x"][0], b["V"][0], b["sigma"])
    assert (np.abs(rec["y"][0] - y0) <= bnd).all()
    idn, ratios = _assert_identities(b, rec, f"case {case}")
    kept = idn["us"]["mask"]
    assert (~kept).mean() <= 0.05
    sat = idn["u_satdlqr"]["mask"]
    print(f"case {case}: target rows dropped {(~kept).mean():.3f}, us rows with an input on a bound {(idn['us']['on_bound'] > 0).mean():.2f}, "
          f"SATDLQR entries on a bound {H.share_on_bound(rec['u'][sat], M['ulb'], M['uub']):.2f}")
    first = idn["u_mpc"]["first"][idn["u_mpc"]["mask"]]
    assert (np.abs(first).max(axis=0) > 100 * H.cl_mpc_tol()).all()
    # the NN slots: cl_expand_k's input rows and cl_post_k's combine + clip, against oracle.nn on the recorded inputs
    worst = 0.0
    for i, s in enumerate(b["inst_slot"]):
        spec = b["slots"][s]
        if spec["kind"] != "nn":
            continue
        free, ref = H.cl_one_step_reference(spec["weights"], spec["xscale"], spec["with_uprev"], M["ulb"], M["uub"], rec["u"][:, i],
                                            rec["xhat"][:, i], rec["xs"][:, i], rec["us"][:, i], M["uprev0"], nx)
        assert (np.abs(free - rec["us"][:, i]).max(axis=0) > 100 * H.CL_STEP_NN_TOL).all(), (case, i, "u - us too small to test anything")
        H.assert_cols_close(rec["u"][:, i], ref, H.CL_STEP_NN_TOL, (case, "NN instance", i))
        worst = max(worst, float(H.col_err(rec["u"][:, i], ref).max()))
    print(f"case {case}: worst NN column error {worst:.3e} (bar {H.CL_STEP_NN_TOL:g})")


def test_single_instance_pointing_at_the_last_scenario():
    """nb = 1: one SATDLQR instance whose scen entry is the last of three scenarios equals the same instance inside the batch."""
    b, rec = _full("c")
    i = int(np.flatnonzero((b["scen"] == H.CL_STEP_NSCEN - 1) & (np.array([b["slots"][s]["kind"] for s in b["inst_slot"]]) == "satdlqr"))[0])
    one = _sub(b, [i])
    assert one["inst_slot"].tolist() == [0] and one["scen"].tolist() == [2] and len(one["slots"]) == 1
    d = _Dev(one)
    try:
        r = d.run()
    finally:
        d.close()
    for k in REC:
        assert r[k][:, 0].tobytes() == np.ascontiguousarray(rec[k][:, i]).tobytes(), k
    assert not r["status"][0].any() and not r["status"][1].any()


def test_chunks_tglob_reset_and_given_y0():
    b, full = _full("c")
    M, mpc, nb = b["M"], _mpc(b), b["inst_slot"].size
    d = _Dev(b)
    try:
        a = d.run(0, 5)
        c = d.run(5, 12)
        _same(_join(a, c), full, mpc, "run(5) + run(7)")
        # the running mean across the boundary: tg counts from the reset, not from the call
        _assert_identities(_window(b, 5, 12), c, "second chunk", tg0=5, uprev_in=a["u"][-1], want=())
        wrong = H.cl_identity_ratios(H.cl_step_reference(_window(b, 5, 12), c, tg0=0, uprev_in=a["u"][-1], want=()))
        assert wrong["avg"] > 1e3                          # (the identity would see the call-local t)
        d.dev.reset()
        again = d.run()
        assert np.array_equal(again["x"][0], np.tile(M["x0"], (nb, 1))) and np.array_equal(again["xhat"][0], np.tile(M["xhat0"], (nb, 1)))
        assert not again["avg"][0].any()
        _same(again, full, mpc, "after reset")
        # y0 given: row 0 of y is y0 itself and row 0 of v is not read
        y0 = np.random.default_rng(3).standard_normal((nb, M["ny"]))
        d.dev.reset()
        g1 = d.run(y0=y0)
        assert g1["y"][0].tobytes() == y0.tobytes() and not np.array_equal(g1["u"], full["u"])
        V2 = b["V"].copy()
        V2[0] = 1e6
        d.dev.reset()
        g2 = d.run(V=V2, y0=y0)
        _same(g2, g1, mpc, "row 0 of v with y0 given")
        _assert_identities(b, g1, "y0 given", want=())
    finally:
        d.close()


def test_single_step_calls():
    """T = 1 on a fresh handle, then T = 1 again (not fresh: y and the running mean are carried over)."""
    b, full = _full("c")
    d = _Dev(b)
    try:
        a = d.run(0, 1)
        c = d.run(1, 2)
    finally:
        d.close()
    assert a["u"].shape[0] == 1 and a["y"].shape[0] == 2
    two = {k: (full[k][:3] if k in ("y", "x", "xhat", "avg") else full[k][:2]) for k in REC}
    two["status"] = tuple(s[:2] for s in full["status"])
    _same(_join(a, c), two, _mpc(b), "run(1) + run(1)")


@pytest.mark.parametrize("T", H.CL_STEP_LONG_T)
def test_event_blocks(T):
    """CL_EV_BLOCK = 256: a run of 257 / 513 steps drains the stream and collects the phase times mid-run once / twice."""
    b = H.cl_step_batch("b", kinds=("us", "satdlqr"), counts=(2, 2), T=T)
    d = _Dev(b)
    try:
        whole = d.run()
        tot, phase, ss = d.dev.last_ms()
        d.dev.reset()
        a = d.run(0, 100)
        c = d.run(100, T)
    finally:
        d.close()
    none = np.zeros(4, bool)
    _same(_join(a, c), whole, none, f"run(100) + run({T - 100})")
    assert np.isfinite(whole["xhat"]).all() and not whole["status"][0].any()
    assert ss.shape == (T, 2) and (ss >= 0).all() and (ss > 0).any(axis=1).all()
    assert all(v >= 0 for v in phase.values()) and all(phase[k] > 0 for k in ("filter", "target", "expand", "post"))
    assert sum(phase.values()) <= tot, (phase, tot)
    _assert_identities(_window(b, T - 12, T), {k: whole[k][T - 12:] for k in REC}, f"last 12 of {T} steps", tg0=T - 12,
                       uprev_in=whole["u"][T - 13])


@pytest.mark.parametrize("record", [("u",), ("avg", "status"), ("y", "xhat")])
def test_record_subsets(record):
    """NULL record pointers: what is recorded equals the full-record run bit for bit."""
    b, full = _full("c")
    d = _Dev(b)
    try:
        r = d.run(record=record)
    finally:
        d.close()
    assert set(r) == set(record)
    for k in record:
        if k == "status":
            assert np.array_equal(r[k][0], full[k][0]) and np.array_equal(r[k][1], full[k][1])
        else:
            assert r[k].tobytes() == full[k].tobytes(), k


@pytest.mark.parametrize("case, given_y0", [("e", False), ("c", True)])
def test_device_pointers_and_scenario_check(case, given_y0):
    """One nnmpc_cl_run with every argument in device memory (NNMPC_DEVICE) equals the host-pointer run bit for bit, on every
    instance; a scen entry out of range is refused with NNMPC_EINVAL before anything is launched (records untouched, state
    unchanged).  Case e has nd = 0 (dist NULL) and no y0; case c brings dist (nd = 5) and a given y0 in device memory too."""
    from industrial_nnmpc_2021_amd import _lib
    b, full = _full(case)
    M = b["M"]
    T, nb = b["T"], b["inst_slot"].size
    assert (M["nd"] > 0) == given_y0                       # (dist may be NULL at nd = 0 only)
    y0 = np.random.default_rng(4).standard_normal((nb, M["ny"])) if given_y0 else None
    if given_y0:
        h = _Dev(b)
        try:
            full = h.run(y0=y0)
        finally:
            h.close()
    shapes = dict(y=(T + 1, nb, M["ny"]), x=(T + 1, nb, M["nx"]), xhat=(T + 1, nb, M["nx"] + M["nd"]), u=(T, nb, M["nu"]),
                  xs=(T, nb, M["nx"]), us=(T, nb, M["nu"]), avg=(T + 1, nb))
    SENT = -7.25
    d = _Dev(b)
    sp, scen, v, sig = [_lib.DeviceArray.from_host(a) for a in (b["SP"], b["scen"], b["V"], b["sigma"])]
    ds = _lib.DeviceArray.from_host(b["DS"]) if M["nd"] else None
    dy0 = _lib.DeviceArray.from_host(y0) if given_y0 else None
    bad_scen = b["scen"].copy()
    bad_scen[nb - 1] = H.CL_STEP_NSCEN
    dev_bad = _lib.DeviceArray.from_host(bad_scen)
    out = {k: _lib.DeviceArray.from_host(np.full(shapes[k], SENT)) for k in REC}
    st = [_lib.DeviceArray.from_host(np.full((T, nb), -5, np.int32)) for _ in range(2)]
    p = lambda a: None if a is None else C.c_void_p(a.data_ptr())

    def call(scen):
        return d.dev._lib.nnmpc_cl_run(d.dev._h, T, H.CL_STEP_NSCEN, p(sp), p(ds), p(scen), p(v), p(sig), p(dy0),
                                       *[p(out[k]) for k in REC], p(st[0]), p(st[1]), _lib.DEVICE)
    try:
        assert call(dev_bad) == _lib.EINVAL
        assert b"scen" in d.dev._lib.nnmpc_last_error()
        for k in REC:
            assert (out[k].to_host() == SENT).all(), k
        assert (st[0].to_host() == -5).all() and (st[1].to_host() == -5).all()
        _lib.check(call(scen), "nnmpc_cl_run")
        got = {k: out[k].to_host() for k in REC}
        got["status"] = (st[0].to_host(), st[1].to_host())
    finally:
        for a in [sp, scen, v, sig, ds, dy0, dev_bad] + list(out.values()) + st:
            if a is not None:
                a.free()
        d.close()
    if given_y0:
        assert got["y"][0].tobytes() == y0.tobytes()
    for k in REC:
        assert got[k].shape == full[k].shape and got[k].tobytes() == full[k].tobytes(), k
    assert np.array_equal(got["status"][0], full["status"][0]) and np.array_equal(got["status"][1], full["status"][1])


def test_rows_do_not_depend_on_the_batch():
    """Case f (every dimension on a second trip): one instance of each non-MPC kind in a batch of four, and one alone, against
    the same instances in the batch of 16, bit for bit."""
    b, full = _full("f")
    kinds = [b["slots"][s]["kind"] + ("_u" if b["slots"][s].get("with_uprev") else "") for s in b["inst_slot"]]
    pick = [kinds.index(k) + 1 for k in ("us", "satdlqr", "nn_u", "nn")]
    for idx in (pick, pick[2:3]):
        d = _Dev(_sub(b, idx))
        try:
            r = d.run()
        finally:
            d.close()
        for k in REC:
            assert r[k].tobytes() == np.ascontiguousarray(full[k][:, idx]).tobytes(), (idx, k)
