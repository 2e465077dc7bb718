"""The chain half of csrc/chain.hip (chain_pre_k, chain_post_k, first_moves_k) beyond one 256-thread trip, step by step against
plain references on the recorded inputs (tests/helpers.py: chain_step_reference).

x_rec[t], uprev_rec[t] are the state before the move of step t; the move must be the first stage of the box QP the recorded
state poses (oracle.qp.solve_exact_box, the bar of tests/test_random_shapes_gpu.py), the next recorded state the model step of
the recorded move (np.longdouble, derived bound), the next recorded previous input the move itself (bit for bit).
"""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

KEYS = ("x", "uprev", "u")


def _close(a, b, tol, what):
    for k in KEYS:
        assert a[k].shape == b[k].shape and np.abs(a[k] - b[k]).max() <= tol, (what, k, np.abs(a[k] - b[k]).max())
    assert np.array_equal(a["status"], b["status"]), what


@pytest.mark.parametrize("nc", [1, 5])
@pytest.mark.parametrize("nx,nu,nd", H.CHAIN_STEP_SHAPES)
def test_chain_identities(nx, nu, nd, nc):
    from industrial_nnmpc_2021_amd import _lib
    from industrial_nnmpc_2021_amd.chain import DeviceChains
    from industrial_nnmpc_2021_amd.qp import BatchedBoxQP
    c = H.chain_step_case(nx, nu, nd, nc)
    T, Xs, Us, D = c["T"], c["Xs"], c["Us"], c["D"]
    qp = BatchedBoxQP(c["spec"]["P"], c["spec"]["tq"], nu, max_batch=64)
    ch = DeviceChains(qp, nc, c["A"], c["B"], c["Bd"], c["ulb"], c["uub"], c["x0"], c["uprev0"])
    dev = []
    try:
        assert (ch.nx, ch.nu, ch.nd) == (nx, nu, nd)
        full = ch.run(Xs, Us, D)
        ch.reset()
        cold = ch.run(Xs, Us, D, warm_start=False)
        ch.reset()
        a = ch.run(Xs[:3], Us[:3], D[:3])
        b = ch.run(Xs[3:], Us[3:], D[3:])
        ch.reset()
        first = ch.run(Xs[:1], Us[:1], D[:1])
        ch.reset()
        # the same call through NNMPC_DEVICE pointers
        up = lambda h: _lib.DeviceArray.from_host(h)
        dev = [up(Xs), up(Us), up(D) if nd else None, up(np.full((T, nc, nx), -7.25)), up(np.full((T, nc, nu), -7.25)),
               up(np.full((T, nc, nu), -7.25)), up(np.full((T, nc), -5, np.int32))]
        ch.run_device(T, *dev)
        on_dev = dict(x=dev[3].to_host(), uprev=dev[4].to_host(), u=dev[5].to_host(), status=dev[6].to_host())
    finally:
        for h in dev:
            if h is not None:
                h.free()
        ch.close()
        qp.close()
    assert not full["status"].any()
    for k in KEYS:
        assert np.isfinite(full[k]).all(), k
    for r in (full, first, on_dev):                                              # after create / reset: the shared initial values
        assert np.array_equal(r["x"][0], np.tile(c["x0"], (nc, 1))) and np.array_equal(r["uprev"][0], np.tile(c["uprev0"], (nc, 1)))
    idn = H.chain_step_reference(c, full, Xs, Us, D)
    ratios = H.cl_identity_ratios(idn)
    print(f"\nchain nx={nx} nu={nu} nd={nd} nc={nc}: error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(ratios.items())))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    assert (np.abs(idn["u"]["first"]).max(axis=(0, 1)) > 100 * H.cl_mpc_tol()).all()          # the regulator decides something
    _close(cold, full, 1e-9, "warm_start=False")
    joined = {k: np.concatenate((a[k], b[k]), axis=0) for k in KEYS + ("status",)}
    _close(joined, full, 1e-12, "run(3) + run(5)")
    jr = H.cl_identity_ratios(H.chain_step_reference(c, joined, Xs, Us, D))    # the step across the two calls included
    assert all(v <= 1.0 for v in jr.values()), jr
    _close(on_dev, full, 1e-12, "device pointers")
    dr = H.cl_identity_ratios(H.chain_step_reference(c, on_dev, Xs, Us, D))
    assert all(v <= 1.0 for v in dr.values()), dr


def _first_moves(lib, u, ldu, us, B, nu, out):
    p = lambda a: None if a is None else C.c_void_p(a.data_ptr())
    return lib.nnmpc_qp_first_moves(p(u), ldu, p(us), B, nu, p(out))


@pytest.mark.parametrize("B,nu,ldu,with_us", H.FIRST_MOVES_CASES)
def test_first_moves(B, nu, ldu, with_us):
    """out[b][k] = u[b ldu + k] + us[b][k] bit for bit (us NULL: + 0.0); the last case walks the grid-stride loop twice
    (4096 x 256 threads, 1 120 000 elements)."""
    from industrial_nnmpc_2021_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(B + nu)
    u = rng.standard_normal((B, ldu))
    us = rng.standard_normal((B, nu))
    assert (B * nu > 4096 * 256) == (B == 70000)
    d = [_lib.DeviceArray.from_host(u), _lib.DeviceArray.from_host(us) if with_us else None, _lib.DeviceArray.from_host(np.full((B, nu), -7.25))]
    try:
        _lib.check(_first_moves(lib, d[0], ldu, d[1], B, nu, d[2]), "nnmpc_qp_first_moves")
        got = d[2].to_host()
    finally:
        for a in d:
            if a is not None:
                a.free()
    ref = u[:, :nu] + (us if with_us else 0.0)
    assert got.tobytes() == np.ascontiguousarray(ref).tobytes()


def test_first_moves_arguments():
    """B = 0 is a no-op that returns OK; ldu < nu is refused."""
    from industrial_nnmpc_2021_amd import _lib
    lib = _lib.load()
    u = _lib.DeviceArray.from_host(np.ones((4, 5)))
    out = _lib.DeviceArray.from_host(np.full((4, 3), -7.25))
    try:
        assert _first_moves(lib, u, 5, None, 0, 3, out) == 0
        assert (out.to_host() == -7.25).all()
        assert _first_moves(lib, u, 2, None, 4, 3, out) == _lib.EINVAL
        assert (out.to_host() == -7.25).all()
    finally:
        u.free()
        out.free()
