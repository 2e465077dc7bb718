"""Ten lives of every handle kind: create, one host-pointer call at a small batch, one at a larger batch (every staging slot
of the handle's owner, csrc/dev_res.h, grows once), destroy.  The results of life 10 equal those of life 1 bit for bit, and
the free device memory does not shrink between the end of life 2 and the end of life 10 by more than it did with the
hand-written bookkeeping this owner replaced (GROWTH_BEFORE, measured on the same machine with this file).

The memory check sees leaks of the size of an allocator granule only (torch.cuda.mem_get_info reports what the driver holds,
in units of 2 MiB and more).  A lost event, stream or small buffer does not show here: tests/host/dev_res_test.cpp
(tests/test_cpu_dev_res.py) counts every object of the owner against a fake runtime, on every failure path too.

Shapes: the smallest the other GPU tests use for each kind (helpers.cl_step_batch case b, chain_step_case (3, 2, 1),
ts_matrices, the [70, 130, 70] network of tests/test_train_hip_gpu.py)."""
import functools

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

LIVES = 10
GROWTH_BEFORE = 0            # bytes of free device memory lost between life 2 and life 10, every kind, before the owner
NX, NU = 5, 3


def _bytes(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


@functools.lru_cache(maxsize=None)
def _regulator():
    c = H.chain_step_case(3, 2, 1, 2)
    rng = np.random.default_rng(71)
    return c, rng.standard_normal((40, 3 + 2)), np.tile(c["ulb"], (40, 1)), np.tile(c["uub"], (40, 1))


def _life_qp():
    from industrial_nnmpc_2021_amd.qp import BatchedBoxQP
    c, x0, lb, ub = _regulator()
    qp = BatchedBoxQP(c["spec"]["P"], c["spec"]["tq"], 2, max_batch=64, seg_max=512)
    try:
        a = qp.solve_batch(x0[:3], lb[:3], ub[:3])
        b = qp.solve_batch(x0, lb, ub)
    finally:
        qp.close()
    assert not a["status"].any() and not b["status"].any()
    return _bytes(a["u"], a["active"], b["u"], b["active"])


@functools.lru_cache(maxsize=None)
def _network():
    rng = np.random.default_rng(72)
    W = H.nn_weights(rng, [2 * NX + 2 * NU, 70, 130, 70, NU])
    d = [rng.standard_normal((300, w)) for w in (NX, NU, NX, NU)]
    return W, d


def _life_nn(use_bf16):
    from industrial_nnmpc_2021_amd.nn import StructuredNN
    W, d = _network()
    net = StructuredNN(W, NX, NU, nnwithuprev=True, max_batch=128, use_bf16=use_bf16)
    try:
        a = net.forward(*[v[:5] for v in d])
        b = net.forward(*d)                                  # three sub-batches: the event pool grows
    finally:
        net.close()
    return _bytes(a, b)


def _life_chain():
    from industrial_nnmpc_2021_amd.chain import DeviceChains
    from industrial_nnmpc_2021_amd.qp import BatchedBoxQP
    c = _regulator()[0]
    qp = BatchedBoxQP(c["spec"]["P"], c["spec"]["tq"], 2, max_batch=64, seg_max=512)
    ch = DeviceChains(qp, 2, c["A"], c["B"], c["Bd"], c["ulb"], c["uub"], c["x0"], c["uprev0"])
    try:
        a = ch.run(c["Xs"][:2], c["Us"][:2], c["D"][:2])
        ch.reset()
        b = ch.run(c["Xs"], c["Us"], c["D"])
    finally:
        ch.close()
        qp.close()
    return _bytes(*[r[k] for r in (a, b) for k in ("x", "uprev", "u", "status")])


@functools.lru_cache(maxsize=None)
def _targets():
    Pr, E, lb, ub = H.ts_matrices(73, 3, 1, 1e2)
    return (Pr, E, lb, ub) + H.ts_rhs(74, Pr, E, lb, ub, 60)


def _life_ts():
    Pr, E, lb, ub, q, e = _targets()
    ts = H.TsHandle(Pr, E, lb, ub)
    try:
        a = ts.solve(q[:3], e[:3])
        b = ts.solve(q, e)
    finally:
        ts.close()
    return _bytes(*a, *b)


@functools.lru_cache(maxsize=None)
def _loop():
    return H.cl_step_batch("b", kinds=("nn", "mpc"), counts=(2, 2))


def _life_cl():
    from industrial_nnmpc_2021_amd import closed_loop as cl
    from industrial_nnmpc_2021_amd.qp import BatchedBoxQP
    b = _loop()
    M, mpc = b["M"], b["slots"][1]
    ts = H.TsHandle(M["Pr"], M["E"], M["ulb"], M["uub"])
    qp = BatchedBoxQP(mpc["P"], mpc["tq"], mpc["nu"], max_batch=64, seg_max=512)
    dev = cl.DeviceClosedLoop(M, ts, [b["slots"][0], dict(kind="mpc", qp=qp)], b["inst_slot"])
    try:
        r1 = dev.run(b["SP"][:, :2], b["DS"][:, :2], b["scen"], b["V"][:3], b["sigma"])
        dev.reset()
        r2 = dev.run(b["SP"], b["DS"], b["scen"], b["V"], b["sigma"])
    finally:
        dev.close()
        qp.close()
        ts.close()
    return _bytes(*[a for r in (r1, r2) for k in sorted(r) for a in (r[k] if isinstance(r[k], tuple) else (r[k],))])


@functools.lru_cache(maxsize=None)
def _training():
    rng = np.random.default_rng(75)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    Ws = [[f32(w) for w in H.nn_weights(rng, [2 * NX + 2 * NU] + h + [NU])] for h in ([70, 130, 70], [64, 128, 64])]
    x, xs = rng.standard_normal((400, NX)), 0.3 * rng.standard_normal((400, NX))
    us = rng.uniform(-.5, .5, (400, NU))
    d = dict(x=x, uprev=us + rng.uniform(-.3, .3, (400, NU)), xs=xs, us=us, u=np.clip(us + 0.5 * rng.standard_normal((400, NU)), -1, 1))
    return Ws, {k: f32(v) for k, v in d.items()}


def _life_train():
    from industrial_nnmpc_2021_amd.train import HipTrainer
    Ws, d = _training()
    tr = HipTrainer(Ws[0], NX, NU, nnwithuprev=True, max_batch=256)
    try:
        tr.set_data(d)
        la = tr.step(np.arange(10))
        lb = tr.epoch(np.arange(400), 256)                   # a longer row list: the call's device buffer and pinned images grow
        w = tr.get_weights()
    finally:
        tr.close()
    return _bytes(np.array([la, lb]), *w)


def _life_group():
    from industrial_nnmpc_2021_amd.train import HipGroupTrainer
    Ws, d = _training()
    tr = HipGroupTrainer(Ws, NX, NU, nnwithuprev=True, max_batch=256)
    try:
        tr.set_data(d)
        la = tr.epoch([np.arange(10), np.arange(5)], 256)
        lb = tr.epoch([np.arange(400), np.arange(300)], 256)
        w = [a for g in range(2) for a in tr.get_weights(g)]
    finally:
        tr.close()
    return _bytes(np.asarray(la), np.asarray(lb), *w)


KINDS = {
    "qp": _life_qp,
    "nn_f32": functools.partial(_life_nn, False),
    "nn_bf16": functools.partial(_life_nn, True),
    "chain": _life_chain,
    "ts": _life_ts,
    "cl_nn_mpc": _life_cl,
    "train": _life_train,
    "train_group": _life_group,
}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_ten_lives(kind):
    import torch
    life = KINDS[kind]
    torch.cuda.mem_get_info()                                # (the first call brings up torch's own context)
    first = life()
    life()
    free2 = torch.cuda.mem_get_info()[0]
    for _ in range(LIVES - 3):
        life()
    last = life()
    free10 = torch.cuda.mem_get_info()[0]
    print(f"\n{kind}: {len(first)} result bytes, free device memory {free2} after life 2, {free10} after life {LIVES}: growth {free2 - free10}")
    assert last == first
    assert free2 - free10 <= GROWTH_BEFORE
