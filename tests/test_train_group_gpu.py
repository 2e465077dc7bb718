"""A sweep of networks in one lock-step launch group (csrc/nn_train_group.hip, C ABI nnmpc_train_group_*,
train.HipGroupTrainer, train.train_nn_controllers) against the single-network HipTrainer, which tests/test_train_hip_gpu.py
pins to torch float64.  The contract is equality of bytes: a member's weights, epoch losses and validation losses are those of
a HipTrainer fed the same weights and rows, whatever else is in the group.  The fit scenario is in addition checked against
torch float64 on the CPU with the rule of test_train_hip_gpu.py: max(8 x the torch-f32 figure measured in the run, 2^-20)."""
import copy
import functools
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-7
NX, NU = 5, 3
HIDDEN = ([70, 130, 70], [64, 128, 64], [130, 70, 130])     # first hidden layer: padded 128, 64, 256 -> both tile classes
NS = (1000, 700, 300)                                       # rows a member uses; the last 5 % of them validate
BATCH = 256


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _weights(nx, nu, uprev, hidden, rng):
    """Glorot-uniform weights, hidden biases 0.1 N(0,1); Keras order, f32-representable."""
    dims = [2 * nx + (2 if uprev else 1) * nu] + list(hidden) + [nu]
    out = []
    for l in range(len(dims) - 1):
        lim = np.sqrt(6.0 / (dims[l] + dims[l + 1]))
        out.append(_f32(rng.uniform(-lim, lim, (dims[l], dims[l + 1]))))
        if l < len(dims) - 2:
            out.append(_f32(0.1 * rng.standard_normal(dims[l + 1])))
    return out


def _draw(n, nx, nu, rng):
    x, xs = rng.standard_normal((n, nx)), 0.3 * rng.standard_normal((n, nx))
    us = rng.uniform(-.5, .5, (n, nu))
    up = us + rng.uniform(-.3, .3, (n, nu))
    u = np.clip(us + 0.5 * rng.standard_normal((n, nu)), -1, 1)
    return {k: _f32(v) for k, v in dict(x=x, uprev=up, xs=xs, us=us, u=u).items()}


def _bytes(weights):
    return b"".join(np.ascontiguousarray(w).tobytes() for w in weights)


def _split(n):
    nval = int(n * 0.05)
    return n - nval, nval


@functools.lru_cache(maxsize=None)
def _scene():
    """Weights of the three members, the 1000-row dataset and two fixed permutations per member (read-only)."""
    rng = np.random.default_rng(21)
    Ws = [_weights(NX, NU, True, h, rng) for h in HIDDEN]
    d = _draw(1000, NX, NU, rng)
    perms = [[np.random.default_rng(40 + 10 * ep + g).permutation(_split(n)[0]) for g, n in enumerate(NS)] for ep in range(2)]
    return Ws, d, perms


def _single(W, d, max_batch=BATCH):
    from industrial_nnmpc_2021_amd.train import HipTrainer
    tr = HipTrainer(W, NX, NU, nnwithuprev=True, max_batch=max_batch, lr=LR, betas=(B1, B2), eps=EPS)
    tr.set_data(d)
    return tr


def _group(Ws, d, max_batch=BATCH, **kw):
    from industrial_nnmpc_2021_amd.train import HipGroupTrainer
    tr = HipGroupTrainer(Ws, NX, NU, nnwithuprev=True, max_batch=max_batch, lr=LR, betas=(B1, B2), eps=EPS, **kw)
    if d is not None:
        tr.set_data(d)
    return tr


def _run_single(W, d, perms, n):
    """(bytes after each epoch, epoch losses, validation losses) of one HipTrainer over the row lists ``perms``."""
    ntr, nval = _split(n)
    tr = _single(W, d)
    try:
        by, loss, val = [], [], []
        for p in perms:
            loss.append(tr.epoch(p, BATCH))
            val.append(tr.eval(ntr, nval))
            by.append(_bytes(tr.get_weights()))
        return by, loss, val
    finally:
        tr.close()


def _run_group(Ws, d, perms, ns):
    """The same per member from one HipGroupTrainer; perms[ep][g]."""
    G = len(Ws)
    tr = _group(Ws, d)
    try:
        by, loss, val = [[] for _ in Ws], [[] for _ in Ws], [[] for _ in Ws]
        for ep in perms:
            lo = tr.epoch(ep, BATCH)
            va = tr.eval([_split(n)[0] for n in ns], [_split(n)[1] for n in ns])
            for g in range(G):
                loss[g].append(lo[g]); val[g].append(va[g]); by[g].append(_bytes(tr.get_weights(g)))
        assert tr.padding_max() == 0.0
        return by, loss, val
    finally:
        tr.close()


@functools.lru_cache(maxsize=None)
def _clean_singles():
    Ws, d, perms = _scene()
    return [_run_single(Ws[g], d, [perms[0][g], perms[1][g]], NS[g]) for g in range(3)]


@functools.lru_cache(maxsize=None)
def _clean_group():
    Ws, d, perms = _scene()
    return _run_group(Ws, d, perms, NS)


def test_members_equal_single_handles_bit_for_bit():
    from industrial_nnmpc_2021_amd.train import group_schedule
    assert group_schedule([_split(n)[0] for n in NS], BATCH) == [[256, 256, 256, 182], [256, 256, 153], [256, 29]]
    Ws, d, perms = _scene()
    by, loss, val = _clean_group()
    for g, (sby, sloss, sval) in enumerate(_clean_singles()):
        print(f"[group] member {g}: losses {loss[g]} single {sloss}; val {val[g]} single {sval}")
        assert by[g] == sby, g
        assert loss[g] == sloss, g
        assert val[g] == sval, g
        assert by[g][0] != by[g][1] and by[g][0] != _bytes(Ws[g])           # and it trained


def test_a_group_of_one_equals_the_single_handle():
    Ws, d, perms = _scene()
    by, loss, val = _run_group([Ws[0]], d, [[perms[0][0]], [perms[1][0]]], NS[:1])
    sby, sloss, sval = _clean_singles()[0]
    assert by[0] == sby and loss[0] == sloss and val[0] == sval


def test_several_dw_slices(monkeypatch):
    """2 Bp = 1280 rows = 40 chunks in slices of 14, 14, 12, for both members, in the group as in the single handles."""
    monkeypatch.setenv("NNMPC_TRAIN_DW_SLICES", "3")
    Ws, d, _ = _scene()
    perm = np.random.default_rng(9).permutation(1000)[:600]
    tr = _group(Ws[:2], d, max_batch=600)
    try:
        loss = tr.epoch([perm, perm], 600)
        got = [_bytes(tr.get_weights(g)) for g in range(2)]
    finally:
        tr.close()
    for g in range(2):
        s = _single(Ws[g], d, max_batch=600)
        try:
            assert s.epoch(perm, 600) == loss[g]
            assert s.dw_slices() == [3] * 4
            assert _bytes(s.get_weights()) == got[g], g
        finally:
            s.close()


def test_it_is_a_group_not_a_loop():
    """Three members of one tile class per layer with 4 / 3 / 2 steps enqueue what one member with 4 steps enqueues."""
    rng = np.random.default_rng(5)
    Ws = [_weights(NX, NU, True, [64, 128, 64], rng) for _ in range(3)]
    _, d, perms = _scene()
    a, b = _group(Ws, d), _group(Ws[:1], d)
    try:
        a.epoch(perms[0], BATCH)
        b.epoch(perms[0][:1], BATCH)
        na, nb = a.last_launches(), b.last_launches()
        print(f"[group] launches: three members {na}, one member {nb} ({nb / 4:.1f} per lock-step step)")
        assert na == nb and nb > 0
        a.eval([950, 665, 285], [50, 35, 15])
        b.eval([950], [50])
        assert a.last_launches() == b.last_launches() > 0
    finally:
        a.close(); b.close()


def test_snapshot_and_restore_by_mask():
    Ws, d, perms = _scene()
    by, _, _ = _clean_group()
    tr = _group(Ws, d)
    try:
        tr.epoch(perms[0], BATCH)
        tr.snapshot([True, False, True])
        tr.epoch(perms[1], BATCH)
        assert [_bytes(tr.get_weights(g)) for g in range(3)] == [by[g][1] for g in range(3)]
        tr.restore([True, False, True])
        got = [_bytes(tr.get_weights(g)) for g in range(3)]
        assert got[0] == by[0][0] and got[2] == by[2][0]                    # epoch-1 bytes
        assert got[1] == by[1][1]                                           # epoch-2 bytes
        tr.restore([False, True, False])                                    # never snapshotted: the initial weights
        assert _bytes(tr.get_weights(1)) == _bytes(Ws[1])
    finally:
        tr.close()


def test_nan_stays_local():
    """Row 800 is among member 0's rows only."""
    Ws, d, perms = _scene()
    bad = {k: v.copy() for k, v in d.items()}
    bad["x"][800, 1] = np.nan
    assert 800 in perms[0][0] and 800 in perms[1][0]
    by, loss, val = _run_group_nan(Ws, bad, perms)
    cby, closs, cval = _clean_group()
    assert np.isnan(loss[0][0]) and np.isnan(loss[0][1])
    for g in (1, 2):
        assert by[g] == cby[g] and loss[g] == closs[g] and val[g] == cval[g], g


def _run_group_nan(Ws, d, perms):
    tr = _group(Ws, d)
    try:
        by, loss, val = [[] for _ in Ws], [[] for _ in Ws], [[] for _ in Ws]
        for ep in perms:
            lo = tr.epoch(ep, BATCH)
            va = tr.eval([_split(n)[0] for n in NS], [_split(n)[1] for n in NS])
            for g in range(3):
                loss[g].append(lo[g]); val[g].append(va[g]); by[g].append(_bytes(tr.get_weights(g)))
        assert np.isnan(tr.get_weights(0)[-1]).any()                        # NaN weights, as in torch
        return by, loss, val
    finally:
        tr.close()


def _einval(fn):
    from industrial_nnmpc_2021_amd import _lib
    with pytest.raises(_lib.NnmpcError) as ei:
        fn()
    assert re.search(r"\(code -1\): \S", str(ei.value)), str(ei.value)              # NNMPC_EINVAL with a message


def test_edges():
    from industrial_nnmpc_2021_amd.train import HipGroupTrainer
    Ws, d, perms = _scene()
    mk = lambda ws, nx=NX, nu=NU, **kw: HipGroupTrainer(ws, nx, nu, nnwithuprev=True, max_batch=BATCH, **kw)
    _einval(lambda: mk([]))                                                           # G < 1
    _einval(lambda: mk(Ws, nx=NX + 1))                                                # dims[0] != 2 nx + 2 nu
    _einval(lambda: mk(Ws, nu=NU + 1))                                                # dims[L] != nu
    _einval(lambda: mk(Ws, eps=0.0))
    tr = _group(Ws, None)
    try:
        _einval(lambda: tr.epoch(perms[0], BATCH))                                    # no dataset
        _einval(lambda: tr.eval([950, 665, 285], [50, 35, 15]))
        _einval(lambda: tr.set_data({k: v for k, v in d.items() if k != "uprev"}))    # with-uprev group, no uprev
        tr.set_data(d)
        before = [_bytes(tr.get_weights(g)) for g in range(3)]
        assert before == [_bytes(w) for w in Ws]
        _einval(lambda: tr.epoch(perms[0], BATCH + 1))                                # batch > max_batch
        for badrow in (1000, -1):
            p = [q.copy() for q in perms[0]]
            p[2][-1] = badrow                                                         # the last entry of the last list
            _einval(lambda: tr.epoch(p, BATCH))
        _einval(lambda: tr.eval([950, 665, 998], [50, 35, 3]))                        # rows past the dataset
        assert [_bytes(tr.get_weights(g)) for g in range(3)] == before                # rejected before any launch
        assert tr.padding_max() == 0.0
    finally:
        tr.close()


def test_a_member_without_rows_sits_the_epoch_out():
    """Neither its bytes nor its Adam step count move: its next epoch equals a single handle's first."""
    Ws, d, perms = _scene()
    tr = _group(Ws[:2], d)
    try:
        l1 = tr.epoch([perms[0][0], None], BATCH)
        assert np.isfinite(l1[0]) and np.isnan(l1[1])
        assert _bytes(tr.get_weights(1)) == _bytes(Ws[1])
        v = tr.eval([950, 0], [50, 0])
        assert np.isfinite(v[0]) and np.isnan(v[1])
        l2 = tr.epoch([perms[1][0], perms[1][1]], BATCH)
        got = [_bytes(tr.get_weights(g)) for g in range(2)]
    finally:
        tr.close()
    assert got[0] == _clean_singles()[0][0][1]
    s = _single(Ws[1], d)
    try:
        assert s.epoch(perms[1][1], BATCH) == l2[1]
        assert _bytes(s.get_weights()) == got[1]
    finally:
        s.close()


def test_fit_and_deploy():
    """The scenario of test_fit_with_the_hip_backend_then_deploy_through_the_hip_forward for a sweep of three."""
    import torch
    from industrial_nnmpc_2021_amd.train import RegulatorModel, train_nn_controller, train_nn_controllers
    from industrial_nnmpc_2021_amd import controller_evaluation as ce
    rng = np.random.default_rng(1)
    nx, nu, n = 6, 3, 8192
    K = rng.standard_normal((nu, nx)) * 0.5
    x, xs = 1.5 * rng.standard_normal((n, nx)), 0.2 * rng.standard_normal((n, nx))
    us = rng.uniform(-.3, .3, (n, nu)); up = us + rng.uniform(-.2, .2, (n, nu))
    u = np.clip(us + (x - xs) @ K.T, -1, 1)
    data, xscale = ce._get_data_for_training(data=dict(x=x, uprev=up, xs=xs, us=us, u=u), num_samples=n)
    hidden, ns = ([64, 64], [64, 64], [128, 64]), [8192, 4096, 8192]
    torch.manual_seed(3)
    models = [RegulatorModel(nx, nu, [None] + h + [nu], nnwithuprev=True) for h in hidden]
    alone = copy.deepcopy(models[0])
    models, ttime, hists = train_nn_controllers(models, data, num_samples=ns, epochs=25, batch_size=512, seed=4)
    assert ttime > 0 and [len(h) for h in hists] == [25] * 3
    t64 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    t32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32)
    for g, m in enumerate(models):
        hist = hists[g]
        assert hist[-1][1] < 0.25 * hist[0][1], g                              # it learns
        s = slice(ns[g] - int(ns[g] * 0.05), ns[g])
        val = lambda mod, tt: float(torch.mean((mod(tt(data["x"][s]), tt(data["uprev"][s]), tt(data["xs"][s]), tt(data["us"][s]))
                                                - tt(data["u"][s])) ** 2))
        with torch.no_grad():
            val64 = val(m.cpu(), t64)
            m32 = RegulatorModel(nx, nu, [None] + hidden[g] + [nu], nnwithuprev=True, dtype=torch.float32)
            m32.set_weights(m.get_weights())
            val32 = val(m32, t32)
        best = min(h[1] for h in hist)
        e, e32 = abs(best - val64) / val64, abs(val32 - val64) / val64
        print(f"[fit {g}] val loss first {hist[0][1]:.3e} last {hist[-1][1]:.3e} best {best:.6e}, returned model in f64 "
              f"{val64:.6e}: hip {e:.2e}, torch f32 {e32:.2e}")
        assert e <= max(8 * e32, 2.0 ** -20), g
    alone, _, hist = train_nn_controller(alone, data, epochs=25, batch_size=512, backend="hip", seed=4)
    assert hist == hists[0]
    assert _bytes(alone.get_weights()) == _bytes(models[0].get_weights())
