"""A sweep of UNSTRUCTURED networks in one lock-step launch group (HipGroupTrainer(form=NN_UNSTD | NN_UNSTD_RELU), C ABI
nnmpc_train_create_group_ex, train.train_unstd_nn_controllers) against the single-network HipTrainer(form=...), which
tests/test_unstd_train_gpu.py pins to torch float64.  The contract is equality of bytes: a member's weights -- the head bias
included --, epoch losses and validation losses are those of a HipTrainer of the same form fed the same weights and rows,
whatever else is in the group.  Modelled on tests/test_train_group_gpu.py: the same widths (the first layers pad to 128 / 64 /
256, so both tile classes meet in one layer; the head pads to 64 columns, so its bias column sum runs over 61 zero pad columns),
the same 1000 / 700 / 300 rows at batch 256 (members drop out mid-epoch, and the last batch of 29 rows gives M = Bp = 128: one
row tile of the 128 class, one column-sum partial).  The fit scenario is in addition checked against torch float64 on the CPU
with the rule of tests/test_unstd_train_gpu.py: max(8 x the torch-f32 figure measured in the run, 2^-20)."""
import copy
import functools

import numpy as np
import pytest

from tests import unstd_train_helpers as T

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = T.LR, T.B1, T.B2, T.EPS
NX, NU = 5, 3
HIDDEN = ([70, 130, 70], [64, 128, 64], [130, 70, 130])
NS = (1000, 700, 300)                                       # rows a member uses; the last 5 % of them validate
BATCH = 256
L = 4
FORMS = ["linear", "relu"]


def _form(head):
    return T.form_of(head == "relu")


def _split(n):
    nval = int(n * 0.05)
    return n - nval, nval


@functools.lru_cache(maxsize=None)
def _scene(head="linear", uprev=True):
    """Weights of the three members ([W1, b1, ..., WL, bL]; under a ReLU head the head bias is centred on the data so that every
    output column is open on about half of the rows), the 1000-row dataset and two fixed permutations per member (read-only)."""
    rng = np.random.default_rng(21)
    d = T.draw(1000, NX, NU, rng)
    Ws = [T.weights(NX, NU, uprev, h, rng) for h in HIDDEN]
    if head == "relu":
        Ws = [T.centre_head_bias(W, d, uprev) for W in Ws]
    perms = [[np.random.default_rng(40 + 10 * ep + g).permutation(_split(n)[0]) for g, n in enumerate(NS)] for ep in range(2)]
    if not uprev:
        d = dict(d, uprev=None)
    return Ws, d, perms


def _single(W, d, head, max_batch=BATCH, uprev=True):
    from industrial_nnmpc_2021_amd.train import HipTrainer
    tr = HipTrainer(W, NX, NU, nnwithuprev=uprev, max_batch=max_batch, lr=LR, betas=(B1, B2), eps=EPS, form=_form(head))
    tr.set_data(d)
    return tr


def _group(Ws, d, head, max_batch=BATCH, uprev=True, form=None):
    from industrial_nnmpc_2021_amd.train import HipGroupTrainer
    tr = HipGroupTrainer(Ws, NX, NU, nnwithuprev=uprev, max_batch=max_batch, lr=LR, betas=(B1, B2), eps=EPS,
                         form=_form(head) if form is None else form)
    if d is not None:
        tr.set_data(d)
    return tr


def _run_single(W, d, perms, n, head, uprev=True):
    """(bytes after each epoch, epoch losses, validation losses) of one HipTrainer over the row lists ``perms``."""
    ntr, nval = _split(n)
    tr = _single(W, d, head, uprev=uprev)
    try:
        by, loss, val = [], [], []
        for p in perms:
            loss.append(tr.epoch(p, BATCH))
            val.append(tr.eval(ntr, nval))
            by.append(T.bytes_of(tr.get_weights()))
        assert tr.padding_max() == 0.0
        return by, loss, val
    finally:
        tr.close()


def _run_group(Ws, d, perms, ns, head, uprev=True, want_nan=False):
    """The same per member from one HipGroupTrainer; perms[ep][g]."""
    G = len(Ws)
    tr = _group(Ws, d, head, uprev=uprev)
    try:
        by, loss, val = [[] for _ in Ws], [[] for _ in Ws], [[] for _ in Ws]
        for ep in perms:
            lo = tr.epoch(ep, BATCH)
            va = tr.eval([_split(n)[0] for n in ns], [_split(n)[1] for n in ns])
            for g in range(G):
                w = tr.get_weights(g)
                assert len(w) == 2 * L and w[-1].shape == (NU,)                 # the head bias is part of the list
                loss[g].append(lo[g]); val[g].append(va[g]); by[g].append(T.bytes_of(w))
        if want_nan:
            assert not all(np.isfinite(a).all() for a in tr.get_weights(0))     # NaN weights, as in torch
        else:
            assert tr.padding_max() == 0.0
        return by, loss, val
    finally:
        tr.close()


@functools.lru_cache(maxsize=None)
def _clean_singles(head):
    Ws, d, perms = _scene(head)
    return [_run_single(Ws[g], d, [perms[0][g], perms[1][g]], NS[g], head) for g in range(3)]


@functools.lru_cache(maxsize=None)
def _clean_group(head):
    Ws, d, perms = _scene(head)
    return _run_group(Ws, d, perms, NS, head)


@pytest.mark.parametrize("head", FORMS)
def test_members_equal_single_handles_bit_for_bit(head):
    from industrial_nnmpc_2021_amd.train import group_schedule
    assert group_schedule([_split(n)[0] for n in NS], BATCH) == [[256, 256, 256, 182], [256, 256, 153], [256, 29]]
    Ws, d, perms = _scene(head)
    by, loss, val = _clean_group(head)
    for g, (sby, sloss, sval) in enumerate(_clean_singles(head)):
        print(f"[group, {head} head] member {g}: losses {loss[g]} single {sloss}; val {val[g]} single {sval}")
        assert by[g] == sby, g
        assert loss[g] == sloss, g
        assert val[g] == sval, g
        assert by[g][0] != by[g][1] and by[g][0] != T.bytes_of(Ws[g])             # and it trained
        nb = 8 * NU                                                              # ... the head bias too: the list's last bytes
        assert by[g][0][-nb:] != T.bytes_of(Ws[g])[-nb:] and by[g][1][-nb:] != by[g][0][-nb:], g


def test_the_two_forms_are_two_different_steps():
    """What tells the ReLU head from the linear one reaches the group: same weights, different bytes after an epoch."""
    Ws, d, perms = _scene("relu")
    out = []
    for head in FORMS:
        tr = _group(Ws[:1], d, head)
        try:
            tr.epoch([perms[0][0]], BATCH)
            out.append(T.bytes_of(tr.get_weights(0)))
        finally:
            tr.close()
    assert out[0] != out[1] and out[1] == _clean_group("relu")[0][0][0]


def test_a_group_of_one_equals_the_single_handle():
    Ws, d, perms = _scene("relu")
    by, loss, val = _run_group([Ws[0]], d, [[perms[0][0]], [perms[1][0]]], NS[:1], "relu")
    sby, sloss, sval = _clean_singles("relu")[0]
    assert by[0] == sby and loss[0] == sloss and val[0] == sval


def test_without_uprev():
    """11 + 3 input columns instead of 16, uprev=None in the data."""
    Ws, d, perms = _scene("linear", uprev=False)
    assert d["uprev"] is None and Ws[0][0].shape[0] == 2 * NX + NU
    by, loss, val = _run_group(Ws[:2], d, [perms[0][:2]], NS[:2], "linear", uprev=False)
    for g in range(2):
        sby, sloss, sval = _run_single(Ws[g], d, [perms[0][g]], NS[g], "linear", uprev=False)
        assert by[g] == sby and loss[g] == sloss and val[g] == sval, g
        assert by[g][0] != T.bytes_of(Ws[g])


def test_several_dw_slices(monkeypatch):
    """One pass: Bp = 640 rows = 20 chunks in slices of 7, 7, 6, for both members, in the group as in the single handles."""
    monkeypatch.setenv("NNMPC_TRAIN_DW_SLICES", "3")
    Ws, d, _ = _scene("relu")
    perm = np.random.default_rng(9).permutation(1000)[:600]
    tr = _group(Ws[:2], d, "relu", max_batch=600)
    try:
        loss = tr.epoch([perm, perm], 600)
        got = [T.bytes_of(tr.get_weights(g)) for g in range(2)]
    finally:
        tr.close()
    for g in range(2):
        s = _single(Ws[g], d, "relu", max_batch=600)
        try:
            assert s.epoch(perm, 600) == loss[g]
            assert s.dw_slices() == [3] * L
            assert T.bytes_of(s.get_weights()) == got[g], g
        finally:
            s.close()


def test_tiny_batches():
    """An epoch whose only batch is one row, one of exactly 128 rows (one whole row tile, no padding row) and one of 129."""
    Ws, d, _ = _scene("linear")
    lists = [np.array([5]), np.random.default_rng(3).permutation(1000)[:128], np.random.default_rng(4).permutation(1000)[:129]]
    tr = _group(Ws, d, "linear")
    try:
        loss = tr.epoch(lists, BATCH)
        val = tr.eval([999, 0, 872], [1, 128, 128])
        got = [T.bytes_of(tr.get_weights(g)) for g in range(3)]
        assert tr.padding_max() == 0.0
    finally:
        tr.close()
    for g, (first, count) in enumerate(((999, 1), (0, 128), (872, 128))):
        s = _single(Ws[g], d, "linear")
        try:
            assert s.epoch(lists[g], BATCH) == loss[g] and np.isfinite(loss[g])
            assert s.eval(first, count) == val[g]
            assert T.bytes_of(s.get_weights()) == got[g] != T.bytes_of(Ws[g]), g
        finally:
            s.close()


def test_it_is_a_group_not_a_loop():
    """Three copies of a member whose layers fall into one tile class each enqueue what a group of one enqueues: 6 L + 2
    kernels per lock-step step (the structured 6 L and the head's column sums and bias update), L + 3 per eval chunk."""
    from industrial_nnmpc_2021_amd import _lib
    rng = np.random.default_rng(5)
    W = T.weights(NX, NU, True, [64, 128, 64], rng)
    _, d, perms = _scene("linear")
    p = perms[0][0]
    steps = -(-len(p) // BATCH)
    assert steps == 4
    a, b = _group([W] * 3, d, "linear"), _group([W], d, "linear")
    s = _group([W[:-1]], d, "linear", form=_lib.NN_STRUCTURED)
    try:
        a.epoch([p, p[:700], p[:300]], BATCH)
        b.epoch([p], BATCH)
        na, nb = a.last_launches(), b.last_launches()
        print(f"[group] launches: three members {na}, one member {nb} ({nb / steps:.1f} per lock-step step)")
        assert na == nb == steps * (6 * L + 2)
        a.eval([950, 665, 285], [50, 35, 15])
        b.eval([950], [50])
        assert a.last_launches() == b.last_launches() == L + 3
        s.epoch([p], BATCH)
        assert s.last_launches() == steps * 6 * L                               # the structured count is untouched
        s.eval([950], [50])
        assert s.last_launches() == L + 3
    finally:
        a.close(); b.close(); s.close()


def test_snapshot_and_restore_by_mask():
    Ws, d, perms = _scene("relu")
    by, _, _ = _clean_group("relu")
    nb = 8 * NU
    tr = _group(Ws, d, "relu")
    try:
        tr.epoch(perms[0], BATCH)
        tr.snapshot([True, False, True])
        tr.epoch(perms[1], BATCH)
        assert [T.bytes_of(tr.get_weights(g)) for g in range(3)] == [by[g][1] for g in range(3)]
        tr.restore([True, False, True])
        got = [T.bytes_of(tr.get_weights(g)) for g in range(3)]
        assert got[0] == by[0][0] and got[2] == by[2][0]                        # epoch-1 bytes
        assert got[0][-nb:] == by[0][0][-nb:] != by[0][1][-nb:]                 # the head bias came back with them
        assert got[1] == by[1][1]                                               # epoch-2 bytes
        tr.restore([False, True, False])                                        # never snapshotted: the initial weights
        assert T.bytes_of(tr.get_weights(1)) == T.bytes_of(Ws[1])
        # upload and read-back: the head bias round-trips, the other members do not move
        new = [T.f32(w + 0.5) for w in Ws[2]]
        tr.set_weights(2, new)
        assert T.bytes_of(tr.get_weights(2)) == T.bytes_of(new)
        assert T.bytes_of(tr.get_weights(0)) == got[0]
        with pytest.raises(ValueError, match="even-length"):
            tr.set_weights(2, new[:-1])
    finally:
        tr.close()


def test_nan_stays_local():
    """Row 800 is among member 0's rows only."""
    Ws, d, perms = _scene("linear")
    bad = {k: v.copy() for k, v in d.items()}
    bad["x"][800, 1] = np.nan
    assert 800 in perms[0][0] and 800 in perms[1][0]
    by, loss, val = _run_group(Ws, bad, perms, NS, "linear", want_nan=True)
    cby, closs, cval = _clean_group("linear")
    assert np.isnan(loss[0][0]) and np.isnan(loss[0][1])
    for g in (1, 2):
        assert by[g] == cby[g] and loss[g] == closs[g] and val[g] == cval[g], g


def test_a_member_without_rows_sits_the_epoch_out():
    """Neither its bytes nor its Adam step count move: its next epoch equals a single handle's first."""
    Ws, d, perms = _scene("relu")
    tr = _group(Ws[:2], d, "relu")
    try:
        l1 = tr.epoch([perms[0][0], None], BATCH)
        assert np.isfinite(l1[0]) and np.isnan(l1[1])
        assert T.bytes_of(tr.get_weights(1)) == T.bytes_of(Ws[1])
        v = tr.eval([950, 0], [50, 0])
        assert np.isfinite(v[0]) and np.isnan(v[1])
        l2 = tr.epoch([perms[1][0], perms[1][1]], BATCH)
        got = [T.bytes_of(tr.get_weights(g)) for g in range(2)]
    finally:
        tr.close()
    assert got[0] == _clean_singles("relu")[0][0][1]
    s = _single(Ws[1], d, "relu")
    try:
        assert s.epoch(perms[1][1], BATCH) == l2[1]
        assert T.bytes_of(s.get_weights()) == got[1]
    finally:
        s.close()


def test_fit_and_deploy():
    """train_unstd_nn_controllers on three small linear-head models with num_samples of three sizes: every returned model
    and history is the one of train_unstd_nn_controller(backend="hip") on its rows; one member against torch float64 on the
    CPU and, deployed through nn.UnstructuredNN (f32), against the torch model at 1e-4 per column (the rule and the bar of
    tests/test_unstd_train_gpu.py)."""
    import torch
    from industrial_nnmpc_2021_amd.train import UnstdRegulatorModel, train_unstd_nn_controller, train_unstd_nn_controllers
    from industrial_nnmpc_2021_amd.nn import UnstructuredNN
    from tests import helpers as H
    nx, nu, n = 4, 2, 8192
    data = T.fit_data(np.random.default_rng(1), n, nx, nu)
    hidden, ns = ([64, 64], [64, 64], [128, 64]), [8192, 4096, 6000]
    torch.manual_seed(0)
    models = [UnstdRegulatorModel(nx, nu, [None] + h + [nu], nnwithuprev=True, head_relu=False) for h in hidden]
    alone = [copy.deepcopy(m) for m in models]
    models, ttime, hists = train_unstd_nn_controllers(models, data, num_samples=ns, epochs=25, batch_size=512, seed=4)
    assert ttime > 0 and [len(h) for h in hists] == [25] * 3
    for g in range(3):
        part = {k: v[:ns[g]] for k, v in data.items()}
        m, _, hist = train_unstd_nn_controller(alone[g], part, epochs=25, batch_size=512, backend="hip", seed=4)
        assert hist == hists[g], g
        assert T.bytes_of(m.get_weights()) == T.bytes_of(models[g].get_weights()), g
        assert hists[g][-1][1] < hists[g][0][1], g                              # it learns
    g = 2
    W = models[g].get_weights()
    assert len(W) == 6
    m = models[g].cpu()
    s = slice(ns[g] - int(ns[g] * 0.1), ns[g])
    t64 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    t32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32)
    val = lambda mod, tt: float(torch.mean((mod(tt(data["x"][s]), tt(data["uprev"][s]), tt(data["xs"][s]), tt(data["us"][s]))
                                            - tt(data["u"][s])) ** 2))
    with torch.no_grad():
        val64 = val(m, t64)
        val32 = val(T.model(W, nx, nu, True, False, torch.float32), t32)
        k = 1000
        ref = m(t64(data["x"][:k]), t64(data["uprev"][:k]), t64(data["xs"][:k]), t64(data["us"][:k])).numpy()
    best = min(h[1] for h in hists[g])
    e, e32 = abs(best - val64) / val64, abs(val32 - val64) / val64
    print(f"[fit {g}] val loss first {hists[g][0][1]:.3e} last {hists[g][-1][1]:.3e} best {best:.6e}, returned model in f64 "
          f"{val64:.6e}: hip {e:.2e}, torch f32 {e32:.2e}")
    assert e <= max(8 * e32, 2.0 ** -20)
    net = UnstructuredNN(W, nx, nu, nnwithuprev=True, max_batch=1024, head_relu=False)
    try:
        got = net.forward(data["x"][:k], data["uprev"][:k], data["xs"][:k], data["us"][:k])
    finally:
        net.close()
    H.assert_cols_close(got, ref, 1e-4, "deployed")


def test_refusals_through_the_device_path():
    from industrial_nnmpc_2021_amd import _lib
    from industrial_nnmpc_2021_amd.train import HipGroupTrainer, UnstdRegulatorModel, train_unstd_nn_controllers
    Ws, d, _ = _scene("linear")
    models = [UnstdRegulatorModel(NX, NU, [None, 8, NU], head_relu=r) for r in (True, False)]
    with pytest.raises(ValueError, match="head_relu"):
        train_unstd_nn_controllers(models, d, epochs=1)
    for form in (_lib.NN_UNSTD, _lib.NN_UNSTD_RELU):
        with pytest.raises(ValueError, match="even-length"):                    # the structured list under an unstructured form
            HipGroupTrainer([Ws[0], Ws[1][:-1]], NX, NU, max_batch=BATCH, form=form)
    with pytest.raises(_lib.NnmpcError, match=r"\(code -1\): nnmpc_train_create_group_ex: member 0: "):
        HipGroupTrainer([Ws[0], Ws[1]], NX + 1, NU, max_batch=BATCH, form=_lib.NN_UNSTD)
