"""The tangent loss in the sweep trainer (csrc/nn_train_group.hip: nnmpc_train_create_group_tan and its three companions,
train.HipGroupTrainer(tangents=True), train.train_nn_controllers(tan_weights=)).

The contract is equality of bytes: a member with w > 0 holds the weights and returns the losses (L, mse, tan_mse) of its own
HipTrainer(tangents=True) at that weight fed the same rows, a member with w == 0 those of a plain HipTrainer, whatever else
is in the group -- and tests/test_tan_train_gpu.py pins that single handle to torch float64 and to the int64 exact case.  Two
tests do not go through the single handle: the exact case (every number equals tan_helpers.exact_int's) and five lock-step
steps against the float64 Adam trajectory (bar: 8 x the float32 torch trajectory's own error, from that test's helpers).

The members are those the feature was specified with: hidden [40, 64] at w 0.5 (every layer in the NB 64 class), [128, 128]
at w 0.25 (every layer NB 128), [70, 130, 70] at w 0 (a plain member inside a tangent group) and [70, 130, 70] at w 1.0, on
600, 333, 129 and 37 rows at batch 128: last batches of 88, 77, 1 and 37 rows, and the members leave the lock step after
5, 3, 2 and 1 steps.  A group has ONE depth, so the four are two groups over the one dataset: A = the two three-layer
networks (both tile classes in every launch, two different weights), B = the two four-layer ones (w == 0 beside w > 0).  The
exact case is split the same way: {narrow} and {wide at 0.5, wide at 0}."""
import copy
import functools

import numpy as np
import pytest

from tests import tan_helpers as H
from tests import test_train_hip_gpu as P

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = P.LR, P.B1, P.B2, P.EPS
NX, NU = 5, 3
N_DATA, MAX_BATCH, BATCH = 700, 256, 128
GROUPS = {                                              # hidden widths, weights, rows of the members
    "A": (([40, 64], [128, 128]), (0.5, 0.25), (600, 333)),
    "B": (([70, 130, 70], [70, 130, 70]), (0.0, 1.0), (129, 37)),
}
EVAL = (600, 50)                                        # rows no member trains on


def _bytes(weights):
    return b"".join(np.ascontiguousarray(w).tobytes() for w in weights)


@functools.lru_cache(maxsize=None)
def _scene():
    """Per group the members' weights; the dataset: 700 rows free of kinks for all four networks (the rule of
    tests/test_train_hip_gpu.py, applied per network) with tangents; two permutations per member (read-only)."""
    rng = np.random.default_rng(77)
    Ws = {k: [P._weights(NX, NU, True, h, rng) for h in g[0]] for k, g in GROUPS.items()}
    d = P._draw(4 * N_DATA + 64, NX, NU, rng)
    keep = np.ones(d["x"].shape[0], bool)
    for W in Ws["A"] + Ws["B"]:
        lo, hi = P._kink_margin(W, d, True)
        keep &= lo > 1e-4 * hi
    sel = np.flatnonzero(keep)
    assert sel.size >= N_DATA, sel.size
    d = H.add_tangents({k: v[sel[:N_DATA]] for k, v in d.items()}, NX, NU, rng)
    perms = {k: [[np.random.default_rng(60 + 10 * ep + 3 * i + ord(k)).permutation(n) for i, n in enumerate(g[2])]
                 for ep in range(2)] for k, g in GROUPS.items()}
    return Ws, d, perms


def _single(W, w, d, max_batch=MAX_BATCH, nx=NX, nu=NU):
    """The member's own handle: a tangent handle at its weight for w > 0, a plain one for w == 0."""
    from industrial_nnmpc_2021_amd.train import HipTrainer
    tr = HipTrainer(W, nx, nu, nnwithuprev=True, max_batch=max_batch, lr=LR, betas=(B1, B2), eps=EPS, tangents=w > 0)
    tr.set_data(d)
    if w > 0:
        tr.set_tangents(d)
        tr.set_tan_weight(w)
    return tr


def _group(Ws, ws, d, max_batch=MAX_BATCH, nx=NX, nu=NU, tangents=True):
    """ws None: a plain group.  Otherwise a tangent group with the tangents loaded (tangents=False: not) at weights ws."""
    from industrial_nnmpc_2021_amd.train import HipGroupTrainer
    tr = HipGroupTrainer(Ws, nx, nu, nnwithuprev=True, max_batch=max_batch, lr=LR, betas=(B1, B2), eps=EPS,
                         **({} if ws is None else {"tangents": True}))
    tr.set_data(d)
    if ws is not None:
        if tangents:
            tr.set_tangents(d)
        tr.set_tan_weights(ws)
    return tr


def _run_single(W, w, d, perms, batch=BATCH, max_batch=MAX_BATCH):
    """Per epoch (bytes, loss, (mse, tan_mse)), then the validation (loss, parts) of one member's own handle."""
    tr = _single(W, w, d, max_batch)
    try:
        out = []
        for p in perms:
            loss = tr.epoch(p, batch)
            out.append((_bytes(tr.get_weights()), loss, tr.last_losses()))
        val = tr.eval(*EVAL)
        return out, (val, tr.last_losses())
    finally:
        tr.close()


def _run_group(Ws, ws, d, perms, batch=BATCH, max_batch=MAX_BATCH, device_tangents=False):
    """The same per member from one group (perms[ep][g]), and per epoch its launches; the padding after the epochs."""
    from industrial_nnmpc_2021_amd import _lib
    G = len(Ws)
    tr = _group(Ws, ws, d, max_batch, tangents=not device_tangents)
    bufs = {}
    try:
        if device_tangents:
            bufs = {k: _lib.DeviceArray.from_host(np.ascontiguousarray(d[k], np.float64)) for k in ("dx", "duprev", "du")}
            tr.set_tangents_device(d["x"].shape[0], bufs["dx"], bufs["duprev"], bufs["du"])
        out, launches = [[] for _ in Ws], []
        for ep in perms:
            loss = tr.epoch(ep, batch)
            launches.append(tr.last_launches())
            mse, tan = tr.last_losses()
            for g in range(G):
                out[g].append((_bytes(tr.get_weights(g)), loss[g], (mse[g], tan[g])))
        pad = tr.padding_max()
        val = tr.eval([EVAL[0]] * G, [EVAL[1]] * G)
        mse, tan = tr.last_losses()
        return out, [(val[g], (mse[g], tan[g])) for g in range(G)], launches, pad
    finally:
        tr.close()
        for v in bufs.values():
            v.free()


@functools.lru_cache(maxsize=None)
def _singles(key):
    Ws, d, perms = _scene()
    return [_run_single(Ws[key][g], GROUPS[key][1][g], d, [perms[key][0][g], perms[key][1][g]]) for g in range(2)]


@functools.lru_cache(maxsize=None)
def _tan_group(key, ws=None):
    Ws, d, perms = _scene()
    return _run_group(Ws[key], GROUPS[key][1] if ws is None else ws, d, perms[key])


@functools.lru_cache(maxsize=None)
def _plain_group(key):
    Ws, d, perms = _scene()
    return _run_group(Ws[key], None, d, perms[key])


@pytest.mark.parametrize("key", sorted(GROUPS))
def test_members_equal_single_handles_bit_for_bit(key):
    """1.  Two epochs with per-member permutations, then an eval: weights, epoch losses and the parts of last_losses."""
    from industrial_nnmpc_2021_amd.train import group_schedule
    assert [s[-1] for s in group_schedule(GROUPS["A"][2] + GROUPS["B"][2], BATCH)] == [88, 77, 1, 37]
    assert [len(s) for s in group_schedule(GROUPS["A"][2] + GROUPS["B"][2], BATCH)] == [5, 3, 2, 1]
    Ws, d, perms = _scene()
    out, val, launches, pad = _tan_group(key)
    for g, (sout, sval) in enumerate(_singles(key)):
        w = GROUPS[key][1][g]
        for ep in range(2):
            print(f"[tan group {key}] member {g} (w {w}) epoch {ep}: L {out[g][ep][1]!r} parts {out[g][ep][2]}; single {sout[ep][1]!r} {sout[ep][2]}")
            assert out[g][ep][0] == sout[ep][0], (g, ep)
            assert out[g][ep][1] == sout[ep][1], (g, ep)
            assert out[g][ep][2] == sout[ep][2], (g, ep)
        assert val[g] == sval, g
        assert out[g][0][0] != out[g][1][0] and out[g][0][0] != _bytes(Ws[key][g])         # and it trained
        mse, tan = out[g][1][2]
        if w > 0:
            assert tan > 0 and abs(out[g][1][1] - (mse + w * tan)) <= 2.0 ** -40 * out[g][1][1]
        else:
            assert tan == 0.0 and mse == out[g][1][1]


@pytest.mark.parametrize("key", sorted(GROUPS))
def test_all_weights_zero_gives_the_plain_groups_bytes_and_launches(key):
    """2.  A tangent group with the tangents loaded and w = 0 everywhere is the plain group, launch for launch."""
    zero, plain = _tan_group(key, (0.0, 0.0)), _plain_group(key)
    assert zero[0] == plain[0] and zero[1] == plain[1]
    assert zero[2] == plain[2]
    if key == "B":                                      # one tile class per layer: 6 L launches per lock-step step, 2 steps
        assert plain[2] == [6 * 4 * 2] * 2


@pytest.mark.parametrize("key", sorted(GROUPS))
def test_it_is_a_group(key):
    """3.  The launches of an epoch are the plain group's on the same members and rows: all members with the tangent rows
    (group A as it is; group B at w = 1 for both) and mixed (group B as it is)."""
    plain = _plain_group(key)[2]
    assert _tan_group(key)[2] == plain
    if key == "B":
        assert _tan_group(key, (1.0, 1.0))[2] == plain


def test_padding_stays_zero_and_device_tangents_match_host_tangents():
    """9."""
    for key in sorted(GROUPS):
        assert _tan_group(key)[3] == 0.0
    Ws, d, perms = _scene()
    dev = _run_group(Ws["A"], GROUPS["A"][1], d, perms["A"], device_tangents=True)
    assert dev == _tan_group("A")


def test_exact_case():
    """4.  eval over the 64 rows equals the int64 result (==); the w = 0 member gives the mse alone.  After one epoch of one
    64-row batch a w = 0.5 member holds the weights of a single tangent handle stepped on the same rows, whose gradient
    tests/test_tan_train_gpu.py::test_exact_case proves exact."""
    for names, ws in ((("narrow",), (0.5,)), (("wide", "wide"), (0.5, 0.0))):
        cases = [H.exact_case(n) for n in names]
        d, rows = cases[0][1], cases[0][2]
        G = len(names)
        ref = [H.exact_int(Wk, d, rows) for Wk, _, _ in cases]
        assert all(r[4] < 2 ** 24 for r in ref)
        tr = _group([c[0] for c in cases], ws, d, max_batch=H.EX_B, nx=H.EX_NX, nu=H.EX_NU)
        try:
            L = tr.eval([0] * G, [H.EX_B] * G)
            mse, tan = tr.last_losses()
            for g in range(G):
                want = (ref[g][0], ref[g][1], ref[g][2]) if ws[g] > 0 else (ref[g][1], ref[g][1], 0.0)
                assert (L[g], mse[g], tan[g]) == want, (names[g], ws[g])
            tr.epoch([rows] * G, H.EX_B)
            for g in range(G):
                one = _single(cases[g][0], ws[g], d, max_batch=H.EX_B, nx=H.EX_NX, nu=H.EX_NU)
                try:
                    one.step(rows)
                    assert _bytes(tr.get_weights(g)) == _bytes(one.get_weights()), (names[g], ws[g])
                finally:
                    one.close()
            assert tr.padding_max() == 0.0
        finally:
            tr.close()


def test_five_lock_step_steps_follow_the_float64_trajectory():
    """5.  Independent of the single handle.  Two members on the kink-free rows of tan_helpers' case (a): all 200, and the
    first 72 (another padded batch, another trajectory).  Six one-batch epochs: the sixth returns L, mse and tan_mse at the
    weights after five steps.  Protocol and bar of test_tan_train_gpu.test_five_steps_follow_the_float64_trajectory: the
    float32 reference takes the float64 reference's side of every kink at every step, and the error is <= 8 x the float32
    trajectory's own, measured here with that test's helpers."""
    import torch
    from tests import test_tan_train_gpu as T
    nx, nu, uprev, hidden, B = H.CASES["a"]
    Wk, d, rows = T._case("a")
    w, steps = H.W_TAN, 5
    lists = [rows, rows[:72]]
    refs = []
    for r in lists:
        r64, m64, s64 = T._adam_run(Wk, uprev, d, r, steps, torch.float64)
        r32, m32, s32 = T._adam_run(Wk, uprev, d, r, steps, torch.float32)
        assert len(s64) == steps and all(np.array_equal(a, b) for a, b in zip(s32, s64))
        refs.append((r64, r32))
    tr = _group([Wk, Wk], (w, w), d, max_batch=B, nx=nx, nu=nu)
    try:
        for _ in range(steps + 1):
            L = tr.epoch(lists, B)
        mse, tan = tr.last_losses()
    finally:
        tr.close()
    for g, (r64, r32) in enumerate(refs):
        for what, got, i in (("L", L[g], 0), ("tan_mse", tan[g], 2)):
            e, e32 = abs(got - r64[i]) / r64[i], abs(r32[i] - r64[i]) / r64[i]
            print(f"[group trajectory] member {g} {what} {r64[i]:.6e}: hip {e:.2e}, torch f32 {e32:.2e}, bar {8 * e32:.2e}")
            assert e <= 8 * e32, (g, what, e, e32)
        assert L[g] < H.ref_loss_grad(Wk, uprev, d, lists[g], w)[0]                         # and it went down


def test_several_dw_slices(monkeypatch):
    """6.  NNMPC_TRAIN_DW_SLICES=3 at B = 600 of max_batch 640: three slices of the 1920 stacked rows of a member with the
    tangent rows, of the 1280 of the plain one.  Bytes equal the singles built under the same setting."""
    monkeypatch.setenv("NNMPC_TRAIN_DW_SLICES", "3")
    Ws, d, _ = _scene()
    perm = np.random.default_rng(9).permutation(600)
    for key in sorted(GROUPS):
        ws = GROUPS[key][1]
        tr = _group(Ws[key], ws, d, max_batch=640)
        try:
            loss = tr.epoch([perm, perm], 600)
            parts = tr.last_losses()
            for g in range(2):
                one = _single(Ws[key][g], ws[g], d, max_batch=640)
                try:
                    assert one.epoch(perm, 600) == loss[g]
                    assert one.dw_slices() == [3] * (len(GROUPS[key][0][g]) + 1)
                    assert one.last_losses() == (parts[0][g], parts[1][g])
                    assert _bytes(one.get_weights()) == _bytes(tr.get_weights(g)), (key, g)
                finally:
                    one.close()
        finally:
            tr.close()


def test_nan_stays_local():
    """7.  A NaN in dx of dataset row 10.  Members (all [70, 130, 70]): w 0 on rows 0..128, w 1 on rows 0..36, w 1 on rows
    40..100.  Only the second gets a NaN tan_mse, L and weights; the others are finite and hold the bytes of the clean run."""
    Ws, d, _ = _scene()
    W3 = [Ws["B"][0], Ws["B"][1], Ws["B"][1]]
    ws = (0.0, 1.0, 1.0)
    lists = [np.random.default_rng(1).permutation(129), np.random.default_rng(2).permutation(37),
             40 + np.random.default_rng(3).permutation(61)]
    bad = dict(d, dx=d["dx"].copy())
    bad["dx"][10, 1] = np.nan
    runs = []
    for data in (d, bad):
        tr = _group(W3, ws, data)
        try:
            L = tr.epoch(lists, BATCH)
            mse, tan = tr.last_losses()
            runs.append((L, mse, tan, [tr.get_weights(g) for g in range(3)]))
        finally:
            tr.close()
    clean, (L, mse, tan, Wn) = runs
    assert np.isnan(L[1]) and np.isnan(tan[1]) and np.isfinite(mse[1])
    assert all(np.isnan(a).any() for a in Wn[1] if a.ndim == 2)                            # (the tangent rows carry no bias gradient)
    for g in (0, 2):
        assert np.isfinite(L[g]) and np.isfinite(tan[g]) and all(np.isfinite(a).all() for a in Wn[g])
        assert (L[g], mse[g], tan[g]) == (clean[0][g], clean[1][g], clean[2][g])
        assert _bytes(Wn[g]) == _bytes(clean[3][g])
    assert np.isfinite(clean[0][1]) and all(np.isfinite(a).all() for a in clean[3][1])


def test_edges_launch_nothing():
    """8.  NNMPC_EINVAL with a message, and the weights afterwards are those from before."""
    from industrial_nnmpc_2021_amd.train import HipGroupTrainer
    from tests.test_tan_train_gpu import _einval
    Ws, d, perms = _scene()
    W, n = Ws["B"], d["x"].shape[0]
    rows = [perms["B"][0][0], perms["B"][0][1]]
    plain = _group(W, None, d)
    try:
        before = [_bytes(plain.get_weights(g)) for g in range(2)]
        _einval(lambda: plain.set_tan_weights([0.5, 0.5]), "nnmpc_train_set_group_tan_weights")
        _einval(lambda: plain.set_tangents(d), "nnmpc_train_set_group_tangents")
        _einval(lambda: plain.last_losses(), "nnmpc_train_last_group_losses")
        assert [_bytes(plain.get_weights(g)) for g in range(2)] == before
        loss = plain.epoch(rows, BATCH)
        assert plain.last_losses() == (loss, [0.0, 0.0])                                    # a plain group: mse is the loss
    finally:
        plain.close()
    tr = HipGroupTrainer(W, NX, NU, nnwithuprev=True, max_batch=MAX_BATCH, lr=LR, betas=(B1, B2), eps=EPS, tangents=True)
    try:
        _einval(lambda: tr.set_tangents(d), "nnmpc_train_set_group_tangents")               # before set_data
        _einval(lambda: tr.last_losses(), "nnmpc_train_last_group_losses")                  # before any epoch or eval
        tr.set_data(d)
        _einval(lambda: tr.set_tangents({k: v[:n - 1] for k, v in d.items()}), "nnmpc_train_set_group_tangents")
        _einval(lambda: tr.set_tangents({k: v for k, v in d.items() if k != "duprev"}), "nnmpc_train_set_group_tangents")
        for w in (-0.5, float("nan"), float("inf")):
            _einval(lambda: tr.set_tan_weights([0.5, w]), "nnmpc_train_set_group_tan_weights")
        with pytest.raises(ValueError, match="entries for a group of 2"):
            tr.set_tan_weights([0.5])
        before = [_bytes(tr.get_weights(g)) for g in range(2)]
        tr.set_tan_weights([0.0, 0.5])

        def refused():                                                                      # a weight > 0 and no tangents
            _einval(lambda: tr.epoch(rows, BATCH), "nnmpc_train_group_epoch")
            _einval(lambda: tr.eval([EVAL[0]] * 2, [EVAL[1]] * 2), "nnmpc_train_group_eval")
            assert [_bytes(tr.get_weights(g)) for g in range(2)] == before

        refused()
        _einval(lambda: tr.last_losses(), "nnmpc_train_last_group_losses")                  # the refused calls were none
        tr.set_tan_weights([0.0, 0.0])                                                      # the rejected entries changed nothing: all 0 runs
        assert all(np.isfinite(v) for v in tr.eval([EVAL[0]] * 2, [EVAL[1]] * 2))
        tr.set_tan_weights([0.0, 0.5])
        tr.set_tangents(d)
        L = tr.eval([EVAL[0]] * 2, [0, EVAL[1]])                                            # a member without rows: NaN, in both parts
        mse, tan = tr.last_losses()
        assert np.isnan(L[0]) and np.isnan(mse[0]) and np.isnan(tan[0]) and tan[1] > 0 and L[1] > mse[1]
        tr.set_data(d)                                                                      # drops the tangents
        refused()
    finally:
        tr.close()


def test_train_nn_controllers_with_tan_weights_equals_separate_fits():
    """10.  A sweep of three through one tangent group: weights and histories of separate train_nn_controller(backend="hip",
    tan_weight=w_i) fits on the first num_samples[i] rows."""
    import torch
    from industrial_nnmpc_2021_amd import train
    _, d, _ = _scene()
    torch.manual_seed(5)
    models = [train.RegulatorModel(NX, NU, [None] + h + [NU]) for h in ([40, 64], [128, 128], [70, 64])]
    ws, ns = [0.3, 0.0, 1.7], [300, 200, 129]           # no powers of two: (float)(gscale w) differs from (float)gscale (float)w
    kw = dict(epochs=3, batch_size=128, validation_split=0.05, lr=LR, seed=4)
    singles = []
    for m, w, n in zip(models, ws, ns):
        part = {k: v[:n] for k, v in d.items()}
        sm, _, hist = train.train_nn_controller(copy.deepcopy(m), part, backend="hip", tan_weight=w, **kw)
        singles.append((_bytes(sm.get_weights()), hist))
    start = [_bytes(m.get_weights()) for m in models]
    out, ttime, hists = train.train_nn_controllers([copy.deepcopy(m) for m in models], d, num_samples=ns, tan_weights=ws,
                                                   backend="hip", **kw)
    for i in range(3):
        assert _bytes(out[i].get_weights()) == singles[i][0] != start[i], i
        assert hists[i] == singles[i][1] and len(hists[i]) == 3, i
