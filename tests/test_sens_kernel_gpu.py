"""sens_k (csrc/qp_sens.h) and its driver through nnmpc_qp_sensitivity, entry by entry.

Exact cases (tests/sens_helpers.exact_case; tests/test_cpu_sens_inputs.py holds the table to its claims): P = diag(4^e) with integer
tq and perturbations, installed with its exact inverse pair, so every pivot, square root, quotient and product is exact and every
entry of du, dmult and the first moves must EQUAL the dyadic result -- every shape, B in {1, 5, 129}, D in {1, 3, 8, 9, 17}, both
out_kinds, host and device pointers, every set family of the shape (sizes 0 .. 768 on both sides of 160 | 161, one of 784 and one of
1028 bounds that must come back as flag 1 with NaN rows).  The buffers hold a sentinel and one row more than the call writes.

Real cases (seeded SPD P, cond ~ 1e3, the pair installed with set_inverse so that the float64 route sens_route_f64 uses the very same
Hinv and Kunc): per set size, the active entries of du are the copied perturbations bit for bit, and on the free rows
|P du + tq dx0| <= tol scale with scale = |P| |du| + |tq| |dx0| and tol = 8 x the ratio the float64 route attains on the same case,
floor 64 2^-53 (n + n_aug) (8: a different summation order and a different factorisation order against LAPACK's).  The first-move
output, put in place of the first nu columns of the sequence, meets the same bound.  dmult is the multiplier kernel's own result on
(dx0, du): within mult_bound of the definition.

Flags and arguments: flag 2 for status 2, both bits of one variable and a NaN in one direction, NaN rows, neighbours' bytes
unchanged; B = 0; D = 0; dmult with FIRST_MOVE; a handle without an inverse; independence of the batch position; the instance a set
size runs in, from nnmpc_qp_get_stats (sens_lds_problems / sens_slab_problems).
"""
import ctypes as C

import numpy as np
import pytest

from tests import mult_helpers as M
from tests import sens_helpers as S

pytestmark = pytest.mark.gpu

_HANDLES = {}
_REAL = {}


@pytest.fixture(scope="module")
def handles():
    yield _HANDLES
    for h in _HANDLES.values():
        h.close()
    _HANDLES.clear()
    _REAL.clear()


def handle(handles, kind, shape):
    """A handle of the exact or the real matrices of a shape, the pair installed with set_inverse."""
    if (kind, shape) not in handles:
        from industrial_nnmpc_2021_amd.qp import BatchedBoxQP
        n, nu, n_aug = shape
        mats = S.exact_matrices(*shape) if kind == "exact" else S.real_matrices(*shape)
        qp = BatchedBoxQP(mats["P"].astype(np.float64), mats["tq"].astype(np.float64), nu, Kunc=None, max_batch=128, seg_max=128)
        assert qp.set_inverse(mats["Hinv"], mats["Kunc"]) == 0
        handles[(kind, shape)] = qp
    return handles[(kind, shape)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def call(qp, words, dx0, dlb, dub, status=None, first=False, dmult=True, device=False, flag=True):
    """nnmpc_qp_sensitivity; every output buffer holds the sentinel and one row (one problem) more than the call writes.
    Returns (rc, du (B + 1, D, ncol), dmult (B + 1, D, n) or None, flag (B + 1,))."""
    from industrial_nnmpc_2021_amd import _lib
    B, D = dx0.shape[:2]
    ncol = qp.nu if first else qp.n
    du = np.full((B + 1, D, ncol), S.SENTINEL)
    dm = np.full((B + 1, D, qp.n), S.SENTINEL) if dmult else None
    fl = np.full(B + 1, -9, np.int32) if flag else None
    ins = [np.ascontiguousarray(words, np.uint32), None if status is None else np.ascontiguousarray(status, np.int32),
           np.ascontiguousarray(dx0), None if dlb is None else np.ascontiguousarray(dlb), None if dub is None else np.ascontiguousarray(dub)]
    kind = _lib.OUT_FIRST_MOVE if first else _lib.OUT_SEQUENCE
    if not device:
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        rc = qp._lib.nnmpc_qp_sensitivity(qp._h, B, D, *(p(a) for a in ins), p(du), p(dm), p(fl), _lib.HOST, kind)
        return rc, du, dm, fl
    DA = _lib.DeviceArray
    bufs = [None if a is None else DA.from_host(a) for a in ins + [du, dm, fl]]
    p = lambda a: None if a is None else C.c_void_p(a.data_ptr())
    rc = qp._lib.nnmpc_qp_sensitivity(qp._h, B, D, *(p(b) for b in bufs), _lib.DEVICE, kind)
    du, dm, fl = (None if b is None else b.to_host() for b in bufs[5:])
    for b in bufs:
        if b is not None:
            b.free()
    return rc, du, dm, fl


def equal_or_both_nan(got, want):
    return (got == want) | (np.isnan(got) & np.isnan(want))


@pytest.mark.parametrize("D", S.DIRECTIONS)
@pytest.mark.parametrize("B", S.BATCHES)
@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: "n%d_nu%d_aug%d" % s)
def test_exact_cases_entry_by_entry(handles, shape, B, D):
    n, nu, n_aug = shape
    qp = handle(handles, "exact", shape)
    c = S.exact_case(n, nu, n_aug, B, D)
    rc, du, dm, fl = call(qp, c["words"], c["dx0"], c["dlb"], c["dub"])
    assert rc == 0, qp._lib.nnmpc_last_error()
    sizes = S.set_size(c["words"], n, nu)
    bad_du, bad_dm = ~equal_or_both_nan(du[:B], c["du"]), ~equal_or_both_nan(dm[:B], c["dmult"])
    print(f"n {n} B {B} D {D}: sets {sorted(set(sizes.tolist()))}, {int(bad_du.sum())} entries of du and {int(bad_dm.sum())} of dmult differ, "
          f"flags {np.bincount(fl[:B], minlength=4).tolist()}")
    assert np.array_equal(fl[:B], c["flag"]) and fl[B] == -9
    assert not bad_du.any(), np.argwhere(bad_du)[:4]
    assert not bad_dm.any(), np.argwhere(bad_dm)[:4]
    free = np.broadcast_to((M.sides(c["words"], n, nu) == 0)[:, None, :], dm[:B].shape) & (c["flag"] == 0)[:, None, None]
    assert (dm[:B][free].view(np.uint64) == 0).all()                            # +0.0 on the free variables, bit for bit
    assert (du[B] == S.SENTINEL).all() and (dm[B] == S.SENTINEL).all()          # the rows behind the batch keep their bytes
    # first moves: the first stage of the same result
    rc, d0, _, f0 = call(qp, c["words"], c["dx0"], c["dlb"], c["dub"], first=True, dmult=False)
    assert rc == 0 and np.array_equal(f0[:B], c["flag"])
    assert equal_or_both_nan(d0[:B], c["du"][:, :, :nu]).all(), np.argwhere(~equal_or_both_nan(d0[:B], c["du"][:, :, :nu]))[:4]
    assert (d0[B] == S.SENTINEL).all()
    # device pointers: the same bytes, both kinds
    rc, du_d, dm_d, fl_d = call(qp, c["words"], c["dx0"], c["dlb"], c["dub"], device=True)
    assert rc == 0 and same_bits(du_d, du) and same_bits(dm_d, dm) and same_bits(fl_d, fl)
    rc, d0_d, _, f0_d = call(qp, c["words"], c["dx0"], c["dlb"], c["dub"], first=True, dmult=False, device=True)
    assert rc == 0 and same_bits(d0_d, d0) and same_bits(f0_d, f0)


def test_null_bound_perturbations_are_zeros(handles):
    shape = S.SHAPES[3]
    n, nu, n_aug = shape
    qp = handle(handles, "exact", shape)
    c = S.exact_case(n, nu, n_aug, 5, 3)
    zero = np.zeros_like(c["dlb"])
    _, du0, dm0, _ = call(qp, c["words"], c["dx0"], zero, zero)
    rc, du1, dm1, fl1 = call(qp, c["words"], c["dx0"], None, None, flag=False)
    assert rc == 0 and fl1 is None and same_bits(du0, du1) and same_bits(dm0, dm1)
    act = np.broadcast_to((M.sides(c["words"], n, nu) > 0)[:, None, :], du1[:5].shape)
    assert (du1[:5][act].view(np.uint64) == 0).all()                            # copied: +0.0


def real_run(handles, m, shape):
    """One GPU call and the float64 route of a real case, shared by the tests."""
    if (m, shape) not in _REAL:
        n, nu, n_aug = shape
        qp = handle(handles, "real", shape)
        mats = S.real_matrices(*shape)
        c = S.real_case(m, shape)
        qp.stats(reset=True)
        rc, du, dm, fl = call(qp, c["words"], c["dx0"], c["dlb"], c["dub"])
        st = qp.stats()
        assert rc == 0, qp._lib.nnmpc_last_error()
        rc0, d0, _, f0 = call(qp, c["words"], c["dx0"], c["dlb"], c["dub"], first=True, dmult=False)
        assert rc0 == 0
        route = S.sens_route_f64(mats["Hinv"], mats["Kunc"], c["words"], c["dx0"], c["dlb"], c["dub"], nu)
        _REAL[(m, shape)] = dict(c=c, mats=mats, du=du, dm=dm, fl=fl, d0=d0, f0=f0, route=route, stats=st)
    return _REAL[(m, shape)]


@pytest.mark.parametrize("m,shape", S.real_case_table(), ids=lambda v: str(v) if isinstance(v, int) else "n%d" % v[0])
def test_real_cases_free_rows_and_copied_bounds(handles, m, shape):
    n, nu, n_aug = shape
    r = real_run(handles, m, shape)
    c, mats, B = r["c"], r["mats"], S.REAL_B
    P, tq = mats["P"], mats["tq"]
    du = r["du"][:B]
    assert (r["fl"][:B] == 0).all() and (r["f0"][:B] == 0).all() and np.isfinite(du).all()
    assert (r["du"][B] == S.SENTINEL).all() and (r["dm"][B] == S.SENTINEL).all() and (r["d0"][B] == S.SENTINEL).all()
    pert = S.tile_pert(c["dlb"], c["dub"], c["words"], n, nu)
    act = ~np.isnan(pert)
    assert same_bits(du[act], pert[act])                                        # copied, bit for bit
    ratio_ref = S.free_ratio(P, tq, c["words"], c["dx0"], r["route"], nu)
    ratio_gpu = S.free_ratio(P, tq, c["words"], c["dx0"], du, nu)
    tol = max(8 * ratio_ref, S.FLOOR * (n + n_aug))
    inst = "lds" if m <= S.M_LDS else "slab"
    print(f"m {m} n {n} {inst}: free residual / scale  gpu {ratio_gpu:.3g}  float64 route {ratio_ref:.3g}  tol {tol:.3g}")
    assert ratio_gpu <= tol
    # the instance
    st = r["stats"]
    assert (st["sens_lds_problems"], st["sens_slab_problems"]) == ((B, 0) if m <= S.M_LDS else (0, B))
    # first moves: put in place of the sequence's first stage they meet the same bound on every free row
    d0 = r["d0"][:B]
    a0 = act[:, :, :nu]
    assert same_bits(d0[a0], pert[:, :, :nu][a0])
    spliced = du.copy()
    spliced[:, :, :nu] = d0
    ratio_first = S.free_ratio(P, tq, c["words"], c["dx0"], spliced, nu)
    print(f"m {m} n {n} {inst}: with the first-move output in place {ratio_first:.3g}, max |first move - sequence| "
          f"{float(np.abs(d0 - du[:, :, :nu]).max()):.3g}")
    assert ratio_first <= tol
    # dmult: the multiplier definition on (dx0, du)
    ref = S.dmult_ref(P, tq, c["words"], c["dx0"], du, nu)
    bound = M.mult_bound(P, tq, c["dx0"].reshape(B * S.REAL_D, -1), du.reshape(B * S.REAL_D, n)).reshape(ref.shape)
    assert (np.abs(r["dm"][:B] - ref) <= bound).all()
    assert (r["dm"][:B][~act].view(np.uint64) == 0).all()


def test_flags_and_unaffected_neighbours(handles):
    shape = S.SHAPES[4]
    n, nu, n_aug = shape
    qp = handle(handles, "real", shape)
    c = S.real_case(63, shape)
    B = S.REAL_B
    rc, du, dm, fl = call(qp, c["words"], c["dx0"], c["dlb"], c["dub"])
    assert rc == 0 and (fl[:B] == 0).all()
    words, dx0, status = c["words"].copy(), c["dx0"].copy(), np.zeros(B, np.int32)
    status[0] = 1                                                               # not certified, but computed like any other row
    status[1] = 2
    up, lo = M.row_index(n, nu)
    i = n // 2
    for bit in (up[i], lo[i]):
        words[2, bit // 32] |= np.uint32(1 << (bit % 32))
    dx0[3, 4, n_aug - 1] = np.nan                                               # one direction of one problem
    for first in (False, True):
        base = call(qp, c["words"], c["dx0"], c["dlb"], c["dub"], first=first, dmult=not first)
        rc, du2, dm2, fl2 = call(qp, words, dx0, c["dlb"], c["dub"], status=status, first=first, dmult=not first)
        assert rc == 0 and fl2.tolist() == [0, 2, 2, 2, 0, -9]
        assert np.isnan(du2[1:4]).all() and (first or np.isnan(dm2[1:4]).all())
        for k in (0, 4, 5):
            assert same_bits(du2[k], base[1][k]) and (first or same_bits(dm2[k], base[2][k]))
        dev = call(qp, words, dx0, c["dlb"], c["dub"], status=status, first=first, dmult=not first, device=True)
        assert dev[0] == 0 and same_bits(dev[1], du2) and same_bits(dev[3], fl2) and (first or same_bits(dev[2], dm2))
    # a NaN in a bound perturbation, and an infinite one
    for name in ("dlb", "dub"):
        pert = {k: c[k].copy() for k in ("dlb", "dub")}
        pert[name][4, 0, 0] = np.inf if name == "dlb" else np.nan
        rc, du3, _, fl3 = call(qp, c["words"], c["dx0"], pert["dlb"], pert["dub"])
        assert rc == 0 and fl3.tolist() == [0, 0, 0, 0, 2, -9] and np.isnan(du3[4]).all() and same_bits(du3[:4], du[:4])


def test_flag_1_beyond_the_ceiling(handles):
    shape = S.SHAPES[-1]
    n, nu, n_aug = shape
    qp = handle(handles, "real", shape)
    rng = np.random.default_rng(3)
    rows = np.array([S.family_rows("head", m, n, nu, rng) for m in (S.M_MAX, S.M_OVER, 17)])
    words = M.pack_rows(rows, n)
    dx0, dlb, dub = rng.standard_normal((3, 2, n_aug)), rng.standard_normal((3, 2, nu)), rng.standard_normal((3, 2, nu))
    qp.stats(reset=True)
    rc, du, dm, fl = call(qp, words, dx0, dlb, dub)
    st = qp.stats()
    assert rc == 0 and fl.tolist() == [0, 1, 0, -9]
    assert np.isnan(du[1]).all() and np.isnan(dm[1]).all() and np.isfinite(du[[0, 2]]).all() and np.isfinite(dm[[0, 2]]).all()
    assert (st["sens_lds_problems"], st["sens_slab_problems"]) == (2, 1)        # (a set beyond the ceiling is flagged by the LDS instance)
    rc, d0, _, f0 = call(qp, words, dx0, dlb, dub, first=True, dmult=False)
    assert rc == 0 and f0.tolist() == [0, 1, 0, -9] and np.isnan(d0[1]).all() and np.isfinite(d0[[0, 2]]).all()


def test_instance_choice_at_the_hand_over(handles):
    shape = S.SHAPES[4]
    n, nu, n_aug = shape
    qp = handle(handles, "real", shape)
    rng = np.random.default_rng(4)
    for m, want in ((S.M_LDS, (3, 0)), (S.M_LDS + 1, (0, 3))):
        rows = np.array([S.family_rows(k, m, n, nu, rng) for k in S.KINDS])
        qp.stats(reset=True)
        qp.set_profiling(True)
        out = qp.sensitivity(M.pack_rows(rows, n), rng.standard_normal((3, n_aug)))
        qp.set_profiling(False)
        st = qp.stats()
        print(m, {k: st[k] for k in ("sens_lds_problems", "sens_slab_problems", "sens_launches", "sens_ms")})
        assert (st["sens_lds_problems"], st["sens_slab_problems"]) == want and st["sens_launches"] == 1 and st["sens_ms"] > 0
        assert out["du"].shape == (3, n) and (out["flag"] == 0).all()           # one direction: the axis is dropped


def test_arguments(handles):
    from industrial_nnmpc_2021_amd import _lib
    from industrial_nnmpc_2021_amd.qp import BatchedBoxQP
    shape = S.SHAPES[1]
    n, nu, n_aug = shape
    qp = handle(handles, "real", shape)
    c = S.real_case(15, shape)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    w, dx0 = c["words"], c["dx0"]
    du, dm, fl = np.full((S.REAL_B, S.REAL_D, n), S.SENTINEL), np.full((S.REAL_B, S.REAL_D, n), S.SENTINEL), np.full(S.REAL_B, -9, np.int32)
    f = qp._lib.nnmpc_qp_sensitivity
    assert f(qp._h, 0, S.REAL_D, p(w), None, p(dx0), None, None, p(du), p(dm), p(fl), _lib.HOST, _lib.OUT_SEQUENCE) == 0
    assert (du == S.SENTINEL).all() and (dm == S.SENTINEL).all() and (fl == -9).all()     # B = 0: nothing written
    for args in ((S.REAL_B, 0, p(w), None, p(dx0), None, None, p(du), p(dm), p(fl), _lib.HOST, _lib.OUT_SEQUENCE),       # D = 0
                 (S.REAL_B, S.REAL_D, None, None, p(dx0), None, None, p(du), None, None, _lib.HOST, _lib.OUT_SEQUENCE),
                 (S.REAL_B, S.REAL_D, p(w), None, None, None, None, p(du), None, None, _lib.HOST, _lib.OUT_SEQUENCE),
                 (S.REAL_B, S.REAL_D, p(w), None, p(dx0), None, None, None, None, None, _lib.HOST, _lib.OUT_SEQUENCE),
                 (S.REAL_B, S.REAL_D, p(w), None, p(dx0), None, None, p(du), None, None, 7, _lib.OUT_SEQUENCE),
                 (S.REAL_B, S.REAL_D, p(w), None, p(dx0), None, None, p(du), None, None, _lib.HOST, 7)):
        assert f(qp._h, *args) == _lib.EINVAL
    # dmult with FIRST_MOVE
    assert f(qp._h, S.REAL_B, S.REAL_D, p(w), None, p(dx0), None, None, p(du), p(dm), p(fl), _lib.HOST, _lib.OUT_FIRST_MOVE) == _lib.EINVAL
    assert b"FIRST_MOVE" in qp._lib.nnmpc_last_error()
    with pytest.raises(ValueError):
        qp.sensitivity(w, dx0, first_move_only=True, multipliers=True)
    assert (du == S.SENTINEL).all() and (dm == S.SENTINEL).all() and (fl == -9).all()
    # a handle without an inverse
    mats = S.real_matrices(*shape)
    bare = BatchedBoxQP(mats["P"], mats["tq"], nu, Kunc=None, method="pdip", max_batch=128, seg_max=128)
    try:
        assert f(bare._h, S.REAL_B, S.REAL_D, p(w), None, p(dx0), None, None, p(du), None, None, _lib.HOST, _lib.OUT_SEQUENCE) == _lib.EINVAL
        assert b"nnmpc_qp_set_inverse" in bare._lib.nnmpc_last_error()
        with pytest.raises(_lib.NnmpcError):
            bare.sensitivity(w, dx0)
    finally:
        bare.close()
    assert (du == S.SENTINEL).all()


def test_rows_do_not_depend_on_their_batch(handles):
    """A problem's outputs are the same bytes alone, in the middle of a batch of 129 of mixed families (more than one segment of
    the handle's 128 problems, both instances in one launch list) and with its neighbours exchanged."""
    shape = S.SHAPES[4]
    n, nu, n_aug = shape
    qp = handle(handles, "real", shape)
    fams = S.families(n, nu)
    rng = np.random.default_rng(8)
    B, D = 129, 3
    rows = np.array([S.family_rows(*fams[b % len(fams)], n, nu, rng) for b in range(B)])
    words = M.pack_rows(rows, n)
    dx0, dlb, dub = rng.standard_normal((B, D, n_aug)), rng.standard_normal((B, D, nu)), rng.standard_normal((B, D, nu))
    rc, du, dm, fl = call(qp, words, dx0, dlb, dub)
    assert rc == 0 and (fl[:B] == 0).all()
    perm = rng.permutation(B)
    rc, du_p, dm_p, fl_p = call(qp, words[perm], dx0[perm], dlb[perm], dub[perm])
    assert rc == 0 and same_bits(du_p[:B], du[perm]) and same_bits(dm_p[:B], dm[perm])
    for b in (0, 64, 127, 128):
        rc, du_1, dm_1, fl_1 = call(qp, words[b:b + 1], dx0[b:b + 1], dlb[b:b + 1], dub[b:b + 1])
        assert rc == 0 and same_bits(du_1[0], du[b]) and same_bits(dm_1[0], dm[b]) and fl_1[0] == 0
