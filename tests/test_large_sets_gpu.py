"""Active sets of a CHOSEN size, 16 .. 800 bounds, through every kernel of the shared-inverse active-set pass that factors them.

The pass picks its multiplier-system kernel from the number of active bounds m (thresholds: qp_asm.h, qp_small.h, launch_multipliers in qp_solver.hip):

    m <= 144        asm_lambda_reg32_k  (f32 rounds)   asm_lambda_reg_k    (fp64 solve)
    145 .. 176      asm_lambda_reg32b_k                asm_lambda_wg64s_k
    177 .. 256      asm_lambda_wg32_k                  asm_lambda_wg64_k
    257 .. 384      asm_lambda_wg32b_k                 asm_lambda_wg64r_k  (f32 factor + fp64 refinement; the slab kernel if that gives up)
    385 .. 768      --                                 asm_lambda_tile_k<1> (tiles in an L2 slab, a queue of asm_pool workgroups)
    > asm_max_active: handed over -- method "asm" reports status 1, method "auto" solves it on the PDIP path

asm_tail_k (calls of <= 256 problems) moves its tiles from LDS to the slab beyond 128 bounds; asm_small_k (padded n <= 724) has three
instances that hand over at 32, 112 and 144 bounds.  tests/helpers.py: large_set_problem builds inputs whose optimal set is exactly
the pushed set and whose first set (the bounds x_unc violates) is that set too, so that both the f32 round and the fp64 solve of a
problem run at size m (tests/test_cpu_large_set_inputs.py holds the oracle to it).

The referee of every row is kkt_check (fp64 numpy: feasibility, active variables on their bounds, stationarity on the free set
within 1e-7 max(1, |q|inf), strict multiplier signs): P is positive definite, so a point that passes is the optimum.  On top of it
every row's u is compared with the fp64 solve on the expected set (solve_on_set), two rows per case with the exact oracle.
Tolerances: first family 1e-9 max(1, |x|inf) and bit-equal sets (tests/test_asm_gpu.py's own); strain family (cond(P) = 1e4)
1e-7 max(1, cond / 1e3) = 1e-6 (tests/test_random_shapes_gpu.py's).  Which kernels these tests launch, and what seeded defects they
catch: profiles/large_sets_coverage.md.
"""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

N_, NU, PSEED = 1024, 8, 5
ROUNDS = dict(method="asm", asm_tail_batch=-1, asm_predict_iters=-1)     # the lock-step round kernels, first sets = the bounds x_unc violates
BOUNDARY = [16, 64, 65, 144, 145, 176, 177, 256, 257, 320, 384, 385, 512, 767, 768]
CLASSES = [(0, 144), (145, 176), (177, 256), (257, 384), (385, 768), (769, 10 ** 6)]
TOL = 1e-9


def _cls(m):
    return next(f"{lo}..{hi}" if hi < 10 ** 6 else f">{lo - 1}" for lo, hi in CLASSES if lo <= m <= hi)


@pytest.fixture(scope="module")
def fam():
    """The first family's Hessian and a cache of row sets: rows(sizes, seed) -> (q, lb, ub, state, expected active, optimum x)."""
    P = H.large_set_hessian(N_, PSEED)
    cache = {}

    def rows(sizes, seed):
        key = (tuple(sizes), seed)
        if key not in cache:
            q, lb, ub, state, x = H.pushed_rows(P, NU, seed, sizes, 1.5, 3.0, exact=True)
            cache[key] = (q, lb, ub, state, H.state_to_active(state, NU), x)
        return cache[key]
    return P, rows


@pytest.fixture(scope="module")
def handles(fam):
    """One handle per configuration, made on first use, closed with the module.  seg_max = 4096 (0.4 GB of workspace each, the
    default's pool of 1024 slabs): left at 0 every handle would take a quarter of the HBM that is still free."""
    from industrial_nnmpc_2021_amd.qp import BatchedBoxQP
    made = {}

    def get(P=None, **opts):
        key = (id(P),) + tuple(sorted(opts.items()))
        if key not in made:
            Pm = fam[0] if P is None else P
            made[key] = BatchedBoxQP(Pm, np.eye(Pm.shape[0]), NU, **{"max_batch": 128, "seg_max": 4096, **opts})     # tq = I: q = x0
        return made[key]
    yield get
    for qp in made.values():
        qp.close()


_ORACLE = {}


def _oracle(P, q, lb, ub, key, r):
    if (key, r) not in _ORACLE:
        _ORACLE[(key, r)] = H.oracle_rows(P, q, lb, ub, NU, [r])[0]
    return _ORACLE[(key, r)]


def _solve(qp, q, lb, ub, **kw):
    qp.stats(reset=True)
    out = qp.solve_batch(q, lb, ub, **kw)
    return out, qp.stats()


def _judge(what, P, q, lb, ub, out, state, xref, rows=None, tol=TOL, oracle=(), okey=None, stat_tol=1e-7):
    """The figures of the listed rows (printed per size class before anything is asserted), then: the returned set is the expected
    one bit for bit, u within tol of xref, the fp64 solve on that set (and of the exact oracle on the rows `oracle`), kkt_check."""
    rows = np.arange(q.shape[0]) if rows is None else np.asarray(rows)
    expect = H.state_to_active(state, NU)
    sub = dict(u=out["u"][rows], active=out["active"][rows])
    m = (state[rows] != 0).sum(axis=1)
    uerr = np.abs(out["u"][rows] - xref[rows]).max(axis=1) / np.maximum(1.0, np.abs(xref[rows]).max(axis=1))
    stat = H.kkt_stationarity(P, q[rows], NU, sub)
    wrong = (out["active"][rows] != expect[rows]).sum(axis=1)
    for c in sorted({_cls(v) for v in m}, key=lambda s: int(s.strip(">").split("..")[0])):
        k = np.array([_cls(v) == c for v in m])
        print(f"LARGE_SETS {what} class {c}: rows {int(k.sum())} worst u error {uerr[k].max():.3e} (tol {tol:.0e}) "
              f"worst stationarity {stat[k].max():.3e} (tol {stat_tol:.0e}) wrong bound states {int(wrong[k].sum())}")
    assert (out["active"][rows].sum(axis=1) == m).all(), (what, out["active"][rows].sum(axis=1), m)
    assert (wrong == 0).all(), (what, "rows with a wrong set", rows[wrong > 0], m[wrong > 0])
    assert (uerr <= tol).all(), (what, "worst u error", float(uerr.max()), "set size", int(m[uerr.argmax()]))
    H.kkt_check(P, np.eye(P.shape[0]), NU, P.shape[0] // NU, q[rows], lb[None, :], ub[None, :], sub, stat_tol)
    for r in oracle:
        x, act = _oracle(P, q, lb, ub, okey, r)
        e = np.abs(out["u"][r] - x).max() / max(1.0, np.abs(x).max())
        print(f"LARGE_SETS {what} oracle row {r} ({int(act.sum())} bounds): u error {e:.3e}")
        assert (out["active"][r] == act).all() and e <= tol, (what, r, e)
    return uerr, stat


# ---- boundary sizes through the rounds --------------------------------------------------------------------------------------

@pytest.mark.parametrize("f32_rounds", [0, -1])       # 0: f32 rounds until the set settles, then the fp64 solve; -1: fp64 throughout
def test_boundary_sizes_through_the_rounds(fam, handles, f32_rounds):
    P, rows = fam
    sizes = BOUNDARY * 3
    q, lb, ub, state, _, xref = rows(sizes, 11)
    out, st = _solve(handles(asm_f32_rounds=f32_rounds, **ROUNDS), q, lb, ub)
    print(f"LARGE_SETS rounds f32={f32_rounds}: status {np.bincount(out['status'], minlength=3)} asm_solved {st['asm_solved']} "
          f"factorizations {st['factorizations']} rounds {st['asm_rounds']}")
    assert (out["status"] == 0).all(), (out["status"], sizes)
    assert st["asm_solved"] == len(sizes) and st["factorizations"] == 0 and st["asm_predict_launches"] == 0
    _judge(f"rounds f32={f32_rounds}", P, q, lb, ub, out, state, xref, oracle=(9, 14), okey="boundary")   # rows 9, 14: 320 and 768 bounds


def test_predictor_names_the_first_sets(fam, handles):
    """asm_predict_iters = 0: the first sets inside the leading 512 columns come from the dual predictor instead of x_unc."""
    P, rows = fam
    sizes = BOUNDARY * 3
    q, lb, ub, state, _, xref = rows(sizes, 11)
    ref, _ = _solve(handles(asm_f32_rounds=0, **ROUNDS), q, lb, ub)
    out, st = _solve(handles(method="asm", asm_tail_batch=-1, asm_predict_iters=0), q, lb, ub)
    print(f"LARGE_SETS predictor: status {np.bincount(out['status'], minlength=3)} asm_solved {st['asm_solved']} "
          f"predict launches {st['asm_predict_launches']} rounds {st['asm_rounds']} |du| {np.abs(out['u'] - ref['u']).max():.3e}")
    assert st["asm_predict_launches"] == 1
    assert (out["status"] == 0).all(), (out["status"], sizes)
    assert st["asm_solved"] == len(sizes) and st["factorizations"] == 0
    _judge("predictor", P, q, lb, ub, out, state, xref, oracle=(9, 14), okey="boundary")
    assert np.array_equal(out["active"], ref["active"]) and np.abs(out["u"] - ref["u"]).max() <= TOL


# ---- the hand-over at asm_max_active -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap,at,over", [(0, [768], [769, 800]), (320, [320], [321])])
def test_hand_over_at_the_cap(fam, handles, cap, at, over):
    """Sets of exactly asm_max_active bounds are solved by the pass; one bound more and the problem is handed over: status 1
    from method "asm" (never a status 0 with a wrong answer), the PDIP path's certified optimum from method "auto".  The small
    sets beside them come out bit for bit as in a batch without any over-cap row."""
    P, rows = fam
    capv = cap if cap else 768
    sizes = (at + over + [40, 150]) * 2
    q, lb, ub, state, _, xref = rows(sizes, 13 + cap)
    m = np.array(sizes)
    keep, big = np.flatnonzero(m <= capv), np.flatnonzero(m > capv)
    opts = dict(asm_max_active=cap) if cap else {}
    qa = handles(asm_f32_rounds=0, **ROUNDS, **opts)
    out, st = _solve(qa, q, lb, ub)
    print(f"LARGE_SETS hand-over cap {capv} asm: sizes {sizes} status {out['status']} asm_solved {st['asm_solved']}")
    assert (out["status"][keep] == 0).all() and (out["status"][big] == 1).all(), (out["status"], sizes)
    assert st["asm_solved"] == keep.size and st["factorizations"] == 0
    _judge(f"hand-over cap {capv} asm", P, q, lb, ub, out, state, xref, rows=keep)
    alone, _ = _solve(qa, q[keep], lb, ub)                                 # the same rows in a batch without over-cap rows
    assert (alone["status"] == 0).all()
    assert np.array_equal(alone["u"], out["u"][keep]) and np.array_equal(alone["active"], out["active"][keep])

    qb = handles(method="auto", asm_tail_batch=-1, asm_predict_iters=-1, **opts)
    auto, sa = _solve(qb, q, lb, ub)
    print(f"LARGE_SETS hand-over cap {capv} auto: status {auto['status']} asm_solved {sa['asm_solved']} factorizations {sa['factorizations']}")
    assert (auto["status"] == 0).all(), (auto["status"], sizes)
    assert sa["factorizations"] > 0 and sa["asm_solved"] == keep.size
    assert (auto["factorizations"][keep] == 0).all() and (auto["factorizations"][big] > 0).all()
    # (the PDIP path's answers: certified by its own fp64 polish -- the same 1e-9 against the solve on the expected set, the oracle on
    # one over-cap row of each size)
    _judge(f"hand-over cap {capv} auto", P, q, lb, ub, auto, state, xref, oracle=[int(r) for r in big[:len(over)]], okey=("cap", cap))
    assert np.array_equal(auto["u"][keep], out["u"][keep]) and np.array_equal(auto["active"][keep], out["active"][keep])


# ---- the device tail alone ---------------------------------------------------------------------------------------------------

def test_tail_kernel_alone(fam, handles):
    """A call of <= 256 problems under the default options never sees a round: asm_tail_k from the first set on, tiles in LDS up
    to 128 bounds and in the slab beyond.  Same demands as the rounds, and the rounds' result."""
    P, rows = fam
    sizes = [127, 128, 129, 256, 385, 768, 769] * 2
    q, lb, ub, state, _, xref = rows(sizes, 17)
    m = np.array(sizes)
    keep, big = np.flatnonzero(m <= 768), np.flatnonzero(m > 768)
    out, st = _solve(handles(method="asm"), q, lb, ub)
    print(f"LARGE_SETS tail: status {out['status']} asm_solved {st['asm_solved']} rounds {st['asm_rounds']}")
    assert (out["status"][keep] == 0).all() and (out["status"][big] == 1).all(), (out["status"], sizes)
    assert st["asm_solved"] == keep.size and st["factorizations"] == 0 and st["asm_rounds"] == 1
    _judge("tail", P, q, lb, ub, out, state, xref, rows=keep, oracle=(4, 5), okey="tail")      # rows 4, 5: 385 and 768 bounds
    ref, _ = _solve(handles(asm_f32_rounds=0, **ROUNDS), q, lb, ub)
    assert np.array_equal(ref["status"], out["status"])
    assert np.array_equal(ref["active"][keep], out["active"][keep]) and np.abs(ref["u"][keep] - out["u"][keep]).max() <= 1e-9
    auto, sa = _solve(handles(method="auto"), q, lb, ub)                               # ... and the over-cap rows on the PDIP path
    assert (auto["status"] == 0).all() and sa["factorizations"] > 0 and (auto["factorizations"][keep] == 0).all()
    _judge("tail auto", P, q, lb, ub, auto, state, xref)


# ---- more slab problems than slab workgroups ---------------------------------------------------------------------------------

def test_slab_queue_longer_than_its_pool(fam, handles):
    """seg_max = 2048 gives a pool of 256 slabs: 300 problems of 385 .. 600 bounds in one round make the workgroups of
    asm_lambda_tile_k<1> walk their queue.  Bit-identical to the same rows in batches of 100."""
    P, rows = fam
    sizes = [385 + (r * 215) // 299 for r in range(300)]
    sizes = [sizes[(7 * r) % 300] for r in range(300)]                     # (7 and 300 are coprime: every size once, mixed along the batch)
    q, lb, ub, state, expect, xref = rows(sizes, 19)
    qp = handles(asm_f32_rounds=0, seg_max=2048, max_batch=512, **ROUNDS)
    out, st = _solve(qp, q, lb, ub)
    print(f"LARGE_SETS queue: status {np.bincount(out['status'], minlength=3)} asm_solved {st['asm_solved']} rounds {st['asm_rounds']}")
    assert (out["status"] == 0).all() and st["asm_solved"] == 300 and st["factorizations"] == 0
    _judge("queue", P, q, lb, ub, out, state, xref, oracle=(0,), okey="queue")
    for b0 in (0, 100, 200):
        part, _ = _solve(qp, q[b0:b0 + 100], lb, ub)
        assert (part["status"] == 0).all()
        assert np.array_equal(part["u"], out["u"][b0:b0 + 100]) and np.array_equal(part["active"], out["active"][b0:b0 + 100]), b0


# ---- a caller's guess ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tail", [-1, 0])
def test_warm_start_on_the_expected_set(fam, handles, tail):
    """guess = the optimum's bound states: fp64 from the first round, at size m."""
    P, rows = fam
    sizes = [257, 384, 385, 768] * 2
    q, lb, ub, state, expect, xref = rows(sizes, 23)
    qp = handles(method="asm", asm_tail_batch=tail, asm_predict_iters=-1)
    cold, _ = _solve(qp, q, lb, ub)
    warm, st = _solve(qp, q, lb, ub, guess=qp.active_to_state(expect))
    assert np.array_equal(qp.active_to_state(expect), state)
    print(f"LARGE_SETS warm tail={tail}: status {warm['status']} rounds {st['asm_rounds']} |du| {np.abs(warm['u'] - cold['u']).max():.3e}")
    assert (warm["status"] == 0).all() and (cold["status"] == 0).all() and st["asm_solved"] == len(sizes) and st["factorizations"] == 0
    _judge(f"warm tail={tail}", P, q, lb, ub, warm, state, xref, oracle=(1, 3), okey="warm")
    assert np.array_equal(warm["active"], cold["active"]) and np.abs(warm["u"] - cold["u"]).max() <= 1e-10


# ---- numerical strain ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def strain():
    P, q, lb, ub = H.strain_problem(N_, NU)
    return P, q, lb, ub, H.oracle_rows(P, q, lb, ub, NU, (2, 7))          # 335 and 546 bounds (tests/test_cpu_large_set_inputs.py)


@pytest.mark.parametrize("tail", [-1, 0])
def test_numerical_strain(handles, strain, tail):
    """cond(P) = 1e4, sets a fifth larger than the pushed ones, ill-conditioned multiplier systems: where an f32 factor with fp64
    refinement is strained.  Method "auto" must solve everything below cond 5e4 (tests/test_random_shapes_gpu.py)."""
    P, q, lb, ub, ref = strain
    tol = 1e-7 * max(1.0, H.STRAIN_COND / 1e3)
    out, st = _solve(handles(P=P, method="auto", asm_tail_batch=tail, asm_predict_iters=-1), q, lb, ub)
    nact = out["active"].sum(axis=1)
    print(f"LARGE_SETS strain tail={tail}: status {out['status']} sets {nact} asm_solved {st['asm_solved']} "
          f"factorizations {st['factorizations']} rounds {st['asm_rounds']} full checks {st['asm_full_checks']}")
    stat = H.kkt_stationarity(P, q, NU, out)
    print(f"LARGE_SETS strain tail={tail}: worst stationarity {stat.max():.3e} (tol 1e-07)")
    assert (out["status"] == 0).all(), out["status"]
    H.kkt_check(P, np.eye(N_), NU, N_ // NU, q, lb[None, :], ub[None, :], out, 1e-7)
    for r, (x, act) in zip((2, 7), ref):
        e = np.abs(out["u"][r] - x).max() / max(1.0, np.abs(x).max())
        print(f"LARGE_SETS strain tail={tail} oracle row {r} ({int(act.sum())} bounds): u error {e:.3e} (tol {tol:.0e})")
        assert (out["active"][r] == act).all() and e <= tol, (r, e)
    # every other row against the fp64 solve on its own returned set (certified above)
    state = H.active_to_state(out["active"], NU)
    e = max(np.abs(out["u"][r] - H.solve_on_set(P, q[r], lb, ub, state[r])).max() for r in range(q.shape[0]))
    print(f"LARGE_SETS strain tail={tail}: worst u error against the solve on the returned set {e:.3e} (tol {tol:.0e})")
    assert e <= tol
    assert ((nact >= 257) & (nact <= 384)).sum() >= 3 and ((nact >= 385) & (nact <= 768)).sum() >= 3, nact


def test_refinement_under_an_ill_conditioned_hessian(handles):
    """cond(P) = 1e7, fp64 from the first round: the sets of 257 .. 384 bounds meet asm_lambda_wg64r_k with multiplier systems on
    which an f32 factor is no preconditioner to speak of -- where its refinement gives up and the set goes to the slab kernel
    (round traces of this batch show slab solves of sets below 385 bounds).  Beyond cond 5e4 a problem may exhaust its budget
    (status 1, tests/test_random_shapes_gpu.py); a status 0 must be the optimum: kkt_check, and u within 1e-7 cond / 1e3 of the
    fp64 solve on the returned set."""
    cond = 1e7
    P = H.spd_logspectrum(N_, H.STRAIN_SEED, cond)
    q, lb, ub, _, _ = H.pushed_rows(P, NU, 77, [150, 200, 230, 260, 290, 320], 1.2, 2.0)
    qp = handles(P=P, method="auto", asm_f32_rounds=-1, asm_tail_batch=-1, asm_predict_iters=-1)
    out, st = _solve(qp, q, lb, ub)
    ok = np.flatnonzero(out["status"] == 0)
    sub = dict(u=out["u"][ok], active=out["active"][ok])
    state = H.active_to_state(out["active"], NU)
    e = np.array([np.abs(out["u"][r] - x).max() / max(1.0, np.abs(x).max()) for r, x in ((r, H.solve_on_set(P, q[r], lb, ub, state[r])) for r in ok)])
    print(f"LARGE_SETS cond 1e7: status {out['status']} sets {out['active'].sum(axis=1)} asm_solved {st['asm_solved']} factorizations "
          f"{st['factorizations']} worst stationarity {H.kkt_stationarity(P, q[ok], NU, sub).max(initial=0.0):.3e} (tol 1e-07) "
          f"worst u error {e.max(initial=0.0):.3e} (tol {1e-7 * cond / 1e3:.0e})")
    assert np.isin(out["status"], (0, 1)).all(), out["status"]
    H.kkt_check(P, np.eye(N_), NU, N_ // NU, q[ok], lb[None, :], ub[None, :], sub, 1e-7)
    assert (e <= 1e-7 * cond / 1e3).all(), e
    nact = out["active"][ok].sum(axis=1)
    assert ((nact >= 257) & (nact <= 384)).sum() >= 3, (out["status"], nact)     # the class under test came back solved


# ---- row independence -----------------------------------------------------------------------------------------------------------

def test_rows_do_not_depend_on_their_neighbours(fam, handles):
    """All classes in one batch; permuted and in two halves every problem keeps its u and its set bit for bit."""
    P, rows = fam
    sizes = [16, 100, 144, 145, 160, 176, 177, 220, 256, 257, 300, 384, 385, 500, 768, 769] * 2
    q, lb, ub, state, _, xref = rows(sizes, 29)
    ok = np.array(sizes) <= 768
    for name, qp in (("rounds", handles(asm_f32_rounds=0, **ROUNDS)), ("tail", handles(method="asm"))):
        out, _ = _solve(qp, q, lb, ub)
        assert ((out["status"] == 0) == ok).all() and ((out["status"] == 1) == ~ok).all(), (name, out["status"])
        _judge(f"mixed {name}", P, q, lb, ub, out, state, xref, rows=np.flatnonzero(ok))
        perm = np.random.default_rng(1).permutation(len(sizes))
        h = len(sizes) // 2 - 3
        for sel in (perm, np.arange(0, h), np.arange(h, len(sizes))):
            o2, _ = _solve(qp, q[sel], lb, ub)
            k = ok[sel]                                                      # (a handed-over row has no answer to compare)
            assert np.array_equal(o2["status"], out["status"][sel]), name
            assert np.array_equal(o2["u"][k], out["u"][sel][k]) and np.array_equal(o2["active"][k], out["active"][sel][k]), name


# ---- the one-wave-per-problem kernels at their edges ---------------------------------------------------------------------------

def test_small_kernels_at_their_edges(monkeypatch):
    """Sets at and around the 32 / 112 / 144 bounds at which the instances of asm_small_k hand over, and 200 (handed to the device
    tail).  With the kernels and without (NNMPC_NO_SMALL): same sets, same u.
    n = 704: the largest horizon of 8 inputs per stage the kernels take.  Their gate (solve_segment_asm) is on the PADDED size --
    rows of P^-1 of n_pad doubles, n_pad^2 * 8 bytes within the 4 MB of an XCD's L2 -- and n pads to a multiple of 64 here:
    n_pad = 704 fits (3.97 MB); n = 720 pads to 768 (4.7 MB) and goes through the rounds / the tail, which the second half of
    this test pins down (asm_small_passes == 0, same demands on the answers)."""
    from industrial_nnmpc_2021_amd.qp import BatchedBoxQP
    from tests.test_small_gpu import _both_ways
    sizes = [31, 32, 33, 111, 112, 113, 143, 144, 145, 200] * 3
    n = 704
    P, q, lb, ub, state, xref = H.large_set_problem(n, NU, 41, sizes)
    res = _both_ways(monkeypatch, lambda: BatchedBoxQP(P, np.eye(n), NU, max_batch=128, method="asm"),
                     lambda qp: qp.solve_batch(q, lb, ub))
    (a, sa), (b, sb) = res[True], res[False]
    print(f"LARGE_SETS small: passes {sa['asm_small_passes']} / {sb['asm_small_passes']} status {np.bincount(a['status'], minlength=3)} "
          f"|du| {np.abs(a['u'] - b['u']).max():.3e}")
    assert sa["asm_small_passes"] >= 1 and sb["asm_small_passes"] == 0
    assert (a["status"] == 0).all() and (b["status"] == 0).all()
    assert sa["asm_solved"] == len(sizes) and sb["asm_solved"] == len(sizes) and sa["factorizations"] == 0 and sb["factorizations"] == 0
    _judge("small", P, q, lb, ub, a, state, xref, oracle=(5, 8), okey="small")                # rows 5, 8: 113 and 145 bounds
    _judge("small off", P, q, lb, ub, b, state, xref)
    assert np.array_equal(a["active"], b["active"]) and np.abs(a["u"] - b["u"]).max() <= 1e-9
    n = 720
    P, q, lb, ub, state, xref = H.large_set_problem(n, NU, 43, sizes)
    monkeypatch.delenv("NNMPC_NO_SMALL", raising=False)
    qp = BatchedBoxQP(P, np.eye(n), NU, max_batch=128, method="asm")
    out, st = _solve(qp, q, lb, ub)
    qp.close()
    assert st["asm_small_passes"] == 0 and (out["status"] == 0).all() and st["asm_solved"] == len(sizes) and st["factorizations"] == 0
    _judge("n = 720", P, q, lb, ub, out, state, xref)


# ---- sizes inside the classes of 145 .. 256 bounds ----------------------------------------------------------------------------

def test_sizes_inside_the_two_and_four_wave_classes(fam, handles):
    """145 .. 176 and 177 .. 256 bounds at sizes between the boundaries (160: a full 10-block set, 200: 13 blocks with a ragged
    last one) next to the ends of both classes, f32 rounds first and fp64 throughout."""
    P, rows = fam
    sizes = [145, 160, 176, 177, 200, 256] * 2
    q, lb, ub, state, _, xref = rows(sizes, 31)
    for f32 in (0, -1):
        out, st = _solve(handles(asm_f32_rounds=f32, **ROUNDS), q, lb, ub)
        print(f"LARGE_SETS inside f32={f32}: status {out['status']} asm_solved {st['asm_solved']} factorizations {st['factorizations']}")
        assert (out["status"] == 0).all(), (out["status"], sizes)
        assert st["asm_solved"] == len(sizes) and st["factorizations"] == 0
        _judge(f"inside f32={f32}", P, q, lb, ub, out, state, xref)
