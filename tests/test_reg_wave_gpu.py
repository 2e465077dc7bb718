"""Who solves what in the register multiplier kernels (csrc/qp_asm.h: asm_lambda_reg_k, asm_lambda_reg32_k, asm_lambda_reg32b_k).

Each wave of these kernels solves one problem on its own; a workgroup holds ASM_REG*_WPB of them (1 or 4).  Workgroup w of a launch
walks the size classes from the largest down, ceil(count / WPB) workgroups per class, and the carried problems' copy
(asm_carry_copy, ASM_CARRY_GROUP = 4 problems per workgroup) rides at the end of asm_lambda_reg32_k's grid.  The arithmetic of a
wave does not depend on any of this; what can go wrong is the bookkeeping -- a problem nobody takes, a problem taken twice, a wave
past the end of its list.  So the batches here are the smallest that reach every edge of the walk: class counts that are no
multiple of four (and one that is), an empty class between full ones, a lone problem, a batch whose only class is the last one
walked, and carried counts around the copy's group.

Problems: the family of tests/test_large_sets_gpu.py (n = 1024, nu = 8, sets of a chosen size) on its handles, judged by its
_judge: the returned set is the pushed set bit for bit, u within its TOL of the fp64 solve on that set, kkt_check, status 0.  The
carry runs use the configuration of tests/test_carry_gpu.py (predictor on, pushes inside its 512 columns) and add its bit-equality
with NNMPC_CARRY=0.  Set sizes by class (class b: at most 16 (b + 4) bounds):

    0: <= 64   1: 65..80   2: 81..96   3: 97..112   4: 113..128   5: 129..144 | 6: 145..160   7: 161..176 (asm_lambda_reg32b_k)
"""
import numpy as np
import pytest

from tests import helpers as H
from tests.test_carry_gpu import _assert_bit_equal, _call, _carry, _leading_rows
from tests.test_large_sets_gpu import N_, NU, ROUNDS, _judge, _solve, fam, handles  # noqa: F401  (fam, handles: fixtures)

pytestmark = pytest.mark.gpu

CARRY_GROUP = 4        # qp_asm.h: ASM_CARRY_GROUP

# problems per class: 0: 2 (16, 64)  1: 3  2: 3  3: 5  4: none  5: 8 (a full last workgroup of four)  6: 2  7: 7
WALK = [16] + [70] * 2 + [85] * 3 + [100] * 5 + [140] * 7 + [150] + [170] * 6 + [64, 65, 144, 145, 176]
LONE = [40]
LAST_CLASS_ONLY = [16, 30, 50, 64, 20]          # class 0 alone: every other class of the walk is empty
CASES = {"walk": (WALK, 71), "lone": (LONE, 72), "class0": (LAST_CLASS_ONLY, 73)}


def _mixed(sizes, seed):
    """The sizes in an order that is a function of the seed alone (the lists of a class are filled in batch order)."""
    return [int(v) for v in np.random.default_rng(seed).permutation(sizes)]


@pytest.mark.parametrize("case", list(CASES))
def test_class_walk_without_the_predictor(fam, handles, case):
    """asm_predict_iters = -1: f32 rounds (asm_lambda_reg32_k, asm_lambda_reg32b_k) until the set settles, then the fp64 solve
    (asm_lambda_reg_k up to 144 bounds, asm_lambda_wg64s_k beyond)."""
    P, rows = fam
    sizes, seed = CASES[case]
    sizes = _mixed(sizes, seed)
    q, lb, ub, state, _, xref = rows(sizes, seed)
    out, st = _solve(handles(asm_f32_rounds=0, **ROUNDS), q, lb, ub)
    print(f"REG_WAVE {case}: sizes {sizes} status {np.bincount(out['status'], minlength=3)} asm_solved {st['asm_solved']} "
          f"rounds {st['asm_rounds']} f32 launches {st['asm_lambda32_launches']} fp64 launches {st['asm_lambda64_launches']}")
    assert (out["status"] == 0).all(), (out["status"], sizes)
    assert st["asm_solved"] == len(sizes) and st["factorizations"] == 0 and st["asm_predict_launches"] == 0
    assert st["asm_carried"] == 0
    _judge(f"reg_wave {case}", P, q, lb, ub, out, state, xref)


@pytest.fixture(scope="module")
def carried(fam):
    """The handle of tests/test_carry_gpu.py's sized sets; solve(sizes, seed) -> (P, q, lb, ub, state, xref, carry on, carry off)."""
    from industrial_nnmpc_2021_amd.qp import BatchedBoxQP
    P = fam[0]
    Ps = np.tril(P) + np.tril(P, -1).T
    qp = BatchedBoxQP(P, np.eye(N_), NU, max_batch=128, seg_max=4096, method="asm", asm_tail_batch=-1, asm_predict_iters=0)

    def solve(monkeypatch, sizes, seed):
        q, lb, ub, state = _leading_rows(P, seed, sizes)
        xref = np.stack([H.solve_on_set(Ps, q[b], lb, ub, state[b]) for b in range(len(sizes))])
        out = {}
        for tag in ("on", "off"):
            _carry(monkeypatch, tag == "on")
            out[tag] = _call(qp, q, lb, ub)
        return P, q, lb, ub, state, xref, out["on"], out["off"]
    yield solve
    qp.close()


def _judge_carry(what, sizes, res):
    """Every row of the carry-on run as _judge demands, the run with NNMPC_CARRY=0 bit for bit the same, and the carried count:
    a row of _leading_rows has the same set from the predictor, the f32 screen and the optimum, so every set of at most 176 bounds
    is carried -- exactly one copy each."""
    P, q, lb, ub, state, xref, on, off = res
    print(f"REG_WAVE {what}: sizes {sizes} status {np.bincount(on['status'], minlength=3)} carried {on['stats']['asm_carried']} "
          f"(off {off['stats']['asm_carried']}) rounds {on['stats']['asm_rounds']} predict launches {on['stats']['asm_predict_launches']}")
    assert on["stats"]["asm_predict_launches"] == 1
    assert (on["status"] == 0).all(), (on["status"], sizes)
    assert on["stats"]["asm_solved"] == len(sizes) and on["stats"]["factorizations"] == 0
    _judge(f"reg_wave {what}", P, q, lb, ub, on, state, xref)
    _assert_bit_equal(on, off, what)
    assert off["stats"]["asm_carried"] == 0
    assert on["stats"]["asm_carried"] == sum(m <= 176 for m in sizes), on["stats"]["asm_carried"]


@pytest.mark.parametrize("case", list(CASES))
def test_class_walk_with_carried_multipliers(carried, monkeypatch, case):
    """Predictor on: round 0 is the f32 screen with the kept correction (the stash), round 1 the grouped copy."""
    sizes, seed = CASES[case]
    sizes = _mixed(sizes, seed + 10)
    _judge_carry(f"carry {case}", sizes, carried(monkeypatch, sizes, seed + 10))


@pytest.mark.parametrize("count", [1, CARRY_GROUP - 1, CARRY_GROUP, CARRY_GROUP + 1])
def test_carried_counts_around_the_copy_group(carried, monkeypatch, count):
    """1, group - 1, group, group + 1 carried problems, of both f32 kernels' classes: a last workgroup of the copy that is full,
    one short of full, and one that holds a single problem."""
    sizes = [100, 150, 60, 170, 130][:count]
    _judge_carry(f"carry count {count}", sizes, carried(monkeypatch, sizes, 90 + count))
