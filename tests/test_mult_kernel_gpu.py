"""asm_mult_k (csrc/qp_mult.h) alone, through nnmpc_qp_multipliers, entry by entry.

Integer data, as tests/test_gemm_kernel_gpu.py uses them: P symmetric and strictly diagonally dominant with |P_ij| <= 8 off the
diagonal, tq, x0, u integers of at most 16 in size, so every partial sum in any order is an integer far below 2^53 and the result
must EQUAL the int64 product (tests/test_cpu_mult_inputs.py holds the table to that).  Shapes (n, nu, n_aug) from one stage of three
variables to 1028 variables -- past one 256-thread trip (260), past the small-problem limit of the solvers (708), past 1024 and not
a multiple of 64 (1028) --, batches of 1, 5 and 129 problems, and per problem row one of: no active bound, only variable 0 (upper),
only variable n - 1 (lower), all n with alternating sides, a seeded tenth.  The result buffer holds B + 1 rows of a sentinel: free
entries must come back as +0.0 bit for bit and row B must keep its bytes.  A second call makes three rows unusable (a NaN in u,
status 2, both bits of one variable): they come back all NaN and every other row as before.  Host and device pointers agree bit
for bit.  Kunc is NULL: the call needs neither an inverse nor far-field factors.
"""
import ctypes as C

import numpy as np
import pytest

from tests import mult_helpers as M

pytestmark = pytest.mark.gpu

_HANDLES = {}


@pytest.fixture(scope="module")
def handles():
    yield _HANDLES
    for h in _HANDLES.values():
        h.close()
    _HANDLES.clear()


def handle(handles, shape):
    if shape not in handles:
        from industrial_nnmpc_2021_amd.qp import BatchedBoxQP
        n, nu, n_aug = shape
        P, tq = M.kernel_matrices(n, nu, n_aug)
        handles[shape] = BatchedBoxQP(P.astype(np.float64), tq.astype(np.float64), nu, Kunc=None, max_batch=128, seg_max=128)
    return handles[shape]


def call_host(qp, x0, u, words, status, B):
    """nnmpc_qp_multipliers on host pointers; the buffer has B + 1 rows of the sentinel."""
    from industrial_nnmpc_2021_amd import _lib
    out = np.full((B + 1, qp.n), M.SENTINEL)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    _lib.check(qp._lib.nnmpc_qp_multipliers(qp._h, B, p(x0), p(u), p(words), p(status), p(out), _lib.HOST), "nnmpc_qp_multipliers")
    return out


def call_device(qp, x0, u, words, status, B):
    from industrial_nnmpc_2021_amd import _lib
    D = _lib.DeviceArray
    bufs = [D.from_host(x0), D.from_host(u), D.from_host(words), None if status is None else D.from_host(status),
            D.from_host(np.full((B + 1, qp.n), M.SENTINEL))]
    p = lambda a: None if a is None else C.c_void_p(a.data_ptr())
    _lib.check(qp._lib.nnmpc_qp_multipliers(qp._h, B, *(p(b) for b in bufs), _lib.DEVICE), "nnmpc_qp_multipliers")
    out = bufs[4].to_host()
    for b in bufs:
        if b is not None:
            b.free()
    return out


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("B", M.KERNEL_BATCHES)
@pytest.mark.parametrize("shape", M.KERNEL_SHAPES, ids=lambda s: "n%d_nu%d_aug%d" % s)
def test_integer_cases_entry_by_entry(handles, shape, B):
    n, nu, n_aug = shape
    qp = handle(handles, shape)
    c = M.kernel_case(n, nu, n_aug, B)
    x0, u, words = c["x0"].astype(np.float64), c["u"].astype(np.float64), c["words"]
    got = call_host(qp, x0, u, words, None, B)
    want = c["want"].astype(np.float64)
    free = M.sides(words, n, nu) == 0
    bad = got[:B] != want
    print(f"n {n} B {B}: {int((~free).sum())} active bounds, {int(bad.sum())} entries differ")
    assert not bad.any(), np.argwhere(bad)[:4]
    assert (got[:B][free].view(np.uint64) == 0).all()                        # +0.0 bit for bit, the sentinel gone
    assert same_bits(got[B], np.full(n, M.SENTINEL))                         # the row behind the batch keeps its bytes
    assert same_bits(got, call_device(qp, x0, u, words, None, B))
    # status given and all zero: the same values
    assert same_bits(got, call_host(qp, x0, u, words, np.zeros(B, np.int32), B))

    rows = M.bad_rows(B)
    if not rows:
        return
    u2, words2, status = u.copy(), words.copy(), np.zeros(B, np.int32)
    u2[rows[0], n - 1] = np.nan
    status[rows[1]] = 2
    status[0] = 1                                                            # not certified, but computed like any other row
    up, lo = M.row_index(n, nu)
    i = n // 2
    for bit in (up[i], lo[i]):
        words2[rows[2], bit // 32] |= np.uint32(1 << (bit % 32))
    got2 = call_host(qp, x0, u2, words2, status, B)
    keep = np.setdiff1d(np.arange(B + 1), rows)
    assert np.isnan(got2[list(rows)]).all()
    assert same_bits(got2[keep], got[keep])
    assert same_bits(got2, call_device(qp, x0, u2, words2, status, B))


def test_empty_batch_and_bad_arguments(handles):
    from industrial_nnmpc_2021_amd import _lib
    qp = handle(handles, M.KERNEL_SHAPES[1])
    out = np.full((1, qp.n), M.SENTINEL)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    x0, u, w = np.zeros((1, qp.n_aug)), np.zeros((1, qp.n)), np.zeros((1, qp.words), np.uint32)
    assert qp._lib.nnmpc_qp_multipliers(qp._h, 0, p(x0), p(u), p(w), None, p(out), _lib.HOST) == 0
    assert same_bits(out, np.full((1, qp.n), M.SENTINEL))                    # B = 0: nothing written
    assert qp._lib.nnmpc_qp_multipliers(qp._h, 1, p(x0), p(u), None, None, p(out), _lib.HOST) == _lib.EINVAL
    assert qp._lib.nnmpc_qp_multipliers(qp._h, 1, p(x0), p(u), p(w), None, None, _lib.HOST) == _lib.EINVAL
    # the Python wrapper: all free, so all +0.0
    m = qp.multipliers(x0, u, w)
    assert m.shape == (1, qp.n) and (m.view(np.uint64) == 0).all()
