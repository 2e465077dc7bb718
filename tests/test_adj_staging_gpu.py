"""nnmpc_qp_adjoint over several segments: host-pointer calls longer than the handle's segment (seg_max = 128 problems), and calls
whose D cuts the segment down -- first-move mode at 1024 rows (problem, cotangent) a segment, sequence mode at the 1 GiB the row
buffers V / Z, Y and GX may take (n = 1028: 56 000 rows).  Against calls that fit one segment: bit for bit in first-move mode (no
GEMM; a cotangent's arithmetic does not depend on its chunk or its wave), within the tolerance of tests/test_adj_kernel_gpu.py in
sequence mode (gemm64 chooses its kernel by the shape of a product, so the products of a large and of a small call need not sum
in the same order).
"""
import numpy as np
import pytest

from tests import adj_helpers as A
from tests import mult_helpers as M
from tests import sens_helpers as S
from tests.test_adj_kernel_gpu import OUTS, call, new_handle, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def big():
    qp = new_handle("real", S.SHAPES[-1])
    yield qp
    qp.close()


def test_more_problems_than_a_segment():
    shape = S.SHAPES[3]
    n, nu, n_aug = shape
    qp = new_handle("real", shape)
    try:
        fams = S.families(n, nu)
        rng = np.random.default_rng(31)
        B, D = 300, 3                                                           # three segments of the handle's 128 problems
        words = M.pack_rows(np.array([S.family_rows(*fams[b % len(fams)], n, nu, rng) for b in range(B)]), n)
        status = np.zeros(B, np.int32)
        status[[5, 130, 299]] = 2
        for first in (False, True):
            v = rng.standard_normal((B, D, nu if first else n))
            rc, o = call(qp, words, v, status=status, first=first)
            assert rc == 0 and np.array_equal(o["flag"][:B], status) and o["flag"][B] == -9
            rc, od = call(qp, words, v, status=status, first=first, device=True)        # device pointers: one launch over the batch
            assert rc == 0 and all(same_bits(od[k], o[k]) for k in OUTS + ("flag",))
            for b0 in (0, 100, 250):                                            # ... and one-segment host calls of 50 problems
                rc, o1 = call(qp, words[b0:b0 + 50], v[b0:b0 + 50], status=status[b0:b0 + 50], first=first)
                assert rc == 0 and all(same_bits(o1[k][:50], o[k][b0:b0 + 50]) for k in OUTS + ("flag",))
    finally:
        qp.close()


def test_first_move_rows_beyond_a_segment(big):
    qp = big
    n, nu, n_aug = S.SHAPES[-1]
    c = S.real_case(161, S.SHAPES[-1])
    rng = np.random.default_rng(32)
    B, D = 3, 600                                                               # 1024 rows a segment: one problem each
    v = rng.standard_normal((B, D, nu))
    rc, o = call(qp, c["words"][:B], v, first=True)
    assert rc == 0 and (o["flag"][:B] == 0).all()
    rc, o1 = call(qp, c["words"][:B], v[:, 593:], first=True)                   # the last seven cotangents, all problems in one segment
    assert rc == 0 and all(same_bits(o1[k][:B], o[k][:B, 593:]) for k in OUTS)


def test_sequence_rows_at_the_row_cap(big):
    qp = big
    shape = S.SHAPES[-1]
    n, nu, n_aug = shape
    m = 161
    c, mats = S.real_case(m, shape), S.real_matrices(*shape)
    B, D = 2, 30600                                                             # 61 200 rows: more than the cap holds, one problem a segment
    small = A.real_cotangents(m, shape)[:B]                                     # (B, REAL_D, n)
    v = np.ascontiguousarray(np.tile(small, (1, -(-D // S.REAL_D), 1))[:, :D])
    rc, o = call(qp, c["words"][:B], v, want=("gx0", "glb", "gub"))
    assert rc == 0 and (o["flag"][:B] == 0).all()
    take = np.r_[0:S.REAL_D, D - S.REAL_D:D]                                    # the first and the last rows of both problems
    rc, o1 = call(qp, c["words"][:B], v[:, take], want=("gx0", "glb", "gub", "gbound"))
    assert rc == 0
    ref = A.adjoint_ref_ld(mats["P"], mats["tq"], c["words"][:B], v[:, take], nu)
    route = A.adjoint_route_f64(mats["Hinv"], mats["Kunc"], c["words"][:B], v[:, take], nu)
    e_route = A.errors(mats["Kunc"], c["words"][:B], v[:, take], nu, route["gx0"], route["gbound"], ref)
    tol = A.tolerance(e_route[0], n, n_aug)
    e_big = A.errors(mats["Kunc"], c["words"][:B], v[:, take], nu, o["gx0"][:B][:, take], o1["gbound"][:B], ref)
    e_small = A.errors(mats["Kunc"], c["words"][:B], v[:, take], nu, o1["gx0"][:B], o1["gbound"][:B], ref)
    print(f"e_x at the row cap {e_big[0]:.3g}, one segment {e_small[0]:.3g}, float64 route {e_route[0]:.3g}, tol {tol:.3g}")
    assert e_big[0] <= tol and e_small[0] <= tol
    # glb / gub of the large call (its gbound is not asked for: 0.5 GB): sums of at most n / nu entries of w, each within tol_w
    tol_w = A.tolerance(e_route[1], n, n_aug) * (np.abs(ref["gbound"]).max() + np.abs(v[:, take]).max()) * (n // nu)
    for k in ("glb", "gub"):
        assert np.abs(o[k][:B][:, take] - o1[k][:B]).max() <= tol_w and np.abs(o1[k][:B] - route[k]).max() <= tol_w
    # the tiled cotangents repeat every REAL_D rows: so do the results, whatever segment and GEMM tile a row fell into
    assert D % S.REAL_D == 0
    for k in ("gx0", "glb", "gub"):
        rep = o[k][:B].reshape(B, -1, S.REAL_D, o[k].shape[2])
        assert same_bits(rep, np.broadcast_to(rep[:, :1], rep.shape)), k
