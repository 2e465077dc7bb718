"""The case table of tests/test_gemm_kernel_gpu.py (helpers.gemm_cases) held to the conditions its comparisons rest on, with the
reference alone -- no GPU.  A case that cannot see the defect it is there for is a failure here, not a pass there."""
import numpy as np
import pytest

from tests import helpers as H

CASES = H.gemm_cases()
IDS = [c["id"] for c in CASES]
KDYN_VALUES = lambda c, K: {-1, 0, c - 2, c - 1, c, 2 * c - 1, K - 1, K + 5}
_MEMO = {}


def built(cid, rounded=False):
    if (cid, rounded) not in _MEMO:
        c = H.gemm_case(cid)
        inp = H.gemm_inputs(c, rounded)
        _MEMO[(cid, rounded)] = (c, inp, H.gemm_case_reference(c, inp, rounded))
    return _MEMO[(cid, rounded)]


def full_product(c, inp):
    A = np.nan_to_num(inp["A"], nan=0.0).astype(np.int64)
    return A @ inp["B"].astype(np.int64).T


def test_reference_against_plain_loops():
    """gemm_reference itself, on a shape small enough for three nested loops: T = 4, c = 2, every argument at once."""
    rng = np.random.default_rng(1)
    M, N, K, T, c = 12, 5, 7, 4, 2
    A, B = rng.integers(-3, 4, (20, K)), rng.integers(-3, 4, (N, K))
    rowmap = np.array([7, -1, 3, 19, 0, 1, -1, 2, 11, 12, 13, 14])
    tags = np.array([0, 0, 5, 0, 0, 0, 0, 0, 1, 1, 1, 1])         # tile 0 has the tag, tile 1 not, tile 2 lies beyond mdyn
    kdyn = np.array([1, 4, -1, -1, 6, 6])
    ref = H.gemm_reference(A, B, M, N, K, T, c, c_rows=20, rowphase=tags, want=5, kdyn=kdyn, kper=2, mdyn=7, rowmap=rowmap)
    want = np.zeros((20, N), np.int64)
    wr = np.zeros((20, N), bool)
    for i in range(4):                                            # tile 0 alone: bound max(1, 4) = 4 -> k < 6
        if rowmap[i] >= 0:
            for j in range(N):
                want[rowmap[i], j] = sum(int(A[rowmap[i], k]) * int(B[j, k]) for k in range(6))
                wr[rowmap[i], j] = True
    assert ref["tiles"] == [0] and ref["left"] == [1, 2] and ref["kk"] == {0: 6}
    assert np.array_equal(ref["written"], wr) and np.array_equal(ref["val"], want)
    ref = H.gemm_reference(A, B, M, N, K, T, c, kdyn=np.array([-1]), kper=0)       # -1: zeros, written
    assert ref["written"].all() and not ref["val"].any() and ref["tiles"] == [0, 1, 2]
    ref = H.gemm_reference(A, B, M, N, K, T, c, kdyn=np.array([9]), kper=0)        # beyond K: K
    assert np.array_equal(ref["val"], A[:M] @ B.T)
    ref = H.gemm_reference(A, B, M, N, K, T, c, mdyn=5)                            # the tile mdyn cuts is written whole
    assert ref["tiles"] == [0, 1] and ref["written"][:8].all() and not ref["written"][8:].any()


def test_table_reaches_every_kernel_and_kper():
    seen = {(c["kind"], H.gemm_inputs(c)["ref"]["kper"]) for c in CASES if c["group"] in ("kdyn", "f32map")}
    assert seen == {(1, 0), (1, 2), (2, 0), (2, 1), (3, 2), (4, 1)}
    assert {c["kind"] for c in CASES} == {1, 2, 3, 4}
    assert len(set(IDS)) == len(IDS)
    assert H.GEMM_SENTINEL != round(H.GEMM_SENTINEL) and np.float32(H.GEMM_SENTINEL) == H.GEMM_SENTINEL and H.GEMM_WANT != 0


@pytest.mark.parametrize("cid", IDS)
def test_exact_sums_stay_exact(cid):
    c, inp, _ = built(cid)
    limit = 2 ** 24 if H.gemm_dtype(c["kind"]) == np.float32 else 2 ** 53
    assert 9 * c["K"] < limit
    for a in (inp["Af"], inp["Bf"]):
        v = a[~np.isnan(a)]
        assert (v == np.round(v)).all() and np.abs(v).max() <= 3
    assert c["K"] % c["c"] == 0 and c["N"] % c["T"] == 0 and (c["M"] % c["T"] == 0 or c["kind"] in (3, 4))
    vec = 16 // inp["Af"].itemsize
    assert inp["Af"].shape[1] % vec == 0 and inp["Bf"].shape[1] % vec == 0        # rows of A and B start on 16 bytes


def test_dispatch_shapes():
    A, B = H.gemm_dispatch_inputs()
    assert np.abs(A).max() <= 3 and np.abs(B).max() <= 3 and (A == np.round(A)).all() and (B == np.round(B)).all()
    for name, (M, N, K) in H.GEMM_DISPATCH.items():
        assert M <= A.shape[0] and N <= B.shape[0] and K <= A.shape[1] and M % 64 == 0 and N % 64 == 0
        on_grid = M % 128 == 0 and N % 128 == 0 and K % 16 == 0
        assert on_grid == (name in ("t128", "k64"))
        assert (M // 128) * (N // 128) == (192 if name == "k64" else 200)           # the rule is "< 200": 200 is the first shape past it


@pytest.mark.parametrize("cid", IDS)
def test_reference_without_skip_arguments_is_the_int64_product(cid):
    c, inp, _ = built(cid)
    rows = -(-c["M"] // c["T"]) * c["T"]
    ref = H.gemm_reference(inp["A"], inp["B"], c["M"], c["N"], c["K"], c["T"], c["c"])
    assert ref["written"].all() and ref["left"] == []
    assert np.array_equal(ref["val"], full_product(c, inp)[:rows])
    assert np.array_equal(ref["absval"], np.abs(np.nan_to_num(inp["A"][:rows], nan=0.0)).astype(np.int64) @ np.abs(inp["B"]).astype(np.int64).T)


@pytest.mark.parametrize("cid", [c["id"] for c in CASES if c["rowphase"] is not None or c["mdyn"] is not None])
def test_skip_cases_have_tiles_of_both_classes(cid):
    c, inp, ref = built(cid)
    ntm = c["M"] // c["T"]
    assert sorted(ref["tiles"] + ref["left"]) == list(range(ntm))
    if c["group"] == "mdyn" and c["mdyn"] in (0, c["M"]):
        # the two ends of the list *mdyn in {0, 1, T - 1, T, T + 1, M}: nothing written / nothing left, by what they are
        assert (ref["tiles"] == []) if c["mdyn"] == 0 else (ref["left"] == [])
    else:
        assert ref["tiles"] and ref["left"], (ref["tiles"], ref["left"])
    if c["group"] == "mdyn":
        assert ref["tiles"] == list(range(-(-c["mdyn"] // c["T"])))
    if c["rowphase"] is not None:
        T, tags = c["T"], np.asarray(c["rowphase"])
        per = [np.flatnonzero(tags[t * T:(t + 1) * T] == H.GEMM_WANT).tolist() for t in range(ntm)]
        if T == H.GEMM_TILE[c["kind"]] and tags.size == 6 * T:
            assert per[0] == [] and per[5] == [] and per[1] == [0] and per[2] == [T - 1] and len(per[3]) == 1 and 0 < per[3][0] < T - 1
            assert len(per[4]) == T and ref["left"] == [0, 5]
        for t in ref["left"]:                                      # a kernel that compares with 0 would run these
            assert (tags[t * T:(t + 1) * T] == 0).any()
    view = inp["C"]
    exp = H.gemm_expected(ref, view)
    for t in ref["left"] if c["rowmap"] is None else ():            # (with a rowmap the rows of C are not the tile's: test_rowmap_cases)
        assert (exp[t * c["T"]:(t + 1) * c["T"]] == H.GEMM_SENTINEL).all()


@pytest.mark.parametrize("cid", [c["id"] for c in CASES if c["kdyn"] is not None])
def test_kdyn_cases_can_see_an_ignored_or_misread_bound(cid):
    c, inp, ref = built(cid)
    T, K, ch = c["T"], c["K"], c["c"]
    full = full_product(c, inp)
    kd = np.asarray(c["kdyn"])
    if c["group"] == "kdyn":
        assert set(kd.tolist()) <= KDYN_VALUES(ch, K)
    if c["variant"] == "a":
        # zeros beyond each block's own bound: the truncated product IS the full product, and the last column inside is in use
        assert np.array_equal(ref["val"][:full.shape[0]], full) and ref["written"][:full.shape[0]].all()
        for b in range(c["M"] // 64):
            kl = int(kd[b] if c["kblocks"] else kd[0])
            assert not inp["A"][64 * b:64 * b + 64, max(kl + 1, 0):].any()
            if 0 <= kl < K:
                assert inp["A"][64 * b:64 * b + 64, kl].any()
        return
    assert c["variant"] == "b"
    truncated = [t for t in ref["tiles"] if ref["kk"][t] < K]
    for t in truncated:                                            # (a tile whose rounded bound is K has nothing beyond it to tell)
        rows = slice(t * T, min((t + 1) * T, c["M"]))
        assert (ref["val"][rows] != full[rows]).any(), (cid, t)
        assert inp["A"][rows, ref["kk"][t]:].all() if c["nan"] is None else True       # non-zero integers beyond the rounded bound
    if c["group"] == "kdyn":
        assert truncated or min(kd.max(), K - 1) // ch + 1 == K // ch, cid
    # a chunk too far, or the neighbouring block's entry, gives another product in every truncated tile
    for t in truncated:
        rows = slice(t * T, min((t + 1) * T, c["M"]))
        longer = inp["A"][rows, :ref["kk"][t] + ch].astype(np.int64) @ inp["B"][:, :ref["kk"][t] + ch].astype(np.int64).T if c["nan"] is None else None
        if longer is not None:
            assert (longer != ref["val"][rows]).any()
    if c["kblocks"] and c["group"] == "kdyn" and c["nan"] is None:
        kper = T // 64
        kks = [ref["kk"][t] for t in ref["tiles"]]
        assert len(set(kks)) >= 3                                  # three extents at least; in o1 no two neighbouring tiles share one
        assert "-o2" in cid or all(a != b for a, b in zip(kks[:-1], kks[1:]))
        if kper == 2:                                              # the larger entry comes first in one tile and second in another
            pairs = kd.reshape(-1, 2)
            assert (pairs[:, 0] > pairs[:, 1]).any() and (pairs[:, 0] < pairs[:, 1]).any()
    if c["nan"]:
        r, col = c["nan"]
        kk = ref["kk"][r // T]
        assert col in (kk, kk - 1) and kk < K
        assert ref["poison"] == ([r] if col == kk - 1 else [])
        exp = H.gemm_expected(ref, inp["C"])
        assert np.isnan(exp).sum() == (c["N"] if col == kk - 1 else 0)


def test_kdyn_orders_cover_the_values():
    for kind in (1, 2, 3, 4):
        ch = H.GEMM_CHUNK[kind]
        K = 4 * ch
        o = H.gemm_kdyn_orders(ch, K)
        assert set(o["o1"]) == KDYN_VALUES(ch, K) and len(o["o1"]) == len(o["o2"]) == 8
        # with two entries per tile (kper = 2) the two orders together make every value the bound of some tile
        assert {max(p) for p in np.reshape(o["o1"] + o["o2"], (-1, 2)).tolist()} == KDYN_VALUES(ch, K)
        one = {c["kdyn"][0] for c in CASES if c["group"] == "kdyn" and not c["kblocks"] and c["kind"] == kind}
        assert one == (KDYN_VALUES(ch, K) if kind in (1, 2) else set())


@pytest.mark.parametrize("cid", [c["id"] for c in CASES if c["group"] == "f32map"])
def test_f32_tile_map_cases(cid):
    c, inp, ref = built(cid)
    T, M = c["T"], c["M"]
    ntm, ntn = -(-M // T), c["N"] // T
    assert ntm in (1, 7, 8, 9, 17) and ntn in (1, 2, 3) and c["K"] == 96
    if c["kind"] == 3:                                             # the last 128-row tile has its first 64-row block in use
        assert M % 128 == 64 and not inp["A"][M:].any() and inp["A"][M - 64:M].any() and c["kdyn"][-1] == -1 and c["kdyn"][-2] >= 0
    assert ref["tiles"] == list(range(ntm)) and ref["written"][:ntm * T].all() and not ref["written"][ntm * T:].any()
    assert len({ref["kk"][t] for t in ref["tiles"]}) >= min(ntm, 2)
    # no two row tiles and no two column tiles hold the same numbers: a tile computed in another one's place shows
    v = ref["val"][:ntm * T]
    blocks = [v[i * T:(i + 1) * T, j * T:(j + 1) * T].tobytes() for i in range(ntm) for j in range(ntn)]
    assert len(set(blocks)) == len(blocks)


@pytest.mark.parametrize("cid", [c["id"] for c in CASES if c["group"] in ("deal", "ring", "k64")])
def test_tiles_are_told_apart(cid):
    c, inp, ref = built(cid)
    T = c["T"]
    ntm, ntn = c["M"] // T, c["N"] // T
    blocks = [ref["val"][i * T:(i + 1) * T, j * T:(j + 1) * T].tobytes() for i in range(ntm) for j in range(ntn)]
    assert len(set(blocks)) == len(blocks)
    assert inp["Cf"].shape[0] >= c["M"] + 2 and inp["Cf"].shape[1] > c["c0"] + c["N"] and (inp["Cf"] == H.GEMM_SENTINEL).all()
    if c["group"] != "deal":
        assert inp["Af"].shape[1] > c["K"] and inp["Bf"].shape[1] > c["K"] and c["c0"] > 0


def test_deal_shapes():
    got = {(c["M"] // 128, c["N"] // 128) for c in CASES if c["group"] == "deal" and c["kind"] == 1}
    assert got == {(m, n) for m in (1, 7, 8, 9, 32, 33) for n in (1, 3)}
    assert {c["K"] for c in CASES if c["group"] == "ring"} == {16, 32, 48, 80}
    assert {(c["M"], c["N"], c["K"]) for c in CASES if c["group"] == "k64"} == {(m, n, k) for m in (64, 192, 320) for n in (64, 192, 320) for k in (16, 32, 48)}


@pytest.mark.parametrize("cid", [c["id"] for c in CASES if c["rowmap"] is not None])
def test_rowmap_cases(cid):
    c, inp, ref = built(cid)
    rm = np.asarray(c["rowmap"])
    named = rm[rm >= 0]
    assert rm.size == c["M"] == 384 and named.size == np.unique(named).size and (rm < 0).any()
    assert named.max() < c["a_rows"] and c["a_rows"] > c["M"] and named.size < c["a_rows"]        # rows no entry names
    assert (rm[[0, 127, 128, 383]] < 0).all() and not np.array_equal(named, np.sort(named))
    lim = c["mdyn"] if c["mdyn"] is not None else c["M"]
    stored = rm[:lim][rm[:lim] >= 0]
    assert np.array_equal(np.flatnonzero(ref["written"].all(axis=1)), np.sort(stored))
    assert not ref["written"][np.setdiff1d(np.arange(inp["C"].shape[0]), stored)].any()
    assert np.array_equal(ref["val"][stored], full_product(c, inp)[stored])
    if c["mdyn"] is not None:
        assert c["mdyn"] % 128 not in (0, 127) and ref["left"] == [2] and (rm[c["mdyn"]:] >= 0).any()


@pytest.mark.parametrize("cid", [c["id"] for c in CASES if c["rounded"]])
def test_numpy_matmul_meets_the_bar(cid):
    """The bar 2 gamma_K |A| |B|' against the longdouble reference is one a plain matmul in the type meets: it is not a bar only the
    reference's own order of summation could pass."""
    assert H.gemm_highprec() is np.longdouble or np.finfo(np.longdouble).eps > 2.0 ** -63
    c, inp, ref = built(cid, True)
    dt = H.gemm_dtype(c["kind"])
    assert inp["A"].dtype == dt
    spread = np.log10(np.abs(inp["A"][inp["A"] != 0]).astype(np.float64))
    assert spread.max() - spread.min() > 6
    rows = ref["written"].all(axis=1)
    got = np.zeros(ref["val"].shape, dt)
    for t in ref["tiles"]:
        r = slice(t * c["T"], (t + 1) * c["T"])
        got[r] = inp["A"][r, :ref["kk"][t]] @ inp["B"][:, :ref["kk"][t]].T
    err = np.abs(got[rows].astype(H.gemm_highprec()) - ref["val"][rows]).astype(np.float64)
    bar = H.gemm_bar(c, ref)[rows]
    used = inp["A"][np.flatnonzero(rows)].any(axis=1)              # (the f32 round's last tile has rows of zeros: bar 0, error 0)
    assert (err <= bar).all() and (bar[used] > 0).all() and used.any(), float((err[bar > 0] / bar[bar > 0]).max())
