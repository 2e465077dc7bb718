"""The inputs, the emulation and the evaluator of tests/test_certificate_gpu.py, checked without a GPU.

The GPU file hands the solver inverses and far-field factors that are only approximately right and holds every status 0 to the
solver's own claim (helpers.cert_property_a).  Here, with e1 = max |P Kunc + tq| and e2 = max |P Pinv - I| computed in numpy:
the ladders reach every class of row (certified by the bound, accepted by the check with P, rejected by it), the emulated
free-set gradient never exceeds the emulated bound ("Certification without an n^2 product per sample", once,
independently of any kernel), and the evaluator accepts an optimum and refuses each kind of wrong result.
"""
import numpy as np
import pytest

from tests import helpers as H


def _gate_ok(e2):
    return e2 < H.CERT_GATE_E2 * (1.0 - H.CERT_GATE_BAND)


def _gate_refuses(e2):
    return e2 > H.CERT_GATE_E2 * (1.0 + H.CERT_GATE_BAND)


_LADDERS = {}


def _ladder(plant):
    """[(eps, e1, e2, emulation)] of the plant's accepted rungs and (eps, e1, e2) of the refused one."""
    if plant not in _LADDERS:
        c = H.cert_case(plant)
        rungs, above = H.CERT_LADDER[plant]
        acc = []
        for eps in rungs:
            Hp, Kp = H.cert_perturb(c, eps)
            e1, e2 = H.cert_errors(c, Hp, Kp)
            acc.append((eps, e1, e2, H.cert_emulate(c, Hp, Kp, e1, e2, precise=eps <= 1e-13)))
        _LADDERS[plant] = (acc, (above,) + H.cert_errors(c, *H.cert_perturb(c, above)))
    return _LADDERS[plant]


def test_every_site_has_a_plant_and_a_ladder():
    assert {s["plant"] for s in H.CERT_SITES.values()} == set(H.CERT_PLANTS) == set(H.CERT_LADDER)
    for plant, (rungs, above) in H.CERT_LADDER.items():
        assert rungs[0] == 0.0 and list(rungs) == sorted(rungs) and above > rungs[-1]


@pytest.mark.parametrize("plant", sorted(H.CERT_PLANTS))
def test_oracle_rows_are_certified_and_agree_with_the_exact_solver(plant):
    """cert_case certifies every row with P in np.longdouble (free-set gradient below 1e-3 of the bar); three rows against
    oracle.qp.solve_exact_box as well."""
    from oracle import qp as oqp
    c = H.cert_case(plant)
    assert c["oracle_ratio"].max() <= 1e-3
    for b in (0, c["B"] // 2, int(np.argmax((c["state"] != 0).sum(axis=1)))):
        info = {"nu": c["nu"]}
        xe = oqp.solve_exact_box(c["Ps"], c["q"][b], c["LB"][b], c["UB"][b], info=info)
        ref = np.zeros(2 * c["n"], bool)
        ref[info["active"]] = True
        if c["kept"][b]:
            assert np.array_equal(ref, c["active"][b]), b
        assert np.abs(xe - c["xs"][b]).max() <= 1e-7 * max(1.0, np.abs(xe).max()), b


@pytest.mark.parametrize("plant", sorted(H.CERT_PLANTS))
def test_ladder_meets_the_gate_and_reaches_every_class(plant):
    c = H.cert_case(plant)
    acc, (above, _, e2_above) = _ladder(plant)
    assert _gate_refuses(e2_above), (above, e2_above)
    best = dict(sure=0, accepted=0, rejected=0)
    lost = 0
    for eps, e1, e2, em in acc:
        assert _gate_ok(e2) and np.isfinite(e1), (eps, e1, e2)
        cl = H.cert_classes(c, em)
        lo, hi = H.cert_full_check_range(c, em)
        print(f"{plant} eps {eps:.0e}: e1 {e1:.2e} e2 {e2:.2e} sure {cl['sure'].sum()} accepted {cl['accepted'].sum()} rejected {cl['rejected'].sum()} "
              f"lost {cl['lost'].sum()} full checks {lo}..{hi} worst gradient/bound {(em['gfree'] / em['bnd']).max():.3f}")
        for k in best:
            best[k] = max(best[k], int(cl[k].sum()))
        lost += int(cl["lost"].sum())
        # the margin rule does what it is for: no accepted rung moves the set of a kept row
        assert em["setok"][c["kept"]].all(), (eps, np.flatnonzero(c["kept"] & ~em["setok"]))
        # the mathematics of the certificate: P x + q = E1 x0 - (I + E2) lam_ext, so on the free set |g| <= e1 |x0|_1 + e2 |lam|_1 <= bnd
        assert (em["gfree"] <= em["bnd"]).all(), (eps, np.flatnonzero(em["gfree"] > em["bnd"]))
    assert lost <= H.CERT_MAX_LOST * len(acc) * c["B"], (lost, len(acc) * c["B"])
    assert best["sure"] >= H.CERT_MIN_CLASS
    if plant != "cstrs":
        # (cstrs: the inverse of the cond-4e7 Hessian is at e2 ~ 1e-9 as it stands and the gate closes at eps = 5e-12: its two
        # accepted rungs certify by the bound or not at all -- the rounding term of the bound is what that site is about)
        assert best["accepted"] >= H.CERT_MIN_CLASS and best["rejected"] >= H.CERT_MIN_CLASS, best


@pytest.mark.parametrize("plant", ["mini_cdu", "mid_cdu"])
def test_row_and_column_family_is_accepted_and_leaves_nothing_sure(plant):
    c = H.cert_case(plant)
    j = H.cert_rowcol_index(c)
    Hp, Kp = H.cert_perturb_rowcol(c, j)
    e1, e2 = H.cert_errors(c, Hp, Kp)
    em = H.cert_emulate(c, Hp, Kp, e1, e2)
    inset = c["state"][:, j] != 0
    print(f"{plant} variable {j}: e2 {e2:.2e}, in the set of {inset.sum()} of {c['B']} rows, gradient/bar {np.median(em['ratio'][inset]):.2f} with it, "
          f"{np.median(em['ratio'][~inset]):.2f} without")
    assert _gate_ok(e2), e2
    assert inset.sum() >= H.CERT_MIN_CLASS and (~inset).sum() >= H.CERT_MIN_CLASS
    assert not em["sure"].any() and not em["undetermined"].any()          # e2max is global: every row goes through the check with P
    assert (em["gfree"] <= em["bnd"]).all()


@pytest.mark.parametrize("plant", ["mini_cdu", "mid_cdu"])
def test_kunc_family_is_accepted_and_leaves_nothing_sure(plant):
    c = H.cert_case(plant)
    Hp, Kp = H.cert_perturb_kunc(c)
    e1, e2 = H.cert_errors(c, Hp, Kp)
    em = H.cert_emulate(c, Hp, Kp, e1, e2)
    assert _gate_ok(e2) and e1 > 1e-4, (e1, e2)                            # e1 is only NaN-checked
    assert not em["sure"].any() and not em["undetermined"].any()
    assert (em["ratio"][em["setok"]] > 4.0).all()                          # the check with P has to refuse every one of them
    assert (em["gfree"] <= em["bnd"]).all()


def test_far_field_settings_meet_their_gate_and_their_classes():
    c = H.cert_case("mid_cdu")
    e1, e2 = H.cert_errors(c, c["H"], c["K"])
    aligned = H.cert_far_aligned_rows(c)
    efar = {}
    for s in H.CERT_FAR_SETTINGS:
        Up, Vx, Vl, efar[s] = H.cert_farfield_perturbed(c, s, row=aligned[0][0])
        assert Up.shape[1] == Vx.shape[0] == Vl.shape[0] and Vl.shape[1] == H.CERT_FAR_W
    print(f"efar {efar}; aligned rows and their gradient/bar with the factored far columns: {aligned}")
    assert efar["exact"] < 1e-12 and 0.5e-11 < efar["small"] < 2e-11
    assert 7e-10 < efar["aligned"] < H.CERT_GATE_FAR * (1.0 - H.CERT_GATE_BAND) and efar["refused"] > H.CERT_GATE_FAR * (1.0 + H.CERT_GATE_BAND)
    ex = H.cert_emulate(c, c["H"], c["K"], e1, e2, ff_err=c["p_inf"] * efar["exact"])
    assert H.cert_classes(c, ex)["sure"].sum() >= H.CERT_MIN_CLASS
    for s in ("small", "aligned"):
        em = H.cert_emulate(c, c["H"], c["K"], e1, e2, ff_err=c["p_inf"] * efar[s])
        assert not em["sure"].any() and not em["undetermined"].any()
        assert H.cert_classes(c, em)["accepted"].sum() >= H.CERT_MIN_CLASS
    # what an uncertified factored product would deliver for an aligned row breaks the claim: the pass has to deliver what it certified
    assert len(aligned) == H.CERT_FAR_ALIGNED and min(r for _, r in aligned) > 1.0


def test_the_evaluator_accepts_the_optimum_and_refuses_each_kind_of_wrong_result():
    c = H.cert_case("mini_cdu")
    b = int(np.argmax(c["kept"] & ((c["state"] == 1).sum(axis=1) > 0) & ((c["state"] == 0).sum(axis=1) > 0)))
    st = c["state"][b]
    one = lambda u, a: H.cert_property_a(c, dict(u=u[None], active=a[None], status=np.zeros(1, np.int32)), rows=[b], precise=True)
    good = one(c["xs"][b], c["active"][b])
    print(f"optimum: gradient/bar {good['ratio'][0]:.2e}, rounding slack/bar {good['slack']:.2e}")
    assert good["ok"].all() and good["slack"] < 0.01
    fr, up = int(np.flatnonzero(st == 0)[0]), int(np.flatnonzero(st == 1)[0])
    k, cc = up // c["nu"], up % c["nu"]
    cases = {}
    u = c["xs"][b].copy(); u[fr] += 1e-6
    cases["free-set gradient"] = (u, c["active"][b])
    a = c["active"][b].copy(); a[k * 2 * c["nu"] + cc] = False                    # the bound is dropped: u stays on it, the gradient there is not zero
    cases["free-set gradient (bit)"] = (c["xs"][b], a)
    a = c["active"][b].copy(); a[k * 2 * c["nu"] + cc] = False; a[k * 2 * c["nu"] + c["nu"] + cc] = True     # upper told as lower: wrong sign, off its bound
    cases["multiplier sign"] = (c["xs"][b], a)
    u = c["xs"][b].copy(); u[fr] = c["UB"][b][fr] + 2e-9
    cases["beyond a bound"] = (u, c["active"][b])
    u = c["xs"][b].copy(); u[fr] = np.nan
    cases["not finite"] = (u, c["active"][b])
    for name, (u, a) in cases.items():
        res = one(u, a)
        assert not res["ok"].any() and any(name.split(" (")[0] == w for _, w in res["why"]), (name, res["why"])
    # a row with another status may hold anything
    assert H.cert_property_a(c, dict(u=np.full((1, c["n"]), np.nan), active=c["active"][b][None], status=np.array([3], np.int32)), rows=[b])["ok"].all()
