"""The QP solver's certificates with inexact inverses and far-field factors, through the C ABI.

Every status 0 is "an optimum certified by fp64 KKT checks".  That rests on one bound,
bnd = 2 (e1max |x0|_1 + e2max |lam|_1) + 1e-14 (tqmax |x0|_1 + |lam|_1) [+ ff_err (|x0|_1 + |lam|_1)], in four kernels (asm_update_k,
asm_wide_k, asm_tail_k, asm_small_k), and on the check with P itself (asm_certify_k) for the rows the bound does not cover.  With an
inverse good to 1e-14 the answer is right whatever the certificate says, so here the inverse is NOT good: relative noise up to the
e2 < 1e-6 gate of nnmpc_qp_set_inverse, one scaled row and column, a Kunc off by 1e-3, far-field factors off by up to the 1e-9 gate.

A (soundness): every row of every call with status 0 satisfies the solver's own claim, evaluated with P in np.longdouble
   (helpers.cert_property_a).
B: the cheap certificate is taken exactly where the emulated bound allows it (asm_full_checks within the emulation's range).
C: rows whose emulated solution misses the stationarity bar by a factor 4 are rejected (the pass marks them 3, "not solved here",
   which a method-"asm" handle reports as NNMPC_ST_MAXITER) and solved by the PDIP path under "auto"; rows a factor 4 inside are
   accepted with the oracle's set.
B and C are about kept rows: far enough from a change of set that no inverse of the ladder can move it (helpers.cert_case).
tests/test_cpu_certificate_inputs.py holds the ladders, the emulation and the evaluator to their purpose without a GPU.
Lines starting with "CERT|" are the record profiles/cert_coverage.md was made from.
"""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu


def _qp(c, site, method, farfield=None):
    from industrial_nnmpc_2021_amd.qp import BatchedBoxQP
    opts = dict(H.CERT_SITES[site]["opts"])
    return BatchedBoxQP(c["P"], c["tq"], c["nu"], method=method, max_batch=512 if c["B"] > 128 else 128, farfield=farfield, **opts)


def _site_env(monkeypatch, site):
    monkeypatch.delenv("NNMPC_NO_SMALL", raising=False)
    for k, v in H.CERT_SITES[site]["env"].items():
        monkeypatch.setenv(k, v)


def _last_error():
    from industrial_nnmpc_2021_amd import _lib
    return _lib.load().nnmpc_last_error()


def _assert_claim(c, out, what):
    """Property A on every row of one call."""
    ev = H.cert_property_a(c, out)
    worst = float(ev["ratio"].max())
    print(f"CERT|{what}|claim|rows {int((out['status'] == 0).sum())}|worst gradient/bar {worst:.3e}|rounding slack/bar {ev['slack']:.2e}|longdouble rows {ev['ld_rows']}")
    assert ev["slack"] < 0.01
    assert ev["ok"].all(), (what, ev["why"][:8], worst)
    return worst


def _assert_sets_and_u(c, out, rows, tol_of, what):
    for b in np.flatnonzero(rows):
        assert out["status"][b] == 0, (what, b, out["status"][b])
        assert np.array_equal(out["active"][b], c["active"][b]), (what, b)
        err = np.abs(out["u"][b] - c["xs"][b]).max()
        assert err <= tol_of(b), (what, b, err, tol_of(b))


def _pdip_tol(c):
    return lambda b: H.CERT_PDIP_TOL * max(1.0, np.abs(c["xs"][b]).max())


def _check_pair(c, qa, qb, Hp, Kp, tag, site_reached):
    """One accepted pair (Hp, Kp) on the "asm" handle qa and the "auto" handle qb: A, B, C."""
    from industrial_nnmpc_2021_amd import _lib
    B = c["B"]
    for q in (qa, qb):
        assert q.set_inverse(Hp, Kp) == 0, _last_error()
    st0 = qa.stats()
    e1n, e2n = H.cert_errors(c, Hp, Kp)
    e1, e2 = st0["asm_e1max"], st0["asm_e2max"]
    r1, r2 = H.cert_errors_rounding(c, Hp, Kp)      # the device's figures are numpy's up to the rounding of the two products
    assert abs(e2 - e2n) <= r2 and abs(e1 - e1n) <= r1, (e1, e1n, r1, e2, e2n, r2)
    em = H.cert_emulate(c, Hp, Kp, e1, e2)
    cl = H.cert_classes(c, em)
    lo, hi = H.cert_full_check_range(c, em)
    qa.stats(reset=True)
    a = qa.solve_batch(c["x0"], c["lb"], c["ub"])
    sa = qa.stats()
    print(f"CERT|{tag}|asm|e1max {e1:.3e}|e2max {e2:.3e}|emulated sure {int(cl['sure'].sum())} accepted {int(cl['accepted'].sum())} rejected {int(cl['rejected'].sum())} "
          f"lost {int(cl['lost'].sum())}|status0 {int((a['status'] == 0).sum())} rejected {int((a['status'] == H.CERT_ST_REJECTED).sum())}|full checks {sa['asm_full_checks']} in {lo}..{hi}|"
          f"small passes {sa['asm_small_passes']} rounds {sa['asm_rounds']} far passes {sa['asm_far_passes']}|factorizations {sa['factorizations']}")
    site_reached(sa)
    assert sa["factorizations"] == 0                                    # method "asm": no PDIP solve behind a status
    _assert_claim(c, a, tag + "|asm")
    assert lo <= sa["asm_full_checks"] <= hi, (tag, sa["asm_full_checks"], lo, hi)
    assert (a["status"][cl["rejected"]] == H.CERT_ST_REJECTED).all(), (tag, np.flatnonzero(cl["rejected"] & (a["status"] != H.CERT_ST_REJECTED)))
    _assert_sets_and_u(c, a, cl["accepted"] | cl["sure"], lambda b: H.cert_u_tol(c, b), tag + "|asm")
    qb.stats(reset=True)
    b = qb.solve_batch(c["x0"], c["lb"], c["ub"])
    sb = qb.stats()
    print(f"CERT|{tag}|auto|status0 {int((b['status'] == 0).sum())}|asm solved {sb['asm_solved']}|pdip solved {B - sb['asm_solved']}|full checks {sb['asm_full_checks']}")
    assert (b["status"] == 0).all(), (tag, np.flatnonzero(b["status"]))
    _assert_claim(c, b, tag + "|auto")
    _assert_sets_and_u(c, b, cl["rejected"], _pdip_tol(c), tag + "|auto, rejected rows")
    _assert_sets_and_u(c, b, cl["accepted"] | cl["sure"], lambda r: H.cert_u_tol(c, r), tag + "|auto")
    return cl, a, b


def _reached(site):
    def check(st):
        if site in ("small", "small_ill"):
            assert st["asm_small_passes"] >= 1 and st["asm_far_passes"] == 0
        elif site == "wide":
            assert st["asm_small_passes"] == 0 and st["asm_rounds"] >= 1 and st["asm_far_passes"] == 0
        else:
            assert st["asm_small_passes"] == 0 and st["asm_far_passes"] == 0
            if site == "update":
                assert st["asm_rounds"] >= 1
    return check


@pytest.mark.parametrize("site", list(H.CERT_SITES))
def test_noise_ladder_at_every_certificate_site(monkeypatch, site):
    """Relative noise from 0 to the gate, then the rung the gate refuses; after the refusal the handle solves by the PDIP path alone,
    and an accepted inverse brings the active-set pass back."""
    from industrial_nnmpc_2021_amd import _lib
    _site_env(monkeypatch, site)
    c = H.cert_case(H.CERT_SITES[site]["plant"])
    rungs, above = H.CERT_LADDER[c["plant"]]
    qa, qb = _qp(c, site, "asm"), _qp(c, site, "auto")
    seen = dict(sure=0, accepted=0, rejected=0)
    for eps in rungs:
        cl, _, _ = _check_pair(c, qa, qb, *H.cert_perturb(c, eps), f"{site}|noise {eps:.0e}", _reached(site))
        for k in seen:
            seen[k] = max(seen[k], int(cl[k].sum()))
    assert seen["sure"] >= H.CERT_MIN_CLASS and (site == "small_ill" or min(seen.values()) >= H.CERT_MIN_CLASS), seen
    # ---- the rung above the gate, and the handle afterwards
    Hp, Kp = H.cert_perturb(c, above)
    rc = qb.set_inverse(Hp, Kp)
    assert rc == _lib.EINVAL and b"not usable" in _last_error(), (rc, _last_error())
    qb.stats(reset=True)
    out = qb.solve_batch(c["x0"], c["lb"], c["ub"])
    st = qb.stats()
    print(f"CERT|{site}|after the refused rung {above:.0e}|status0 {int((out['status'] == 0).sum())}|asm solved {st['asm_solved']}|small passes {st['asm_small_passes']} rounds {st['asm_rounds']}")
    assert (out["status"] == 0).all()
    _assert_claim(c, out, f"{site}|after the refused rung")
    # (correct by the claim every status 0 makes: the stationarity bar, through P_FF^-1, on top of the 1e-8 of an exact solve)
    _assert_sets_and_u(c, out, c["kept"], lambda b: H.cert_u_tol(c, b), f"{site}|after the refused rung")
    assert st["asm_solved"] == 0 and st["asm_small_passes"] == 0 and st["asm_rounds"] == 0      # no inverse: nothing of the refused pair is in use
    assert qb.set_inverse(c["H"], c["K"]) == 0
    qb.stats(reset=True)
    out = qb.solve_batch(c["x0"], c["lb"], c["ub"])
    assert (out["status"] == 0).all() and qb.stats()["asm_solved"] == c["B"]
    _assert_claim(c, out, f"{site}|restored")
    qa.close(); qb.close()


@pytest.mark.parametrize("site", ["small", "update", "tail", "wide"])
def test_one_scaled_row_and_column_sends_every_row_through_the_check_with_P(monkeypatch, site):
    """Row and column of a first-stage variable of Hinv scaled by 1 + 1e-7: e2max is global, so rows without that bound in their set
    -- whose x the scaling barely touches -- lose the cheap certificate too."""
    _site_env(monkeypatch, site)
    c = H.cert_case(H.CERT_SITES[site]["plant"])
    qa, qb = _qp(c, site, "asm"), _qp(c, site, "auto")
    j = H.cert_rowcol_index(c)
    cl, a, _ = _check_pair(c, qa, qb, *H.cert_perturb_rowcol(c, j), f"{site}|row and column {j}", _reached(site))
    assert not cl["sure"].any()                       # (property B then holds asm_full_checks to every kept row at least)
    qa.close(); qb.close()


@pytest.mark.parametrize("site", ["small", "update", "tail", "wide"])
def test_kunc_off_by_a_thousandth_is_accepted_and_nothing_wrong_leaves_with_status_0(monkeypatch, site):
    """e1 is only NaN-checked: the pair is accepted, the bound is far above the bar, nothing is certified by it, and the check with P
    refuses what the pass computes; "auto" solves everything by the PDIP path."""
    _site_env(monkeypatch, site)
    c = H.cert_case(H.CERT_SITES[site]["plant"])
    qa, qb = _qp(c, site, "asm"), _qp(c, site, "auto")
    cl, a, b = _check_pair(c, qa, qb, *H.cert_perturb_kunc(c), f"{site}|Kunc 1e-3", _reached(site))
    assert not cl["sure"].any() and not cl["accepted"].any()
    _assert_sets_and_u(c, b, c["kept"], _pdip_tol(c), f"{site}|Kunc 1e-3|auto")
    qa.close(); qb.close()


def _set_farfield(qp, W, U, Vx, Vl):
    from industrial_nnmpc_2021_amd import _lib
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    qp._ff_done.add(W)                                # the wrapper must not factor this window itself
    return _lib.load().nnmpc_qp_set_farfield(qp._h, W, U.shape[1], p(U), p(Vx), p(Vl))


def _far_windows(qp, c):
    """The windows this batch's full-width passes run at: a first call in the dense form, after which the wrapper factored them."""
    out = qp.solve_batch(c["x0"], c["lb"], c["ub"])
    assert (out["status"] == 0).all()
    windows = sorted(W for W, info in qp.farfield_info.items() if info.get("rank", 0) > 0)
    assert H.CERT_FAR_W in windows, qp.farfield_info
    return windows


def test_far_field_factors_enter_the_certificate_and_what_is_delivered_is_what_was_certified():
    """Factors off by 1e-11 and, rank one and aligned with one row's [x0; lam], by 8e-10: the bound grows by |P|_inf efar (|x0|_1 +
    |lam|_1), nothing that went through the far-field pass is certified by it, and what the check with P then sees -- the far
    variables again, from Pinv itself -- is what the caller gets.  Rows the device tail finishes (the stragglers of the rounds:
    all columns straight from Pinv) carry no far-field term and keep the cheap certificate, so the number of rows checked with P
    is the number the pass handled: the same for every inexact setting, and at least CERT_MIN_CLASS."""
    from industrial_nnmpc_2021_amd import _lib
    c = H.cert_case("mid_cdu")
    nu = c["nu"]
    qp = _qp(c, "wide", "asm", farfield="auto")
    windows = _far_windows(qp, c)
    e1, e2 = qp.stats()["asm_e1max"], qp.stats()["asm_e2max"]
    plain = H.cert_emulate(c, c["H"], c["K"], e1, e2)                 # the certificate of a row the pass did not handle
    settings = [("exact", None, None), ("small", None, None)] + [("aligned", r, g) for r, g in H.cert_far_aligned_rows(c)]
    through_pass = None
    for setting, row, predicted in settings:
        efar = 0.0
        for W in windows:
            Up, Vx, Vl, e = H.cert_farfield_perturbed(c, setting, row=row, W=W)
            assert _set_farfield(qp, W, Up, Vx, Vl) == 0, _last_error()
            efar = max(efar, e)
        em = H.cert_emulate(c, c["H"], c["K"], e1, e2, ff_err=c["p_inf"] * efar)
        cl = H.cert_classes(c, em)
        lo, hi = H.cert_full_check_range(c, plain)[0], H.cert_full_check_range(c, em)[1]
        qp.stats(reset=True)
        seq = qp.solve_batch(c["x0"], c["lb"], c["ub"])
        st = qp.stats()
        tag = f"far|{setting}" + ("" if row is None else f" with row {row}")
        print(f"CERT|{tag}|asm|windows {windows}|efar {efar:.3e} (numpy)|emulated sure {int(cl['sure'].sum())} accepted {int(cl['accepted'].sum())}|status0 {int((seq['status'] == 0).sum())}|"
              f"full checks {st['asm_full_checks']} in {lo}..{hi}|small passes {st['asm_small_passes']} rounds {st['asm_rounds']} far passes {st['asm_far_passes']}")
        assert st["asm_far_passes"] >= 1 and st["factorizations"] == 0
        if row is not None:
            print(f"CERT|{tag}|gradient/bar {H.cert_property_a(c, seq)['ratio'][row]:.3e} delivered, {predicted:.2f} had the factored far columns been delivered")
        _assert_claim(c, seq, tag)                                    # on the DELIVERED u
        assert lo <= st["asm_full_checks"] <= hi, (tag, st["asm_full_checks"], lo, hi)
        _assert_sets_and_u(c, seq, cl["sure"] | cl["accepted"], lambda b: H.cert_u_tol(c, b), tag)
        if setting == "exact":
            assert cl["sure"].sum() >= H.CERT_MIN_CLASS
        else:
            assert not cl["sure"].any() and (seq["status"] == 0).all()      # nothing the pass handled is sure; checked with P and accepted
            if through_pass is None:
                through_pass = st["asm_full_checks"]
            assert st["asm_full_checks"] == through_pass >= H.CERT_MIN_CLASS + lo, (tag, st["asm_full_checks"], through_pass, lo)
        fm = qp.solve_batch(c["x0"], c["lb"], c["ub"], first_move_only=True)
        assert np.array_equal(fm["status"], seq["status"]) and np.array_equal(fm["active"], seq["active"])
        ok = seq["status"] == 0
        assert np.abs(fm["u"][ok] - seq["u"][ok][:, :nu]).max() <= 1e-12
    Up, Vx, Vl, efar = H.cert_farfield_perturbed(c, "refused")
    rc = _set_farfield(qp, H.CERT_FAR_W, Up, Vx, Vl)
    assert rc == _lib.EINVAL and b"not usable" in _last_error()
    qp.close()


def test_a_second_inverse_releases_the_far_field_factors_and_queues_their_windows():
    """The factors and their verified error belong to the inverse they were checked against: after an accepted
    nnmpc_qp_set_inverse the next call runs in the dense form and the window is asked for again."""
    from industrial_nnmpc_2021_amd import _lib
    c = H.cert_case("mid_cdu")
    W = H.CERT_FAR_W
    qp = _qp(c, "wide", "asm", farfield="auto")
    _far_windows(qp, c)
    qp.stats(reset=True)
    out = qp.solve_batch(c["x0"], c["lb"], c["ub"])
    assert qp.stats()["asm_far_passes"] >= 1 and (out["status"] == 0).all()
    src = qp._ff_src
    assert qp.set_inverse(*H.cert_perturb(c, 1e-13)) == 0
    assert qp._ff_done == set()
    qp._ff_src = None                                 # (the wrapper does not poll: the queue is read below)
    qp.stats(reset=True)
    out = qp.solve_batch(c["x0"], c["lb"], c["ub"])
    assert qp.stats()["asm_far_passes"] == 0 and (out["status"] == 0).all()
    _assert_claim(c, out, "far|after a second inverse")
    missing, w = [], C.c_int32(0)
    for _ in range(17):
        _lib.check(_lib.load().nnmpc_qp_farfield_missing(qp._h, C.byref(w)), "nnmpc_qp_farfield_missing")
        if not w.value:
            break
        missing.append(w.value)
    assert W in missing, missing
    # ... and with the wrapper polling again the window is factored from the new inverse and the pass is back in the far-field form
    qp._ff_src = src
    assert qp.set_inverse(c["H"], c["K"]) == 0
    qp.solve_batch(c["x0"], c["lb"], c["ub"])
    assert W in qp._ff_done and qp.farfield_info[W]["rank"] > 0
    qp.stats(reset=True)
    out = qp.solve_batch(c["x0"], c["lb"], c["ub"])
    assert qp.stats()["asm_far_passes"] >= 1 and (out["status"] == 0).all()
    _assert_claim(c, out, "far|factored again")
    qp.close()
