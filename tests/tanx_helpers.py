"""What the tests of the tangent loss with several directions per row and whole-input directions share
(tests/test_cpu_tanx_inputs.py, tests/test_tanx_train_gpu.py): the reference -- the loss

    L = mean over B nu of (pred - u)^2 + w mean over B D nu of (J d - t)^2

of the structured network and its Keras-order gradients in stock torch float64 on the CPU, written out explicitly:
  partial input   a'_0 = [dx, (duprev), 0, 0],      a'_l = (a'_{l-1} W_l) * [a_l(pass 1) > 0],  J d = a'_{L-1} W_L
  whole input     a'_0 = [dx, (duprev), dxs, dus]   under the masks of pass 1,
                  a''_0 = [dxs, (dus), dxs, dus]    under the masks of pass 2,               J d = dus + (a'_{L-1} W_L - a''_{L-1} W_L)
with the masks as constants -- never train.tangent_loss and never the library --, its four deliberately wrong variants, the
tangent inputs of the parity cases (data builders of tests/tan_helpers.py) and the exact case: integer / dyadic data with
D = 2 and whole input for which every f32 quantity of the native step is exact, with the int64 recomputation that proves it."""
import numpy as np

from tests import tan_helpers as H
from tests.test_train_hip_gpu import FILL, _f32, _kink_free, _weights

W_TAN = H.W_TAN
CASES = H.CASES
# pass-2 tangents masked by pass 1; directions d >= 1 of pass 1 masked by the other primal block (pass 2); the dus term left
# out of J d; the tangent mean over B nu instead of B D nu
VARIANTS = ("pass2_by_pass1", "dir_other_block", "no_dus", "mean_B_nu")
RUNS = [("a", 3, False), ("a", 2, True), ("b", 2, True), ("c", 3, True), ("d", 2, True), ("d", 5, False)]   # case, D, whole input
RUN_E = ("e", 2, True)                                                                                    # NNMPC_TRAIN_DW_SLICES=3


def stacked_rows(Bp, D, whole):
    return (2 + (2 if whole else 1) * D) * Bp


def inputs(d, rows, uprev, whole):
    """(z1, z2, a'_0 (B, D, din), a''_0 (B, D, din) or None) of dataset rows ``rows`` as float64 numpy arrays."""
    x, xs, us = d["x"][rows], d["xs"][rows], d["us"][rows]
    dx = d["dx"][rows]
    zx, zu = np.zeros_like(dx), np.zeros_like(d["du"][rows])
    sx, su = (d["dxs"][rows], d["dus"][rows]) if whole else (zx, zu)
    if uprev:
        z1, z2 = np.hstack((x, d["uprev"][rows], xs, us)), np.hstack((xs, us, xs, us))
        ta, tb = np.concatenate((dx, d["duprev"][rows], sx, su), -1), np.concatenate((sx, su, sx, su), -1)
    else:
        z1, z2 = np.hstack((x, xs, us)), np.hstack((xs, xs, us))
        ta, tb = np.concatenate((dx, sx, su), -1), np.concatenate((sx, sx, su), -1)
    return z1, z2, ta, (tb if whole else None)


def ref_loss_grad(W, uprev, d, rows, w, dtype=None, variant=None):
    """(L, mse, tan_mse, Keras-order gradients) at the Keras-order weights W on dataset rows ``rows`` of d = dict(x, uprev, xs,
    us, u, dx, duprev, du (n, D, .), and for the whole-input form dxs, dus (n, D, .)), in torch ``dtype`` (default float64) on
    the CPU.  ``variant``: one of VARIANTS, a wrong reference."""
    import torch
    dtype = dtype or torch.float64
    whole = d.get("dxs") is not None
    P = [torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in W]
    z1, z2, ta, tb = (None if a is None else torch.as_tensor(a, dtype=dtype) for a in inputs(d, rows, uprev, whole))
    us, u, t = (torch.as_tensor(d[k][rows], dtype=dtype) for k in ("us", "u", "du"))
    D = t.shape[1]
    a1, a2 = z1, z2
    for l in range(0, len(P) - 1, 2):
        p1, p2 = a1 @ P[l] + P[l + 1], a2 @ P[l] + P[l + 1]
        m1, m2 = (~(p1 <= 0)).to(dtype)[:, None, :], (~(p2 <= 0)).to(dtype)[:, None, :]   # derivative 0 at 0, a NaN passes; constants
        ma = m1
        if variant == "dir_other_block":
            ma = torch.cat((m1, m2.expand(-1, D - 1, -1)), 1)
        ta = (ta @ P[l]) * ma
        if whole:
            tb = (tb @ P[l]) * (m1 if variant == "pass2_by_pass1" else m2)
        a1, a2 = torch.relu(p1), torch.relu(p2)
    mse = torch.mean((us + a1 @ P[-1] - a2 @ P[-1] - u) ** 2)
    jd = ta @ P[-1]
    if whole:
        jd = jd - tb @ P[-1]
        if variant != "no_dus":
            jd = torch.as_tensor(d["dus"][rows], dtype=dtype) + jd
    tan = torch.mean((jd - t) ** 2)
    if variant == "mean_B_nu":
        tan = tan * D
    L = mse + w * tan
    L.backward()
    g = [np.zeros(tuple(p.shape)) if p.grad is None else p.grad.double().numpy().copy() for p in P]
    return float(L.detach()), float(mse.detach()), float(tan.detach()), g


def add_tangents(d, nx, nu, rng, D, whole):
    """Standard-normal directions and targets of the size a local gain gives, f32-representable, D per row of d."""
    n = d["x"].shape[0]
    out = {k: v for k, v in d.items() if k not in ("dx", "duprev", "du", "dxs", "dus")}
    out["dx"], out["duprev"] = _f32(rng.standard_normal((n, D, nx))), _f32(rng.standard_normal((n, D, nu)))
    out["du"] = _f32(0.5 * rng.standard_normal((n, D, nu)))
    if whole:
        out["dxs"], out["dus"] = _f32(rng.standard_normal((n, D, nx))), _f32(rng.standard_normal((n, D, nu)))
    return out


def case(name, D, whole):
    """(W, d with tangents, rows) of parity case ``name`` at D directions: kink-free rows by the rule of tests/test_train_hip_gpu.py."""
    nx, nu, uprev, hidden, B = CASES[name]
    rng = np.random.default_rng(700 + ord(name) + 16 * D + int(whole))
    W = _weights(nx, nu, uprev, hidden, rng)
    d = add_tangents(_kink_free(W, nx, nu, uprev, B, rng), nx, nu, rng, D, whole)
    return W, d, FILL + rng.permutation(B)


def repeat_rows(d, D):
    """The dataset that repeats each row D times, one direction each: what a one-direction handle needs for the same tangents."""
    out = {}
    for k, v in d.items():
        out[k] = v.reshape(-1, v.shape[-1]) if k in ("dx", "duprev", "du") else np.repeat(v, D, axis=0)
    return out


# ---- the exact case ----

EXACT = H.EXACT
EX_NX, EX_NU, EX_B, EX_D, EX_W = H.EX_NX, H.EX_NU, H.EX_B, 2, 1.0
UNIT = H.UNIT


def exact_case(name):
    """(W, d, rows): tan_helpers.exact_case (nx 3, nu 2, with uprev, B = 64; its weights, biases, x, uprev, xs, us, u: the
    zeros of row 0's pass-1 pre-activation in units 0..5, both signs, a pass 2 with other signs) with D = 2 whole-input
    directions: dx, duprev, dxs, dus small integers, the targets half-integers.  w = 1 and B D nu = 256, so the tangent rows'
    upstream gradient 2 w (J d - t) / (B D nu) = (J d - t) 2^-7 is a whole count of UNIT = 2^-8, as 2 (pred - u) / (B nu) is."""
    W, d, rows = H.exact_case(name)
    rng = np.random.default_rng(90 + len(EXACT[name]))
    n, D = EX_B, EX_D
    ri = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape).astype(np.float64)
    d = {k: v for k, v in d.items() if k not in ("dx", "duprev", "du")}
    d.update(dx=ri(-1, 1, (n, D, EX_NX)), duprev=ri(-1, 1, (n, D, EX_NU)), dxs=ri(-1, 1, (n, D, EX_NX)),
             dus=ri(-1, 1, (n, D, EX_NU)), du=ri(-4, 4, (n, D, EX_NU)) / 2)
    return W, d, rows


def exact_int(W, d, rows, w=EX_W, variant=None):
    """The exact case recomputed in int64, as tan_helpers.exact_int does for one direction: every quantity the step forms in
    f32 is an integer count of UNIT, each product has one integer-valued operand, and ``peak`` is the largest absolute-value sum
    over the terms of any entry of any product or column sum.  Below 2^24 f32 holds every partial sum exactly whatever the
    order.  Returns (L, mse, tan_mse, Keras-order gradients as float64, peak)."""
    S = int(round(1 / UNIT))
    units = lambda a: np.rint(np.asarray(a) * S).astype(np.int64)
    assert all((units(d[k]) == np.asarray(d[k]) * S).all() for k in d)
    Wi = [np.rint(a).astype(np.int64) for a in W]
    assert all((wi == a).all() for wi, a in zip(Wi, W))
    B, nu, L, D = len(rows), d["us"].shape[1], (len(W) + 1) // 2, d["du"].shape[1]
    peak = 0

    def mm(a, b):
        nonlocal peak
        peak = max(peak, int((np.abs(a) @ np.abs(b)).max()))
        return a @ b

    z1, z2, ta, tb = inputs(d, rows, True, True)
    A1, A2 = [units(z1)], [units(z2)]
    TA, TB = [[units(ta[:, k])] for k in range(D)], [[units(tb[:, k])] for k in range(D)]
    masks = []
    for i in range(L - 1):
        Wl, bl = Wi[2 * i], Wi[2 * i + 1] * S
        p1, p2 = mm(A1[-1], Wl) + bl, mm(A2[-1], Wl) + bl
        m1, m2 = p1 > 0, p2 > 0
        ma = [m2 if (variant == "dir_other_block" and k >= 1) else m1 for k in range(D)]
        mb = m1 if variant == "pass2_by_pass1" else m2
        masks.append((m1, m2, ma, mb))
        A1.append(np.maximum(p1, 0)); A2.append(np.maximum(p2, 0))
        for k in range(D):
            TA[k].append(mm(TA[k][-1], Wl) * ma[k]); TB[k].append(mm(TB[k][-1], Wl) * mb)
        peak = max(peak, int(np.abs(p1).max()), int(np.abs(p2).max()))
    e = units(d["us"][rows]) + (mm(A1[-1], Wi[-1]) - mm(A2[-1], Wi[-1])) - units(d["u"][rows])
    et = []
    for k in range(D):
        j = mm(TA[k][-1], Wi[-1]) - mm(TB[k][-1], Wi[-1])
        if variant != "no_dus":
            j = units(d["dus"][rows][:, k]) + j
        et.append(j - units(d["du"][rows][:, k]))
    mse = float((e * e).sum()) / S ** 2 / (B * nu)
    tan = float(sum((a * a).sum() for a in et)) / S ** 2 / (B * nu * (1 if variant == "mean_B_nu" else D))
    den = B * nu // 2                                            # dZ_L = 2 e / (B nu): whole counts
    dent = den * (1 if variant == "mean_B_nu" else D)            # dZ'_L = 2 w et / (B D nu), w = 1
    assert w == 1.0 and (e % den == 0).all() and all((a % dent == 0).all() for a in et)
    dz = [e // den, -(e // den)] + [a // dent for a in et] + [-(a // dent) for a in et]
    grads = [None] * len(W)
    for i in range(L - 1, -1, -1):
        acts = [A1[i], A2[i]] + [TA[k][i] for k in range(D)] + [TB[k][i] for k in range(D)]
        assert all((a % S == 0).all() for a in acts)
        grads[2 * i] = mm(np.vstack(acts).T // S, np.vstack(dz)).astype(np.float64) * UNIT
        if i < L - 1:
            peak = max(peak, int((np.abs(dz[0]).sum(0) + np.abs(dz[1]).sum(0)).max()))
            grads[2 * i + 1] = (dz[0].sum(0) + dz[1].sum(0)).astype(np.float64) * UNIT
        if i > 0:
            m1, m2, ma, mb = masks[i - 1]
            mk = [m1, m2] + ma + [mb] * D
            dz = [mm(a, Wi[2 * i].T) * m for a, m in zip(dz, mk)]
    return mse + w * tan, mse, tan, grads, peak
