"""What the tangent-loss tests share (tests/test_cpu_tan_inputs.py, tests/test_tan_train_gpu.py): the reference -- the loss

    L = mean (pred - u)^2 + w mean (J d - t)^2

of the structured network and its Keras-order gradients in stock torch on the CPU, by the explicit propagation
a'_0 = [dx, (duprev), 0, 0], a'_l = (a'_{l-1} W_l) * [a_l(pass 1) > 0], J d = a'_{L-1} W_L with the masks as constants --
never the code under test (train.tangent_loss is compared WITH it) --, its three deliberately wrong variants, the tangent
inputs of the parity cases, and the exact case: small integer / dyadic data for which every f32 quantity of the native step
is exact, with the int64 recomputation that proves it."""
import numpy as np

from tests.test_train_hip_gpu import FILL, _f32, _kink_free, _weights

W_TAN = 0.5
VARIANTS = ("own", "pass2", "bias")   # mask from the tangent's own sign; mask from pass 2; a bias added to the tangent rows
CASES = {                             # nx, nu, uprev, hidden widths, B
    "a": (5, 3, True, [70, 130, 70], 200),       # NB 128 pair tiles and the 64-wide head
    "b": (5, 3, True, [70, 130, 70], 1),         # a single row
    "c": (12, 6, True, [224, 240, 224], 129),    # one row in the second row tile
    "d": (7, 4, False, [40, 64], 128),           # every layer in the NB 64 class, no uprev
    "e": (5, 3, True, [70, 130, 70], 600),       # NNMPC_TRAIN_DW_SLICES=3: three slices of the 1920 stacked rows
}


def stack(d, rows, uprev):
    """(z1, z2, a'_0) of dataset rows ``rows`` as float64 numpy arrays."""
    x, xs, us = d["x"][rows], d["xs"][rows], d["us"][rows]
    zx, zu = np.zeros_like(xs), np.zeros_like(us)
    if uprev:
        return (np.hstack((x, d["uprev"][rows], xs, us)), np.hstack((xs, us, xs, us)),
                np.hstack((d["dx"][rows], d["duprev"][rows], zx, zu)))
    return np.hstack((x, xs, us)), np.hstack((xs, xs, us)), np.hstack((d["dx"][rows], zx, zu))


def ref_loss_grad(W, uprev, d, rows, w, dtype=None, variant=None):
    """(L, mse, tan_mse, Keras-order gradients) at the Keras-order weights W on dataset rows ``rows`` of d = dict(x, uprev,
    xs, us, u, dx, duprev, du), in torch ``dtype`` (default float64) on the CPU.  ``variant``: one of VARIANTS, a wrong reference."""
    import torch
    dtype = dtype or torch.float64
    P = [torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in W]
    z1, z2, ta = (torch.as_tensor(a, dtype=dtype) for a in stack(d, rows, uprev))
    us, u, t = (torch.as_tensor(d[k][rows], dtype=dtype) for k in ("us", "u", "du"))
    a1, a2 = z1, z2
    for l in range(0, len(P) - 1, 2):
        p1, p2, tz = a1 @ P[l] + P[l + 1], a2 @ P[l] + P[l + 1], ta @ P[l]
        if variant == "bias":
            tz = tz + P[l + 1]
        src = {None: p1, "bias": p1, "own": tz, "pass2": p2}[variant]
        ta = tz * (~(src <= 0)).to(dtype)                       # derivative 0 at 0, a NaN passes; a constant of the backward pass
        a1, a2 = torch.relu(p1), torch.relu(p2)
    mse = torch.mean((us + a1 @ P[-1] - a2 @ P[-1] - u) ** 2)
    tan = torch.mean((ta @ P[-1] - t) ** 2)
    L = mse + w * tan
    L.backward()
    g = [np.zeros(tuple(p.shape)) if p.grad is None else p.grad.double().numpy().copy() for p in P]
    return float(L.detach()), float(mse.detach()), float(tan.detach()), g


def add_tangents(d, nx, nu, rng):
    """Standard-normal directions and targets of the size a local gain gives, f32-representable, for every row of d."""
    n = d["x"].shape[0]
    out = dict(d)
    out["dx"], out["duprev"] = _f32(rng.standard_normal((n, nx))), _f32(rng.standard_normal((n, nu)))
    out["du"] = _f32(0.5 * rng.standard_normal((n, nu)))
    return out


def case(name):
    """(W, d with tangents, rows) of parity case ``name``: kink-free rows by the rule of tests/test_train_hip_gpu.py."""
    nx, nu, uprev, hidden, B = CASES[name]
    rng = np.random.default_rng(300 + ord(name))
    W = _weights(nx, nu, uprev, hidden, rng)
    d = add_tangents(_kink_free(W, nx, nu, uprev, B, rng), nx, nu, rng)
    return W, d, FILL + rng.permutation(B)


# ---- the exact case ----

EXACT = {"narrow": [24, 40], "wide": [24, 130, 24]}            # all widths <= 64; a 130-wide layer
EX_NX, EX_NU, EX_B = 3, 2, 64
UNIT = 2.0 ** -8                                                # every f32 quantity of the step is a multiple of it


def exact_case(name):
    """(W, d, rows): nx 3, nu 2, with uprev, B = 64, w = 0.5, so gscale = 2^-6 and gscale w = 2^-7.  Weights in {-1, 0, 1},
    sparse; x, uprev, xs, us and the directions small integers, u and the targets half-integers.  The first-layer biases of
    units 0..5 cancel row 0's pass-1 pre-activation exactly (a zero in a known place: the derivative there is 0), the others
    are small integers, so pre-activations of both signs occur, and pass 2 (fed xs, us instead of x, uprev) has other signs."""
    hidden = EXACT[name]
    rng = np.random.default_rng(40 + len(hidden))
    nx, nu, n = EX_NX, EX_NU, EX_B
    dims = [2 * nx + 2 * nu] + hidden + [nu]
    ri = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape).astype(np.float64)
    d = dict(x=ri(-2, 2, (n, nx)), uprev=ri(-1, 1, (n, nu)), xs=ri(-1, 1, (n, nx)), us=ri(-1, 1, (n, nu)),
             u=ri(-4, 4, (n, nu)) / 2, dx=ri(-1, 1, (n, nx)), duprev=ri(-1, 1, (n, nu)), du=ri(-4, 4, (n, nu)) / 2)
    W = []
    for l in range(len(dims) - 1):
        dens = 0.5 if l == 0 else 4.0 / dims[l]
        W.append(ri(-1, 1, (dims[l], dims[l + 1])) * (rng.random((dims[l], dims[l + 1])) < dens))
        if l < len(dims) - 2:
            W.append(ri(-1, 1, dims[l + 1]))
    z1 = stack(d, np.arange(n), True)[0]
    W[1][:6] = -(z1[0] @ W[0])[:6]
    return W, d, rng.permutation(n)


def exact_int(W, d, rows, w=W_TAN, variant=None):
    """The exact case recomputed in int64.  Every quantity the step forms in f32 -- activations, tangents, pred - u, dZ, dZ',
    dW, db -- is held as an integer count of UNIT; each product has one operand that is integer-valued as it stands (the
    weights, or the activations and tangents under dW), so the counts multiply without a scale.  Returns (L, mse, tan_mse,
    Keras-order gradients) as float64 and ``peak``: the largest absolute-value sum, sum_k |a_k| |b_k| over the terms of any
    entry of any such product or column sum, as a count of UNIT.  Below 2^24 every partial sum of every entry is a multiple
    of UNIT smaller than 2^24 UNIT, so f32 holds it exactly whatever the order of summation."""
    S = int(round(1 / UNIT))
    units = lambda a: np.rint(np.asarray(a) * S).astype(np.int64)
    assert all((units(d[k]) == np.asarray(d[k]) * S).all() for k in d)
    Wi = [np.rint(a).astype(np.int64) for a in W]
    assert all((wi == a).all() for wi, a in zip(Wi, W))
    B, nu, L = len(rows), d["us"].shape[1], (len(W) + 1) // 2
    peak = 0

    def mm(a, b):                                                # a @ b, its absolute-value sum folded into peak
        nonlocal peak
        peak = max(peak, int((np.abs(a) @ np.abs(b)).max()))
        return a @ b

    A1, A2, TA = ([units(a)] for a in stack(d, rows, True))     # inputs of layer i, as counts
    masks = []
    for i in range(L - 1):
        Wl, bl = Wi[2 * i], Wi[2 * i + 1] * S
        p1, p2, tz = mm(A1[-1], Wl) + bl, mm(A2[-1], Wl) + bl, mm(TA[-1], Wl)
        if variant == "bias":
            tz = tz + bl
        src = {None: p1, "bias": p1, "own": tz, "pass2": p2}[variant]
        masks.append((p1 > 0, p2 > 0, src > 0))
        A1.append(np.maximum(p1, 0)); A2.append(np.maximum(p2, 0)); TA.append(tz * (src > 0))
        peak = max(peak, int(np.abs(p1).max()), int(np.abs(p2).max()), int(np.abs(tz).max()))
    e = units(d["us"][rows]) + (mm(A1[-1], Wi[-1]) - mm(A2[-1], Wi[-1])) - units(d["u"][rows])
    et = mm(TA[-1], Wi[-1]) - units(d["du"][rows])
    mse, tan = float((e * e).sum()) / S ** 2 / (B * nu), float((et * et).sum()) / S ** 2 / (B * nu)
    den = B * nu // 2                                            # dZ_L = 2 e / (B nu), dZ'_L = 2 w et / (B nu): whole counts
    assert w == 0.5 and (e % den == 0).all() and (et % (2 * den) == 0).all()
    dz = [e // den, -(e // den), et // (2 * den)]
    grads = [None] * len(W)
    for i in range(L - 1, -1, -1):
        grads[2 * i] = mm(np.vstack((A1[i], A2[i], TA[i])).T // S, np.vstack(dz)).astype(np.float64) * UNIT
        assert all((a % S == 0).all() for a in (A1[i], A2[i], TA[i]))
        if i < L - 1:
            db = [a for a in (dz if variant == "bias" else dz[:2])]
            peak = max(peak, int(sum(np.abs(a).sum(0) for a in db).max()))
            grads[2 * i + 1] = sum(a.sum(0) for a in db).astype(np.float64) * UNIT
        if i > 0:
            m1, m2, ms = masks[i - 1]
            mt = ms if variant in ("own", "pass2") else m1
            dz = [mm(dz[0], Wi[2 * i].T) * m1, mm(dz[1], Wi[2 * i].T) * m2, mm(dz[2], Wi[2 * i].T) * mt]
    return mse + w * tan, mse, tan, grads, peak
