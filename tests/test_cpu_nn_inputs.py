"""CPU-side guard of the NN parity tests' inputs (no GPU): judged with the fp64 oracle alone, the generators of
tests/test_nn_paths_gpu.py and tests/test_closed_loop_nn_gpu.py
  * leave at most 5 % of the compared entries on a bound wherever bounds are passed (a clipped entry equals the oracle
    whatever a kernel computed),
  * give every output column a scale (max |ref[:, col]| > 0: a relative check of an all-zero column is vacuous),
  * leave the plain-bf16 tolerance reachable: the numpy forward with the bf16 path's roundings is within 3e-2 - 4e-3 of the
    oracle per column, so a kernel within 4e-3 of that forward (what the GPU test asserts) meets the 3e-2 it asserts as well;
and helpers.bf16_round is a bit-level round-to-nearest-even."""
import struct

import numpy as np
import pytest

from tests import helpers as H


@pytest.mark.parametrize("i", range(len(H.NN_SHAPE_CASES)), ids=[c[0] for c in H.NN_SHAPE_CASES])
def test_shape_matrix_inputs(i):
    name, hidden, nx, nu, withu, xsc, B, mb, dev = H.NN_SHAPE_CASES[i]
    c = H.nn_shape_case(i)
    assert c["dims"][0] == 2 * nx + (2 if withu else 1) * nu and c["ref"].shape == (B, nu)
    assert np.isfinite(c["ref"]).all()
    scale = np.abs(c["ref"]).max(axis=0)
    assert (scale > 0).all(), name
    assert (np.abs(c["ref"] - c["us"]).max(axis=0) > 0).all() or B == 1, name    # the networks contribute to every column
    emu = H.bf16_forward(c["W"], c["x"], c["uprev"], c["xs"], c["us"], c["xscale"])
    assert (H.col_err(emu, c["ref"]) <= 3e-2 - 4e-3).all(), (name, H.col_err(emu, c["ref"]).max())


def test_shape_matrix_covers_every_axis_value():
    """Every value the shape matrix is meant to contain does appear (so a later edit cannot quietly drop one)."""
    cs = H.NN_SHAPE_CASES
    widths = {w for c in cs for w in c[1]}
    assert {1, 63, 64, 65, 127, 128, 129, 130, 200, 384, 385, 415, 416, 417, 831, 832, 833, 1024} <= widths
    assert {len(c[1]) for c in cs} >= {0, 1, 3, 5}
    assert {c[3] for c in cs} >= {1, 5, 32, 64, 65, 80}
    for h in ([832, 416, 64], [64, 832], [130, 417, 200]):
        assert any(c[1] == h for c in cs)
    din = [2 * c[2] + (2 if c[4] else 1) * c[3] for c in cs]
    assert any(d % 64 == 0 for d in din) and any(d % 64 for d in din)
    assert {c[4] for c in cs} == {True, False} and {c[5] for c in cs} == {True, False}
    for mb in (128, 256):
        assert {c[6] for c in cs if c[7] == mb} >= {mb - 1, mb, mb + 1, 3 * mb + 7}
    assert {c[6] for c in cs} >= {1, 127, 128, 129}
    assert sum(c[8] for c in cs) == 2


@pytest.mark.parametrize("net_i", range(len(H.NN_PROPERTY_NETS)), ids=[n[0] for n in H.NN_PROPERTY_NETS])
def test_bounded_inputs_stay_within_the_cap(net_i):
    """The bounded cases of test_nn_paths_gpu (seeds 40.., 50.., 70..; bounds -1 / +1, NN_BOUNDED_EPS from the steady state):
    at most 5 % of the oracle's entries on a bound, and the networks still move u off us by far more than the f32 tolerance."""
    name, hidden, nx, nu, withu = H.NN_PROPERTY_NETS[net_i]
    for seed, B in ((40 + net_i, 300), (50 + net_i, 129), (70 + net_i, 200)):
        c = H.nn_case(seed, hidden, nx, nu, withu, B, eps=H.NN_BOUNDED_EPS, ulb=-np.ones(nu), uub=np.ones(nu))
        assert c["share"] <= 0.05, (name, seed, c["share"])
        assert (np.abs(c["ref"]).max(axis=0) > 0).all()
        assert (np.abs(c["ref"] - c["us"]).max(axis=0) > 1e-2).all(), name


def test_clip_case_puts_a_third_on_each_side():
    name, hidden, nx, nu, withu = H.NN_PROPERTY_NETS[0]
    c = H.nn_case(80, hidden, nx, nu, withu, 300)
    lb, ub = np.quantile(c["ref"], 1 / 3, axis=0), np.quantile(c["ref"], 2 / 3, axis=0)
    assert (lb < ub).all()
    r = np.minimum(np.maximum(c["ref"], lb), ub)
    assert 0.3 < (r == lb).mean() < 0.37 and 0.3 < (r == ub).mean() < 0.37


@pytest.mark.parametrize("j", range(len(H.CL_NN_MIX)), ids=[n[0] for n in H.CL_NN_MIX])
def test_closed_loop_mix_networks(j):
    """The closed-loop mix on the mini_cstrs sizes (Nx = 6, Nu = 3).  The loop's own inputs exist only after a device run (the GPU
    test asserts the cap on them); here: inputs at the loop's scale (|xhat - xs| ~ 0.1, bounds -1 / +1) stay within the cap, every
    column has a scale and the network moves it by more than 100 x the f32 tolerance."""
    from oracle import nn as onn
    name, hidden, withu, ninst = H.CL_NN_MIX[j]
    nx, nu = 6, 3
    din = 2 * nx + (2 if withu else 1) * nu
    W = H.cl_nn_weights(300 + j, din, hidden, nu)
    assert [w.shape for w in W[0::2]] == [(a, b) for a, b in zip([din] + hidden, hidden + [nu])]
    assert max([din] + hidden) <= 2048
    rng = np.random.default_rng(j)
    B = 200
    xs, us = 0.1 * rng.standard_normal((B, nx)), rng.uniform(-0.3, 0.3, (B, nu))
    x, up = xs + 0.1 * rng.standard_normal((B, nx)), us + 0.1 * rng.uniform(-1, 1, (B, nu))
    xscale = rng.uniform(0.5, 2.0, nx)
    free = onn.control_input(W, x, up, xs, us, xscale, None, None, withu)
    ref = onn.control_input(W, x, up, xs, us, xscale, -np.ones(nu), np.ones(nu), withu)
    assert H.share_on_bound(ref, -np.ones(nu), np.ones(nu)) <= 0.05
    assert (np.abs(free).max(axis=0) > 0).all() and (np.abs(free - us).max(axis=0) > 1e-2).all()


def test_closed_loop_mix_covers_every_axis_value():
    mix = H.CL_NN_MIX
    assert {w for n in mix for w in n[1]} >= {40, 64, 65, 130, 832, 1024, 2048}
    assert {len(n[1]) + 1 for n in mix} >= {1, 2, 3, 5}
    assert {n[2] for n in mix} == {True, False}
    assert {n[3] for n in mix} >= {1, 3, 8, 9}
    assert (2 * 6 + 2 * 3) % 4 and (2 * 6 + 3) % 4               # first-layer K of both layouts: uneven K slices


def _rne_bits(bits):
    """bf16 bits of an f32 bit pattern by exact integer arithmetic: the upper half, plus one if the lower half is beyond
    a half ulp, or exactly a half ulp with an odd upper half."""
    hi, lo = bits >> 16, bits & 0xFFFF
    if (bits & 0x7F800000) == 0x7F800000 and (bits & 0x007FFFFF):
        return None                                             # NaN
    if lo > 0x8000 or (lo == 0x8000 and (hi & 1)):
        hi += 1                                                 # (the carry may run into the exponent: the next binade, or Inf)
    return hi & 0xFFFF


def test_bf16_round_is_round_to_nearest_even():
    rng = np.random.default_rng(0)
    bits = list(rng.integers(0, 1 << 32, 3000, dtype=np.uint64))
    bits += [(int(h) << 16) | 0x8000 for h in rng.integers(0, 1 << 16, 600)]                 # ties, odd and even upper halves
    bits += [(int(h) << 16) | l for h in rng.integers(0, 1 << 16, 200) for l in (0x7FFF, 0x8001, 0x0000, 0xFFFF)]
    bits += [int(b) for b in rng.integers(0, 1 << 23, 300)] + [0x80000000 | int(b) for b in rng.integers(0, 1 << 23, 300)]   # subnormals
    bits += [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,               # +-0, +-Inf, largest
             0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFFFFFFFF, 0xFFFF8000, 0x00008000, 0x00018000, 0x007FFFFF]   # NaNs, smallest ties
    bits = np.array(bits, dtype=np.uint64).astype(np.uint32)
    got = H.bf16_round(bits.view(np.float32))
    assert got.dtype == np.float32 and got.shape == bits.shape
    gb = got.view(np.uint32)
    assert (gb & 0xFFFF == 0).all()                               # representable in bf16
    for b, g, f in zip(bits.tolist(), gb.tolist(), got.tolist()):
        want = _rne_bits(b)
        if want is None:
            assert f != f, hex(b)                                 # NaN stays NaN
        else:
            assert g >> 16 == want, (hex(b), hex(g), hex(want))
    # the same through float64 inputs, and against struct's own view of a few values
    assert np.array_equal(H.bf16_round(np.array([1.0, -2.5, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])),
                          np.array([1.0, -2.5, 1.0, 1.0 + 2.0 ** -6], np.float32))
    assert struct.unpack("<I", struct.pack("<f", float(H.bf16_round(np.array([3.1415927]))[0])))[0] == 0x40490000
