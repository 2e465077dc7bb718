"""cl_nn_layer_k (csrc/closed_loop.hip: all networks of a closed-loop batch in one launch per layer index) at the shapes it is
used at, step by step against the fp64 oracle (oracle/nn.py).

One-step identity instead of trajectory agreement: with the records u, xs, us, xhat of a run, every step of every NN instance
must satisfy, per column and within 1e-4 max(1, |ref|) (f32 sums),

    u[t] == clip(oracle.nn.control_input(W, xhat_used[t], u[t - 1], xs[t], us[t], xscale, ulb, uub))

(helpers.cl_one_step_reference says where xhat_used comes from).  Errors do not compound over steps, every step of every network
is a test vector, and the reference is numpy in fp64 rather than the library's other forward."""
import numpy as np
import pytest

from tests import helpers as H
from tests.test_closed_loop_gpu import _mini_problem

pytestmark = pytest.mark.gpu

NSIM = 50
TOL = 1e-4


def _nn_controllers(common, mix, seed0=300):
    from industrial_nnmpc_2021_amd import controller_evaluation as ce
    Nx, Nu = common["B"].shape
    out = []
    for j, (name, hidden, withu, _) in enumerate(mix):
        W = H.cl_nn_weights(seed0 + j, 2 * Nx + (2 if withu else 1) * Nu, hidden, Nu)
        xscale = np.random.default_rng(seed0 + 50 + j).uniform(0.5, 2.0, Nx)
        out.append(ce.NeuralNetworkController(regulator_weights=W, xscale=xscale, nnwithuprev=withu, build_forward=False, **common))
    return out


def _instances(mix, only=None):
    """(controller, scenario, seed): instance k of a network takes scenario k % 2 and seed 1 + k."""
    return [(c, k % 2, 1 + k) for c, m in enumerate(mix) if only is None or c == only for k in range(m[3])]


def _plant(pl, common):
    from industrial_nnmpc_2021_amd import linearMPC as lm
    return lm.LinearPlantSimulator(x0=np.zeros((pl["A"].shape[0], 1)), sample_time=1.0, A=pl["A"], B=pl["B"], C=pl["C"],
                                   Bp=common["Bd"], Rv=common["Rv"])


@pytest.fixture(scope="module")
def mix_run():
    from industrial_nnmpc_2021_amd.closed_loop import simulate_closed_loop_batch
    pl, common, scen = _mini_problem()
    plant = _plant(pl, common)
    ctls = _nn_controllers(common, H.CL_NN_MIX)
    res = simulate_closed_loop_batch(plant, ctls, scenarios=scen, Nsim=NSIM, seeds=[0], instances=_instances(H.CL_NN_MIX))
    return dict(pl=pl, common=common, scen=scen, plant=plant, ctls=ctls, res=res)


def test_one_step_identity_of_a_network_mix_in_one_batch(mix_run):
    """helpers.CL_NN_MIX in ONE batch: 22 instances x 50 steps, each a test vector.  At most 5 % of the oracle's entries on a
    bound (a clipped entry equals the oracle whatever the kernel summed)."""
    m = mix_run
    assert len(m["res"]["instances"]) == sum(n[3] for n in H.CL_NN_MIX)
    for k in ("y", "u", "x", "xhat", "avg"):
        assert np.isfinite(m["res"][k]).all(), k
    share, worst = H.cl_assert_one_step_identity(m["res"], m["ctls"], m["common"], TOL, "mix")
    print(f"mix: share on a bound {share:.4f}, worst column error {worst:.3e}")
    assert share <= 0.05, share


def test_mix_is_batch_independent_bitwise(mix_run):
    """The comment above cl_nn_layer_k: a row's value "does not depend on how many rows or networks share the launch".  Each
    network alone against the same network in the mix: u and avg bit for bit over 50 steps."""
    from industrial_nnmpc_2021_amd.closed_loop import simulate_closed_loop_batch
    m = mix_run
    res = m["res"]
    for c, net in enumerate(H.CL_NN_MIX):
        inst = _instances(H.CL_NN_MIX, only=c)
        one = simulate_closed_loop_batch(m["plant"], m["ctls"], scenarios=m["scen"], Nsim=NSIM, seeds=[0], instances=inst)
        idx = [res["instances"].index(t) for t in inst]
        assert np.array_equal(one["u"], res["u"][idx]), net[0]
        assert np.array_equal(one["avg"], res["avg"][idx]), net[0]
    # and one instance of the 9-instance network alone (2 rows instead of 18: another walk through the blocks of 8 rows)
    c = 3
    inst = [_instances(H.CL_NN_MIX, only=c)[8]]
    one = simulate_closed_loop_batch(m["plant"], m["ctls"], scenarios=m["scen"], Nsim=NSIM, seeds=[0], instances=inst)
    assert np.array_equal(one["u"][0], res["u"][res["instances"].index(inst[0])])


def test_closed_loop_step_agrees_with_structured_nn(mix_run):
    """Additional check only (the reference of both is the oracle): the recorded inputs of every step through StructuredNN (f32)
    give the recorded moves within 2e-4 -- two f32 results, each within 1e-4 of the oracle."""
    from industrial_nnmpc_2021_amd.nn import StructuredNN
    m = mix_run
    res, common = m["res"], m["common"]
    Nx, Nu = common["B"].shape
    for c, net in enumerate(H.CL_NN_MIX):
        ctl = m["ctls"][c]
        i = res["instances"].index(_instances(H.CL_NN_MIX, only=c)[0])
        up = np.concatenate((np.ravel(common["uprev"])[None, :], res["u"][i][:-1]), axis=0)
        snn = StructuredNN(ctl.regulator_weights, Nx, Nu, nnwithuprev=ctl.nnwithuprev, xscale=np.ravel(ctl.xscale),
                           ulb=common["ulb"], uub=common["uub"], max_batch=128)
        u = snn.forward(res["xhat"][i][1:, :Nx], up if ctl.nnwithuprev else None, res["xs"][i], res["us"][i])
        snn.close()
        H.assert_cols_close(u, res["u"][i], 2e-4, net[0])


def test_hidden_width_beyond_nn_maxk_is_refused(mix_run):
    """NN_MAXK = 2048 runs (in the mix); 2049 must be refused by nnmpc_cl_create, not truncated."""
    from industrial_nnmpc_2021_amd import _lib
    from industrial_nnmpc_2021_amd.closed_loop import simulate_closed_loop_batch
    m = mix_run
    ctls = _nn_controllers(m["common"], [("w2049", [2049], True, 1)])
    with pytest.raises(_lib.NnmpcError, match="2048"):
        simulate_closed_loop_batch(m["plant"], ctls, scenarios=m["scen"], Nsim=2, seeds=[0], instances=[(0, 0, 1)])


def test_nan_measurement_surfaces_and_stays_in_its_instance(mix_run):
    """A NaN in y0 of one NN instance: the filter hands that instance's network a NaN estimate.  Its moves must come back
    non-finite (fmaxf(v + b, 0) in the layer kernel made them ordinary numbers), and every other instance is bitwise unchanged."""
    from industrial_nnmpc_2021_amd import closed_loop as cl
    m = mix_run
    ctls, common = m["ctls"], m["common"]
    slots = [dict(kind="nn", weights=c.regulator_weights, with_uprev=c.nnwithuprev, xscale=np.ravel(c.xscale)) for c in ctls]
    inst_slot = np.repeat(np.arange(len(slots)), [n[3] for n in H.CL_NN_MIX]).astype(np.int32)
    nb, Ny, T = inst_slot.size, m["pl"]["C"].shape[0], 5
    scen = (np.arange(nb) % 2).astype(np.int32)
    V = np.random.default_rng(5).standard_normal((T + 1, nb, Ny))
    sig = np.sqrt(np.diag(common["Rv"]))
    SP = np.stack([s[0][:T] for s in m["scen"]])
    DS = np.stack([s[1][:T] for s in m["scen"]])
    dev = cl.DeviceClosedLoop(cl._model(m["plant"], ctls[0]), ctls[0].target_selector._device(), slots, inst_slot)
    y0 = 0.01 * np.random.default_rng(6).standard_normal((nb, Ny))
    clean = dev.run(SP, DS, scen, V, sig, y0=y0)
    dev.reset()
    bad = 6                                                    # an instance in the middle of the 8-instance network's rows
    y0n = y0.copy(); y0n[bad, 2] = np.nan
    pois = dev.run(SP, DS, scen, V, sig, y0=y0n)
    dev.close()
    assert np.isfinite(clean["u"]).all()
    assert not np.isfinite(pois["u"][:, bad]).any(), pois["u"][:, bad]
    others = np.arange(nb) != bad
    for k in ("u", "y", "x", "xhat", "avg"):
        assert np.array_equal(pois[k][:, others], clean[k][:, others]), k


def test_nan_weight_surfaces_and_stays_in_its_network(mix_run):
    """A network whose training diverged: one NaN in a hidden-layer kernel.  The oracle's move is NaN in every column at every
    step (the NaN hidden unit meets every head weight); the device must say so too -- with fmaxf(v + b, 0) as the ReLU the NaN
    unit became 0 and the evaluation reported ordinary moves and a finite cost -- and the other networks of the batch are
    bitwise unchanged.  (A NaN measurement, the test above, reaches u through us as well, whatever the layer kernel does.)"""
    import copy
    from industrial_nnmpc_2021_amd.closed_loop import simulate_closed_loop_batch
    from oracle import nn as onn
    m = mix_run
    res, common = m["res"], m["common"]
    Nx = common["A"].shape[0]
    bad = 2                                                    # "w64_65": 8 instances, three weight matrices
    ctls = list(m["ctls"])
    ctls[bad] = copy.copy(ctls[bad])
    W = [w.copy() for w in ctls[bad].regulator_weights]
    W[2][3, 5] = np.nan                                        # second hidden layer, unit 5
    ctls[bad].regulator_weights = W
    inst = _instances(H.CL_NN_MIX)
    pois = simulate_closed_loop_batch(m["plant"], ctls, scenarios=m["scen"], Nsim=10, seeds=[0], instances=inst,
                                      allow_uncertified=True)
    for i, (c, s, seed) in enumerate(inst):
        if c == bad:
            z = np.zeros((1, Nx))
            with np.errstate(all="ignore"):
                ref = onn.control_input(W, z, np.zeros((1, 3)), z, np.zeros((1, 3)), np.ravel(ctls[bad].xscale), None, None, True)
            assert np.isnan(ref).all()
            assert not np.isfinite(pois["u"][i]).any(), (i, pois["u"][i][:2])
        else:
            assert np.array_equal(pois["u"][i], res["u"][i][:10]), i
            assert np.array_equal(pois["avg"][i], res["avg"][i][:11]), i
