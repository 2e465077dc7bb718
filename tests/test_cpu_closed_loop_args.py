"""simulate_closed_loop_batch checks its arguments and the shared controller data before the HIP library is touched."""
import numpy as np
import pytest


@pytest.fixture
def setup(monkeypatch):
    from industrial_nnmpc_2021_amd import _lib, linearMPC as lm, controller_evaluation as ce

    def no_device():
        raise AssertionError("the library must not be loaded before the arguments are validated")
    monkeypatch.setattr(_lib, "load", no_device)
    rng = np.random.default_rng(0)
    Nx, Nu, Ny, Nd = 4, 2, 3, 1
    W = rng.standard_normal((Nx, Nx))
    A = 0.8 * W / np.abs(np.linalg.eigvals(W)).max()
    B, C = rng.standard_normal((Nx, Nu)), rng.standard_normal((Ny, Nx))
    Bd = rng.standard_normal((Nx, Nd))
    common = dict(A=A, B=B, C=C, H=np.eye(1, Ny), Qwx=1e-4 * np.eye(Nx), Qwd=1e-2 * np.eye(Nd), Rv=1e-4 * np.eye(Ny),
                  xprior=np.zeros((Nx, 1)), dprior=np.zeros((Nd, 1)), Rs=1e-3 * np.eye(Nu), Qs=np.eye(Ny), Bd=Bd,
                  Cd=np.zeros((Ny, Nd)), usp=np.zeros((Nu, 1)), uprev=np.zeros((Nu, 1)), Q=C.T @ C, R=0.1 * np.eye(Nu),
                  S=0.1 * np.eye(Nu), ulb=-np.ones((Nu, 1)), uub=np.ones((Nu, 1)))
    plant = lm.LinearPlantSimulator(A=A, B=B, C=C, Bp=Bd, Rv=common["Rv"], sample_time=1.0, x0=np.zeros((Nx, 1)))
    ctls = [lm.LinearMPCController(N=5, **common), ce.SatDlqrController(**common), ce.SteadyStateController(**common)]
    scen = [(np.zeros((10, Ny)), np.zeros((10, Nd)))]
    return plant, ctls, scen, common


def _run(plant, ctls, scen, **kw):
    from industrial_nnmpc_2021_amd.closed_loop import simulate_closed_loop_batch
    args = dict(scenarios=scen, Nsim=10, seeds=[0])
    args.update(kw)
    return simulate_closed_loop_batch(plant, ctls, **args)


def test_mismatched_shared_data_raises(setup):
    from industrial_nnmpc_2021_amd import controller_evaluation as ce
    plant, ctls, scen, common = setup
    with pytest.raises(ValueError, match="differs .* in Q"):
        _run(plant, ctls + [ce.SteadyStateController(**dict(common, Q=2 * common["Q"]))], scen)
    with pytest.raises(ValueError, match="Qwx"):
        _run(plant, ctls + [ce.SatDlqrController(**dict(common, Qwx=2 * common["Qwx"]))], scen)


def test_bad_arguments_raise(setup):
    plant, ctls, scen, _ = setup
    with pytest.raises(ValueError):
        _run(plant, ctls, scen, Nsim=0)
    with pytest.raises(ValueError):
        _run(plant, ctls, scen, Nsim=11)                                        # longer than the scenario
    with pytest.raises(ValueError):
        _run(plant, ctls, [(np.zeros((10, 2)), np.zeros((10, 1)))])             # wrong Ny
    with pytest.raises(ValueError):
        _run(plant, ctls, scen, instances=[(3, 0, 0)])                          # no controller 3
    with pytest.raises(ValueError):
        _run(plant, ctls, scen, instances=[(0, 1, 0)])                          # no scenario 1
    with pytest.raises(ValueError):
        _run(plant, ctls, scen, seeds=[])
    with pytest.raises(ValueError):
        _run(plant, ctls, scen, record=("u", "nope"))
    with pytest.raises(ValueError):
        _run(plant, [], scen)
    with pytest.raises(TypeError):
        _run(plant, ctls + [object()], scen)


def test_baseline_controllers_build_on_the_host(setup):
    """SatDlqrController's gain is the augmented regulator's LQR gain (u = Kaug [x - xs; uprev - us] + us)."""
    from industrial_nnmpc_2021_amd.linearMPC_build import dlqr, augmented_matrices_for_regulator
    _, (mpc, sat, ss), _, common = setup
    Aa, Ba, Qa, Ra, Ma = augmented_matrices_for_regulator(common["A"], common["B"], common["Q"], common["R"], common["S"])
    assert np.array_equal(sat.Kaug, dlqr(Aa, Ba, Qa, Ra, Ma)[0]) and sat.Kaug.shape == (2, 6)
    for c in (sat, ss):
        assert np.array_equal(c.Qaug, mpc.Qaug) and np.array_equal(c.Maug, mpc.Maug) and c.average_stage_costs[0].shape == (1, 1)
    assert np.array_equal(sat._clip_control_input(np.array([[2.0], [-3.0]])), np.array([[1.0], [-1.0]]))


def test_satdlqr_gain_matches_reference_fixture(golden_dir):
    """Kaug of SatDlqrController against the reference's own (closed_loop_baselines.npz, make_golden_baselines.py)."""
    import os
    from industrial_nnmpc_2021_amd import controller_evaluation as ce
    g = np.load(os.path.join(golden_dir, "closed_loop.npz"))
    f = np.load(os.path.join(golden_dir, "closed_loop_baselines.npz"))
    Nx, Nu = g["B"].shape
    Nd = g["Bd"].shape[1]
    c = ce.SatDlqrController(A=g["A"], B=g["B"], C=g["C"], H=g["H"], Qwx=g["Qwx"], Qwd=g["Qwd"], Rv=g["Rv"], xprior=np.zeros((Nx, 1)),
                             dprior=np.zeros((Nd, 1)), Rs=g["Rs"], Qs=g["Qs"], Bd=g["Bd"], Cd=g["Cd"], usp=np.zeros((Nu, 1)),
                             uprev=np.zeros((Nu, 1)), Q=g["Q"], R=g["R"], S=g["S"], ulb=g["ulb"], uub=g["uub"])
    assert np.abs(c.Kaug - f["satdlqr_Kaug"]).max() < 1e-10
