"""Nonlinear plant simulation (the reference's lib/nonlinearMPC.py:11-48) without casadi.

The reference integrates its ODE with ``mpctools.DiscreteSimulator`` (casadi / CVODES).  Here the flow map over one sample is a
fixed-step fp64 classical Runge-Kutta method with a fixed number of substeps: the loop count does not depend on the data, and
the device's CSTRs flow map (``nnmpc_cstrs_flow`` and the closed loop's plant step, csrc/closed_loop.hip) applies the same
tableau and substep count.
"""
import numpy as np

# classical RK4, 32 substeps per sample: 1.4e-8 / 8.6e-10 / 5.3e-11 relative to ||Phi||_inf with 16 / 32 / 64 substeps against
# DOP853 on the CSTRs operating box
SUBSTEPS = 32


class DiscreteSimulator:
    """x+ = Phi(x, u, p) over one sample of the ODE dx/dt = fxup(x, u, p), with u and p held (zero-order hold).

    Signature of ``mpctools.DiscreteSimulator(ode, Delta, [Nx, Nu, Np], ["x", "u", "p"])``; ``sim`` returns a 1-D array like
    the casadi one.  ``x`` may also be (Nx, n) columns of n states (u, p then (Nu, 1) / (Np, 1) or (Nu, n) / (Np, n)) when
    ``fxup`` maps columns to columns, as ``cstrs_parameters.CstrsOde`` does; that returns (Nx, n)."""

    def __init__(self, fxup, sample_time, sizes, names=("x", "u", "p"), substeps=SUBSTEPS):
        if int(substeps) < 1:
            raise ValueError("DiscreteSimulator: substeps must be >= 1")
        self.fxup = fxup
        self.sample_time = float(sample_time)
        self.sizes = [int(s) for s in sizes]
        self.names = list(names)
        self.substeps = int(substeps)

    def sim(self, x, u, p):
        f, M = self.fxup, self.substeps
        h = self.sample_time / M
        x = np.asarray(x, dtype=float)
        cols = x.ndim == 2 and x.shape[1] > 1
        x = x.copy() if cols else x.ravel().copy()
        u = np.asarray(u, dtype=float)
        p = np.asarray(p, dtype=float)
        if not cols:
            u, p = u.ravel(), p.ravel()
            fast = getattr(f, "rk4", None)                        # one real state of a model with a scalar RK4 (CstrsOde)
            if fast is not None and not np.iscomplexobj(x):
                r = fast(x, u, p, self.sample_time, M)
                if r is not None:
                    return r
        for _ in range(M):
            k1 = f(x, u, p)
            k2 = f(x + (0.5 * h) * k1, u, p)
            k3 = f(x + (0.5 * h) * k2, u, p)
            k4 = f(x + h * k3, u, p)
            x = x + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
        return x


class NonlinearPlantSimulator:
    """Nonlinear plant with additive measurement noise (reference lib/nonlinearMPC.py:11-48).

    ``fxup(x, u, p)``: the continuous-time right-hand side, ``hx(x)``: the measurement.  Noise is drawn in the reference's
    order: one (Ny, 1) standard-normal draw for y[0] here, then one per ``step``."""

    def __init__(self, *, fxup, hx, Rv, Nx, Nu, Np, Ny, sample_time, x0, substeps=SUBSTEPS):
        self.fxup = DiscreteSimulator(fxup, sample_time, [Nx, Nu, Np], ["x", "u", "p"], substeps=substeps)
        self.hx = hx
        (self.Nx, self.Nu, self.Ny, self.Np) = (Nx, Nu, Ny, Np)
        self.measurement_noise_std = np.sqrt(np.diag(Rv)[:, np.newaxis])
        self.sample_time = sample_time
        self.x = [x0]
        self.u = []
        self.p = []
        self.y = [self._h(x0) + self.measurement_noise_std * np.random.randn(self.Ny, 1)]
        self.t = [0.]

    def _h(self, x):
        return np.asarray(self.hx(x), dtype=float).reshape(self.Ny, 1)

    def step(self, u, p):
        x = self.fxup.sim(self.x[-1], u, p)[:, np.newaxis]
        y = self._h(x) + self.measurement_noise_std * np.random.randn(self.Ny, 1)
        self._append_data(x, u, p, y)
        return y

    def _append_data(self, x, u, p, y):
        self.x.append(x)
        self.u.append(u)
        self.p.append(p)
        self.y.append(y)
        self.t.append(self.t[-1] + self.sample_time)
