"""Training step of the structured NN controller in PyTorch(-ROCm), stock ops only.

Counterpart of the reference's ``cdu_train.py`` / ``cstrs_train.py``
(create_nn_controller :24-38, train_nn_controller :40-62): Keras
``RegulatorModel`` (lib/LinearMPCLayers.py:117-133) compiled with Adam + MSE,
``fit(batch_size=2048, validation_split=0.05)``, ``ModelCheckpoint(monitor=
'val_loss', save_best_only=True)``; afterwards the weights are exchanged as the
Keras ``get_weights()`` list, which is exactly what ``nn.StructuredNN`` /
``LinearMPCLayers.RegulatorLayer*`` take for the HIP forward.

``backend="torch"`` (the default) is the only place PyTorch does arithmetic
(BASELINE.json north_star).  ``backend="hip"`` runs the same step -- forward,
backward, Adam, the epoch loop -- in f32 on hand-written gfx950 kernels
(csrc/nn_train.hip, ``HipTrainer``); the model object then only carries the
trained weights.  ``train_nn_controllers`` trains a whole sweep of networks in
one lock-step launch group (csrc/nn_train_group.hip, ``HipGroupTrainer``).
``train_unstd_nn_controller`` trains the reference's unstructured comparison
network (``cstrs_train_unstd.py``) on the one-pass form of the single-network step,
``train_unstd_nn_controllers`` a sweep of them in one launch group of that form.

``train_nn_controller(..., tan_weight=w)`` trains the structured network on the MPC's value AND its local slope (the
tangent loss, ``tangent_loss``); ``tangent_data`` makes the slope targets from a solved batch -- one direction per row in
[dx, (duprev)], or D directions per row and directions over the whole input [dx, (duprev), dxs, dus]
(``tangent_data(directions=, whole_input=)``, ``whole_input_perturbation``, ``HipTrainer(tan_dirs=, tan_whole_input=)``).
"""
import copy
import ctypes as C
import time

import numpy as np
import torch

from . import _lib


class RegulatorModel(torch.nn.Module):
    """u = us + MLP(x,[uprev],xs,us) - MLP(xs,[us],xs,us); hidden Dense(relu), bias-free head.

    ``regulator_dims = [d_in, h1, ..., nu]``: like the reference, element 0 is ignored
    (lib/LinearMPCLayers.py:128-131) and the input width follows from Nx, Nu, nnwithuprev.
    Float64 like the reference (``set_floatx('float64')``, :13).
    """

    def __init__(self, Nx, Nu, regulator_dims, nnwithuprev=True, dtype=torch.float64):
        super().__init__()
        self.Nx, self.Nu, self.nnwithuprev = Nx, Nu, nnwithuprev
        widths = [2 * Nx + (2 if nnwithuprev else 1) * Nu] + list(regulator_dims[1:])
        layers = []
        for i in range(len(widths) - 1):
            last = i == len(widths) - 2
            layers.append(torch.nn.Linear(widths[i], widths[i + 1], bias=not last, dtype=dtype))
        self.layers = torch.nn.ModuleList(layers)
        for lin in self.layers:                       # Keras Dense default: glorot_uniform, zero bias
            torch.nn.init.xavier_uniform_(lin.weight)
            if lin.bias is not None:
                torch.nn.init.zeros_(lin.bias)

    def _mlp(self, z):
        for lin in self.layers[:-1]:
            z = torch.relu(lin(z))
        return self.layers[-1](z)

    def forward(self, x, uprev, xs, us):
        if self.nnwithuprev:
            z1, z2 = torch.cat((x, uprev, xs, us), -1), torch.cat((xs, us, xs, us), -1)
        else:
            z1, z2 = torch.cat((x, xs, us), -1), torch.cat((xs, xs, us), -1)
        return us + self._mlp(z1) - self._mlp(z2)

    def get_weights(self):
        """Keras order: [W1 (in x h), b1, ..., Wout (h x Nu)] as float64 numpy arrays."""
        out = []
        for lin in self.layers:
            out.append(lin.weight.detach().cpu().double().numpy().T.copy())
            if lin.bias is not None:
                out.append(lin.bias.detach().cpu().double().numpy().copy())
        return out

    def set_weights(self, weights):
        it = iter(weights)
        with torch.no_grad():
            for lin in self.layers:
                lin.weight.copy_(torch.as_tensor(np.asarray(next(it)).T, dtype=lin.weight.dtype))
                if lin.bias is not None:
                    lin.bias.copy_(torch.as_tensor(np.asarray(next(it)), dtype=lin.bias.dtype))


class UnstdRegulatorModel(torch.nn.Module):
    """u = MLP(x, [uprev], xs, us): the reference's unstructured comparison network (lib/LinearMPCLayers.py:135-174,
    trained by cstrs_train_unstd.py).  One pass, a bias on every Dense, ``regulator_dims[0]`` ignored like there.

    ``head_relu``: the Keras layer builds every Dense with activation='relu', the output one included (:147-148), while the
    numpy controller that runs the trained weights ends in a linear head (lib/controller_evaluation.py:907-908).  True
    (the default) is the Keras code as written, False the controller's form.  Trains natively through
    ``train_unstd_nn_controller`` (the one-pass form of the HIP step, one network per handle),
    ``train_unstd_nn_controllers`` (a sweep in one launch group) or in stock PyTorch
    through ``train_nn_controller(backend="torch")``; ``backend="hip"`` of the structured entry points refuses it."""

    unstructured = True

    def __init__(self, Nx, Nu, regulator_dims, nnwithuprev=True, head_relu=True, dtype=torch.float64):
        super().__init__()
        self.Nx, self.Nu, self.nnwithuprev, self.head_relu = Nx, Nu, nnwithuprev, bool(head_relu)
        widths = [2 * Nx + (2 if nnwithuprev else 1) * Nu] + list(regulator_dims[1:])
        self.layers = torch.nn.ModuleList([torch.nn.Linear(widths[i], widths[i + 1], bias=True, dtype=dtype)
                                           for i in range(len(widths) - 1)])
        for lin in self.layers:                       # Keras Dense default: glorot_uniform, zero bias
            torch.nn.init.xavier_uniform_(lin.weight)
            torch.nn.init.zeros_(lin.bias)

    def forward(self, x, uprev, xs, us):
        z = torch.cat((x, uprev, xs, us), -1) if self.nnwithuprev else torch.cat((x, xs, us), -1)
        for lin in self.layers[:-1]:
            z = torch.relu(lin(z))
        z = self.layers[-1](z)
        return torch.relu(z) if self.head_relu else z

    def get_weights(self):
        """Keras order: [W1 (in x h), b1, ..., WL (h x Nu), bL] as float64 numpy arrays."""
        out = []
        for lin in self.layers:
            out.append(lin.weight.detach().cpu().double().numpy().T.copy())
            out.append(lin.bias.detach().cpu().double().numpy().copy())
        return out

    def set_weights(self, weights):
        weights = list(weights)
        if len(weights) != 2 * len(self.layers):
            raise ValueError(f"set_weights: {len(weights)} arrays for {len(self.layers)} layers with a bias each")
        with torch.no_grad():
            for l, lin in enumerate(self.layers):
                lin.weight.copy_(torch.as_tensor(np.asarray(weights[2 * l]).T, dtype=lin.weight.dtype))
                lin.bias.copy_(torch.as_tensor(np.asarray(weights[2 * l + 1]), dtype=lin.bias.dtype))


def _refuse_unstructured(model, who):
    """This entry point builds the structured form of the native step (two passes, bias-free head), which would misread
    the unstructured weight list."""
    if getattr(model, "unstructured", False):
        raise ValueError(f"{who}: this entry point runs the structured form of the native HIP training step; train an "
                         "UnstdRegulatorModel natively with train_unstd_nn_controller (a sweep of them with "
                         "train_unstd_nn_controllers), or through stock PyTorch with train_nn_controller(..., backend=\"torch\")")


def _unstd_form(model, who):
    """The native step's form for an UnstdRegulatorModel; a structured model is refused (on the host)."""
    if not getattr(model, "unstructured", False):
        raise ValueError(f"{who}: takes an UnstdRegulatorModel; train a structured RegulatorModel with "
                         "train_nn_controller / train_nn_controllers")
    return _lib.NN_UNSTD_RELU if model.head_relu else _lib.NN_UNSTD


def _check_form(form):
    if form not in (_lib.NN_STRUCTURED, _lib.NN_UNSTD, _lib.NN_UNSTD_RELU):
        raise ValueError(f"form {form!r}: _lib.NN_STRUCTURED, _lib.NN_UNSTD or _lib.NN_UNSTD_RELU")
    return int(form)


def _split_keras(weights, form):
    """The Keras list as (Ws, bs), bs padded with None to one entry per layer: [W1, b1, ..., Wout] for the structured form,
    [W1, b1, ..., WL, bL] (even-length: a bias on the head too) for the unstructured ones.  Host only."""
    weights = list(weights)
    if form != _lib.NN_STRUCTURED:
        if not weights or len(weights) % 2:
            raise ValueError(f"the unstructured forms take an even-length list [W1, b1, ..., WL, bL], got {len(weights)} arrays")
        Ws = [np.ascontiguousarray(w, np.float64) for w in weights[0::2]]
        bs = [np.ascontiguousarray(b, np.float64).ravel() for b in weights[1::2]]
        return Ws, bs
    Ws = [np.ascontiguousarray(w, np.float64) for w in weights[0:-1:2]] + [np.ascontiguousarray(weights[-1], np.float64)]
    bs = [np.ascontiguousarray(b, np.float64).ravel() for b in weights[1::2]]
    if len(bs) != len(Ws) - 1:
        raise ValueError("weights must be [W1, b1, ..., W_{L-1}, b_{L-1}, Wout]")
    return Ws, bs + [None]


class HipTrainer:
    """The native training step (C ABI ``nnmpc_train_*``): f32 master weights, Adam moments, dataset and workspaces
    live on the device; ``weights`` is the Keras ``get_weights()`` list the network starts from.

    ``form``: ``_lib.NN_STRUCTURED`` (RegulatorModel: two stacked passes, bias-free head, the list ends in Wout),
    ``_lib.NN_UNSTD`` (UnstdRegulatorModel with a linear head: one pass, the list is [W1, b1, ..., WL, bL]) or
    ``_lib.NN_UNSTD_RELU`` (the same with relu on the head).  ``grad``, ``get_weights`` and ``set_weights`` exchange the
    list of the form.

    ``tangents=True`` (structured form only) builds the handle of the tangent loss (``nnmpc_train_create_tan``):
    ``set_tangents`` after ``set_data``, ``set_tan_weight(w)``; then ``grad``, ``step``, ``epoch`` and ``eval`` work on
    L = mse + w tan_mse (``tangent_loss``) and ``last_losses()`` returns the two parts.  With w = 0 (as created) it
    computes the bytes of a plain handle.

    ``tan_dirs=D`` (1 .. 16) and ``tan_whole_input=True`` build the handle of ``nnmpc_train_create_tan_ex``: D directions
    per dataset row, each with its own target, behind ONE primal pair of stacked rows, and directions over the whole network
    input [dx, (duprev), dxs, dus] (pass 2 then carries tangents too).  ``set_tangents`` takes every column as (n, D, width),
    ``dxs`` and ``dus`` with them on a whole-input handle.  The defaults go through ``nnmpc_train_create_tan`` /
    ``nnmpc_train_set_tangents`` as before.

    Adam as ``torch.optim.Adam(lr, betas, eps)``.  There is no CPU fallback: without a device the constructor raises
    ``_lib.NnmpcError``."""

    def __init__(self, weights, nx, nu, *, nnwithuprev=True, max_batch=2048, lr=1e-3, betas=(0.9, 0.999), eps=1e-7,
                 form=_lib.NN_STRUCTURED, tangents=False, tan_dirs=1, tan_whole_input=False):
        self.form = _check_form(form)
        self.tangents = bool(tangents)
        self.tan_dirs, self.tan_whole = int(tan_dirs), int(tan_whole_input)
        self._tan_ex = self.tan_dirs != 1 or self.tan_whole != 0
        if self._tan_ex and not self.tangents:
            raise ValueError("HipTrainer: tan_dirs / tan_whole_input describe a tangent handle (tangents=True)")
        Ws, bs = _split_keras(weights, self.form)               # refused on the host, before the library is loaded
        lib = _lib.load()
        L = len(Ws)
        self.dims = [Ws[0].shape[0]] + [w.shape[1] for w in Ws]
        self.L, self.nx, self.nu, self.nnwithuprev, self.n = L, nx, nu, bool(nnwithuprev), 0
        self._lib, self._h = lib, C.c_void_p()
        create, who, more = ((lib.nnmpc_train_create_tan_ex, "nnmpc_train_create_tan_ex", (self.tan_dirs, self.tan_whole)) if self._tan_ex
                             else (lib.nnmpc_train_create_tan, "nnmpc_train_create_tan", ()) if self.tangents
                             else (lib.nnmpc_train_create_ex, "nnmpc_train_create_ex", ()))
        _lib.check(create(C.byref(self._h), L, (C.c_int32 * (L + 1))(*self.dims), self._plist(Ws), self._plist(bs), nx, nu,
                          int(self.nnwithuprev), int(max_batch), lr, betas[0], betas[1], eps, self.form, *more), who)

    @staticmethod
    def _plist(arrays):
        return (C.c_void_p * len(arrays))(*[None if a is None else a.ctypes.data for a in arrays])

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.nnmpc_train_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def set_data(self, data):
        """dict(x, uprev, xs, us, u), rows = samples, already scaled; uploaded once as f32."""
        c = lambda a, w: np.ascontiguousarray(a, np.float64).reshape(-1, w)
        x, xs, us, u = c(data["x"], self.nx), c(data["xs"], self.nx), c(data["us"], self.nu), c(data["u"], self.nu)
        up = c(data["uprev"], self.nu) if self.nnwithuprev and data.get("uprev") is not None else None
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        _lib.check(self._lib.nnmpc_train_set_data(self._h, x.shape[0], p(x), p(up), p(xs), p(us), p(u), _lib.HOST),
                   "nnmpc_train_set_data")
        self.n = x.shape[0]

    def set_data_device(self, n, x, uprev, xs, us, u):
        """The same from HBM-resident f64 buffers (objects with data_ptr(); ``uprev`` None without uprev)."""
        q = lambda a: None if a is None else C.c_void_p(a.data_ptr())
        _lib.check(self._lib.nnmpc_train_set_data(self._h, int(n), q(x), q(uprev), q(xs), q(us), q(u), _lib.DEVICE),
                   "nnmpc_train_set_data")
        self.n = int(n)

    def set_tangents(self, tangents):
        """dict(dx, duprev, du): per dataset row one direction [dx, (duprev)] in the units of the dataset's x and the
        target du (``tangent_data`` returns them); after ``set_data``, which drops earlier ones.  Uploaded once as f32.

        A handle with ``tan_dirs=D``: every column is (n, D, width) -- (n, width) also serves D = 1 --, and a whole-input
        handle takes ``dxs`` and ``dus`` beside them (on any other handle they are refused)."""
        D = self.tan_dirs

        def c(a, w):
            a = np.ascontiguousarray(a, np.float64)
            if a.ndim == 3 and a.shape[1:] != (D, w) or a.ndim != 3 and D != 1:
                raise ValueError(f"set_tangents: a column of shape {a.shape}, the handle takes (n, {D}, {w})")
            return a.reshape(-1, D * w)
        dx, du = c(tangents["dx"], self.nx), c(tangents["du"], self.nu)
        dup = c(tangents["duprev"], self.nu) if self.nnwithuprev and tangents.get("duprev") is not None else None
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        if not self._tan_ex:
            if tangents.get("dxs") is not None or tangents.get("dus") is not None:
                raise ValueError("set_tangents: dxs / dus are the columns of a whole-input handle (tan_whole_input=True)")
            _lib.check(self._lib.nnmpc_train_set_tangents(self._h, dx.shape[0], p(dx), p(dup), p(du), _lib.HOST),
                       "nnmpc_train_set_tangents")
            return
        dxs = c(tangents["dxs"], self.nx) if tangents.get("dxs") is not None else None
        dus = c(tangents["dus"], self.nu) if tangents.get("dus") is not None else None
        _lib.check(self._lib.nnmpc_train_set_tangents_ex(self._h, dx.shape[0], D, p(dx), p(dup), p(dxs), p(dus), p(du), _lib.HOST),
                   "nnmpc_train_set_tangents_ex")

    def set_tangents_device(self, n, dx, duprev, du, dxs=None, dus=None):
        """The same from HBM-resident f64 buffers (objects with data_ptr(); ``duprev`` None without uprev), laid out
        (n, D, width) on a handle with ``tan_dirs=D``; ``dxs`` / ``dus`` on a whole-input handle."""
        q = lambda a: None if a is None else C.c_void_p(a.data_ptr())
        if not self._tan_ex and dxs is None and dus is None:
            _lib.check(self._lib.nnmpc_train_set_tangents(self._h, int(n), q(dx), q(duprev), q(du), _lib.DEVICE),
                       "nnmpc_train_set_tangents")
            return
        _lib.check(self._lib.nnmpc_train_set_tangents_ex(self._h, int(n), self.tan_dirs, q(dx), q(duprev), q(dxs), q(dus), q(du),
                                                         _lib.DEVICE), "nnmpc_train_set_tangents_ex")

    def set_tan_weight(self, w):
        """The weight of the tangent term, finite and >= 0 (0: the plain step)."""
        _lib.check(self._lib.nnmpc_train_set_tan_weight(self._h, float(w)), "nnmpc_train_set_tan_weight")

    def last_losses(self):
        """(mse, tan_mse) of what the last grad / step / epoch / eval returned (L = mse + w tan_mse)."""
        a, b = C.c_double(), C.c_double()
        _lib.check(self._lib.nnmpc_train_last_losses(self._h, C.byref(a), C.byref(b)), "nnmpc_train_last_losses")
        return a.value, b.value

    @staticmethod
    def _rows(rows):
        return np.ascontiguousarray(rows, np.int32).ravel()

    def _empty(self):
        return self._empty_for(self.dims, self.form)

    @staticmethod
    def _empty_for(d, form):
        """(Ws, bs) to read a network of widths ``d`` into; bs has one entry per layer, None where the form has no bias."""
        L = len(d) - 1
        nb = L if form != _lib.NN_STRUCTURED else L - 1
        return [np.empty((d[l], d[l + 1])) for l in range(L)], [np.empty(d[l + 1]) for l in range(nb)] + [None] * (L - nb)

    @staticmethod
    def _keras(Ws, bs):
        out = []
        for l, w in enumerate(Ws):
            out.append(w)
            if l < len(bs) and bs[l] is not None:
                out.append(bs[l])
        return out

    def grad(self, rows):
        """(loss, gradients in Keras order) of the batch of dataset rows ``rows``; no update."""
        r, loss = self._rows(rows), C.c_double()
        gW, gb = self._empty()
        _lib.check(self._lib.nnmpc_train_grad(self._h, r.size, r.ctypes.data_as(C.c_void_p), C.byref(loss),
                                              self._plist(gW), self._plist(gb)), "nnmpc_train_grad")
        return loss.value, self._keras(gW, gb)

    def step(self, rows, want_loss=True):
        """One Adam update; without ``want_loss`` the call does not wait for the device and returns None."""
        r, loss = self._rows(rows), C.c_double()
        _lib.check(self._lib.nnmpc_train_step(self._h, r.size, r.ctypes.data_as(C.c_void_p),
                                              C.byref(loss) if want_loss else None), "nnmpc_train_step")
        return loss.value if want_loss else None

    def epoch(self, perm, batch):
        """All steps of an epoch over the rows ``perm`` (the last batch is the short one); the row-weighted mean loss."""
        r, loss = self._rows(perm), C.c_double()
        _lib.check(self._lib.nnmpc_train_epoch(self._h, r.size, r.ctypes.data_as(C.c_void_p), int(batch), C.byref(loss)),
                   "nnmpc_train_epoch")
        return loss.value

    def eval(self, first, count):
        """Mean squared error over dataset rows [first, first + count), forward only."""
        mse = C.c_double()
        _lib.check(self._lib.nnmpc_train_eval(self._h, int(first), int(count), C.byref(mse)), "nnmpc_train_eval")
        return mse.value

    def get_weights(self):
        Ws, bs = self._empty()
        _lib.check(self._lib.nnmpc_train_get_weights(self._h, self._plist(Ws), self._plist(bs)), "nnmpc_train_get_weights")
        return self._keras(Ws, bs)

    def set_weights(self, weights):
        Ws, bs = _split_keras(weights, self.form)
        if [Ws[0].shape[0]] + [w.shape[1] for w in Ws] != self.dims:
            raise ValueError("set_weights: shapes differ from the network's")
        _lib.check(self._lib.nnmpc_train_set_weights(self._h, self._plist(Ws), self._plist(bs)), "nnmpc_train_set_weights")

    def snapshot(self):
        _lib.check(self._lib.nnmpc_train_snapshot(self._h), "nnmpc_train_snapshot")

    def restore(self):
        _lib.check(self._lib.nnmpc_train_restore(self._h), "nnmpc_train_restore")

    def last_ms(self):
        """(hipEvent ms of the GEMM spans, of the whole last call)."""
        g, t = C.c_double(), C.c_double()
        _lib.check(self._lib.nnmpc_train_last_ms(self._h, C.byref(g), C.byref(t)), "nnmpc_train_last_ms")
        return g.value, t.value

    def dw_slices(self):
        s = (C.c_int32 * self.L)()
        _lib.check(self._lib.nnmpc_train_dw_slices(self._h, s), "nnmpc_train_dw_slices")
        return list(s)

    def padding_max(self):
        m = C.c_double()
        _lib.check(self._lib.nnmpc_train_padding_max(self._h, C.byref(m)), "nnmpc_train_padding_max")
        return m.value


def group_schedule(nrows, batch):
    """Per member the batch sizes of its lock-step steps: ``ceil(nrows[g] / batch)`` steps, the last one the short one;
    a member without rows has none.  Step k of the group runs the members that have a k-th entry."""
    out = []
    for n in nrows:
        n = int(n)
        out.append([min(batch, n - i) for i in range(0, n, batch)])
    return out


class HipGroupTrainer:
    """A sweep of networks in one handle (C ABI ``nnmpc_train_group_*``): what a list of ``HipTrainer`` does, with every
    layer of every member in one launch.  ``weights`` is a list of Keras ``get_weights()`` lists, one per member; the
    members share nx, nu, nnwithuprev, the depth, max_batch, Adam's parameters and one dataset, of which each uses the rows
    it is given.  A member's weights and losses are, byte for byte, those of a ``HipTrainer`` fed the same rows.

    ``form``: one per group, the values ``HipTrainer`` takes.  ``_lib.NN_STRUCTURED`` (the default): every list ends in
    Wout.  ``_lib.NN_UNSTD`` / ``_lib.NN_UNSTD_RELU``: every member is the one-pass network with a bias (and relu) on the
    head, the lists are [W1, b1, ..., WL, bL] and ``get_weights`` / ``set_weights`` exchange that list.

    ``tangents=True`` (structured form only) builds the group of the tangent loss (``nnmpc_train_create_group_tan``):
    ``set_tangents`` after ``set_data``, ``set_tan_weights(ws)`` with one weight per member; then ``epoch`` and ``eval``
    return each member's L = mse + w tan_mse and ``last_losses()`` the two parts.  A member with weight 0 (all are, as
    created) computes the bytes of a member of a plain group, one with w > 0 those of a ``HipTrainer(tangents=True)`` at
    that weight; the lock-step step has the plain group's launches whatever the mix.

    No device: ``_lib.NnmpcError`` (no CPU fallback)."""

    def __init__(self, weights, nx, nu, *, nnwithuprev=True, max_batch=2048, lr=1e-3, betas=(0.9, 0.999), eps=1e-7,
                 form=_lib.NN_STRUCTURED, tangents=False):
        self.form = _check_form(form)
        self.tangents = bool(tangents)
        if self.tangents and self.form != _lib.NN_STRUCTURED:   # refused on the host, before the library is loaded
            raise ValueError("HipGroupTrainer: the tangent loss is built for the structured form only (_lib.NN_STRUCTURED)")
        lib = _lib.load()
        self.G = len(weights)
        Ws, bs, self.dims = [], [], []
        for w in weights:
            Wg, bg = _split_keras(w, self.form)
            Ws.append(Wg); bs.append(bg)
            self.dims.append([Wg[0].shape[0]] + [a.shape[1] for a in Wg])
        L = len(Ws[0]) if Ws else 1
        if any(len(Wg) != L for Wg in Ws):
            raise ValueError("the members of a group have the same depth")
        self.L, self.nx, self.nu, self.nnwithuprev, self.n = L, nx, nu, bool(nnwithuprev), 0
        self.max_batch = int(max_batch)
        self._lib, self._h = lib, C.c_void_p()
        flat = lambda ll: [a for l in ll for a in l]
        create, who = ((lib.nnmpc_train_create_group_tan, "nnmpc_train_create_group_tan") if self.tangents
                       else (lib.nnmpc_train_create_group_ex, "nnmpc_train_create_group_ex"))
        _lib.check(create(C.byref(self._h), self.G, L, (C.c_int32 * max(1, self.G * (L + 1)))(*flat(self.dims)),
                          HipTrainer._plist(flat(Ws)), HipTrainer._plist(flat(bs)), nx, nu, int(self.nnwithuprev),
                          self.max_batch, lr, betas[0], betas[1], eps, self.form), who)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.nnmpc_train_group_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def set_data(self, data):
        """dict(x, uprev, xs, us, u), rows = samples, already scaled; uploaded once as f32 for all members."""
        c = lambda a, w: np.ascontiguousarray(a, np.float64).reshape(-1, w)
        x, xs, us, u = c(data["x"], self.nx), c(data["xs"], self.nx), c(data["us"], self.nu), c(data["u"], self.nu)
        up = c(data["uprev"], self.nu) if self.nnwithuprev and data.get("uprev") is not None else None
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        _lib.check(self._lib.nnmpc_train_group_set_data(self._h, x.shape[0], p(x), p(up), p(xs), p(us), p(u), _lib.HOST),
                   "nnmpc_train_group_set_data")
        self.n = x.shape[0]

    def set_data_device(self, n, x, uprev, xs, us, u):
        """The same from HBM-resident f64 buffers (objects with data_ptr(); ``uprev`` None without uprev)."""
        q = lambda a: None if a is None else C.c_void_p(a.data_ptr())
        _lib.check(self._lib.nnmpc_train_group_set_data(self._h, int(n), q(x), q(uprev), q(xs), q(us), q(u), _lib.DEVICE),
                   "nnmpc_train_group_set_data")
        self.n = int(n)

    def set_tangents(self, tangents):
        """dict(dx, duprev, du) for every row of the shared dataset, as ``HipTrainer.set_tangents`` takes them; after
        ``set_data``, which drops earlier ones.  Uploaded once as f32 for all members."""
        _refuse_fan_in_a_sweep(tangents)
        c = lambda a, w: np.ascontiguousarray(a, np.float64).reshape(-1, w)
        dx, du = c(tangents["dx"], self.nx), c(tangents["du"], self.nu)
        dup = c(tangents["duprev"], self.nu) if self.nnwithuprev and tangents.get("duprev") is not None else None
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        _lib.check(self._lib.nnmpc_train_set_group_tangents(self._h, dx.shape[0], p(dx), p(dup), p(du), _lib.HOST),
                   "nnmpc_train_set_group_tangents")

    def set_tangents_device(self, n, dx, duprev, du):
        """The same from HBM-resident f64 buffers (objects with data_ptr(); ``duprev`` None without uprev)."""
        q = lambda a: None if a is None else C.c_void_p(a.data_ptr())
        _lib.check(self._lib.nnmpc_train_set_group_tangents(self._h, int(n), q(dx), q(duprev), q(du), _lib.DEVICE),
                   "nnmpc_train_set_group_tangents")

    def set_tan_weights(self, ws):
        """One weight of the tangent term per member, each finite and >= 0 (0: the member runs the plain step)."""
        w = np.ascontiguousarray(ws, np.float64).ravel()
        if w.size != self.G:
            raise ValueError(f"set_tan_weights: {w.size} entries for a group of {self.G}")
        _lib.check(self._lib.nnmpc_train_set_group_tan_weights(self._h, w.ctypes.data_as(C.c_void_p)),
                   "nnmpc_train_set_group_tan_weights")

    def last_losses(self):
        """(mse list, tan_mse list) of what the last epoch / eval returned per member (L = mse + w tan_mse); NaN for a
        member that had no rows in it."""
        a, b = np.empty(max(1, self.G)), np.empty(max(1, self.G))
        _lib.check(self._lib.nnmpc_train_last_group_losses(self._h, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)),
                   "nnmpc_train_last_group_losses")
        return [float(v) for v in a[:self.G]], [float(v) for v in b[:self.G]]

    def _i32(self, values, what):
        a = np.ascontiguousarray(values, np.int32).ravel()
        if a.size != self.G:
            raise ValueError(f"{what}: {a.size} entries for a group of {self.G}")
        return a

    def epoch(self, perms, batch):
        """One epoch of every member over its own row list ``perms[g]`` (empty or None: the member sits the epoch out);
        member g takes ``len(group_schedule(...)[g])`` lock-step steps.  Returns the members' row-weighted mean losses
        (NaN for a member without rows)."""
        if len(perms) != self.G:
            raise ValueError(f"epoch: {len(perms)} row lists for a group of {self.G}")
        lists = [np.empty(0, np.int32) if p is None else HipTrainer._rows(p) for p in perms]
        nrows = self._i32([p.size for p in lists], "epoch")
        self.steps = max((len(s) for s in group_schedule(nrows, int(batch))), default=0)
        rows = np.ascontiguousarray(np.concatenate(lists)) if self.G else np.empty(0, np.int32)
        if rows.size == 0:
            rows = np.zeros(1, np.int32)
        loss = np.empty(max(1, self.G))
        _lib.check(self._lib.nnmpc_train_group_epoch(self._h, nrows.ctypes.data_as(C.c_void_p),
                                                     rows.ctypes.data_as(C.c_void_p), int(batch),
                                                     loss.ctypes.data_as(C.c_void_p)), "nnmpc_train_group_epoch")
        return [float(v) for v in loss[:self.G]]

    def eval(self, first, count):
        """Per member the mean squared error over dataset rows [first[g], first[g] + count[g]), forward only
        (count 0: skipped, NaN)."""
        f, c = self._i32(first, "eval"), self._i32(count, "eval")
        mse = np.empty(max(1, self.G))
        _lib.check(self._lib.nnmpc_train_group_eval(self._h, f.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p),
                                                    mse.ctypes.data_as(C.c_void_p)), "nnmpc_train_group_eval")
        return [float(v) for v in mse[:self.G]]

    def _empty(self, g):
        return HipTrainer._empty_for(self.dims[g], self.form)

    def get_weights(self, g):
        """Member g's Keras list of the group's form."""
        Ws, bs = self._empty(g)
        _lib.check(self._lib.nnmpc_train_group_get_weights(self._h, int(g), HipTrainer._plist(Ws),
                                                           HipTrainer._plist(bs)), "nnmpc_train_group_get_weights")
        return HipTrainer._keras(Ws, bs)

    def set_weights(self, g, weights):
        Ws, bs = _split_keras(weights, self.form)
        if [Ws[0].shape[0]] + [w.shape[1] for w in Ws] != self.dims[g]:
            raise ValueError("set_weights: shapes differ from the member's")
        _lib.check(self._lib.nnmpc_train_group_set_weights(self._h, int(g), HipTrainer._plist(Ws),
                                                           HipTrainer._plist(bs)), "nnmpc_train_group_set_weights")

    def snapshot(self, mask):
        m = self._i32([1 if v else 0 for v in mask], "snapshot")
        _lib.check(self._lib.nnmpc_train_group_snapshot(self._h, m.ctypes.data_as(C.c_void_p)), "nnmpc_train_group_snapshot")

    def restore(self, mask):
        m = self._i32([1 if v else 0 for v in mask], "restore")
        _lib.check(self._lib.nnmpc_train_group_restore(self._h, m.ctypes.data_as(C.c_void_p)), "nnmpc_train_group_restore")

    def last_ms(self):
        """(hipEvent ms of the GEMM spans, of the whole last epoch / eval)."""
        g, t = C.c_double(), C.c_double()
        _lib.check(self._lib.nnmpc_train_group_last_ms(self._h, C.byref(g), C.byref(t)), "nnmpc_train_group_last_ms")
        return g.value, t.value

    def last_launches(self):
        """Kernel launches the last epoch / eval enqueued."""
        n = C.c_int64()
        _lib.check(self._lib.nnmpc_train_group_last_launches(self._h, C.byref(n)), "nnmpc_train_group_last_launches")
        return n.value

    def padding_max(self):
        m = C.c_double()
        _lib.check(self._lib.nnmpc_train_group_padding_max(self._h, C.byref(m)), "nnmpc_train_group_padding_max")
        return m.value


def _sweep_args(who, models, data, num_samples, backend):
    """The checks train_nn_controllers and train_unstd_nn_controllers share (host only): (models, rows per member)."""
    models = list(models)
    if backend not in ("hip", "torch"):
        raise ValueError(f"unknown backend {backend!r}: 'torch' or 'hip'")
    if not models:
        raise ValueError(f"{who}: no models")
    n = int(np.asarray(data["x"]).shape[0])
    ns = [n] * len(models) if num_samples is None else [int(v) for v in num_samples]
    if len(ns) != len(models) or any(v < 1 or v > n for v in ns):
        raise ValueError(f"num_samples: one entry per model, each in [1, {n}]")
    return models, ns


def _tan_form(data):
    """(D, whole_input) of a dataset's tangent columns: D from a direction axis of dx ((n, D, nx); (n, nx) is D = 1), the
    whole-input form from the presence of dxs / dus (both, or neither)."""
    has = [data.get(k) is not None for k in ("dxs", "dus")]
    if has[0] != has[1]:
        raise ValueError("train_nn_controller: dxs and dus come together (tangent_data(whole_input=True) makes both)")
    dx = np.asarray(data["dx"])
    return (int(dx.shape[1]) if dx.ndim == 3 else 1), has[0]


def _refuse_fan_in_a_sweep(data):
    """The grouped step stacks one direction in [dx, (duprev)] per row; the richer forms are the single trainer's."""
    if data.get("dx") is not None and (np.asarray(data["dx"]).ndim == 3 or data.get("dxs") is not None or data.get("dus") is not None):
        raise ValueError("the sweep trainers take one direction [dx, (duprev)] per row; several directions per row (a direction "
                         "axis) and whole-input directions (dxs, dus) are built for train_nn_controller / HipTrainer only")


def _first_rows(data, n):
    """The first n rows of the dataset, the tangent columns (``tangent_data``) with them where it has any."""
    out = {k: (None if data.get(k) is None else np.asarray(data[k])[:n]) for k in ("x", "uprev", "xs", "us", "u")}
    out.update({k: np.asarray(data[k])[:n] for k in ("dx", "duprev", "du", "dxs", "dus") if data.get(k) is not None})
    return out


def _sweep_tan_weights(who, models, data, tan_weights):
    """One finite weight >= 0 per model from a scalar, a list or None (all 0); with any > 0 the models are structured and
    ``data`` holds the tangent columns.  Host only."""
    if tan_weights is None:
        return [0.0] * len(models)
    ws = [float(v) for v in np.atleast_1d(np.asarray(tan_weights, dtype=np.float64)).ravel()]
    if np.ndim(tan_weights) == 0:
        ws = ws * len(models)
    if len(ws) != len(models):
        raise ValueError(f"tan_weights: a scalar or one entry per model, got {len(ws)} for {len(models)} models")
    for i, w in enumerate(ws):
        if not (w >= 0.0 and np.isfinite(w)):
            raise ValueError(f"tan_weights[{i}] {w!r}: finite and >= 0")
    if any(w > 0 for w in ws):
        _refuse_fan_in_a_sweep(data)
        for m in models:
            if getattr(m, "unstructured", False):
                raise ValueError(f"{who}: the tangent loss is built for the structured RegulatorModel only")
        need = ("dx", "du") + (("duprev",) if models[0].nnwithuprev else ())
        if any(data.get(k) is None for k in need):
            raise ValueError(f"{who}: tan_weight > 0 needs {', '.join(need)} in data (tangent_data makes them)")
    return ws


def _train_group_hip(models, data, ns, epochs, batch_size, validation_split, lr, seed, log, form=_lib.NN_STRUCTURED,
                     tan_weights=None):
    """The "hip" backend of train_nn_controllers / train_unstd_nn_controllers: one ``HipGroupTrainer`` of ``form``, the
    epoch loop of ``_train_hip`` for every member at once (own rows, own generator, own best epoch).  ``tan_weights`` with
    an entry > 0: the tangent group at those weights, so the members' run and validation losses are their L."""
    m0, G = models[0], len(models)
    tan = tan_weights is not None and any(w > 0 for w in tan_weights)
    tr = HipGroupTrainer([m.get_weights() for m in models], m0.Nx, m0.Nu, nnwithuprev=m0.nnwithuprev,
                         max_batch=batch_size, lr=lr, eps=1e-7, form=form, **({"tangents": True} if tan else {}))
    try:
        tr.set_data(data)
        if tan:
            tr.set_tangents(data)
            tr.set_tan_weights(tan_weights)
        nval = [int(v * validation_split) for v in ns]
        ntr = [v - w for v, w in zip(ns, nval)]
        rngs = [np.random.default_rng(seed) for _ in range(G)]
        best, hists = [float("inf")] * G, [[] for _ in range(G)]
        t0 = time.time()
        for ep in range(epochs):
            run = tr.epoch([rngs[g].permutation(ntr[g]) for g in range(G)], batch_size)
            vl = tr.eval(ntr, nval) if any(nval) else run
            better = []
            for g in range(G):
                v = vl[g] if nval[g] else run[g]
                hists[g].append((run[g], v))
                better.append(v < best[g])                  # ModelCheckpoint(save_best_only=True), per member
                if better[g]:
                    best[g] = v
            if any(better):
                tr.snapshot(better)
            if log:
                log(f"epoch {ep + 1}/{epochs} " + " ".join(f"[{g}] loss {hists[g][-1][0]:.3e} val_loss {hists[g][-1][1]:.3e}"
                                                          for g in range(G)))
        tr.restore([b < float("inf") for b in best])
        ttime = time.time() - t0
        for g, m in enumerate(models):
            m.set_weights(tr.get_weights(g))
    finally:
        tr.close()
    return models, ttime, hists


def train_nn_controllers(models, data, *, num_samples=None, epochs=1500, batch_size=2048, validation_split=0.05,
                         lr=1e-3, seed=1, log=None, backend="hip", tan_weights=None):
    """``train_nn_controller`` for a sweep: member i is ``models[i]`` trained on the first ``num_samples[i]`` rows of
    ``data`` (default: all), which is what the reference's loop over ``itertools.product(regulator_dims, num_samples)``
    hands each of its calls.  Keras semantics per member: the last ``int(n_i * validation_split)`` of its rows are its
    validation set, the rest is reshuffled every epoch by the member's own ``np.random.default_rng(seed)`` -- the row
    order a separate ``train_nn_controller(..., backend="hip", seed=seed)`` would give it -- and the weights of its best
    validation epoch are restored at the end.  Returns (models, training_time, hists), hists[i] as that call's history.

    ``backend="hip"``: one ``HipGroupTrainer``, all members in lock step; the models must agree in Nx, Nu, nnwithuprev
    and depth (``ValueError`` otherwise; build one group per depth), and an ``UnstdRegulatorModel`` is refused: its sweep
    is ``train_unstd_nn_controllers``.  ``backend="torch"``: a loop over ``train_nn_controller``.

    ``tan_weights``: a scalar or one weight per model, each finite and >= 0: member i trains on
    L = mse + tan_weights[i] tan_mse (``train_nn_controller(tan_weight=...)``; ``data`` then also holds dx, (duprev), du)
    and its history holds L.  ``backend="hip"`` builds one tangent group when any weight is > 0 -- a member's weights and
    history are, byte for byte, those of its own ``train_nn_controller(..., backend="hip", tan_weight=w_i, seed=seed)`` --
    and the plain group otherwise; ``backend="torch"`` loops over ``train_nn_controller(tan_weight=w_i)``."""
    models, ns = _sweep_args("train_nn_controllers", models, data, num_samples, backend)
    ws = _sweep_tan_weights("train_nn_controller", models, data, tan_weights)
    if backend == "torch":
        t0, hists = time.time(), []
        for i, m in enumerate(models):
            models[i], _, h = train_nn_controller(m, _first_rows(data, ns[i]), epochs=epochs, batch_size=batch_size,
                                                  validation_split=validation_split, lr=lr, seed=seed, log=log,
                                                  tan_weight=ws[i])
            hists.append(h)
        return models, time.time() - t0, hists
    for m in models:
        _refuse_unstructured(m, "train_nn_controllers(backend=\"hip\")")
    m0 = models[0]
    for m in models[1:]:
        if (m.Nx, m.Nu, bool(m.nnwithuprev), len(m.layers)) != (m0.Nx, m0.Nu, bool(m0.nnwithuprev), len(m0.layers)):
            raise ValueError("train_nn_controllers: the models of a group agree in Nx, Nu, nnwithuprev and depth")
    return _train_group_hip(models, data, ns, epochs, batch_size, validation_split, lr, seed, log,
                            tan_weights=ws if any(w > 0 for w in ws) else None)


def train_unstd_nn_controllers(models, data, *, num_samples=None, epochs=2000, batch_size=1024, validation_split=0.1,
                               lr=1e-3, seed=1, log=None, backend="hip"):
    """``train_unstd_nn_controller`` for a sweep, with the semantics of ``train_nn_controllers`` and the defaults of
    ``cstrs_train_unstd.py``: member i is the ``UnstdRegulatorModel`` ``models[i]`` trained on the first
    ``num_samples[i]`` rows of ``data`` (default: all), validated on the last ``int(n_i * validation_split)`` of them,
    shuffled by its own ``np.random.default_rng(seed)``, and comes back with the weights of its own best validation epoch.
    Weights and histories are, byte for byte, those of a separate ``train_unstd_nn_controller(..., backend="hip",
    seed=seed)`` on those rows.  Returns (models, training_time, hists).

    ``backend="hip"``: one ``HipGroupTrainer`` of the models' form; they must agree in Nx, Nu, nnwithuprev, depth and
    ``head_relu`` (a group has one form; ``ValueError`` otherwise, as for a structured model, before the library is
    loaded).  ``backend="torch"``: a loop over ``train_unstd_nn_controller(backend="torch")``."""
    models, ns = _sweep_args("train_unstd_nn_controllers", models, data, num_samples, backend)
    forms = [_unstd_form(m, "train_unstd_nn_controllers") for m in models]
    m0 = models[0]
    for m in models[1:]:
        if (m.Nx, m.Nu, bool(m.nnwithuprev), len(m.layers), m.head_relu) != (m0.Nx, m0.Nu, bool(m0.nnwithuprev), len(m0.layers), m0.head_relu):
            raise ValueError("train_unstd_nn_controllers: the models of a group agree in Nx, Nu, nnwithuprev, depth and head_relu")
    if backend == "torch":
        t0, hists = time.time(), []
        for i, m in enumerate(models):
            models[i], _, h = train_unstd_nn_controller(m, _first_rows(data, ns[i]), epochs=epochs, batch_size=batch_size,
                                                        validation_split=validation_split, lr=lr, seed=seed, log=log,
                                                        backend="torch")
            hists.append(h)
        return models, time.time() - t0, hists
    return _train_group_hip(models, data, ns, epochs, batch_size, validation_split, lr, seed, log, forms[0])


def _train_hip(model, data, epochs, batch_size, validation_split, lr, device, seed, log, form=_lib.NN_STRUCTURED,
               tan_weight=0.0):
    """The "hip" backend of train_nn_controller / train_unstd_nn_controller: same Keras semantics, every step on the
    device in f32.  ``tan_weight > 0``: the tangent handle, so run and validation losses are L."""
    D, whole = _tan_form(data) if tan_weight > 0 else (1, False)
    more = dict(tan_dirs=D, tan_whole_input=whole) if (D, whole) != (1, False) else {}   # the defaults: the one-direction entry points
    tr = HipTrainer(model.get_weights(), model.Nx, model.Nu, nnwithuprev=model.nnwithuprev, max_batch=batch_size,
                    lr=lr, eps=1e-7, form=form, tangents=tan_weight > 0, **more)
    try:
        tr.set_data(data)
        if tan_weight > 0:
            tr.set_tangents(data)
            tr.set_tan_weight(tan_weight)
        n = tr.n
        nval = int(n * validation_split)
        ntr = n - nval
        rng = np.random.default_rng(seed)
        best, hist = float("inf"), []
        t0 = time.time()
        for ep in range(epochs):
            run = tr.epoch(rng.permutation(ntr), batch_size)
            vl = tr.eval(ntr, nval) if nval else run
            hist.append((run, vl))
            if vl < best:                                   # ModelCheckpoint(save_best_only=True)
                best = vl
                tr.snapshot()
            if log:
                log(f"epoch {ep + 1}/{epochs} loss {run:.3e} val_loss {vl:.3e}")
        if best < float("inf"):
            tr.restore()
        ttime = time.time() - t0
        model.set_weights(tr.get_weights())
    finally:
        tr.close()
    if device:
        model = model.to(device)
    return model, ttime, hist


def tangent_loss(model, x, uprev, xs, us, u, dx, duprev, du, w, dxs=None, dus=None):
    """(L, mse, tan_mse) of a structured ``RegulatorModel`` on a batch, in stock torch:

        L = mean (pred - u)^2 + w mean (J d - du)^2,

    J d the tangent of pred along d = [dx, (duprev)], propagated forward through the same weights -- a'_0 = [dx, (duprev), 0, 0],
    a'_l = (a'_{l-1} W_l) * [a_l(pass 1) > 0], J d = a'_{L-1} W_L; no bias, ReLU derivative 0 at 0 (a NaN activation passes,
    as in the native step), pass 2 does not depend on x or uprev.  The masks carry no gradient (ReLU has no second
    derivative), so autograd through this is the gradient the native step computes.  ``duprev`` is ignored without uprev.

    ``dx``, ``duprev``, ``du`` may carry a direction axis, (B, D, width): D directions per row, each with its target, and the
    second mean runs over B D nu.  With ``dxs`` and ``dus`` (both, same shape rule) the direction is over the whole input,
    d = [dx, (duprev), dxs, dus]: a'_0 = [dx, (duprev), dxs, dus] under the masks of pass 1, a''_0 = [dxs, (dus), dxs, dus]
    under the masks of pass 2, and J d = dus + (a'_{L-1} W_L - a''_{L-1} W_L)."""
    if (dxs is None) != (dus is None):
        raise ValueError("tangent_loss: dxs and dus come together")
    whole = dxs is not None
    ax = lambda a: a if a.dim() == 3 else a.unsqueeze(1)       # (B, D, width)
    dx, du = ax(dx), ax(du)
    zx, zu = torch.zeros_like(dx), torch.zeros_like(du)
    sx, su = (ax(dxs), ax(dus)) if whole else (zx, zu)
    if model.nnwithuprev:
        z1, z2 = torch.cat((x, uprev, xs, us), -1), torch.cat((xs, us, xs, us), -1)
        ta, tb = torch.cat((dx, ax(duprev), sx, su), -1), torch.cat((sx, su, sx, su), -1)
    else:
        z1, z2 = torch.cat((x, xs, us), -1), torch.cat((xs, xs, us), -1)
        ta, tb = torch.cat((dx, sx, su), -1), torch.cat((sx, sx, su), -1)
    a, a2 = z1, z2
    for lin in model.layers[:-1]:
        a, a2 = torch.relu(lin(a)), torch.relu(lin(a2))
        ta = (ta @ lin.weight.T) * (~(a <= 0)).to(a.dtype).unsqueeze(1)
        if whole:
            tb = (tb @ lin.weight.T) * (~(a2 <= 0)).to(a.dtype).unsqueeze(1)
    head = model.layers[-1]
    pred = us + head(a) - head(a2)
    mse = torch.mean((pred - u) ** 2)
    jd = su + (ta @ head.weight.T - tb @ head.weight.T) if whole else ta @ head.weight.T
    tan = torch.mean((jd - du) ** 2)
    return mse + w * tan, mse, tan


def whole_input_perturbation(dx, duprev, dxs, dus, xscale):
    """(dX0, dulb, duub): what a whole-input direction [dx, duprev, dxs, dus] of the scaled dataset does to the regulator's
    problem.  The MPC law is u = us + kappa(x - xs, uprev - us; ulb - us, uub - us), so along the direction

        dX0 = [dx * xscale - dxs * xscale, duprev - dus],    dulb = duub = -dus,

    and the absolute first move changes by dus + du0, du0 the regulator's ``sensitivity_batch(info, dX0, dulb, duub,
    first_move_only=True)``.  Arrays of any leading shape; the last axis is nx or nu."""
    dx, dup, dxs, dus = (np.asarray(a, float) for a in (dx, duprev, dxs, dus))
    xscale = np.asarray(xscale, float).reshape(-1)
    dX0 = np.concatenate((dx * xscale - dxs * xscale, dup - dus), axis=-1)
    return dX0, -dus, -dus


def tangent_data(regulator, data, xscale, *, ulb, uub, seed=0, nnwithuprev=True, directions=1, whole_input=False):
    """Tangent targets for ``train_nn_controller(..., tan_weight=w)`` from the regulator's own solves.

    ``data``: the raw generated rows dict(x, uprev, xs, us) (before scaling); ``xscale``: what
    ``_get_data_for_training`` divides x and xs by; ``ulb`` / ``uub``: the plant's input bounds (Nu,).  Per row one
    standard-normal direction is drawn in the units of the scaled dataset, d = [dx, duprev] (``seed``); the batch
    X0 = [x - xs, uprev - us] is solved with bounds ulb - us, uub - us and ``first_move_only=True``, and
    ``regulator.sensitivity_batch(info, dX0=[dx * xscale, duprev], first_move_only=True)`` gives du, the change of the
    MPC's first move along the direction inside the row's critical region.  ``nnwithuprev=False`` (a network that
    does not see uprev; the regulator still starts from ``data["uprev"]``): the duprev part of dX0, and the returned
    ``duprev``, are zero.

    Returns dict(dx (n, Nx), duprev (n, Nu), du (n, Nu), flag (n,)).  A row whose sensitivity flag is not 0, or whose
    solve status is not 0, has no certified slope: its direction AND its target are set to zero, so J d = 0 = du and the
    row contributes exactly nothing to the tangent term or its gradient.  The mean's denominator stays B nu all the same
    (such rows weigh the term down, they do not bias it).

    ``directions=D`` and ``whole_input``: D directions per row from the same one solve and ONE ``sensitivity_batch`` call;
    dx, duprev, du are then (n, D, .) -- whenever either argument is given, so ``directions=1, whole_input=True`` has the axis
    too.  With ``whole_input`` the direction is over the whole network input: dxs (n, D, Nx) and dus (n, D, Nu) are drawn
    and returned as well, the regulator's problem moves along ``whole_input_perturbation`` and the target is the change of
    the absolute first move, du = dus + du0.  A row without a certified slope is zero in every direction, dxs and dus
    included (so J d = 0 = du still holds).  The defaults draw and return exactly what they did before the arguments existed."""
    x, xs = np.asarray(data["x"], float), np.asarray(data["xs"], float)
    us, up = np.asarray(data["us"], float), np.asarray(data["uprev"], float)
    n, nx, nu = x.shape[0], x.shape[1], us.shape[1]
    xscale = np.asarray(xscale, float).reshape(1, nx)
    rng = np.random.default_rng(seed)
    D = int(directions)
    if D < 1:
        raise ValueError(f"tangent_data: directions {directions!r} (>= 1)")
    fan = D != 1 or bool(whole_input)
    shape = (lambda w: (n, D, w)) if fan else (lambda w: (n, w))
    dx = rng.standard_normal(shape(nx))
    dup = rng.standard_normal(shape(nu)) if nnwithuprev else np.zeros(shape(nu))
    lb = np.asarray(ulb, float).reshape(1, nu) - us
    ub = np.asarray(uub, float).reshape(1, nu) - us
    _, info = regulator.solve_batch(np.concatenate((x - xs, up - us), axis=1), lb, ub, first_move_only=True)
    if whole_input:
        dxs, dus = rng.standard_normal(shape(nx)), rng.standard_normal(shape(nu))
        dX0, dlb, dub = whole_input_perturbation(dx, dup, dxs, dus, xscale)
        out = regulator.sensitivity_batch(info, dX0, dulb=dlb, duub=dub, first_move_only=True)
    else:
        out = regulator.sensitivity_batch(info, np.concatenate((dx * xscale, dup), axis=-1), first_move_only=True)
    flag = np.asarray(out["flag"]).astype(np.int32).ravel().copy()
    bad = (flag != 0) | (np.asarray(info["status"]).ravel() != 0)
    du = np.array(out["du"], float).reshape(shape(nu))
    if whole_input:
        du = dus + du
        dxs[bad] = 0.0; dus[bad] = 0.0
    dx[bad] = 0.0; dup[bad] = 0.0; du[bad] = 0.0
    res = dict(dx=dx, duprev=dup, du=du, flag=flag)
    if whole_input:
        res.update(dxs=dxs, dus=dus)
    return res


def train_nn_controller(model, data, *, epochs=1500, batch_size=2048, validation_split=0.05, lr=1e-3,
                        device=None, seed=1, log=None, backend="torch", tan_weight=0.0):
    """Adam + MSE on ``data`` = dict(x, uprev, xs, us, u) (rows = samples, already scaled like
    the reference's _get_data_for_training).  Keras semantics: the LAST fraction of the rows is
    the validation set, the rest is reshuffled every epoch; the weights of the best validation
    epoch are restored at the end.  Returns (model, training_time, history).

    ``backend="torch"``: stock PyTorch ops in the model's dtype on ``device``.  ``backend="hip"``: the native f32
    step (``HipTrainer``), shuffled by a numpy generator seeded with ``seed``; ``model`` comes back carrying the
    trained weights.  No device: ``_lib.NnmpcError`` (no CPU fallback).

    ``tan_weight = w > 0`` (a structured ``RegulatorModel`` only): the loss is ``tangent_loss``, L = mse + w tan_mse, and
    ``data`` also holds dx, (duprev) and du, one direction and one slope target per row (``tangent_data``).  Both backends
    serve it; the history, the validation loss and the best-epoch checkpoint are then those of L.  0 (the default) is
    the plain loss, exactly as without the argument.  The form is read from ``data``: dx of shape (n, D, Nx) means D
    directions per row (duprev and du likewise), and dxs / dus beside them mean directions over the whole network input
    (``tangent_data(directions=D, whole_input=True)``)."""
    tan_weight = float(tan_weight)
    if not (tan_weight >= 0.0 and np.isfinite(tan_weight)):
        raise ValueError(f"tan_weight {tan_weight!r}: finite and >= 0")
    if tan_weight > 0:
        if getattr(model, "unstructured", False):
            raise ValueError("train_nn_controller: the tangent loss is built for the structured RegulatorModel only")
        need = ("dx", "du") + (("duprev",) if model.nnwithuprev else ())
        if any(data.get(k) is None for k in need):
            raise ValueError(f"train_nn_controller: tan_weight > 0 needs {', '.join(need)} in data (tangent_data makes them)")
        whole = _tan_form(data)[1]
    if backend == "hip":
        _refuse_unstructured(model, "train_nn_controller(backend=\"hip\")")
        return _train_hip(model, data, epochs, batch_size, validation_split, lr, device, seed, log, tan_weight=tan_weight)
    if backend != "torch":
        raise ValueError(f"unknown backend {backend!r}: 'torch' or 'hip'")
    torch.manual_seed(seed)
    device = device or ("cuda" if torch.cuda.is_available() else "cpu")
    model = model.to(device)
    dt = next(model.parameters()).dtype
    T = {k: torch.as_tensor(np.asarray(data[k]), dtype=dt, device=device) for k in ("x", "xs", "us", "u")}
    T["uprev"] = (torch.as_tensor(np.asarray(data["uprev"]), dtype=dt, device=device)
                  if model.nnwithuprev else torch.zeros_like(T["us"]))
    if tan_weight > 0:
        T["dx"], T["du"] = (torch.as_tensor(np.asarray(data[k]), dtype=dt, device=device) for k in ("dx", "du"))
        T["duprev"] = (torch.as_tensor(np.asarray(data["duprev"]), dtype=dt, device=device)
                       if model.nnwithuprev else torch.zeros_like(T["du"]))
        keys = ("x", "uprev", "xs", "us", "u", "dx", "duprev", "du")
        if whole:
            T["dxs"], T["dus"] = (torch.as_tensor(np.asarray(data[k]), dtype=dt, device=device) for k in ("dxs", "dus"))
            keys += ("dxs", "dus")

        def loss_of(S, idx):
            a = [S[k][idx] for k in keys]
            return tangent_loss(model, *a[:8], tan_weight, *a[8:])[0]
    else:
        def loss_of(S, idx):
            return torch.mean((model(S["x"][idx], S["uprev"][idx], S["xs"][idx], S["us"][idx]) - S["u"][idx]) ** 2)
    n = T["x"].shape[0]
    nval = int(n * validation_split)
    ntr = n - nval
    tr = {k: v[:ntr] for k, v in T.items()}
    va = {k: v[ntr:] for k, v in T.items()}
    opt = torch.optim.Adam(model.parameters(), lr=lr, eps=1e-7)   # Keras Adam defaults
    best, best_state, hist = float("inf"), None, []
    t0 = time.time()
    for ep in range(epochs):
        model.train()
        perm = torch.randperm(ntr, device=device)
        run = 0.0
        for i in range(0, ntr, batch_size):
            idx = perm[i:i + batch_size]
            loss = loss_of(tr, idx)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            run += float(loss.detach()) * idx.numel()
        model.eval()
        with torch.no_grad():
            vl = float(loss_of(va, slice(None))) if nval else run / ntr
        hist.append((run / ntr, vl))
        if vl < best:                                   # ModelCheckpoint(save_best_only=True)
            best, best_state = vl, copy.deepcopy(model.state_dict())
        if log:
            log(f"epoch {ep + 1}/{epochs} loss {run / ntr:.3e} val_loss {vl:.3e}")
    if best_state is not None:
        model.load_state_dict(best_state)
    return model, time.time() - t0, hist


def train_unstd_nn_controller(model, data, *, epochs=2000, batch_size=1024, validation_split=0.1, lr=1e-3,
                              device=None, seed=1, log=None, backend="hip"):
    """``train_nn_controller`` of the reference's ``cstrs_train_unstd.py`` (:40-57), with that script's defaults, for an
    ``UnstdRegulatorModel``.  ``backend="hip"``: the native f32 step in its one-pass form (``HipTrainer(form=...)``, the
    form taken from ``model.head_relu``), Keras semantics as ``train_nn_controller(backend="hip")``: the last fraction of
    the rows validates, the rest is reshuffled every epoch by ``np.random.default_rng(seed)``, the weights of the best
    validation epoch come back in ``model``.  ``backend="torch"``: ``train_nn_controller(backend="torch")``.
    Returns (model, training_time, history).  No device: ``_lib.NnmpcError`` (no CPU fallback)."""
    if backend not in ("hip", "torch"):
        raise ValueError(f"unknown backend {backend!r}: 'torch' or 'hip'")
    form = _unstd_form(model, "train_unstd_nn_controller")
    if backend == "torch":
        return train_nn_controller(model, data, epochs=epochs, batch_size=batch_size, validation_split=validation_split,
                                   lr=lr, device=device, seed=seed, log=log, backend="torch")
    return _train_hip(model, data, epochs, batch_size, validation_split, lr, device, seed, log, form)
