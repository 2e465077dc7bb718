"""NN controller forwards on the GPU (host wrappers over the C ABI).

Structured:
    u = clip(us + NN(x/xscale, [uprev], xs/xscale, us) - NN(xs/xscale, [us], xs/xscale, us))
Reference: RegulatorLayerWithUprev / RegulatorLayerWithoutUprev.call
(lib/LinearMPCLayers.py:40-61, :91-112) and NeuralNetworkController
._get_control_input (lib/controller_evaluation.py:863-892).

Unstructured:
    u = clip(NN(x/xscale, [uprev], xs/xscale, us))
Reference: NeuralNetworkControllerUnstd (lib/controller_evaluation.py:895-916) and
UnstdRegulatorLayer.call (lib/LinearMPCLayers.py:135-156).
"""
import ctypes as C
import numpy as np

from . import _lib


class _DeviceNN:
    """What the two forwards share: the handle's life, ``forward``, ``forward_device`` and the timers.  A subclass splits the
    Keras list into kernels and biases (``_split``) and names its form (``_form``)."""

    def _split(self, weights):
        raise NotImplementedError

    def _form(self):
        raise NotImplementedError

    def _create(self, weights, nx, nu, nnwithuprev, xscale, ulb, uub, max_batch, use_bf16):
        Ws, bs = self._split(weights)                          # bs: one entry per layer, None where the layer has no bias
        lib = _lib.load()
        L = len(Ws)
        dims = [Ws[0].shape[0]] + [w.shape[1] for w in Ws]
        self.nx, self.nu, self.nnwithuprev = nx, nu, bool(nnwithuprev)
        dims_c = (C.c_int32 * (L + 1))(*dims)
        Wp = (C.c_void_p * L)(*[w.ctypes.data for w in Ws])
        bp = (C.c_void_p * L)(*[None if b is None else b.ctypes.data for b in bs])
        opt = lambda a: None if a is None else np.ascontiguousarray(np.ravel(a), np.float64)
        xs_, lb_, ub_ = opt(xscale), opt(ulb), opt(uub)
        self._keep = (Ws, bs, xs_, lb_, ub_)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        self._h = C.c_void_p()
        mode = 2 if use_bf16 in ("split", 2) else int(bool(use_bf16))
        form = self._form()
        if form == _lib.NN_STRUCTURED:
            _lib.check(lib.nnmpc_nn_create(C.byref(self._h), L, dims_c, Wp, bp, nx, nu, int(nnwithuprev),
                                           p(xs_), p(lb_), p(ub_), mode, max_batch), "nnmpc_nn_create")
        else:
            _lib.check(lib.nnmpc_nn_create_ex(C.byref(self._h), L, dims_c, Wp, bp, nx, nu, int(nnwithuprev),
                                              p(xs_), p(lb_), p(ub_), mode, max_batch, form), "nnmpc_nn_create_ex")
        self._lib = lib

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.nnmpc_nn_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def forward(self, x, uprev, xs, us):
        """numpy (B, nx), (B, nu), (B, nx), (B, nu) -> (B, nu)."""
        c = lambda a, w: np.ascontiguousarray(a, np.float64).reshape(-1, w)
        x, xs, us = c(x, self.nx), c(xs, self.nx), c(us, self.nu)
        up = c(uprev, self.nu) if self.nnwithuprev else None
        B = x.shape[0]
        u = np.empty((B, self.nu))
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        _lib.check(self._lib.nnmpc_nn_forward(self._h, B, p(x), p(up), p(xs), p(us), p(u), _lib.HOST),
                   "nnmpc_nn_forward")
        return u

    def forward_device(self, B, x, uprev, xs, us, u):
        """HBM-resident f64 buffers (objects with data_ptr())."""
        q = lambda a: None if a is None else C.c_void_p(a.data_ptr())
        _lib.check(self._lib.nnmpc_nn_forward(self._h, B, q(x), q(uprev), q(xs), q(us), q(u), _lib.DEVICE),
                   "nnmpc_nn_forward")

    def last_ms(self):
        g, t = C.c_double(), C.c_double()
        self._lib.nnmpc_nn_last_ms(self._h, C.byref(g), C.byref(t))
        return g.value, t.value

    def last_hidden_ms(self):
        """(hipEvent ms of the hidden-layer GEMMs of the last forward, number of those launches)."""
        g, k = C.c_double(), C.c_int32()
        self._lib.nnmpc_nn_last_hidden_ms(self._h, C.byref(g), C.byref(k))
        return g.value, k.value


class StructuredNN(_DeviceNN):
    """``weights``: Keras get_weights() order [W1 (in x h), b1, ..., Wout (h x nu)].

    ``use_bf16``: False -- f32 MFMA GEMMs; True -- bf16 operands, f32 accumulation (~2e-2 relative error on the CDU
    architecture); "split" (or 2) -- activations and weights as bf16 pairs hi + lo, every layer ONE bf16 GEMM of three times
    the depth (hi hi' + hi lo' + lo hi'): f32-grade results (~1e-5) from the bf16 matrix pipes."""

    def __init__(self, weights, nx, nu, *, nnwithuprev=True, xscale=None, ulb=None, uub=None,
                 max_batch=65536, use_bf16=False):
        self._create(weights, nx, nu, nnwithuprev, xscale, ulb, uub, max_batch, use_bf16)

    def _form(self):
        return _lib.NN_STRUCTURED

    def _split(self, weights):
        Ws = [np.ascontiguousarray(w, np.float64) for w in weights[0:-1:2]] + \
             [np.ascontiguousarray(weights[-1], np.float64)]
        bs = [np.ascontiguousarray(b, np.float64).ravel() for b in weights[1::2]]
        if len(bs) != len(Ws) - 1:
            raise ValueError("weights must be [W1, b1, ..., W_{L-1}, b_{L-1}, Wout]")
        return Ws, bs + [None]


def split_unstd_weights(weights):
    """The Keras get_weights() list of UnstdRegulatorModel, [W1, b1, ..., WL, bL], as (kernels, biases) in fp64;
    ``ValueError`` for a list of odd length, a bias that does not fit its kernel or kernels that do not chain."""
    weights = list(weights)
    if not weights or len(weights) % 2:
        raise ValueError("unstructured weights must be [W1, b1, ..., WL, bL] (every layer has a bias: an even-length list), "
                         f"got {len(weights)} arrays")
    Ws = [np.ascontiguousarray(w, np.float64) for w in weights[0::2]]
    bs = [np.ascontiguousarray(b, np.float64).ravel() for b in weights[1::2]]
    for l, (w, b) in enumerate(zip(Ws, bs)):
        if w.ndim != 2 or b.size != w.shape[1] or (l and w.shape[0] != Ws[l - 1].shape[1]):
            raise ValueError(f"unstructured weights: layer {l} has kernel {w.shape} and bias ({b.size},)")
    return Ws, bs


class UnstructuredNN(_DeviceNN):
    """u = clip(MLP([x / xscale, (uprev), xs / xscale, us])): one pass, hidden layers relu(W'z + b), the head with a bias.

    ``weights``: Keras get_weights() order of UnstdRegulatorModel, [W1, b1, ..., WL, bL] (an odd-length list: ``ValueError``).
    ``head_relu``: False -- linear head, what NeuralNetworkControllerUnstd computes (lib/controller_evaluation.py:907-908);
    True -- relu on the head as well, what the Keras UnstdRegulatorLayer computes (lib/LinearMPCLayers.py:147-148).
    ``use_bf16`` as for ``StructuredNN``."""

    def __init__(self, weights, nx, nu, *, nnwithuprev=True, xscale=None, ulb=None, uub=None,
                 max_batch=65536, use_bf16=False, head_relu=False):
        self.head_relu = bool(head_relu)
        self._create(weights, nx, nu, nnwithuprev, xscale, ulb, uub, max_batch, use_bf16)

    def _form(self):
        return _lib.NN_UNSTD_RELU if self.head_relu else _lib.NN_UNSTD

    def _split(self, weights):
        return split_unstd_weights(weights)
