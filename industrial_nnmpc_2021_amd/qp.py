"""Batched box-constrained condensed QP on the GPU (host wrapper over the C ABI).

    min 1/2 u'Pu + (tq x0)'u   s.t.  lb <= u_k <= ub,  k = 0..N-1

is what DenseQPRegulator.solve hands to cvxopt.solvers.qp for a stable plant
(reference lib/linearMPC.py:495-512 with G = tE, :476-482).  ``BatchedBoxQP``
solves B of them per call in HIP kernels (see csrc/qp_solver.hip).
"""
import ctypes as C
import numpy as np

from . import _lib


def _ptr(a):
    """Pointer of a numpy array (host) or of anything exposing data_ptr() (device)."""
    if a is None:
        return None, None
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr()), _lib.DEVICE
    return a.ctypes.data_as(C.c_void_p), _lib.HOST


def _staircase(U0, tol, block=128, chunk=16):
    """Rotate the basis of the far-field factors so that far column tiles use few coordinates.

    U0 (rows of the far block x r).  The row space of the suffix U0[128 j:] shrinks as j grows -- the closed loop forgets its
    fast modes first.  Going down the blocks, the coordinates (within the ones still in use) whose singular values over ALL the
    remaining rows are below tol are moved behind the ones that stay (SVD of the suffix in the current basis; what is dropped is
    small on every later row by construction, nothing is ever estimated from a weak block).  With the orthonormal G (r' x r) this
    gives  U0 = U1 G,  U1[block j, k_j:] = 0  up to tol per dropping step: a staircase.  Returns (U1 with those entries set to
    exact zeros, k_j rounded up to whole K chunks of the GEMM; G).  The library's GEMM stops a column tile's K loop at k_j
    (nnmpc_qp_set_farfield finds the zeros), and its device check of U V' against M covers the truncation."""
    import scipy.linalg as sla
    nf, r = U0.shape
    nb = -(-nf // block)
    Rs = [None] * nb                                     # R factor of the suffix U0[128 j:], bottom-up (same singular values / row space)
    below = np.zeros((0, r))
    for j in range(nb - 1, -1, -1):
        below = Rs[j] = sla.qr(np.vstack((U0[j * block:(j + 1) * block], below)), mode="r")[0][:r]
    cur = np.eye(r)                                      # rows: the coordinates still in use
    drops, kj = [], np.zeros(nb, int)
    for j in range(nb):
        if cur.shape[0]:
            _, sv, vt = sla.svd(Rs[j] @ cur.T)           # (full: vt is square, the rows beyond the rank span what is dropped)
            k = int((sv > tol).sum())
            drops.append(vt[k:] @ cur)
            cur = vt[:k] @ cur
        else:
            drops.append(np.zeros((0, r)))
        kj[j] = cur.shape[0]
    G = np.vstack([cur] + drops[:0:-1])                  # (what block 0 drops is below tol everywhere: not part of the factors)
    if G.shape[0] == 0:
        G = np.eye(1, r)
    kj = np.minimum(-(-kj // chunk) * chunk, G.shape[0])
    U1 = U0 @ G.T
    for j in range(nb):
        U1[j * block:(j + 1) * block, kj[j]:] = 0.0
    return np.ascontiguousarray(U1), G


class BatchedBoxQP:
    """Owns the device copies of (P, tq) and the solver workspace.

    P: (n, n) condensed Hessian (lower triangle read, as cvxopt does),
    tq: (n, n_aug) so that q = tq @ x0, nu: inputs per stage (bounds are per
    stage and tiled along the horizon like the reference's _get_h).
    """

    def __init__(self, P, tq, nu, *, Kunc="auto", method="auto", farfield="auto", max_batch=1024, nb=0, ipm_tol=0.0,
                 max_rounds=0, max_ipm_iters=0, max_polish_rounds=0, max_refine=0, sub_steps=0, stale_max_changes=0, stale_cg_limit=0, asm_max_active=0,
                 asm_max_rounds=0, asm_f32_rounds=0, seg_max=0, asm_tail_batch=0, asm_predict_iters=0, asm_overlap=0):
        lib = _lib.load()
        P = np.ascontiguousarray(P, dtype=np.float64)
        tq = np.ascontiguousarray(tq, dtype=np.float64)
        n, n_aug = tq.shape
        if P.shape != (n, n) or n % nu:
            raise ValueError("P must be (n, n), tq (n, n_aug), n a multiple of nu")
        meth = {"auto": 0, "pdip": 1, "asm": 2}[method]
        Hinv = None
        if isinstance(Kunc, str) and Kunc == "auto":
            # one-time host setup in fp64 (like the reference's DARE/condensing in
            # DenseQPRegulator.__init__): u_unc = Kunc x0 = -P^-1 tq x0 (warm start), and, for
            # the shared-inverse active-set pass, P^-1 itself
            import scipy.linalg as sla
            Ps = np.tril(P) + np.tril(P, -1).T
            cf = sla.cho_factor(Ps, lower=True)
            Kunc = -sla.cho_solve(cf, tq)
            if meth != 1:
                Hinv = sla.cho_solve(cf, np.eye(n))
        elif meth == 2:
            raise ValueError("method='asm' needs Kunc='auto' (the inverse Hessian is built with it)")
        if Kunc is not None:
            Kunc = np.ascontiguousarray(Kunc, dtype=np.float64)
        self.n, self.n_aug, self.nu = n, n_aug, nu
        self.words = (2 * n + 31) // 32
        opts = _lib.QpOpts(max_batch=max_batch, nb=nb, max_ipm_iters=max_ipm_iters,
                           max_polish_rounds=max_polish_rounds, max_refine=max_refine,
                           max_rounds=max_rounds, sub_steps=sub_steps, stale_max_changes=stale_max_changes,
                           stale_cg_limit=stale_cg_limit, method=meth, asm_max_active=asm_max_active,
                           asm_max_rounds=asm_max_rounds, asm_f32_rounds=asm_f32_rounds, seg_max=seg_max, asm_tail_batch=asm_tail_batch,
                           asm_predict_iters=asm_predict_iters, asm_overlap=asm_overlap,
                           ipm_tol=ipm_tol, refine_tol=0.0, bound_tol=0.0)
        self._h = C.c_void_p()
        kp = Kunc.ctypes.data_as(C.c_void_p) if Kunc is not None else None
        _lib.check(lib.nnmpc_qp_create(C.byref(self._h), n, nu, n_aug,
                                       P.ctypes.data_as(C.c_void_p), tq.ctypes.data_as(C.c_void_p),
                                       kp, C.byref(opts)), "nnmpc_qp_create")
        self._lib = lib
        self.have_inverse = False
        if Hinv is not None:
            Hinv = np.ascontiguousarray(Hinv, dtype=np.float64)
            rc = lib.nnmpc_qp_set_inverse(self._h, Hinv.ctypes.data_as(C.c_void_p), Kunc.ctypes.data_as(C.c_void_p))
            if rc == _lib.EINVAL and meth == 0:
                # the fp64 inverse of an ill-conditioned P missed the library's |P Pinv - I| check: the active-set
                # pass cannot be certified with it, the PDIP path needs no inverse -- method "auto" goes on without
                import warnings
                warnings.warn("BatchedBoxQP: " + lib.nnmpc_last_error().decode(errors="replace") +
                              " -- continuing with the PDIP path only", RuntimeWarning)
            else:
                _lib.check(rc, "nnmpc_qp_set_inverse")
                self.have_inverse = True
        # far-field form of the full-width pass (include/nnmpc.h: nnmpc_qp_set_farfield): "auto" factors the far block
        # for a window the first time a call's full-width pass had to do without (one-time host setup like the inverse:
        # an fp64 SVD, ~1.5 s at the CDU size); a list of windows factors them now; None / False never
        # (kept for those factorisations: the leading half of the columns of P^-1 and Kunc -- a window beyond n / 2 cannot pay --,
        # 80 of the 160 MB at the CDU size; released by close())
        self._ff_wmax = (n // 2 // 128) * 128
        self._ff_src = (np.ascontiguousarray(Hinv[:, :self._ff_wmax]), Kunc) if (self.have_inverse and farfield and self._ff_wmax > 0) else None
        nb_lib = nb if nb else (128 if n > 1024 else 64)     # the library pads n to its tile size (nnmpc_qp_create)
        self._np = -(-n // nb_lib) * nb_lib
        self._ff_done = set()
        self.farfield_info = {}        # window -> dict(rank, tiles' K extents ...) of the factors handed to the library (0: not usable)
        if self._ff_src is not None and not isinstance(farfield, str):
            for W in farfield:
                self.prepare_farfield(int(W))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.nnmpc_qp_destroy(self._h)
            self._h = C.c_void_p()
        self._ff_src = None

    __del__ = close

    def set_inverse(self, Hinv, Kunc):
        """Replace the inverse (nnmpc_qp_set_inverse on a live handle).  The library drops every far-field factorisation -- they were
        verified against the previous inverse -- and queues their windows as missing again; the wrapper forgets which windows it
        factored and factors from the new pair.  Returns the library's code: 0, or EINVAL when the pair was refused, after which the
        handle has NO inverse and solves by the PDIP path until a later call is accepted."""
        Hinv = np.ascontiguousarray(Hinv, dtype=np.float64)
        Kunc = np.ascontiguousarray(Kunc, dtype=np.float64)
        if Hinv.shape != (self.n, self.n) or Kunc.shape != (self.n, self.n_aug):
            raise ValueError("Hinv must be (n, n), Kunc (n, n_aug)")
        rc = self._lib.nnmpc_qp_set_inverse(self._h, Hinv.ctypes.data_as(C.c_void_p), Kunc.ctypes.data_as(C.c_void_p))
        factoring = self._ff_src is not None
        self.have_inverse = rc == 0
        self._ff_done, self.farfield_info, self._ff_src = set(), {}, None
        if rc != _lib.EINVAL:
            _lib.check(rc, "nnmpc_qp_set_inverse")
            if factoring:
                self._ff_src = (np.ascontiguousarray(Hinv[:, :self._ff_wmax]), Kunc)
        return rc

    def prepare_farfield(self, W, rtol=1e-13):
        """Factor M = [Kunc[W:] | -Hinv[W:, 0:W]] = U [Vx | Vl] (truncated SVD: singular values above rtol times the
        largest; M has numerical rank ~Nx; basis rotated so that U is a staircase, see _staircase) and hand the factors to the
        library, which verifies them on the device.  Returns the rank, or 0 when W is not a window the full-width pass can use."""
        if self._ff_src is None or W in self._ff_done:
            return 0
        self._ff_done.add(W)
        self.farfield_info[W] = dict(rank=0, reason="window not on the 128-column grid")
        Hinv, Kunc = self._ff_src
        if W <= 0 or W % 128 or W >= self.n or self._np % 128 or W > self._ff_wmax:   # (the library's own gate is on the PADDED n)
            return 0
        import scipy.linalg as sla
        M = np.hstack((Kunc[W:], -Hinv[W:, :W]))
        U, s, Vt = sla.svd(M, full_matrices=False, lapack_driver="gesdd")
        r = max(1, int((s > rtol * s[0]).sum()))
        rp, nf, k = -(-r // 128) * 128, self.n - W, -(-self.n_aug // 32) * 32 + W
        self.farfield_info[W] = dict(rank=0, numerical_rank=r, sigma_ratio_at_rank=float(s[min(r, s.size - 1)] / s[0]),
                                     reason="the factored form would not pay: numerical rank too large")
        if rp * (k + nf) > 0.8 * k * nf:             # the factored form would not pay (the library refuses such factors too):
            return 0                                 # a generic Hessian's far block has full rank, the MPC structure makes it ~Nx
        Uf, G = _staircase(U[:, :r] * s[:r], rtol * s[0])
        r = G.shape[0]
        Vt = G @ Vt[:G.shape[1]]
        Vx, Vl = np.ascontiguousarray(Vt[:, :self.n_aug]), np.ascontiguousarray(Vt[:, self.n_aug:])
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = self._lib.nnmpc_qp_set_farfield(self._h, W, r, p(Uf), p(Vx), p(Vl))
        if rc == _lib.EINVAL:                        # refused (rank too large for the workspace, factors too inaccurate): dense form stays
            import warnings
            self.farfield_info[W] = dict(rank=0, numerical_rank=r, reason=self._lib.nnmpc_last_error().decode(errors="replace"))
            warnings.warn("BatchedBoxQP.prepare_farfield: " + self.farfield_info[W]["reason"], RuntimeWarning)
            return 0
        _lib.check(rc, "nnmpc_qp_set_farfield")
        kj = [int(np.flatnonzero(np.abs(Uf[j:j + 128]).max(axis=0) > 0).max(initial=-1)) + 1 for j in range(0, Uf.shape[0], 128)]
        self.farfield_info[W] = dict(rank=int(r), staircase_mean_k=float(np.mean(kj)), staircase_max_k=int(max(kj)))
        return r

    def prepare_farfield_windows(self, lo=128, hi=None):
        """Factor every window lo, lo + 128, ... <= hi (default: a quarter of the horizon) now -- one-time setup like the inverse,
        ~0.5 s of host SVD and ~10 MB of HBM per window at the CDU size -- so that no later call meets a window without factors
        (the window of a call follows its batch: the last active bound of any of its problems).  Returns {W: rank}."""
        hi = self.n // 4 if hi is None else hi
        return {W: self.prepare_farfield(W) for W in range(lo, hi + 1, 128)}

    def _farfield_auto(self):
        if self._ff_src is None:
            return
        for _ in range(32):                           # every window the call met without factors
            W = C.c_int32(0)
            _lib.check(self._lib.nnmpc_qp_farfield_missing(self._h, C.byref(W)), "nnmpc_qp_farfield_missing")
            if not W.value:
                break
            self.prepare_farfield(W.value)

    def solve_batch(self, x0, lb, ub, guess=None, first_move_only=False, multipliers=False):
        """numpy in / numpy out.  x0 (B, n_aug), lb/ub (B, nu) or (nu,); guess: optional (B, n) uint8
        active-set estimate (0 free, 1 upper, 2 lower) that replaces the PDIP phase (warm start).

        Returns dict(u (B, n) -- or (B, nu) with first_move_only, all the reference keeps of a solve in its
        simulation loops (lib/linearMPC.py:856) --, active (B, 2n) bool in the row order of the reference's G,
        status (B,), ipm_iters (B,), factorizations (B,)).  multipliers=True adds mult (B, n): the bound multipliers
        of the delivered u (include/nnmpc.h: nnmpc_qp_multipliers -- -(P u + q) at an upper bound, +(P u + q) at a lower
        one, +0.0 on free variables, NaN rows for problems that were not solved); not available with first_move_only.
        """
        if multipliers and first_move_only:
            raise ValueError("multipliers=True needs the whole sequence: not available with first_move_only=True")
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1, self.n_aug)
        B = x0.shape[0]
        lb = np.ascontiguousarray(np.broadcast_to(np.asarray(lb, np.float64).reshape(-1, self.nu), (B, self.nu)))
        ub = np.ascontiguousarray(np.broadcast_to(np.asarray(ub, np.float64).reshape(-1, self.nu), (B, self.nu)))
        u = np.empty((B, self.nu if first_move_only else self.n))
        act = np.zeros((B, self.words), np.uint32)
        status = np.empty(B, np.int32)
        iters = np.empty((B, 2), np.int32)
        gp = None
        if guess is not None:
            guess = np.ascontiguousarray(guess, dtype=np.uint8).reshape(B, self.n)
            gp = guess.ctypes.data_as(C.c_void_p)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        mult = np.empty((B, self.n)) if multipliers else None
        if multipliers:
            _lib.check(self._lib.nnmpc_qp_solve_batch_dual(
                self._h, B, p(x0), p(lb), p(ub), gp, p(u), p(act), p(status), p(iters), p(mult), _lib.HOST,
                _lib.OUT_SEQUENCE), "nnmpc_qp_solve_batch_dual")
        else:
            _lib.check(self._lib.nnmpc_qp_solve_batch_ex(
                self._h, B, p(x0), p(lb), p(ub), gp, p(u), p(act), p(status), p(iters), _lib.HOST,
                _lib.OUT_FIRST_MOVE if first_move_only else _lib.OUT_SEQUENCE), "nnmpc_qp_solve_batch_ex")
        self._farfield_auto()
        bits = np.unpackbits(act.view(np.uint8), axis=1, bitorder="little")[:, :2 * self.n].astype(bool)
        out = dict(u=u, active=bits, status=status, ipm_iters=iters[:, 0], factorizations=iters[:, 1])
        if multipliers:
            out["mult"] = mult
        return out

    def multipliers(self, x0, u, active_words, status=None):
        """The bound multipliers of ANY (x0, u, active) alone (nnmpc_qp_multipliers): a pure function of the handle's P and
        tq.  x0 (B, n_aug), u (B, n), active_words (B, ceil(2n/32)) uint32 as the C ABI packs them (active_to_words), status
        (B,) or None; numpy in, numpy out.  Returns mult (B, n).  (With a solve, on device buffers: solve_batch_device(mult=...).)"""
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1, self.n_aug)
        B = x0.shape[0]
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(B, self.n)
        act = np.ascontiguousarray(active_words, dtype=np.uint32).reshape(B, self.words)
        st = None if status is None else np.ascontiguousarray(status, dtype=np.int32).reshape(B)
        mult = np.empty((B, self.n))
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        _lib.check(self._lib.nnmpc_qp_multipliers(self._h, B, p(x0), p(u), p(act), p(st), p(mult), _lib.HOST),
                   "nnmpc_qp_multipliers")
        return mult

    def sensitivity(self, active_words, dx0, dlb=None, dub=None, status=None, first_move_only=False, multipliers=False):
        """Directional derivatives of u*(x0, lb, ub) restricted to the delivered active sets (nnmpc_qp_sensitivity, include/nnmpc.h).
        active_words (B, ceil(2n/32)) uint32 (active_to_words), dx0 (B, D, n_aug), dlb / dub (B, D, nu) or None (zeros), status (B,) or
        None; numpy in, numpy out.  dx0 (B, n_aug) is one direction (D = 1), and the outputs then drop that axis too.
        Returns dict(du (B, D, n) -- (B, D, nu) with first_move_only --, flag (B,) int32: 0 computed, 1 more than 768 bounds, 2 no
        answer, 3 non-positive pivot; NaN rows where flag != 0); multipliers=True adds dmult (B, D, n), the change of mult (not with
        first_move_only).  Needs the inverse (Kunc="auto" or set_inverse)."""
        if multipliers and first_move_only:
            raise ValueError("multipliers=True needs the whole sequence: not available with first_move_only=True")
        act = np.ascontiguousarray(active_words, dtype=np.uint32).reshape(-1, self.words)
        B = act.shape[0]
        dx0 = np.asarray(dx0, dtype=np.float64)
        one = dx0.ndim == 2
        dx0 = np.ascontiguousarray(dx0.reshape(B, -1, self.n_aug))
        D = dx0.shape[1]
        pert = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, np.float64).reshape(B, D, self.nu))
        dlb, dub = pert(dlb), pert(dub)
        st = None if status is None else np.ascontiguousarray(status, dtype=np.int32).reshape(B)
        du = np.empty((B, D, self.nu if first_move_only else self.n))
        dmult = np.empty((B, D, self.n)) if multipliers else None
        flag = np.empty(B, np.int32)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        _lib.check(self._lib.nnmpc_qp_sensitivity(self._h, B, D, p(act), p(st), p(dx0), p(dlb), p(dub), p(du), p(dmult), p(flag), _lib.HOST,
                                                  _lib.OUT_FIRST_MOVE if first_move_only else _lib.OUT_SEQUENCE), "nnmpc_qp_sensitivity")
        out = dict(du=du[:, 0] if one else du, flag=flag)
        if multipliers:
            out["dmult"] = dmult[:, 0] if one else dmult
        return out

    def adjoint(self, active_words, v, status=None, first_move_only=False, bounds=False, per_variable=False):
        """The adjoint (vector-Jacobian) product of the same map: J'v where sensitivity gives J d (nnmpc_qp_adjoint, include/nnmpc.h).
        active_words (B, ceil(2n/32)) uint32 (active_to_words), v (B, D, n) cotangents of the sequence -- (B, D, nu) of the first moves
        with first_move_only --, status (B,) or None; numpy in, numpy out.  v (B, n) is one cotangent (D = 1), and the outputs then drop
        that axis too.
        Returns dict(gx0 (B, D, n_aug), flag (B,) int32: 0 computed, 1 more than 768 bounds, 2 no answer, 3 non-positive pivot; NaN rows
        where flag != 0); bounds=True adds glb, gub (B, D, nu), the cotangents of the stage bounds; per_variable=True adds gbound
        (B, D, n), the cotangent of each variable's own bound (+0.0 on free variables).  For every direction of sensitivity:
        <v, du> = <gx0, dx0> + <glb, dlb> + <gub, dub>.  Needs the inverse (Kunc="auto" or set_inverse)."""
        act = np.ascontiguousarray(active_words, dtype=np.uint32).reshape(-1, self.words)
        B = act.shape[0]
        ncol = self.nu if first_move_only else self.n
        v = np.asarray(v, dtype=np.float64)
        one = v.ndim == 2
        v = np.ascontiguousarray(v.reshape(B, -1, ncol))
        D = v.shape[1]
        st = None if status is None else np.ascontiguousarray(status, dtype=np.int32).reshape(B)
        gx0 = np.empty((B, D, self.n_aug))
        glb = np.empty((B, D, self.nu)) if bounds else None
        gub = np.empty((B, D, self.nu)) if bounds else None
        gbound = np.empty((B, D, self.n)) if per_variable else None
        flag = np.empty(B, np.int32)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        _lib.check(self._lib.nnmpc_qp_adjoint(self._h, B, D, p(act), p(st), p(v), p(gx0), p(glb), p(gub), p(gbound), p(flag), _lib.HOST,
                                              _lib.OUT_FIRST_MOVE if first_move_only else _lib.OUT_SEQUENCE), "nnmpc_qp_adjoint")
        drop = (lambda a: a[:, 0]) if one else (lambda a: a)
        out = dict(gx0=drop(gx0), flag=flag)
        if bounds:
            out.update(glb=drop(glb), gub=drop(gub))
        if per_variable:
            out["gbound"] = drop(gbound)
        return out

    def first_move_gain(self, active_words, status=None, bounds=False):
        """The local feedback law of every problem's critical region: K (B, nu, n_aug) = du0/dx0 on the delivered active set, from ONE
        adjoint call with the nu unit cotangents of the first stage (forward mode needs n_aug directions).  bounds=True: returns
        (K, Klb, Kub, flag) with Klb, Kub (B, nu, nu) = du0/dlb, du0/dub and flag (B,) as adjoint's; NaN where flag != 0."""
        act = np.ascontiguousarray(active_words, dtype=np.uint32).reshape(-1, self.words)
        v = np.ascontiguousarray(np.broadcast_to(np.eye(self.nu), (act.shape[0], self.nu, self.nu)))
        out = self.adjoint(act, v, status=status, first_move_only=True, bounds=bounds)
        return (out["gx0"], out["glb"], out["gub"], out["flag"]) if bounds else out["gx0"]

    def mult_to_z(self, mult, active):
        """mult (B, n) per variable + active (B, 2n) bool -> z (B, 2n) in the row order of the reference's G: the
        variable's multiplier on its active row, zero on the others; a NaN row of mult stays a NaN row."""
        n, nu = self.n, self.nu
        k, c = np.arange(n) // nu, np.arange(n) % nu
        up, lo = k * 2 * nu + c, k * 2 * nu + nu + c
        z = np.zeros((mult.shape[0], 2 * n))
        z[:, up] = np.where(active[:, up], mult, 0.0)
        z[:, lo] = np.where(active[:, lo], mult, 0.0)
        z[np.isnan(mult).all(axis=1)] = np.nan
        return z

    def active_to_words(self, active):
        """(B, 2n) bool rows of G -> (B, ceil(2n/32)) uint32 words as the C ABI packs them (bit i = row i)."""
        a = np.zeros((active.shape[0], self.words * 32), np.uint8)
        a[:, :2 * self.n] = active
        return np.ascontiguousarray(np.packbits(a, axis=1, bitorder="little")).view(np.uint32)

    def active_to_state(self, active):
        """(B, 2n) bool rows of G -> (B, n) uint8 per-variable state (the `guess` format)."""
        n, nu = self.n, self.nu
        k, c = np.arange(n) // nu, np.arange(n) % nu
        return (active[:, k * 2 * nu + c].astype(np.uint8) + 2 * active[:, k * 2 * nu + nu + c].astype(np.uint8))

    def solve_batch_device(self, B, x0, lb, ub, u, active=None, status=None, iters=None, guess=None,
                           first_move_only=False, mult=None):
        """HBM-resident buffers (objects with data_ptr(): _lib.DeviceArray, torch CUDA tensors; f64/u32/i32/u8).
        u is (B, n), or (B, nu) with first_move_only.  mult: optional (B, n) f64 buffer for the bound multipliers
        (nnmpc_qp_solve_batch_dual; not with first_move_only)."""
        q = lambda a: (_ptr(a)[0] if a is not None else None)
        if mult is not None:
            if first_move_only:
                raise ValueError("mult needs the whole sequence: not available with first_move_only=True")
            _lib.check(self._lib.nnmpc_qp_solve_batch_dual(
                self._h, B, q(x0), q(lb), q(ub), q(guess), q(u), q(active), q(status), q(iters), q(mult), _lib.DEVICE,
                _lib.OUT_SEQUENCE), "nnmpc_qp_solve_batch_dual")
            self._farfield_auto()
            return
        _lib.check(self._lib.nnmpc_qp_solve_batch_ex(
            self._h, B, q(x0), q(lb), q(ub), q(guess), q(u), q(active), q(status), q(iters), _lib.DEVICE,
            _lib.OUT_FIRST_MOVE if first_move_only else _lib.OUT_SEQUENCE), "nnmpc_qp_solve_batch_ex")
        self._farfield_auto()

    def set_profiling(self, on=True):
        _lib.check(self._lib.nnmpc_qp_set_profiling(self._h, int(on)), "nnmpc_qp_set_profiling")

    def stats(self, reset=False):
        s = _lib.QpStats()
        _lib.check(self._lib.nnmpc_qp_get_stats(self._h, C.byref(s), int(reset)), "nnmpc_qp_get_stats")
        return {k: getattr(s, k) for k, _ in s._fields_}

    def debug_factor_solve(self, dvec, mask, rhs):
        """Kernel-level hook: solve (mask mask' o P + diag(dvec)) sol = rhs per row (f32)."""
        dvec = np.ascontiguousarray(dvec, np.float32)
        mask = np.ascontiguousarray(mask, np.float32)
        rhs = np.ascontiguousarray(rhs, np.float32)
        B = dvec.shape[0]
        sol = np.empty((B, self.n), np.float32)
        _lib.check(self._lib.nnmpc_qp_debug_factor_solve(
            self._h, B, *(a.ctypes.data_as(C.c_void_p) for a in (dvec, mask, rhs, sol))),
            "nnmpc_qp_debug_factor_solve")
        return sol

    def debug_predict(self, x0, lb, ub, iters=0, wide=0):
        """Kernel-level hook: the first-set predictor alone (csrc/qp_predict.h), through the launch code of a solve.
        iters: 0 adaptive, 1 .. 64 fixed; wide: 0 the 512-column window, 1 the 1024-column one, -1 chosen by the extent kernel.
        Returns dict(state (B, n) uint8 -- 0 free, 1 upper, 2 lower --, W, MR (problems per workgroup), count (the extent kernel's,
        -1 if it did not run), wide (the window chosen), L (that window's step constant))."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1, self.n_aug)
        B = x0.shape[0]
        lb = np.ascontiguousarray(np.broadcast_to(np.asarray(lb, np.float64).reshape(-1, self.nu), (B, self.nu)))
        ub = np.ascontiguousarray(np.broadcast_to(np.asarray(ub, np.float64).reshape(-1, self.nu), (B, self.nu)))
        state = np.full((B, self.n), 255, np.uint8)
        info = np.full(4, -9, np.int32)
        L = C.c_double(0.0)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(self._lib.nnmpc_qp_debug_predict(self._h, B, p(x0), p(lb), p(ub), int(iters), int(wide), p(state), p(info),
                                                    C.byref(L)), "nnmpc_qp_debug_predict")
        return dict(state=state, W=int(info[0]), MR=int(info[1]), count=int(info[2]), wide=int(info[3]), L=float(L.value))

    def debug_gemm(self, kind, M, N, K, A, B, C_, rowphase=None, want=0, kdyn=None, kblocks=False, mdyn=None, rowmap=None):
        """Kernel-level hook: one GEMM kernel of the active-set path alone, C = A B' (include/nnmpc.h: nnmpc_qp_debug_gemm), through the
        launch code of a solve.  kind: 0 the dispatch of the solves, 1 / 2 the 128 x 128 / 64 x 64 fp64 kernel, 3 / 4 the f32 k-range
        kernel with 128 / 64 tiles.  A, B, C_: 2-D arrays (float64, kinds 3 / 4 float32) whose rows are contiguous; views into wider
        arrays give the leading dimensions.  C_ goes up with its contents and is overwritten IN PLACE with what comes back.
        Returns dict(kernel, grid (workgroups), kper, tile)."""
        dt = np.float32 if kind in (3, 4) else np.float64
        for a in (A, B, C_):
            if a.dtype != dt or a.ndim != 2 or a.strides[1] != a.itemsize or a.strides[0] % a.itemsize:
                raise ValueError("debug_gemm: operands are 2-D arrays of the kind's type with contiguous rows")
        if not C_.flags.writeable:
            raise ValueError("debug_gemm: C is written in place")
        ld = lambda a: a.strides[0] // a.itemsize
        ints = lambda v, n=None: None if v is None else np.ascontiguousarray(np.asarray(v, np.int32).reshape(-1 if n is None else n))
        rowphase, kdyn, mdyn, rowmap = ints(rowphase), ints(kdyn), ints(mdyn, 1), ints(rowmap)
        T = 128 if kind in (1, 3) else 64
        nk = -(-M // T) * (T // 64) if (kblocks or kind in (3, 4)) else 1
        for v, need, what in ((rowphase, M, "rowphase"), (rowmap, M, "rowmap"), (kdyn, nk, "kdyn")):
            if v is not None and v.size < need:
                raise ValueError(f"debug_gemm: {what} has {v.size} entries, the kernel reads {need}")
        # (a leading dimension shorter than the row is the library's to refuse; a VIEW narrower than the row, or B shorter than N rows,
        # would have it read past the view)
        for a, cols, what in ((A, K, "A"), (B, K, "B"), (C_, N, "C")):
            if ld(a) >= cols and a.shape[1] < cols:
                raise ValueError(f"debug_gemm: {what} has {a.shape[1]} columns, the call names {cols}")
        if B.shape[0] < N:
            raise ValueError(f"debug_gemm: B has {B.shape[0]} rows, the call names {N}")
        info = np.full(4, -9, np.int32)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        _lib.check(self._lib.nnmpc_qp_debug_gemm(self._h, int(kind), int(M), int(N), int(K), p(A), ld(A), A.shape[0], p(B), ld(B),
                                                 p(C_), ld(C_), C_.shape[0], p(rowphase), int(want), p(kdyn), int(bool(kblocks)),
                                                 p(mdyn), p(rowmap), p(info)), "nnmpc_qp_debug_gemm")
        return dict(kernel=int(info[0]), grid=int(info[1]), kper=int(info[2]), tile=int(info[3]))

    def debug_factor_fail(self, B):
        """(B,) int32: 1 where the last debug_factor_solve met a non-positive pivot in that row's factorisation."""
        fail = np.empty(B, np.int32)
        _lib.check(self._lib.nnmpc_qp_debug_factor_fail(self._h, B, fail.ctypes.data_as(C.c_void_p)),
                   "nnmpc_qp_debug_factor_fail")
        return fail
