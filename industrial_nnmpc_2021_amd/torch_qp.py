"""The regulator's first move as a differentiable torch function: u0 = MPC(x0, ulb, uub), backward through the adjoint product of the
QP solution on the delivered active set (DenseQPRegulator.adjoint_batch; include/nnmpc.h: nnmpc_qp_adjoint).

Not imported by the package: ``from industrial_nnmpc_2021_amd.torch_qp import first_move``.  Tensors of any device and dtype go in;
the solve and the adjoint run in the library from host numpy float64, and the results come back on the inputs' device and dtype (a
device-pointer path is not built).  The gradient is that of the affine law of the critical region each x0 lies in: exact wherever
the active set is locally constant.  A problem the adjoint flags (DenseQPRegulator.adjoint_batch: flag != 0 -- not solved, or a set
of more than 768 bounds) gets NaN gradients in its row, the other rows are not affected.
"""
import numpy as np
import torch


class _FirstMove(torch.autograd.Function):
    @staticmethod
    def forward(ctx, reg, x0, ulb, uub):
        host = lambda t: t.detach().to("cpu", torch.float64).numpy()
        B = x0.shape[0]
        lb = np.broadcast_to(host(ulb).reshape(-1, reg.Nu), (B, reg.Nu))
        ub = np.broadcast_to(host(uub).reshape(-1, reg.Nu), (B, reg.Nu))
        u0, info = reg.solve_batch(host(x0), lb, ub, first_move_only=True)
        ctx.reg = reg
        ctx.saved = dict(active=info["active"], status=info["status"])
        ctx.like = (x0, ulb, uub)
        return torch.from_numpy(np.ascontiguousarray(u0)).to(device=x0.device, dtype=x0.dtype)

    @staticmethod
    def backward(ctx, grad_u0):
        reg = ctx.reg
        g = reg.adjoint_batch(ctx.saved, grad_u0.detach().to("cpu", torch.float64).numpy(), first_move_only=True, bounds=True)
        x0, ulb, uub = ctx.like

        def back(a, like):
            if not like.requires_grad:
                return None
            t = torch.from_numpy(np.ascontiguousarray(a))
            if like.shape != t.shape:                        # bounds shared by the batch: (Nu,) or (Nu, 1) or (1, Nu)
                t = t.sum(dim=0).reshape(like.shape)
            return t.to(device=like.device, dtype=like.dtype)

        return None, back(g["gx0"], x0), back(g["glb"], ulb), back(g["gub"], uub)


def first_move(reg, x0, ulb=None, uub=None):
    """u0 (B, Nu) of ``reg`` (a DenseQPRegulator) at x0 (B, n_aug), differentiable in x0, ulb and uub ((B, Nu), or one row shared by the
    batch; default: the regulator's own bounds, as constants).  Forward: reg.solve_batch(..., first_move_only=True); backward:
    reg.adjoint_batch(..., first_move_only=True, bounds=True) on the saved active rows and status."""
    const = lambda a: torch.as_tensor(np.asarray(a, float).reshape(1, -1), dtype=x0.dtype, device=x0.device)
    ulb = const(reg.ulb) if ulb is None else ulb
    uub = const(reg.uub) if uub is None else uub
    return _FirstMove.apply(reg, x0, ulb, uub)
