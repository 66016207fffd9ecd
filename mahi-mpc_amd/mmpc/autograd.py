"""The batched solve as a differentiable torch operation (mmpc_solve_vjp_batch, mmpc_solve_jvp_batch).

``DifferentiableSolver(solver)`` wraps a ``mmpc.Solver``: calling it runs ``Solver.solve_batch`` on the current torch
stream, and ``.backward()`` through the returned V* runs one ``Solver.solve_vjp`` launch at the saved solution -- the
gradients with respect to x0, u_prev, traj and the weights for about the cost of one SQP iteration.  Control bounds
and the warm start get no gradient.  A solver with finite state bounds needs its sensitivity barrier switched on
(``Solver.set_sensitivity_barrier()``): the backward pass then runs the barrier recursion with the
control bounds it saved, and raises MmpcError -4 otherwise.  Forward-mode AD (``torch.autograd.forward_ad``,
``torch.func.jvp``) through the call runs one ``Solver.solve_jvp`` launch at the solution: the tangent of V* for the
tangents of x0, u_prev, traj and the weights.  This module imports torch; ``import mmpc`` does not import it.
"""
from __future__ import annotations

import torch

from . import JVP_FAILED, STATUS_CONVERGED, VJP_FAILED


def _stride(t, n):
    """row stride of a shared [n] or per-instance [B, n] tensor (0 = shared)"""
    return 0 if t.dim() == 1 else n


def _plain(t):
    """the tensor under torch.func's wrappers: its transforms hand jvp wrapped tensors, the library reads raw memory"""
    f = torch._C._functorch
    while t is not None and f.is_functorch_wrapped_tensor(t):
        t = f.get_unwrapped(t)
    return t


def _inputs(s, B, u_prev, traj, weights, u_lb, u_ub):
    """the detached, contiguous inputs a solve and its sensitivity calls read, and the stride of the bounds"""
    u_prev, traj, weights = (t.detach().contiguous() for t in (u_prev, traj, weights))
    u_lb = None if u_lb is None else u_lb.detach().contiguous()
    u_ub = None if u_ub is None else u_ub.detach().contiguous()
    bs = max((_stride(t, s.nu) for t in (u_lb, u_ub) if t is not None), default=0)
    if bs:   # one stride serves both bounds: a shared row beside a table is repeated
        u_lb = None if u_lb is None else u_lb.expand(B, s.nu).contiguous()
        u_ub = None if u_ub is None else u_ub.expand(B, s.nu).contiguous()
    return u_prev, traj, weights, u_lb, u_ub, bs


class _Solve(torch.autograd.Function):
    # forward and setup_context apart: the form torch.func's transforms need
    @staticmethod
    def forward(ds, x0, u_prev, traj, weights, u_lb, u_ub, V0):
        s = ds.solver
        B = x0.shape[0]
        x0 = x0.detach().contiguous()
        u_prev, traj, weights, u_lb, u_ub, bs = _inputs(s, B, u_prev, traj, weights, u_lb, u_ub)
        V = (torch.zeros((B, s.NV), dtype=torch.float64, device=x0.device) if V0 is None
             else V0.detach().to(torch.float64).reshape(B, s.NV).clone())
        status = torch.empty((B,), dtype=torch.int32, device=x0.device)
        iters = torch.empty((B,), dtype=torch.int32, device=x0.device)
        s.solve_batch(B, x0, u_prev, traj, weights, V, status=status, iters=iters,
                      weights_stride=_stride(weights, s.nx + 2 * s.nu), u_lb=u_lb, u_ub=u_ub, bounds_stride=bs,
                      stream=torch.cuda.current_stream(x0.device).cuda_stream)
        return V, status, iters

    @staticmethod
    def setup_context(ctx, inputs, output):
        ds, x0, u_prev, traj, weights, u_lb, u_ub, _V0 = inputs
        V, status, iters = output
        u_prev, traj, weights, u_lb, u_ub, bs = _inputs(ds.solver, x0.shape[0], u_prev, traj, weights, u_lb, u_ub)
        ctx.ds, ctx.bounds, ctx.bs = ds, (u_lb, u_ub), bs
        ctx.save_for_backward(V, u_prev, traj, weights, status)
        ctx.save_for_forward(V, u_prev, traj, weights, status)
        ctx.mark_non_differentiable(status, iters)

    @staticmethod
    def backward(ctx, V_bar, _status_bar, _iters_bar):
        ds = ctx.ds
        s = ds.solver
        V, u_prev, traj, weights, status = ctx.saved_tensors
        u_lb, u_ub = ctx.bounds
        B = V.shape[0]
        V_bar = torch.zeros_like(V) if V_bar is None else V_bar.to(torch.float64).contiguous()
        r = s.solve_vjp(B, V, u_prev, traj, weights, V_bar, weights_stride=_stride(weights, s.nx + 2 * s.nu),
                        u_lb=u_lb, u_ub=u_ub, bounds_stride=ctx.bs,
                        stream=torch.cuda.current_stream(V.device).cuda_stream)
        ds.last_vjp_status = r["vjp_status"]
        # an instance that did not converge has no solution map to differentiate; a failed VJP wrote zeros already
        keep = (status == STATUS_CONVERGED) & (r["vjp_status"] != VJP_FAILED)
        row = lambda t: torch.where(keep.reshape((B,) + (1,) * (t.dim() - 1)), t, torch.zeros_like(t))  # noqa: E731
        w_bar = row(r["weights_bar"])
        if weights.dim() == 1:
            w_bar = w_bar.sum(0)
        return None, row(r["x0_bar"]), row(r["u_prev_bar"]), row(r["traj_bar"]), w_bar, None, None, None

    @staticmethod
    def jvp(ctx, _ds, dx0, du_prev, dtraj, dweights, _dlb, _dub, _dV0):
        ds = ctx.ds
        s = ds.solver
        V, u_prev, traj, weights, status = (_plain(t) for t in ctx.saved_tensors)
        u_lb, u_ub = (_plain(t) for t in ctx.bounds)
        B = V.shape[0]
        tan = lambda t, shape: (None if t is None  # noqa: E731
                                else _plain(t.detach().to(torch.float64).expand(shape).contiguous()))
        dx0, du_prev, dtraj = tan(dx0, (B, s.nx)), tan(du_prev, (B, s.nu)), tan(dtraj, (B, s.N, s.nx))
        dweights = tan(dweights, (B, s.nx + 2 * s.nu))   # the tangent of shared weights is every row's
        if dx0 is None and du_prev is None and dtraj is None and dweights is None:   # bounds and warm start: no tangent
            return torch.zeros_like(V), None, None
        # the outputs are made here: under torch.func even a new tensor comes wrapped
        new = lambda n, dtype: _plain(torch.empty(n, dtype=dtype, device=V.device))  # noqa: E731
        r = s.solve_jvp(B, V, u_prev, traj, weights, dx0=dx0, du_prev=du_prev, dtraj=dtraj, dweights=dweights,
                        dV=new((B, s.NV), torch.float64), du0=new((B, s.nu), torch.float64),
                        jvp_status=new((B,), torch.int32),
                        workspace=new((max(s.solve_jvp_workspace_bytes(B), 8) // 8,), torch.float64),
                        weights_stride=_stride(weights, s.nx + 2 * s.nu), u_lb=u_lb, u_ub=u_ub, bounds_stride=ctx.bs,
                        stream=torch.cuda.current_stream(V.device).cuda_stream)
        ds.last_jvp_status = r["jvp_status"]
        # an instance that did not converge has no solution map to differentiate; a failed JVP wrote zeros already
        keep = (status == STATUS_CONVERGED) & (r["jvp_status"] != JVP_FAILED)
        return torch.where(keep.reshape(B, 1), r["dV"], torch.zeros_like(r["dV"])), None, None


class DifferentiableSolver:
    """``V, status, iters = ds(x0, u_prev, traj, weights, u_lb=None, u_ub=None, V0=None)`` on float64 device tensors:
    x0 [B, nx], u_prev [B, nu], traj [B, N, nx], weights [nx + 2 nu] (shared: its gradient is the sum over the batch)
    or [B, nx + 2 nu] (its gradient has the rows), u_lb / u_ub [nu] or [B, nu], V0 [B, NV] a warm start.  V [B, NV]
    carries the gradient; status and iters are not differentiable.  Instances whose solve did not converge, or whose
    vjp_status is 2, contribute zero rows.  ``last_vjp_status`` holds the vjp_status tensor of the last backward.  The
    VJP runs with HESSIAN_AUTO: the exact Hessian wherever the model has second derivatives, the true derivative.
    Under forward-mode AD V carries the tangent of one solve_jvp launch for the tangents of x0, u_prev, traj and the
    weights (a shared weights tangent [nx + 2 nu] is every row's); it is zero on instances that did not converge or
    whose jvp_status is 2, and ``last_jvp_status`` holds the jvp_status tensor of the last forward-mode call."""

    def __init__(self, solver):
        self.solver = solver
        self.last_vjp_status = None
        self.last_jvp_status = None

    def __call__(self, x0, u_prev, traj, weights, u_lb=None, u_ub=None, V0=None):
        return _Solve.apply(self, x0, u_prev, traj, weights, u_lb, u_ub, V0)
