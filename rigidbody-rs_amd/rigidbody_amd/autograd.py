"""torch.autograd support for the fused rollout: `rollout(mb, q0, qd0, tau_seq, dt)` is
Multibody.rollout_batch as a differentiable function of (q0, qd0, tau_seq), its backward one
Multibody.rollout_vjp_batch launch (rigidbody_batch.h "reverse-mode gradient of the fused rollout").

    traj, qd_final = rollout(mb, q0, qd0, tau_seq, dt)      # [K, n, B], [n, B]
    cost = ((traj - target) ** 2).sum() + (qd_final ** 2).sum()
    cost.backward()                                          # q0.grad, qd0.grad, tau_seq.grad

traj[k] is q after step k.  The velocity after an intermediate step is not returned, but the
integrator is semi-implicit Euler, q_{k+1} = q_k + dt qd_{k+1}, so it is a difference of returned
positions and a cost on it is written in torch:

    qd_k1 = (traj[k + 1] - traj[k]) / dt                     # qd after step k + 1
    qd_1 = (traj[0] - q0) / dt                               # ... after the first step

Scope: the gradient's (serial revolute chains on the mass-matrix forward dynamics, up to 12 links).
For chains of 9 to 12 links the forward rollout integrates the articulated-body form and the
gradient differentiates the mass-matrix form: the same function to rounding.

`rollout_contact(mc, q0, qd0, tau_seq, dt)` is the same function of a handle that carries a contact
set: Multibody.rollout_contact_batch forward, one Multibody.rollout_contact_vjp_batch launch backward.

`rnea(mb, q, qd, qdd, fext=None)` is the inverse dynamics tau [n, B] as a differentiable function of
its tensor arguments, on every model (kinematic trees, prismatic joints, a floating base included):
one Multibody.rnea_batch / rnea_ext_batch launch forward, one Multibody.rnea_vjp_batch launch backward
(rigidbody_batch.h "reverse-mode gradient of the inverse dynamics").

    tau = rnea(mb, q, qd, qdd, fext)                         # [n, B]; fext [6 n, B] or None
    cost = (tau ** 2).sum()
    cost.backward()                                          # q.grad, qd.grad, qdd.grad, fext.grad

`fd(mb, q, qd, tau, fext=None)` is the forward dynamics qdd [n, B] in the same way, on every model: one
Multibody.fd_batch / fd_ext_batch launch forward, one Multibody.fd_vjp_batch launch backward
(rigidbody_batch.h "reverse-mode gradient of the forward dynamics").
"""
import torch


class _Rollout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mb, q0, qd0, tau_seq, dt, contact=False):
        q, qd = q0.detach().clone(), qd0.detach().clone()
        tau = tau_seq.detach().contiguous()
        traj = mb.rollout_contact_batch(q, qd, tau, dt) if contact else mb.rollout_batch(q, qd, tau, dt, traj=True)
        ctx.mb, ctx.dt, ctx.contact = mb, dt, contact
        ctx.save_for_backward(q0.detach(), qd0.detach(), tau)
        return traj, qd

    @staticmethod
    def backward(ctx, grad_traj, grad_qd_final):
        q0, qd0, tau = ctx.saved_tensors
        gq = torch.zeros_like(tau) if grad_traj is None else grad_traj.contiguous()
        gqd = torch.zeros_like(tau)
        if grad_qd_final is not None:
            gqd[-1] = grad_qd_final
        vjp = ctx.mb.rollout_contact_vjp_batch if ctx.contact else ctx.mb.rollout_vjp_batch
        g_q0, g_qd0, g_tau = vjp(q0.contiguous(), qd0.contiguous(), tau, ctx.dt, gq, gqd)
        return None, g_q0, g_qd0, g_tau, None, None


def rollout(mb, q0, qd0, tau_seq, dt):
    """K semi-implicit Euler steps of the forward dynamics from (q0, qd0) [n, B] under tau_seq
    [K, n, B] (CUDA tensors, fp32 or fp64; the inputs are not modified): returns (traj [K, n, B],
    the positions after every step, and qd_final [n, B]), differentiable with respect to q0, qd0 and
    tau_seq."""
    if tau_seq.shape[0] < 1:
        raise ValueError("rollout needs at least one step (tau_seq [K, n, B], K >= 1)")
    return _Rollout.apply(mb, q0, qd0, tau_seq, float(dt))


def rollout_contact(mb, q0, qd0, tau_seq, dt):
    """rollout on a handle that carries a contact set (Multibody.with_contacts): the forward is one
    Multibody.rollout_contact_batch launch, the backward one Multibody.rollout_contact_vjp_batch launch
    (rigidbody_batch.h "reverse-mode gradient of the fused contact rollout"); the same values returned."""
    if tau_seq.shape[0] < 1:
        raise ValueError("rollout_contact needs at least one step (tau_seq [K, n, B], K >= 1)")
    return _Rollout.apply(mb, q0, qd0, tau_seq, float(dt), True)


class _Rnea(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mb, q, qd, qdd, fext):
        ins = [t.detach().contiguous() for t in (q, qd, qdd)]
        f = None if fext is None else fext.detach().contiguous()
        tau = mb.rnea_batch(*ins) if f is None else mb.rnea_ext_batch(*ins, f)
        ctx.mb, ctx.ext = mb, f is not None
        ctx.save_for_backward(*ins, *([f] if f is not None else []))
        return tau

    @staticmethod
    def backward(ctx, grad_tau):
        saved = ctx.saved_tensors
        g = ctx.mb.rnea_vjp_batch(*saved[:3], grad_tau.contiguous(), fext=saved[3] if ctx.ext else None)
        g = list(g) + ([] if ctx.ext else [None])
        return (None, *[x if need else None for x, need in zip(g, ctx.needs_input_grad[1:])])


def rnea(mb, q, qd, qdd, fext=None):
    """tau = rnea_ext(q, qd, qdd, fext) [n, B] (fext=None: the plain RNEA) of CUDA tensors q, qd, qdd [n, B]
    and fext [6 n, B], fp32 or fp64 (the inputs are not modified), differentiable with respect to every
    tensor argument; an input without requires_grad gets None."""
    return _Rnea.apply(mb, q, qd, qdd, fext)


class _Fd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mb, q, qd, tau, fext):
        ins = [t.detach().contiguous() for t in (q, qd, tau)]
        f = None if fext is None else fext.detach().contiguous()
        qdd = mb.fd_batch(*ins) if f is None else mb.fd_ext_batch(*ins, f)
        ctx.mb, ctx.ext = mb, f is not None
        ctx.save_for_backward(*ins, *([f] if f is not None else []))
        return qdd

    @staticmethod
    def backward(ctx, grad_qdd):
        saved = ctx.saved_tensors
        g = ctx.mb.fd_vjp_batch(*saved[:3], grad_qdd.contiguous(), fext=saved[3] if ctx.ext else None)
        g = list(g[1:]) + ([] if ctx.ext else [None])  # (the launch's own qdd is not needed here)
        return (None, *[x if need else None for x, need in zip(g, ctx.needs_input_grad[1:])])


def fd(mb, q, qd, tau, fext=None):
    """qdd = fd_ext(q, qd, tau, fext) [n, B] (fext=None: the plain forward dynamics) of CUDA tensors q, qd, tau
    [n, B] and fext [6 n, B], fp32 or fp64 (the inputs are not modified), differentiable with respect to every
    tensor argument; an input without requires_grad gets None."""
    return _Fd.apply(mb, q, qd, tau, fext)
