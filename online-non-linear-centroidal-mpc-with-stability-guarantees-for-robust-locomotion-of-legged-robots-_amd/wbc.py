"""Batched whole-body inverse-dynamics QP: the QP that the reference's
``InverseDynamics.get_joint_torques`` (code/inverse_dynamics.py:30-134) assembles and hands to ``QPSolver`` (CasADi conic
+ OSQP, code/utils.py:40-92) once per tick, for B robots at once on the GPU (csrc/wbc_qp.hip through the C ABI of
include/cmpc_wbc.h).  The Jacobians, the mass matrix and the Coriolis forces come from the caller's rigid-body library
(DART in the reference, :46-66, :107-111) as device tensors; nothing here imports the oracle, and there is no CPU
fallback.  ``solve`` takes the assembled task cost (Hq, Fq) and the flag-scaled Jc with one foot size and friction for the
launch; ``solve_tasks`` takes the task Jacobians themselves (``stack_tasks``) and forms the cost inside the kernel, with
every instance's own contact flags, foot size and friction."""
import ctypes

import torch

from . import capi

DOFS, BASE, CONTACT = 30, 6, 12
TASK_ROWS, NACC = 21, 51          # CMPC_WBC_TASK_ROWS, CMPC_WBC_NACC: the stacked task Jacobians; those rows + the 30 joints

# weights and gains of code/inverse_dynamics.py:41-44
TASKS = ('lfoot', 'rfoot', 'com', 'torso', 'base', 'joints')
WEIGHTS = {'lfoot': 1., 'rfoot': 1., 'com': 1., 'torso': 1., 'base': 1., 'joints': 1.e-1}
POS_GAINS = {'lfoot': 10., 'rfoot': 10., 'com': 5., 'torso': 10., 'base': 10., 'joints': 10.}
VEL_GAINS = {'lfoot': 5., 'rfoot': 5., 'com': 10., 'torso': 5., 'base': 3., 'joints': 5.}


def assemble_task_cost(J, Jdot, ff, pos_error, vel_error, qd):
    """Hq (B,30,30), Fq (B,30) of code/inverse_dynamics.py:92-103 from batched task Jacobians J[task] (B,r,30), their
    derivatives, feed-forward accelerations and errors (B,r), and the joint velocities qd (B,30).  Plain torch
    (device-memory plumbing: two batched GEMMs per task)."""
    Hq = Fq = None
    for task in TASKS:
        Jt = J[task]
        acc = ff[task] + VEL_GAINS[task] * vel_error[task] + POS_GAINS[task] * pos_error[task] \
            - torch.einsum('brn,bn->br', Jdot[task], qd)
        Ht = WEIGHTS[task] * Jt.transpose(1, 2) @ Jt
        Ft = -WEIGHTS[task] * torch.einsum('brn,br->bn', Jt, acc)
        Hq = Ht if Hq is None else Hq + Ht
        Fq = Ft if Fq is None else Fq + Ft
    return Hq.contiguous(), Fq.contiguous()


def stack_tasks(J, Jdot, ff, pos_error, vel_error):
    """The dict-of-tasks form of ``assemble_task_cost`` as the stacked tensors of ``solve_tasks``: J, Jdot (B,21,30) -- rows
    lfoot 6, rfoot 6, com 3, torso 3, base 3 (the joint task's Jacobian is the shared ``joint_selection``, its derivative
    zero, :52, :65) -- and ff, pos_error, vel_error (B,51): those 21 rows, then the 30 joints.  Jdot may be None."""
    rows = TASKS[:-1]
    Js = torch.cat([J[k] for k in rows], dim=1).contiguous()
    Jds = None if Jdot is None else torch.cat([Jdot[k] for k in rows], dim=1).contiguous()
    return (Js, Jds) + tuple(torch.cat([v[k] for k in TASKS], dim=1).contiguous() for v in (ff, pos_error, vel_error))


def make_gains(weights=None, pos_gains=None, vel_gains=None):
    """A ``cmpc_wbc_gains`` from dicts by task name; what is not given is the reference's literal (:42-44)."""
    g = capi.WbcGains()
    g.struct_size = ctypes.sizeof(capi.WbcGains)
    for field, given, default in (("weight", weights, WEIGHTS), ("pos_gain", pos_gains, POS_GAINS), ("vel_gain", vel_gains, VEL_GAINS)):
        for i, task in enumerate(TASKS):
            getattr(g, field)[i] = dict(default, **(given or {}))[task]
    return g


class BatchedInverseDynamicsQP:
    """``InverseDynamics`` of the reference for a batch: ``solve`` returns what ``get_joint_torques`` returns
    (``tau[6:]``, :134) for every instance, plus the accelerations and contact wrenches of the QP."""

    def __init__(self, foot_size=0.1, mu=0.5, device=None, tol=1e-9, max_iter=60):
        if not torch.cuda.is_available():
            raise RuntimeError("BatchedInverseDynamicsQP needs a ROCm GPU: there is no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.d, self.mu, self.tol, self.max_iter = foot_size / 2.0, mu, tol, max_iter
        self._lib = capi.load()

    def solve(self, Hq, Fq, M, h, Jc):
        """Hq (B,30,30), Fq (B,30), M (B,30,30), h (B,30), Jc (B,12,30: rows already scaled by the contact flags, :109),
        contiguous fp64 on this GPU -> (tau_actuated (B,24), qdd (B,30), f_c (B,12), status (B,), iters (B,))."""
        B = Hq.shape[0]
        for name, t, shape in (("Hq", Hq, (B, DOFS, DOFS)), ("Fq", Fq, (B, DOFS)), ("M", M, (B, DOFS, DOFS)),
                               ("h", h, (B, DOFS)), ("Jc", Jc, (B, CONTACT, DOFS))):
            if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shape
                    and t.device == self.device):
                raise ValueError(f"{name} must be a contiguous fp64 tensor of shape {shape} on {self.device}")
        tau = torch.empty((B, DOFS), dtype=torch.float64, device=self.device)
        qdd = torch.empty((B, DOFS), dtype=torch.float64, device=self.device)
        f = torch.empty((B, CONTACT), dtype=torch.float64, device=self.device)
        status = torch.empty(B, dtype=torch.int32, device=self.device)
        iters = torch.empty(B, dtype=torch.int32, device=self.device)
        if B == 0:
            return tau[:, BASE:], qdd, f, status, iters
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self._lib.cmpc_wbc_qp_solve_batch(self.device.index, B, Hq.data_ptr(), Fq.data_ptr(), M.data_ptr(), h.data_ptr(),
                                               Jc.data_ptr(), self.d, self.mu, self.tol, self.max_iter, tau.data_ptr(),
                                               qdd.data_ptr(), f.data_ptr(), status.data_ptr(), iters.data_ptr(),
                                               ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(self._lib.cmpc_wbc_last_error().decode())
        return tau[:, BASE:], qdd, f, status, iters

    def _per_instance(self, name, v, B):
        """A scalar or a (B,) tensor as a (B,) fp64 tensor on this GPU."""
        if not torch.is_tensor(v):
            return torch.full((B,), float(v), dtype=torch.float64, device=self.device)
        if not (v.is_cuda and v.dtype == torch.float64 and tuple(v.shape) == (B,) and v.device == self.device):
            raise ValueError(f"{name} must be a scalar or an fp64 tensor of shape ({B},) on {self.device}")
        return v

    def solve_tasks(self, J, Jdot, ff, pos_error, vel_error, qd, M, h, contact, mu=None, foot_size=None,
                    joint_selection=None, gains=None):
        """The same QP from the task form (code/inverse_dynamics.py:46-103; ``stack_tasks`` makes it from the dicts): J,
        Jdot (B,21,30), ff, pos_error, vel_error (B,51), qd (B,30), M (B,30,30), h (B,30), contact (B,2) = the left and
        right contact flags (they multiply the feet's Jacobian rows in Jc, :114), contiguous fp64 on this GPU.  Hq, Fq
        and Jc are formed inside the kernel.  Jdot = None: the caller folded -Jdot qd into ff (qd may be None then).
        mu, foot_size: scalars or (B,) tensors, every instance its own friction pyramid and foot (default: the object's);
        joint_selection (30,): the diagonal of :24-28, shared by the batch (default: every joint); gains: ``make_gains``
        (default: the reference's).  Returns what ``solve`` returns.  A row whose mu or foot size is not finite and > 0
        comes back with status 2, iters 0 and zeros -- checked on the device, the call does not synchronise."""
        B = J.shape[0]
        checks = [("J", J, (B, TASK_ROWS, DOFS)), ("ff", ff, (B, NACC)), ("pos_error", pos_error, (B, NACC)),
                  ("vel_error", vel_error, (B, NACC)), ("M", M, (B, DOFS, DOFS)), ("h", h, (B, DOFS)), ("contact", contact, (B, 2))]
        if Jdot is not None:
            checks += [("Jdot", Jdot, (B, TASK_ROWS, DOFS)), ("qd", qd, (B, DOFS))]
        if joint_selection is None:
            joint_selection = torch.ones(DOFS, dtype=torch.float64, device=self.device)
        checks.append(("joint_selection", joint_selection, (DOFS,)))
        for name, t, shape in checks:
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
                    and tuple(t.shape) == shape and t.device == self.device):
                raise ValueError(f"{name} must be a contiguous fp64 tensor of shape {shape} on {self.device}")
        d = self._per_instance("foot_size", 2.0 * self.d if foot_size is None else foot_size, B) / 2.0
        foot_mu = torch.stack([d, self._per_instance("mu", self.mu if mu is None else mu, B)], dim=1).contiguous()
        gains = make_gains() if gains is None else gains
        tau = torch.empty((B, DOFS), dtype=torch.float64, device=self.device)
        qdd = torch.empty((B, DOFS), dtype=torch.float64, device=self.device)
        f = torch.empty((B, CONTACT), dtype=torch.float64, device=self.device)
        status = torch.empty(B, dtype=torch.int32, device=self.device)
        iters = torch.empty(B, dtype=torch.int32, device=self.device)
        if B == 0:
            return tau[:, BASE:], qdd, f, status, iters
        stream = torch.cuda.current_stream(self.device).cuda_stream
        ptr = lambda t: None if t is None else t.data_ptr()
        rc = self._lib.cmpc_wbc_qp_solve_tasks(self.device.index, B, J.data_ptr(), ptr(Jdot), ff.data_ptr(), pos_error.data_ptr(),
                                               vel_error.data_ptr(), ptr(qd if Jdot is not None else None),
                                               joint_selection.data_ptr(), M.data_ptr(), h.data_ptr(), contact.data_ptr(),
                                               foot_mu.data_ptr(), ctypes.byref(gains), self.tol, self.max_iter,
                                               tau.data_ptr(), qdd.data_ptr(), f.data_ptr(), status.data_ptr(),
                                               iters.data_ptr(), ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(self._lib.cmpc_wbc_last_error().decode())
        return tau[:, BASE:], qdd, f, status, iters
