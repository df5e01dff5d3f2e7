"""Batched solver front end: torch tensors in, torch tensors out, HIP kernels in between.

``BatchedCentroidalMPC`` owns one C-ABI handle (one GPU).  PyTorch is only the allocator
and stream provider; all arithmetic happens in libcmpc_amd.so.  It replaces the
reference's ``self.opt.solve()`` (code/centroidal_mpc_vertices.py:606) for B instances at once.
"""
import ctypes

import torch

from . import capi
from .problem import NCONST, NX, ProblemSpec, to_cspec

# per-instance outcome (include/cmpc.h): 3 = stopped short of `tol` with a KKT error within `acc_tol`
# (IPOPT's "Solved To Acceptable Level", which CasADi's Opti.solve() returns without raising)
STATUS_CONVERGED, STATUS_MAX_ITER, STATUS_INFEASIBLE, STATUS_ACCEPTABLE = 0, 1, 2, 3
STATUS_NUMERICAL = STATUS_INFEASIBLE


def usable(status):
    """Boolean mask of the instances whose solution a caller may use: converged or acceptable."""
    return (status == STATUS_CONVERGED) | (status == STATUS_ACCEPTABLE)


def _device_of(device):
    """torch.device with an explicit index ('cuda' -> the current device)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError("the solver runs on ROCm GPUs only (device must be a cuda device)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


class BatchedCentroidalMPC:
    def __init__(self, spec: ProblemSpec, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("BatchedCentroidalMPC needs a ROCm GPU: there is no CPU fallback")
        self.spec = spec
        self.device = _device_of(device)
        self._lib = capi.load()
        self._cspec = to_cspec(spec)
        h = ctypes.c_void_p()
        rc = self._lib.cmpc_create(ctypes.byref(self._cspec), self.device.index, ctypes.byref(h))
        if rc != 0:
            raise RuntimeError("cmpc_create failed: " + self._lib.cmpc_last_error(None).decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.cmpc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def workspace_bytes(self, B):
        return self._lib.cmpc_workspace_bytes(ctypes.byref(self._cspec), B)

    def solve(self, records, warm=None, out=None, state=None, state_out=None):
        """records (B, nrec) fp64 on this GPU -> (XU (B, nsol), status, iters, kkt), all on the GPU.

        Asynchronous on torch's current stream.  ``warm`` (B, nsol) is the previous solution
        (initial guess and proximal centre), the batched form of ``opt.set_initial``
        (code/centroidal_mpc_vertices.py:630-631).  Closed-loop ticks additionally hand the solver state over:
        ``state`` (B, nstate) = the previous tick's ``state_out`` (``new_state()`` for the first tick), and this
        tick's state is written to ``state_out`` (a different tensor): ``cmpc_solve_batch_state``.
        """
        return self._solve(records, warm, out, state, state_out, None)

    def solve_with_consts(self, records, consts, warm=None, out=None, state=None, state_out=None):
        """``solve`` with per-instance constants: ``consts`` (B, 18) fp64 on this GPU, one row per instance in the order
        of ``problem.CONST_FIELDS`` (``ProblemSpec.consts_row()``, ``problem.consts_rows(specs)``).  Instance b is solved
        with this handle's spec in which those eighteen fields are replaced by ``consts[b]``; N, nv, max_iter, tol,
        acc_tol and the kernel choice stay the handle's.  Rows that reproduce the handle's spec give bit for bit what
        ``solve`` gives.  A row the solver cannot use (non-finite; a length, g or delta <= 0; a negative weight, prox or
        relax) makes that instance -- and no other -- return status 2 with a NaN solution: checked on the GPU, no
        synchronisation (``cmpc_solve_batch_consts``, include/cmpc.h)."""
        if not isinstance(consts, torch.Tensor):
            raise ValueError(f"consts must be a contiguous fp64 CUDA tensor of shape (B, {NCONST})")
        return self._solve(records, warm, out, state, state_out, None, consts)

    def _solve(self, records, warm, out, state, state_out, gain, consts=None):
        sp = self.spec
        if not (records.is_cuda and records.dtype == torch.float64 and records.is_contiguous()):
            raise ValueError("records must be a contiguous fp64 CUDA tensor")
        if records.device != self.device:
            raise ValueError(f"records live on {records.device}, this handle on {self.device}")
        if records.dim() != 2 or records.shape[1] != sp.nrec:
            raise ValueError(f"records must have shape (B, {sp.nrec})")
        B = records.shape[0]
        if warm is not None:
            if not (warm.is_cuda and warm.dtype == torch.float64 and warm.is_contiguous()
                    and tuple(warm.shape) == (B, sp.nsol) and warm.device == self.device):
                raise ValueError(f"warm must be a contiguous fp64 CUDA tensor of shape (B, {sp.nsol})")
        if consts is not None:
            if not (consts.is_cuda and consts.dtype == torch.float64 and consts.is_contiguous()
                    and tuple(consts.shape) == (B, NCONST) and consts.device == self.device):
                raise ValueError(f"consts must be a contiguous fp64 CUDA tensor of shape (B, {NCONST}) on {self.device}")
        for name, t in (("state", state), ("state_out", state_out)):
            if t is not None and not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
                                      and tuple(t.shape) == (B, sp.nstate) and t.device == self.device):
                raise ValueError(f"{name} must be a contiguous fp64 CUDA tensor of shape (B, {sp.nstate})")
        if state is not None and state_out is not None:
            a, b, nb = state.data_ptr(), state_out.data_ptr(), B * sp.nstate * 8
            if a < b + nb and b < a + nb:                      # (views of one buffer included; the C entry point checks too)
                raise ValueError("state and state_out must not overlap")
        if out is None:
            out = torch.empty((B, sp.nsol), dtype=torch.float64, device=records.device)
        status = torch.empty(B, dtype=torch.int32, device=records.device)
        iters = torch.empty(B, dtype=torch.int32, device=records.device)
        kkt = torch.empty(B, dtype=torch.float64, device=records.device)
        if B == 0:
            return out, status, iters, kkt
        stream = torch.cuda.current_stream(records.device).cuda_stream
        args = (self._h, B, records.data_ptr(), warm.data_ptr() if warm is not None else None,
                state.data_ptr() if state is not None else None, out.data_ptr(),
                state_out.data_ptr() if state_out is not None else None,
                status.data_ptr(), iters.data_ptr(), kkt.data_ptr())
        if consts is not None and gain is not None:
            rc = self._lib.cmpc_solve_batch_gain_consts(*args[:3], consts.data_ptr(), *args[3:], gain.data_ptr(),
                                                        ctypes.c_void_p(stream))
        elif consts is not None:
            rc = self._lib.cmpc_solve_batch_consts(*args[:3], consts.data_ptr(), *args[3:], ctypes.c_void_p(stream))
        elif gain is None:
            rc = self._lib.cmpc_solve_batch_state(*args, ctypes.c_void_p(stream))
        else:
            rc = self._lib.cmpc_solve_batch_gain(*args, gain.data_ptr(), ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError("cmpc_solve_batch failed: " + self._lib.cmpc_last_error(self._h).decode())
        return out, status, iters, kkt

    def solve_with_gain(self, records, warm=None, out=None, state=None, state_out=None, gain=None, consts=None):
        """``solve`` plus the first-stage feedback gain: (XU, status, iters, kkt, G), G (B, 20 + nu, 20) on the GPU.
        With ``consts`` (B, 18), as ``solve_with_consts`` takes them, every instance is solved -- and its gain taken -- with
        its own row (``cmpc_solve_batch_gain_consts``); an instance whose row is refused has a gain of NaN.

        G[b] = d(x_1, u_0)/dx0 of instance b: rows X[:,1] (20) then U[:,0] (nu), one column per component of
        x0 = records[b, 0:20]; every other record entry and the proximal centre ``warm`` stay fixed.  XU, status,
        iters, kkt and ``state_out`` are bit for bit those of ``solve``.  Rows of NaN: no gain (status 1 / 2, or a KKT
        system at the returned point that needs an inertia correction) -- include/cmpc.h, INTEGRATION.md.
        ``cmpc_solve_batch_gain``; its first call on a handle synchronises the device (not under graph capture).
        """
        sp = self.spec
        if not (isinstance(records, torch.Tensor) and records.dim() == 2):
            raise ValueError(f"records must be a contiguous fp64 CUDA tensor of shape (B, {sp.nrec})")
        shape = (records.shape[0], NX + sp.nu, NX)
        if gain is None:
            if not records.is_cuda:
                raise ValueError("records must be a contiguous fp64 CUDA tensor")
            gain = torch.empty(shape, dtype=torch.float64, device=records.device)
        elif not (gain.is_cuda and gain.dtype == torch.float64 and gain.is_contiguous() and tuple(gain.shape) == shape
                  and gain.device == self.device):
            raise ValueError(f"gain must be a contiguous fp64 CUDA tensor of shape {shape}")
        if consts is not None and not isinstance(consts, torch.Tensor):
            raise ValueError(f"consts must be a contiguous fp64 CUDA tensor of shape (B, {NCONST})")
        out, status, iters, kkt = self._solve(records, warm, out, state, state_out, gain, consts)
        return out, status, iters, kkt, gain

    def track(self, records, XU, gain, x_meas, columns=0xFFF, x1_out=None, u0_out=None):
        """The gain applied between two solves, one launch that reads the gains once (``cmpc_gain_track``, include/cmpc.h):
        (x1, u0, used) with x1 (B, 20) = X[:,1] + G[:20] dx, u0 (B, nu) = U[:,0] + G[20:] dx and used (B,) bool, where
        dx = x_meas - x0 on the columns whose bit is set in ``columns`` (default: the centroidal state; INTEGRATION.md on why
        the foot columns are usually left out) and 0 elsewhere, x0 = records[:, 0:20].  An instance holds -- X[:,1], U[:,0]
        as they are, used False -- when any word of its gain, or a chosen word of x_meas or x0, is not finite.
        Asynchronous on torch's current stream, no allocation beyond the outputs."""
        sp, dev, f64 = self.spec, self.device, torch.float64

        def ok(x, dtype, shape):
            return (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == dtype and x.is_contiguous()
                    and tuple(x.shape) == shape and x.device == dev)
        if not (isinstance(records, torch.Tensor) and records.dim() == 2):
            raise ValueError(f"records must be a contiguous fp64 CUDA tensor of shape (B, {sp.nrec})")
        B = records.shape[0]
        if not (ok(records, f64, (B, sp.nrec)) and ok(XU, f64, (B, sp.nsol)) and ok(gain, f64, (B, NX + sp.nu, NX))
                and ok(x_meas, f64, (B, NX))):
            raise ValueError(f"track: records (B, {sp.nrec}), XU (B, {sp.nsol}), gain (B, {NX + sp.nu}, {NX}) and x_meas "
                             f"(B, {NX}) must be contiguous fp64 tensors on {dev}")
        columns = int(columns)
        if columns < 0 or columns >> NX:
            raise ValueError(f"columns must name bits 0..{NX - 1} only")
        if x1_out is None:
            x1_out = torch.empty((B, NX), dtype=f64, device=dev)
        if u0_out is None:
            u0_out = torch.empty((B, sp.nu), dtype=f64, device=dev)
        if not (ok(x1_out, f64, (B, NX)) and ok(u0_out, f64, (B, sp.nu))):
            raise ValueError(f"track: x1_out (B, {NX}) and u0_out (B, {sp.nu}) must be contiguous fp64 tensors on {dev}")
        used = torch.empty(B, dtype=torch.bool, device=dev)
        if B == 0:
            return x1_out, u0_out, used
        with torch.cuda.device(dev):                           # (the entry point takes no handle: the current device's)
            stream = torch.cuda.current_stream(dev).cuda_stream
            rc = self._lib.cmpc_gain_track(sp.N, sp.nv, B, records.data_ptr(), XU.data_ptr(), gain.data_ptr(), x_meas.data_ptr(),
                                           columns, x1_out.data_ptr(), u0_out.data_ptr(), used.data_ptr(), ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError("cmpc_gain_track failed: " + self._lib.cmpc_last_error(None).decode())
        return x1_out, u0_out, used

    def new_state(self, B):
        """An empty solver state for B instances (barrier word 0 = "no state": the first tick starts cold)."""
        return torch.zeros((B, self.spec.nstate), dtype=torch.float64, device=self.device)

    def last_kernel_name(self):
        """Name of the solver kernel the last solve launched, as the library reports it (cmpc_last_kernel_name)."""
        return self._lib.cmpc_last_kernel_name(self._h).decode()

    def last_kernel_ms(self):
        """Duration of the last solve's kernel (HIP events on the launch stream); synchronises."""
        ms = ctypes.c_float()
        rc = self._lib.cmpc_last_kernel_ms(self._h, ctypes.byref(ms))
        if rc != 0:
            raise RuntimeError(self._lib.cmpc_last_error(self._h).decode())
        return ms.value


class DeviceRecordBuilder:
    """Device-side front half of ``centroidal_mpc.solve`` (code/centroidal_mpc_vertices.py:482-600): the
    per-tick tables of a ``workloads.Scene`` are uploaded once, then records for a whole batch are
    gathered on the GPU (``cmpc_build_records``) - no host loop, no host-to-device copy per tick.
    With a ``workloads.SceneSet`` the tables of all its walks are uploaded and every instance names its own by
    ``scene_id`` (``cmpc_build_records_scenes``)."""

    def __init__(self, scene, device=None):
        import numpy as np
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceRecordBuilder needs a ROCm GPU: there is no CPU fallback")
        self.device = _device_of(device)
        self._lib = capi.load()
        self.S = getattr(scene, "S", None)     # a workloads.SceneSet has S scenes; None: one Scene, today's entry points
        if self.S is not None:
            self._init_set(scene)
            return
        T = scene.T
        arrs = [np.ascontiguousarray(a[:T], dtype=np.float64) for a in
                (scene.com_tab, scene.pose_l, scene.pose_r, scene.gl_tab, scene.gr_tab, scene.cur_l, scene.cur_r)]
        h = ctypes.c_void_p()
        rc = self._lib.cmpc_tables_create(self.device.index, T, *[a.ctypes.data_as(ctypes.c_void_p) for a in arrs],
                                          ctypes.byref(h))
        if rc != 0:
            raise RuntimeError("cmpc_tables_create failed: " + self._lib.cmpc_last_error(None).decode())
        self._h, self.T = h, T
        self.n_steps = int(scene.plan_pos.shape[0])
        sl, sr = (np.ascontiguousarray(a[:T], dtype=np.int32) for a in (scene.slot_l, scene.slot_r))
        rc = self._lib.cmpc_tables_set_plan_slots(self._h, self.n_steps, sl.ctypes.data_as(ctypes.c_void_p),
                                                  sr.ctypes.data_as(ctypes.c_void_p))
        if rc != 0:
            raise RuntimeError("cmpc_tables_set_plan_slots failed: " + self._lib.cmpc_last_error(None).decode())

    def _init_set(self, sset):
        import numpy as np
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        T = np.ascontiguousarray(sset.T, dtype=np.int32)
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in
                (sset.com_tab, sset.pose_l, sset.pose_r, sset.gl_tab, sset.gr_tab, sset.cur_l, sset.cur_r)]
        sl, sr = (np.ascontiguousarray(a, dtype=np.int32) for a in (sset.slot_l, sset.slot_r))
        h = ctypes.c_void_p()
        rc = self._lib.cmpc_scenes_create(self.device.index, sset.S, sset.T_max, p(T), *[p(a) for a in arrs],
                                          sset.n_steps_max, p(sl), p(sr), ctypes.byref(h))
        if rc != 0:
            raise RuntimeError("cmpc_scenes_create failed: " + self._lib.cmpc_last_error(None).decode())
        self._h, self.T, self.n_steps = h, T.copy(), int(sset.n_steps_max)

    def set_schedule(self, sset, N, rate=1):
        """Upload ``sset.schedule(N, rate)``, the write-back tables ``advance`` reads (``cmpc_scenes_set_schedule``)."""
        import numpy as np
        cond, is_ds, wb_slot, wb_row = sset.schedule(N, rate)
        arrs = [np.ascontiguousarray(cond, dtype=np.uint8), np.ascontiguousarray(is_ds, dtype=np.uint8),
                np.ascontiguousarray(wb_slot, dtype=np.int32), np.ascontiguousarray(wb_row, dtype=np.int32)]
        rc = self._lib.cmpc_scenes_set_schedule(self._h, N, rate, *[a.ctypes.data_as(ctypes.c_void_p) for a in arrs])
        if rc != 0:
            raise RuntimeError("cmpc_scenes_set_schedule failed: " + self._lib.cmpc_last_error(None).decode())

    def _check_scene_id(self, scene_id, B):
        if self.S is None:
            raise ValueError("scene_id goes with a SceneSet: this builder holds one Scene")
        if not (isinstance(scene_id, torch.Tensor) and scene_id.is_cuda and scene_id.dtype == torch.int32
                and scene_id.is_contiguous() and tuple(scene_id.shape) == (B,) and scene_id.device == self.device):
            raise ValueError(f"scene_id must be a contiguous int32 CUDA tensor of shape (B,) on {self.device}")

    def advance(self, spec, rate, scene_id, XU, status, t, state, alive, warm, flag=None, counter=None, plan_pos=None,
                hw_next=None, push_dv=None, update_contact=True, copy_all_warm=False):
        """Back half of a closed-loop tick in one launch (``cmpc_rollout_advance``, include/cmpc.h): t, state, alive, flag,
        counter, plan_pos and warm are updated in place from the solve's XU and status; flag, counter and plan_pos go with
        update_contact and are left alone (and may be None) without it.  Scene sets only."""
        B = t.shape[0]
        self._check_scene_id(scene_id, B)
        f64, dev = torch.float64, self.device

        def ok(x, dtype, shape):
            return x.is_cuda and x.dtype == dtype and x.is_contiguous() and tuple(x.shape) == shape and x.device == dev
        if not (ok(XU, f64, (B, spec.nsol)) and ok(warm, f64, (B, spec.nsol)) and ok(status, torch.int32, (B,))
                and ok(t, torch.int32, (B,)) and ok(state, f64, (B, 16)) and ok(alive, torch.bool, (B,))):
            raise ValueError(f"advance: every buffer must be a contiguous tensor of its documented shape and type on {dev}")
        if update_contact and not (ok(flag, torch.bool, (B,)) and ok(counter, torch.bool, (B,))
                                   and ok(plan_pos, f64, (B, self.n_steps, 3))):
            raise ValueError(f"advance: flag, counter (B,) bool and plan_pos (B, {self.n_steps}, 3) fp64 go with update_contact")
        if not update_contact:                                   # the kernel touches none of the three
            flag = counter = plan_pos = None
        for x in (hw_next, push_dv):
            if x is not None and not ok(x, f64, (B, 3)):
                raise ValueError("advance: hw_next / push_dv must be contiguous fp64 CUDA tensors of shape (B, 3)")
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = self._lib.cmpc_rollout_advance(self._h, spec.N, spec.nv, rate, B, scene_id.data_ptr(), XU.data_ptr(), status.data_ptr(),
                                            hw_next.data_ptr() if hw_next is not None else None,
                                            push_dv.data_ptr() if push_dv is not None else None,
                                            int(bool(update_contact)), int(bool(copy_all_warm)), t.data_ptr(), state.data_ptr(),
                                            alive.data_ptr(), *[x.data_ptr() if x is not None else None for x in (flag, counter, plan_pos)],
                                            warm.data_ptr(), ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError("cmpc_rollout_advance failed: " + self._lib.cmpc_last_error(None).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.cmpc_tables_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def build(self, spec, t, state, rate=1, out=None, plan_pos=None, scene_id=None):
        """t (B,) int32 and state (B, 16) fp64 on the GPU -> records (B, nrec) on the GPU.  plan_pos
        (B, n_steps, 3): per-instance contact plans (the x0 foot positions of :493-509 come from them).
        scene_id (B,) int32 on the GPU: the walk of every instance -- required with a ``SceneSet`` (n_steps is then
        its n_steps_max), refused with one ``Scene``.  A scene index or tick outside its range gives a NaN record."""
        if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
            raise ValueError("t must be a contiguous int32 CUDA tensor")
        if t.device != self.device or state.device != self.device:
            raise ValueError(f"t / state must live on {self.device}")
        B = t.shape[0]
        if not (state.is_cuda and state.dtype == torch.float64 and state.is_contiguous()
                and tuple(state.shape) == (B, 16)):
            raise ValueError("state must be a contiguous fp64 CUDA tensor of shape (B, 16)")
        if out is None:
            out = torch.empty((B, spec.nrec), dtype=torch.float64, device=t.device)
        if plan_pos is not None and not (plan_pos.is_cuda and plan_pos.dtype == torch.float64 and plan_pos.is_contiguous()
                                         and tuple(plan_pos.shape) == (B, self.n_steps, 3) and plan_pos.device == self.device):
            raise ValueError(f"plan_pos must be a contiguous fp64 tensor of shape (B, {self.n_steps}, 3) on {self.device}")
        stream = torch.cuda.current_stream(t.device).cuda_stream
        if self.S is not None or scene_id is not None:
            if scene_id is None:
                raise ValueError("this builder holds a SceneSet: build() needs scene_id")
            self._check_scene_id(scene_id, B)
            rc = self._lib.cmpc_build_records_scenes(self._h, spec.N, rate, B, t.data_ptr(), scene_id.data_ptr(), state.data_ptr(),
                                                     plan_pos.data_ptr() if plan_pos is not None else None,
                                                     out.data_ptr(), ctypes.c_void_p(stream))
            if rc != 0:
                raise RuntimeError("cmpc_build_records_scenes failed: " + self._lib.cmpc_last_error(None).decode())
            return out
        rc = self._lib.cmpc_build_records_planned(self._h, spec.N, rate, B, t.data_ptr(), state.data_ptr(),
                                                  plan_pos.data_ptr() if plan_pos is not None else None,
                                                  out.data_ptr(), ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError("cmpc_build_records failed: " + self._lib.cmpc_last_error(None).decode())
        return out
