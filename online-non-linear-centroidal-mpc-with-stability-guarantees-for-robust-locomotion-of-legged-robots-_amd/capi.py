"""ctypes binding of the C ABI in include/cmpc.h (libcmpc_amd.so, built by build.py).

There is no CPU fallback: if the HIP library is missing or fails to load, ``load()``
raises, and so does every solver entry point.
"""
import ctypes
import os

from .problem import CSpec

_HERE = os.path.dirname(os.path.abspath(__file__))
# CMPC_LIB_PATH: developer knob for A/B measurements of two builds of the HIP library in one GPU session
# (tools/ab_bench.sh); there is still no fallback of any kind
LIB_PATH = os.environ.get("CMPC_LIB_PATH") or os.path.join(_HERE, "libcmpc_amd.so")

#: every symbol include/cmpc.h declares
SYMBOLS = ("cmpc_default_spec", "cmpc_create", "cmpc_destroy", "cmpc_workspace_bytes",
           "cmpc_solve_batch", "cmpc_solve_batch_state", "cmpc_solve_batch_gain", "cmpc_solve_batch_consts", "cmpc_spec_consts",
           "cmpc_solve_batch_gain_consts", "cmpc_gain_track",
           "cmpc_last_kernel_ms", "cmpc_last_kernel_name", "cmpc_last_error",
           "cmpc_version",
           "cmpc_tables_create", "cmpc_tables_destroy", "cmpc_build_records",
           "cmpc_tables_set_plan_slots", "cmpc_build_records_planned",
           "cmpc_scenes_create", "cmpc_build_records_scenes", "cmpc_scenes_set_schedule", "cmpc_rollout_advance")
#: every symbol include/cmpc_wbc.h declares (batched whole-body QP, same library)
WBC_SYMBOLS = ("cmpc_wbc_qp_solve_batch", "cmpc_wbc_qp_solve_tasks", "cmpc_wbc_default_gains", "cmpc_wbc_last_error")
#: every symbol include/cmpc_rbd.h declares (batched rigid-body model, same library)
RBD_SYMBOLS = ("cmpc_rbd_model_create", "cmpc_rbd_model_destroy", "cmpc_rbd_eval", "cmpc_rbd_eval_inertial", "cmpc_rbd_last_error")

#: every symbol include/cmpc_walk.h declares (task references and state integrator of the walking loop, same library)
WALK_SYMBOLS = ("cmpc_walk_gait_create", "cmpc_walk_gait_destroy", "cmpc_walk_task_refs", "cmpc_walk_integrate",
                "cmpc_walk_measure", "cmpc_walk_plant_step", "cmpc_walk_plant_default_params", "cmpc_walk_last_error")


class WbcGains(ctypes.Structure):
    """``cmpc_wbc_gains`` of include/cmpc_wbc.h; task order lfoot, rfoot, com, torso, base, joints."""
    _fields_ = [("struct_size", ctypes.c_int32), ("reserved", ctypes.c_int32), ("weight", ctypes.c_double * 6),
                ("pos_gain", ctypes.c_double * 6), ("vel_gain", ctypes.c_double * 6)]


class PlantParams(ctypes.Structure):
    """``cmpc_walk_plant_params`` of include/cmpc_walk.h."""
    _fields_ = [("struct_size", ctypes.c_int32), ("sweeps", ctypes.c_int32), ("dt", ctypes.c_double), ("ground_z", ctypes.c_double),
                ("erp", ctypes.c_double), ("cfm", ctypes.c_double)]


_lib = None


def load():
    """Load libcmpc_amd.so (raises OSError with a build hint when it is absent)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError(f"{LIB_PATH} not found: build the HIP extension first "
                      f"(python -c 'import __graft_entry__ as g; g.build()')")
    lib = ctypes.CDLL(LIB_PATH)
    c_spec_p = ctypes.POINTER(CSpec)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.cmpc_default_spec.argtypes = [c_spec_p, i32, i32]
    lib.cmpc_default_spec.restype = None
    lib.cmpc_create.argtypes = [c_spec_p, ctypes.c_int, ctypes.POINTER(vp)]
    lib.cmpc_create.restype = ctypes.c_int
    lib.cmpc_destroy.argtypes = [vp]
    lib.cmpc_destroy.restype = ctypes.c_int
    lib.cmpc_workspace_bytes.argtypes = [c_spec_p, i32]
    lib.cmpc_workspace_bytes.restype = ctypes.c_size_t
    lib.cmpc_solve_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.cmpc_solve_batch.restype = ctypes.c_int
    lib.cmpc_solve_batch_state.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.cmpc_solve_batch_state.restype = ctypes.c_int
    lib.cmpc_solve_batch_gain.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.cmpc_solve_batch_gain.restype = ctypes.c_int
    lib.cmpc_solve_batch_consts.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.cmpc_solve_batch_consts.restype = ctypes.c_int
    lib.cmpc_solve_batch_gain_consts.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.cmpc_solve_batch_gain_consts.restype = ctypes.c_int
    lib.cmpc_gain_track.argtypes = [i32, i32, i32, vp, vp, vp, vp, ctypes.c_uint32, vp, vp, vp, vp]
    lib.cmpc_gain_track.restype = ctypes.c_int
    lib.cmpc_spec_consts.argtypes = [c_spec_p, ctypes.POINTER(ctypes.c_double)]
    lib.cmpc_spec_consts.restype = None
    lib.cmpc_last_kernel_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    lib.cmpc_last_kernel_ms.restype = ctypes.c_int
    lib.cmpc_last_kernel_name.argtypes = [vp]
    lib.cmpc_last_kernel_name.restype = ctypes.c_char_p
    lib.cmpc_last_error.argtypes = [vp]
    lib.cmpc_last_error.restype = ctypes.c_char_p
    lib.cmpc_tables_create.argtypes = [ctypes.c_int, i32] + [vp] * 7 + [ctypes.POINTER(vp)]
    lib.cmpc_tables_create.restype = ctypes.c_int
    lib.cmpc_tables_destroy.argtypes = [vp]
    lib.cmpc_tables_destroy.restype = ctypes.c_int
    lib.cmpc_build_records.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp]
    lib.cmpc_build_records.restype = ctypes.c_int
    lib.cmpc_tables_set_plan_slots.argtypes = [vp, i32, vp, vp]
    lib.cmpc_tables_set_plan_slots.restype = ctypes.c_int
    lib.cmpc_build_records_planned.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.cmpc_build_records_planned.restype = ctypes.c_int
    lib.cmpc_scenes_create.argtypes = [ctypes.c_int, i32, i32, vp] + [vp] * 7 + [i32, vp, vp, ctypes.POINTER(vp)]
    lib.cmpc_scenes_create.restype = ctypes.c_int
    lib.cmpc_build_records_scenes.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.cmpc_build_records_scenes.restype = ctypes.c_int
    lib.cmpc_scenes_set_schedule.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    lib.cmpc_scenes_set_schedule.restype = ctypes.c_int
    lib.cmpc_rollout_advance.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.cmpc_rollout_advance.restype = ctypes.c_int
    f64 = ctypes.c_double
    lib.cmpc_wbc_qp_solve_batch.argtypes = [ctypes.c_int, i32, vp, vp, vp, vp, vp, f64, f64, f64, i32, vp, vp, vp, vp, vp, vp]
    lib.cmpc_wbc_qp_solve_batch.restype = ctypes.c_int
    lib.cmpc_wbc_qp_solve_tasks.argtypes = [ctypes.c_int, i32] + [vp] * 11 + [ctypes.POINTER(WbcGains), f64, i32] + [vp] * 6
    lib.cmpc_wbc_qp_solve_tasks.restype = ctypes.c_int
    lib.cmpc_wbc_default_gains.argtypes = [ctypes.POINTER(WbcGains)]
    lib.cmpc_wbc_default_gains.restype = None
    lib.cmpc_wbc_last_error.argtypes = []
    lib.cmpc_wbc_last_error.restype = ctypes.c_char_p
    lib.cmpc_rbd_model_create.argtypes = [ctypes.c_int] + [vp] * 10 + [ctypes.POINTER(vp)]
    lib.cmpc_rbd_model_create.restype = ctypes.c_int
    lib.cmpc_rbd_model_destroy.argtypes = [vp]
    lib.cmpc_rbd_model_destroy.restype = ctypes.c_int
    lib.cmpc_rbd_eval.argtypes = [vp, i32, vp, vp, f64] + [vp] * 8
    lib.cmpc_rbd_eval.restype = ctypes.c_int
    lib.cmpc_rbd_eval_inertial.argtypes = [vp, i32, vp, vp, vp, f64] + [vp] * 8
    lib.cmpc_rbd_eval_inertial.restype = ctypes.c_int
    lib.cmpc_rbd_last_error.argtypes = []
    lib.cmpc_rbd_last_error.restype = ctypes.c_char_p
    lib.cmpc_walk_gait_create.argtypes = [ctypes.c_int, i32, i32, i32] + [vp] * 8 + [f64, f64, ctypes.POINTER(vp)]
    lib.cmpc_walk_gait_create.restype = ctypes.c_int
    lib.cmpc_walk_gait_destroy.argtypes = [vp]
    lib.cmpc_walk_gait_destroy.restype = ctypes.c_int
    lib.cmpc_walk_task_refs.argtypes = [vp, i32] + [vp] * 15
    lib.cmpc_walk_task_refs.restype = ctypes.c_int
    lib.cmpc_walk_integrate.argtypes = [ctypes.c_int, i32, vp, vp, vp, f64, vp, vp, vp, vp]
    lib.cmpc_walk_integrate.restype = ctypes.c_int
    lib.cmpc_walk_measure.argtypes = [ctypes.c_int, i32, vp, vp, f64, f64, vp, vp, vp, vp, vp]
    lib.cmpc_walk_measure.restype = ctypes.c_int
    lib.cmpc_walk_plant_step.argtypes = [ctypes.c_int, i32] + [vp] * 7 + [i32, vp, vp, vp, ctypes.POINTER(PlantParams)] + [vp] * 6
    lib.cmpc_walk_plant_step.restype = ctypes.c_int
    lib.cmpc_walk_plant_default_params.argtypes = [ctypes.POINTER(PlantParams)]
    lib.cmpc_walk_plant_default_params.restype = None
    lib.cmpc_walk_last_error.argtypes = []
    lib.cmpc_walk_last_error.restype = ctypes.c_char_p
    lib.cmpc_version.argtypes = []
    lib.cmpc_version.restype = ctypes.c_char_p
    _lib = lib
    return lib
