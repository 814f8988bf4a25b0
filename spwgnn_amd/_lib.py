"""ctypes binding of libspwgnn_hip.so (the C-ABI in include/spwgnn.h).

The product path has no fallback: if the library is missing or cannot be loaded, every entry
point raises. Device pointers are passed as plain integers (torch ``data_ptr()``).
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import Optional

_LIB_PATH = Path(__file__).resolve().parent / "libspwgnn_hip.so"
_lib: Optional[C.CDLL] = None


class SpwgnnError(RuntimeError):
    pass


class ParamInfo(C.Structure):
    _fields_ = [("name", C.c_char_p), ("offset", C.c_int64), ("rows", C.c_int32), ("cols", C.c_int32)]


class PlanSizes(C.Structure):
    _fields_ = [("n_wtiles", C.c_int32), ("n_eblocks", C.c_int32), ("nw_max", C.c_int32)]


class BatchC(C.Structure):
    _fields_ = [
        ("n_towers", C.c_int32), ("n_nodes", C.c_int32), ("n_wtiles", C.c_int32), ("n_eblocks", C.c_int32),
        ("nw_max", C.c_int32), ("flags", C.c_int32),
        ("pos", C.c_void_p), ("prop", C.c_void_p), ("node_tower", C.c_void_p), ("node_local", C.c_void_p),
        ("wtile", C.c_void_p), ("edge_src", C.c_void_p), ("edge_dst", C.c_void_p), ("blk_csr", C.c_void_p),
    ]


class PrologueC(C.Structure):
    """spwgnn_prologue: a replayed step's batch upload and key/step advance, run by the forward's
    first launch."""
    _fields_ = [("copy_src", C.c_void_p), ("copy_dst", C.c_void_p), ("copy_bytes", C.c_int64),
                ("key", C.c_void_p), ("step", C.c_void_p), ("mode", C.c_int32), ("rank", C.c_int32),
                ("seed", C.c_uint64)]


class RunC(C.Structure):
    _fields_ = [("mp_steps", C.c_int32), ("training", C.c_int32), ("dropout", C.c_float), ("math", C.c_int32),
                ("seed", C.c_uint64), ("prof_kernel", C.c_int32), ("prof_count", C.c_int32),
                ("prof_events", C.c_void_p), ("seed_dev", C.c_void_p), ("prologue", C.c_void_p),
                ("grads_early_event", C.c_void_p)]


class LossWeightsC(C.Structure):
    """spwgnn_loss_weights: per-node loss weights and their divisor (added within ABI 8)."""
    _fields_ = [("w", C.c_void_p), ("norm_dev", C.c_void_p), ("norm", C.c_double)]


class PlanDeviceC(C.Structure):
    """spwgnn_plan_device: the static geometry and the output arrays of a device-filled plan (added
    within ABI 8)."""
    _fields_ = [("n_towers", C.c_int32), ("n_nodes", C.c_int32), ("n_wtiles", C.c_int32), ("n_eblocks", C.c_int32),
                ("nw_max", C.c_int32), ("reserved", C.c_int32),
                ("wtile", C.c_void_p), ("node_local", C.c_void_p), ("wtile_tower", C.c_void_p),
                ("tower_cap", C.c_void_p), ("edge_src", C.c_void_p), ("edge_dst", C.c_void_p),
                ("blk_csr", C.c_void_p), ("pos", C.c_void_p), ("tower_edges", C.c_void_p), ("status", C.c_void_p),
                ("prof_events", C.c_void_p)]


class ClipC(C.Structure):
    """spwgnn_clip: the options and outputs of a clipped / guarded Adam step (added within ABI 8)."""
    _fields_ = [("clipnorm", C.c_float), ("clipvalue", C.c_float), ("skip_nonfinite", C.c_int32),
                ("reserved", C.c_int32), ("out4", C.c_void_p), ("total4", C.c_void_p)]


MAX_STEPS = 64   # mp_steps' bound (the library's validate) and spwgnn_step_weights' lambda slots


class StepWeightsC(C.Structure):
    """spwgnn_step_weights: the per-step loss weights of spwgnn_bce_steps, by value (added within ABI 8)."""
    _fields_ = [("count", C.c_int32), ("reserved", C.c_int32), ("lam", C.c_float * MAX_STEPS)]


EVAL_BINS = 256    # SPWGNN_EVAL_BINS: 1/8-logit histogram bins over [-16, 16), the ends clamped
EVAL_SIZES = 33    # SPWGNN_EVAL_SIZES: tower-size buckets 1..32; bucket 0 = any other size


class EvalC(C.Structure):
    """spwgnn_eval: the options, inputs and int64 tables of spwgnn_eval_metrics (added within ABI 8)."""
    _fields_ = [("rows", C.c_int32), ("n_towers", C.c_int32), ("threshold", C.c_float), ("reserved", C.c_int32),
                ("w", C.c_void_p), ("tower_offsets", C.c_void_p), ("node4", C.c_void_p), ("tower6", C.c_void_p),
                ("by_size", C.c_void_p), ("hist", C.c_void_p)]


class TowerLossC(C.Structure):
    """spwgnn_tower_loss: the towers, weights, divisor and outputs of spwgnn_bce_tower (added within ABI 8)."""
    _fields_ = [("n_towers", C.c_int32), ("reserved", C.c_int32), ("tower_offsets", C.c_void_p),
                ("tower_targets", C.c_void_p), ("alpha", C.c_float), ("mu", C.c_float), ("norm_t_dev", C.c_void_p),
                ("norm_t", C.c_double), ("out6", C.c_void_p), ("per_tower", C.c_void_p), ("weights6", C.c_void_p),
                ("total6", C.c_void_p)]


K_EDGE_FWD, K_NODE_FWD, K_EDGE_BWD, K_NODE_BWD, K_ENC_EDGE, K_ENC_EDGE_BWD, K_WGRAD_W2, K_DA = 1, 2, 3, 4, 5, 6, 7, 8
K_WGRAD_WS, K_ENC_NODE, K_ENC_NODE_BWD, K_INPUT_BWD, K_PLAN_DEVICE, K_STATE = 9, 10, 11, 12, 13, 14
K_REL_BWD = 15
K_DROPEDGE = 16
DROPEDGE_SYMMETRIC, DROPEDGE_RESCALE = 1, 2   # spwgnn_dropedge_gates flags
MATH_F32, MATH_X6, MATH_BF16, MATH_X3, MATH_H3 = 0, 1, 2, 3, 4
E_ARG, E_WORKSPACE, E_NOTRAIN = -1, -4, -6   # SPWGNN_E_* statuses the bindings name
E_SHAPE, E_RELATION, E_CAPACITY = -2, -3, -5
STEP_KEY_COUNTER, STEP_KEY_SPLITMIX = 0, 1
ABI_VERSION = 8        # SPWGNN_ABI_VERSION this binding's structs follow
BATCH_RECV_BLOCKS = 1  # spwgnn_batch.flags: a receiver-block plan (spwgnn_plan_fill_recv)
READOUT_SUM_PROB, READOUT_MEAN_PROB, READOUT_SUM_LOGIT, READOUT_MEAN_LOGIT = 0, 1, 2, 3


def _declare(lib: C.CDLL) -> None:
    i32, i64, vp, f32 = C.c_int32, C.c_int64, C.c_void_p, C.c_float
    sig = {
        "spwgnn_version": (i32, []),
        "spwgnn_struct_size": (i32, [i32]),
        "spwgnn_strerror": (C.c_char_p, [i32]),
        "spwgnn_param_tensor_count": (i32, []),
        "spwgnn_param_count": (i64, []),
        "spwgnn_param_real_count": (i64, []),
        "spwgnn_param_tensor": (i32, [i32, C.POINTER(ParamInfo)]),
        "spwgnn_dense_to_edges": (i32, [vp, vp, i32, i32, vp, vp, vp, i64, C.POINTER(i64), vp]),
        "spwgnn_plan_size": (i32, [i32, vp, vp, i32, C.POINTER(PlanSizes)]),
        "spwgnn_plan_fill": (i32, [i32, vp, vp, vp, vp, i32, C.POINTER(PlanSizes), vp, vp, vp, vp, vp]),
        "spwgnn_plan_size_cap": (i32, [i32, vp, vp, i32, C.POINTER(PlanSizes)]),
        "spwgnn_plan_order": (i32, [i32, vp, vp, i32, vp]),
        "spwgnn_plan_fill_cap": (i32, [i32, vp, vp, vp, vp, vp, i32, C.POINTER(PlanSizes), vp, vp, vp, vp, vp]),
        "spwgnn_plan_size_recv": (i32, [i32, vp, i32, C.POINTER(PlanSizes)]),
        "spwgnn_plan_fill_recv": (i32, [i32, vp, vp, vp, vp, i32, C.POINTER(PlanSizes), vp, vp, vp, vp, vp]),
        "spwgnn_workspace_bytes": (i64, [i32, i32, i32, i32]),
        "spwgnn_fused_path": (i32, [C.POINTER(BatchC), C.POINTER(RunC)]),
        "spwgnn_fused_path_gated": (i32, [C.POINTER(BatchC), C.POINTER(RunC)]),
        "spwgnn_team_max_blocks": (i32, [i32]),
        "spwgnn_da_stored_steps": (i32, [i32]),
        "spwgnn_math_products": (i32, [i32]),
        "spwgnn_math_products_bwd": (i32, [i32]),
        "spwgnn_host_device_ptr": (i32, [vp, C.POINTER(vp)]),
        "spwgnn_forward": (i32, [vp, C.POINTER(BatchC), C.POINTER(RunC), vp, i64, vp, vp]),
        "spwgnn_backward": (i32, [vp, C.POINTER(BatchC), C.POINTER(RunC), vp, i64, vp, vp, vp, vp]),
        "spwgnn_forward_state": (i32, [vp, C.POINTER(BatchC), C.POINTER(RunC), vp, i64, vp, vp, vp]),
        "spwgnn_backward_state": (i32, [vp, C.POINTER(BatchC), C.POINTER(RunC), vp, i64, vp, vp, vp, vp, vp]),
        "spwgnn_forward_steps": (i32, [vp, C.POINTER(BatchC), C.POINTER(RunC), vp, i64, vp, vp, vp]),
        "spwgnn_backward_steps": (i32, [vp, C.POINTER(BatchC), C.POINTER(RunC), vp, i64, vp, vp, vp, vp, vp]),
        "spwgnn_bce_steps_scratch_bytes": (i64, [i64, i32]),
        "spwgnn_bce_steps": (i32, [vp, vp, i64, i32, C.POINTER(StepWeightsC), C.POINTER(LossWeightsC), vp, vp, vp, vp,
                                   vp, vp, vp, vp]),
        "spwgnn_backward_inputs": (i32, [vp, C.POINTER(BatchC), C.POINTER(RunC), vp, i64, vp, vp]),
        "spwgnn_backward_relations": (i32, [vp, C.POINTER(BatchC), C.POINTER(RunC), vp, i64, vp, vp, vp]),
        "spwgnn_gates_supported": (i32, [i32]),
        "spwgnn_forward_gated": (i32, [vp, C.POINTER(BatchC), C.POINTER(RunC), vp, i64, vp, vp, vp, vp]),
        "spwgnn_backward_gated": (i32, [vp, C.POINTER(BatchC), C.POINTER(RunC), vp, i64, vp, vp, vp, vp, vp, vp]),
        "spwgnn_dropedge_gates": (i32, [C.POINTER(BatchC), C.POINTER(RunC), f32, i32, vp, vp, vp]),
        "spwgnn_dropedge_keep_host": (i32, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, f32, i32]),
        "spwgnn_forward_step_gated": (i32, [vp, C.POINTER(BatchC), C.POINTER(RunC), vp, i64, vp, i64, vp, vp, vp]),
        "spwgnn_backward_step_gated": (i32, [vp, C.POINTER(BatchC), C.POINTER(RunC), vp, i64, vp, i64, vp, vp, vp, vp,
                                             vp]),
        "spwgnn_dropedge_step_gates": (i32, [C.POINTER(BatchC), C.POINTER(RunC), f32, i32, vp, i64, vp, i64, vp]),
        "spwgnn_dropedge_keep_host_step": (i32, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, f32,
                                                 i32]),
        "spwgnn_plan_device_positions": (i32, [C.POINTER(PlanDeviceC), vp, i32, f32, f32, vp]),
        "spwgnn_plan_device_dense": (i32, [C.POINTER(PlanDeviceC), vp, vp, i32, i32, vp]),
        "spwgnn_bce_scratch_bytes": (i64, [i64]),
        "spwgnn_bce": (i32, [vp, vp, i64, vp, vp, vp, vp]),
        "spwgnn_bce_accumulate": (i32, [vp, vp, i64, vp, vp, vp, vp, vp, vp]),
        "spwgnn_bce_backward": (i32, [vp, vp, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]),
        "spwgnn_bce_weighted": (i32, [vp, vp, i64, C.POINTER(LossWeightsC), vp, vp, vp, vp, vp, vp]),
        "spwgnn_bce_backward_weighted": (i32, [vp, vp, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp,
                                               C.POINTER(LossWeightsC), vp]),
        "spwgnn_adam": (i32, [vp, vp, vp, vp, i64, i32, f32, f32, f32, f32, f32, f32, vp]),
        "spwgnn_adam_dev": (i32, [vp, vp, vp, vp, i64, vp, vp, i32, f32, f32, f32, f32, f32, vp]),
        "spwgnn_adam_lr_table": (i32, [f32, f32, f32, i32, vp]),
        "spwgnn_clip_scratch_bytes": (i64, []),
        "spwgnn_adam_clipped": (i32, [vp, vp, vp, vp, i64, i32, f32, f32, f32, f32, f32, f32, C.POINTER(ClipC), vp, vp]),
        "spwgnn_adam_clipped_dev": (i32, [vp, vp, vp, vp, i64, vp, vp, i32, f32, f32, f32, f32, f32, C.POINTER(ClipC),
                                          vp, vp]),
        "spwgnn_adam_lr_decayed": (f32, [f32, f32, i64]),
        "spwgnn_adam_lr_table_decay": (i32, [f32, f32, f32, f32, i32, vp]),
        "spwgnn_step_advance": (i32, [vp, vp, i32, C.c_uint64, i32, vp]),
        "spwgnn_sigmoid": (i32, [vp, vp, i64, vp]),
        "spwgnn_copy_in": (i32, [vp, vp, i64, vp]),
        "spwgnn_accumulate_out3": (i32, [vp, vp, vp, vp]),
        "spwgnn_tower_readout": (i32, [vp, vp, i32, i32, vp, vp]),
        "spwgnn_eval_metrics": (i32, [vp, vp, i64, C.POINTER(EvalC), vp]),
        "spwgnn_bce_tower_scratch_bytes": (i64, [i64, i32]),
        "spwgnn_bce_tower": (i32, [vp, vp, i64, C.POINTER(LossWeightsC), C.POINTER(TowerLossC), vp, vp, vp, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args


def lib() -> C.CDLL:
    """Load (once) the in-tree HIP library. Raises if it is absent: there is no fallback."""
    global _lib
    if _lib is None:
        path = Path(os.environ.get("SPWGNN_LIB", _LIB_PATH))
        if not path.exists():
            raise SpwgnnError(f"{path} not found — build it with `python -m spwgnn_amd.build` "
                              "(the HIP path has no CPU fallback)")
        lib_ = C.CDLL(str(path), mode=C.RTLD_GLOBAL)
        _declare(lib_)
        if lib_.spwgnn_version() != ABI_VERSION:
            raise SpwgnnError(f"{path} implements ABI {lib_.spwgnn_version()}, this binding expects {ABI_VERSION}: "
                              "rebuild with `python -m spwgnn_amd.build`")
        for which, st in ((0, BatchC), (1, RunC), (2, PlanSizes), (3, ParamInfo), (4, LossWeightsC), (6, PlanDeviceC),
                          (7, ClipC), (9, StepWeightsC), (10, EvalC), (12, TowerLossC)):
            if lib_.spwgnn_struct_size(which) != C.sizeof(st):
                raise SpwgnnError(f"{path} was built with a different {st.__name__} layout "
                                  f"({lib_.spwgnn_struct_size(which)} vs {C.sizeof(st)} bytes): rebuild it")
        _lib = lib_
    return _lib


_hip = None


def hip_runtime() -> C.CDLL:
    """The HIP runtime already mapped into this process — the copy torch and libspwgnn_hip.so run on —
    opened by its mapped path (never a second runtime found by soname). For the event calls of the
    bench's timing hook."""
    global _hip
    if _hip is None:
        lib()
        with open("/proc/self/maps") as f:
            paths = {ln.split()[-1] for ln in f if "libamdhip64.so" in ln}
        if not paths:
            raise SpwgnnError("the HIP runtime is not mapped into this process")
        _hip = C.CDLL(sorted(paths)[0])
    return _hip


def host_device_ptr(ptr: int) -> int:
    """spwgnn_host_device_ptr: the device address of pinned, device-mapped host memory."""
    out = C.c_void_p()
    check(lib().spwgnn_host_device_ptr(C.c_void_p(ptr), C.byref(out)), "host_device_ptr (not device-mapped?)")
    return int(out.value)


def check(status: int, what: str = "") -> None:
    if status != 0:
        msg = lib().spwgnn_strerror(status).decode()
        raise SpwgnnError(f"{what}: {msg} (status {status})")


def param_tensors():
    L = lib()
    out = []
    info = ParamInfo()
    for i in range(L.spwgnn_param_tensor_count()):
        check(L.spwgnn_param_tensor(i, C.byref(info)), "param_tensor")
        out.append((info.name.decode(), int(info.offset), int(info.rows), int(info.cols)))
    return out
