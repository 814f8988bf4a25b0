"""Thin host wrapper over the C-ABI: workspace management and the per-call entry points.

torch provides device memory (caching allocator) and the current HIP stream; every byte of
arithmetic happens in libspwgnn_hip.so. Nothing here falls back to CPU.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib, params as P
from .batch import TowerBatch

REF_MP_STEPS = 5       # Networks.py:83
REF_DROPOUT = 0.1      # Networks.py:77-78


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _require_gpu(t: torch.Tensor, what: str):
    if t.device.type != "cuda":
        raise _lib.SpwgnnError(f"{what} must be a HIP device tensor (got {t.device}); the HIP path has no CPU fallback")


MATH_MODES = {"f32": _lib.MATH_F32, "x6": _lib.MATH_X6, "bf16": _lib.MATH_BF16, "x3": _lib.MATH_X3,
              "h3": _lib.MATH_H3}


# Replayed steps fold their batch upload and key/step advance into the forward's first launch
# (spwgnn_run.prologue); SPWGNN_NO_PROLOGUE=1 issues them as launches of their own (A/B).
FOLD_PROLOGUE = os.environ.get("SPWGNN_NO_PROLOGUE", "0") in ("", "0")


@dataclass
class RunConfig:
    mp_steps: int = REF_MP_STEPS
    training: bool = False
    dropout: float = 0.0
    seed: int = 0
    math: str = "x6"                     # "x6" 3-part split-bf16 products (fp32-class, the parity path) | "f32" f32 MFMA |
                                         # "x3" 2-part split, 3 products (16-bit operand mantissa) | "bf16" |
                                         # "h3" forward on 2 fp16 parts, 3 products (fp32-class), backward x6 (spwgnn.h)
    prof_kernel: int = 0                 # SPWGNN_K_* to bracket with HIP events (bench only)
    prof_events: Optional[list] = None   # raw hipEvent_t handles, 2 per launch
    seed_dev: Optional[torch.Tensor] = None   # (1,) int64 device word holding the dropout key (replayable steps)
    prologue: Optional["Prologue"] = None      # forward only: a replayed step's upload + key/step advance
    grads_early_event: Optional[torch.cuda.Event] = None   # backward only: spwgnn_run.grads_early_event

    def cstruct(self, with_prologue: bool = False) -> _lib.RunC:
        r = _lib.RunC()
        r.mp_steps = int(self.mp_steps)
        r.training = 1 if self.training else 0
        r.dropout = float(self.dropout)
        r.seed = int(self.seed) & 0xFFFFFFFFFFFFFFFF
        if self.math not in MATH_MODES:
            raise ValueError(f"math must be one of {sorted(MATH_MODES)}")
        r.math = MATH_MODES[self.math]
        if self.prof_kernel and self.prof_events:
            arr = (C.c_void_p * len(self.prof_events))(*self.prof_events)
            self._prof_arr = arr   # keep alive for the call
            r.prof_kernel = int(self.prof_kernel)
            r.prof_count = len(self.prof_events) // 2
            r.prof_events = C.cast(arr, C.c_void_p)
        if self.seed_dev is not None:
            if self.seed_dev.device.type != "cuda" or self.seed_dev.dtype != torch.int64:
                raise ValueError("seed_dev must be a (1,) int64 device tensor")
            r.seed_dev = self.seed_dev.data_ptr()
        if self.grads_early_event is not None:
            h = self.grads_early_event.cuda_event
            if not h:
                raise ValueError("grads_early_event: record the event once first (it has no hipEvent_t yet)")
            r.grads_early_event = h
        if with_prologue and self.prologue is not None:   # spwgnn_forward only
            self._pro_c = self.prologue.cstruct()   # keep alive for the call
            r.prologue = C.cast(C.pointer(self._pro_c), C.c_void_p)
        return r


@dataclass
class Prologue:
    """spwgnn_prologue (include/spwgnn.h): what a replayed step does before its forward, run by the
    forward's first launch instead of two launches of its own — the batch upload (spwgnn_copy_in:
    `nbytes` from the pinned, device-mapped `src_dev_ptr` into `dst`) and the key/step advance
    (spwgnn_step_advance: `key`, `step` device words, `mode` STEP_KEY_*)."""
    dst: Optional[torch.Tensor] = None
    src_dev_ptr: int = 0
    nbytes: int = 0
    key: Optional[torch.Tensor] = None
    step: Optional[torch.Tensor] = None
    mode: int = _lib.STEP_KEY_COUNTER
    seed: int = 0
    rank: int = 0

    def cstruct(self) -> _lib.PrologueC:
        p = _lib.PrologueC()
        if self.nbytes:
            if self.dst is None or not self.src_dev_ptr:
                raise ValueError("prologue copy needs dst and src_dev_ptr")
            _require_gpu(self.dst, "prologue copy destination")
            if self.nbytes > self.dst.numel() * self.dst.element_size():
                raise ValueError("prologue copy beyond its destination")
            p.copy_src, p.copy_dst, p.copy_bytes = int(self.src_dev_ptr), self.dst.data_ptr(), int(self.nbytes)
        if self.key is not None:
            if self.step is None:
                raise ValueError("prologue advance needs key and step words")
            p.key, p.step = self.key.data_ptr(), self.step.data_ptr()
            p.mode, p.seed, p.rank = int(self.mode), int(self.seed) & 0xFFFFFFFFFFFFFFFF, int(self.rank)
        return p


# SPWGNN_POISON_WORKSPACE=1: fill every newly allocated workspace with 0xFF bytes (and the logits,
# gradient, d/d'propagation' and d/d'objects' outputs with NaN), so a kernel that reads workspace it did not write,
# or leaves part of an output unwritten, turns results into NaN (run the GPU suite with it;
# tests/test_gpu_determinism.py does the same per case)
POISON_WORKSPACE = os.environ.get("SPWGNN_POISON_WORKSPACE", "0") not in ("", "0")


def _poison(t: torch.Tensor) -> torch.Tensor:
    """An output buffer the library must write in full: NaN-filled under SPWGNN_POISON_WORKSPACE."""
    if POISON_WORKSPACE and t.is_floating_point():
        t.fill_(float("nan"))
    return t


class Workspace:
    """Device scratch for one forward (+ its backward). Sized by spwgnn_workspace_bytes."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.buf: Optional[torch.Tensor] = None
        self.fwd_key: Optional[tuple] = None   # what the last forward on this workspace stored
        self.fwd_batch = None                  # weakref to the batch that forward ran on
        self.bwd_key: Optional[tuple] = None   # fwd_key once a backward of that forward has run (backward_inputs)
        self.has_state = False                 # that forward returned the final state (backward's dstate needs it)
        self.gate_key: Optional[tuple] = None  # that forward's relation gates (pointer, version), None: ungated

    @staticmethod
    def key(batch: TowerBatch, run: "RunConfig") -> tuple:
        # sizes and run fields, plus the device arrays the stored activations were computed from:
        # two same-shape batches (equal micro-batches under one seed) must not pass for each other
        return (run.math, int(run.mp_steps), bool(run.training), float(run.dropout), int(run.seed),
                run.seed_dev.data_ptr() if run.seed_dev is not None else 0, batch.n_nodes, batch.n_eblocks, batch.n_wtiles, batch.pos.data_ptr(), batch.edge_src.data_ptr(),
                batch.prop.data_ptr() if batch.prop is not None else 0,
                # device-built batches are refilled in place (TowerBatch.refill): same arrays, new contents
                int(getattr(batch, "generation", 0)))

    def holds(self, batch: TowerBatch, run: "RunConfig") -> bool:
        """True when the last forward on this workspace ran `batch` (the same object) with `run`."""
        return (self.buf is not None and self.fwd_batch is not None and self.fwd_batch() is batch
                and self.fwd_key == Workspace.key(batch, run))

    def stored(self, batch: TowerBatch, run: "RunConfig", ok: bool, has_state: bool, gates=None):
        """What a forward that returned `ok` left here (a failed one: nothing a backward may read)."""
        self.gate_key = _gate_key(gates) if ok else None
        self.fwd_key = Workspace.key(batch, run) if ok else None
        self.fwd_batch = weakref.ref(batch) if ok else None
        self.bwd_key = None
        self.has_state = bool(has_state) and ok

    def get(self, nbytes: int) -> torch.Tensor:
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = None
            self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
            if POISON_WORKSPACE:   # debugging: every fresh workspace byte 0xFF (NaN as fp32)
                self.buf.fill_(0xFF)
        return self.buf


def _gate_key(gates: Optional[torch.Tensor]) -> Optional[tuple]:
    """What identifies a gate tensor's values between a forward and its backward: the storage address and the
    tensor's version counter (an in-place write bumps it)."""
    return None if gates is None else (gates.data_ptr(), int(gates._version))


def gates_supported(math) -> bool:
    """Whether `forward` / `backward` take ``gates=`` in this math — a `MATH_MODES` name or a SPWGNN_MATH_* id
    (spwgnn_gates_supported): x6, x3 and h3 do, f32 and bf16 do not."""
    if isinstance(math, str):
        if math not in MATH_MODES:
            raise ValueError(f"math must be one of {sorted(MATH_MODES)}")
        math = MATH_MODES[math]
    st = int(_lib.lib().spwgnn_gates_supported(int(math)))
    if st < 0:
        raise ValueError(f"unknown math id {math}")
    return st == 1


def _check_gates(batch: TowerBatch, run: "RunConfig", gates: torch.Tensor) -> torch.Tensor:
    """A relation-gate tensor of `forward` / `backward`, validated before the library call: (32·n_eblocks,) fp32,
    contiguous, 16-byte aligned, on the GPU, in a math that takes gates. Returns it detached."""
    if not gates_supported(run.math):
        raise ValueError(f"relation gates are not supported in math {run.math} (spwgnn_gates_supported: x6, x3 and h3 "
                         "take them, f32 and bf16 do not)")
    slots = 32 * batch.n_eblocks
    if not isinstance(gates, torch.Tensor) or tuple(gates.shape) != (slots,):
        raise ValueError(f"gates must be a ({slots},) tensor in the plan's edge-slot order (TowerBatch.edge_gates "
                         f"builds it; got {tuple(getattr(gates, 'shape', ()))})")
    _require_gpu(gates, "gates")
    if gates.dtype != torch.float32 or not gates.is_contiguous() or gates.data_ptr() % 16:
        raise ValueError("gates must be a contiguous, 16-byte aligned fp32 tensor")
    return gates.detach()


def _check_step_gates(batch: TowerBatch, run: "RunConfig", step_gates: torch.Tensor) -> torch.Tensor:
    """A per-step relation-gate tensor of `forward` / `backward` (``step_gates=``): (mp_steps, 32·n_eblocks) fp32,
    contiguous, 16-byte aligned, on the GPU, in a math that takes gates. Returns it detached."""
    if not gates_supported(run.math):
        raise ValueError(f"relation gates are not supported in math {run.math} (spwgnn_gates_supported: x6, x3 and h3 "
                         "take them, f32 and bf16 do not)")
    shape = (int(run.mp_steps), 32 * batch.n_eblocks)
    if not isinstance(step_gates, torch.Tensor) or tuple(step_gates.shape) != shape:
        raise ValueError(f"step_gates must be a {shape} tensor, one row per propagation step in the plan's edge-slot "
                         f"order (TowerBatch.edge_step_gates builds it; got {tuple(getattr(step_gates, 'shape', ()))})")
    _require_gpu(step_gates, "step_gates")
    if step_gates.dtype != torch.float32 or not step_gates.is_contiguous() or step_gates.data_ptr() % 16:
        raise ValueError("step_gates must be a contiguous, 16-byte aligned fp32 tensor")
    return step_gates.detach()


def _gate_args(batch, run, gates, step_gates):
    """The validated gate tensor of a call (shared or per-step, never both) and the arguments the library's
    symbol takes for it: (pointer,) or (pointer, row stride)."""
    if step_gates is not None:
        if gates is not None:
            raise ValueError("gates and step_gates are mutually exclusive: one gate per edge, or one per edge and step")
        step_gates = _check_step_gates(batch, run, step_gates)
        return step_gates, (step_gates.data_ptr(), int(step_gates.shape[1]))
    if gates is not None:
        gates = _check_gates(batch, run, gates)
        return gates, (gates.data_ptr(),)
    return None, ()


def check_dropedge(rate) -> float:
    """A DropEdge rate: a float in [0, 1) (0 = off), what spwgnn_dropedge_gates refuses otherwise."""
    rate = float(rate)
    if not 0.0 <= rate < 1.0:   # False for a NaN
        raise ValueError(f"dropedge must be in [0, 1) (got {rate})")
    return rate


def dropedge_gates(batch: TowerBatch, run: RunConfig, rate: float, *, symmetric: bool = True, rescale: bool = False,
                   base: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                   per_step: bool = False) -> torch.Tensor:
    """The relation gates of a DropEdge draw (spwgnn_dropedge_gates): (32·n_eblocks,) fp32 in the plan's edge-slot
    order, what ``forward(..., gates=)`` / ``backward(..., gates=)`` take. Edge k is dropped (gate 0) with
    probability ``rate``, drawn from the run's dropout key (``run.seed``, or the device word ``run.seed_dev``) with
    a kind of its own on (tower id, sender's local index, receiver's local index): independent of the feature
    dropout's masks, and the same for a tower wherever a plan, a shard or a micro-batch puts it. ``symmetric``: both
    directions of a contact share one draw. ``rescale``: a kept edge's gate is 1/(1 − rate) instead of 1.
    ``base``: (32·n_eblocks,) fp32 weights multiplied into the mask (`TowerBatch.edge_gates` builds them).
    Padding slots get 0. One launch, no host sync; ``out``: the buffer to write (a captured step's static one).
    ``per_step`` (layer-wise DropEdge, spwgnn_dropedge_step_gates): a fresh subset at every propagation step,
    (mp_steps, 32·n_eblocks) fp32 for ``forward(..., step_gates=)``; row 0 is the mask without ``per_step``. ``base``
    is then one row multiplied into every step's, or a (mp_steps, 32·n_eblocks) tensor of per-step weights."""
    rate = check_dropedge(rate)
    slots = 32 * batch.n_eblocks
    shape = (int(run.mp_steps), slots) if per_step else (slots,)
    base_step = 0
    if base is not None:
        if per_step and isinstance(base, torch.Tensor) and base.dim() == 2:
            base = _check_step_gates(batch, run, base)
            base_step = slots
        else:
            base = _check_gates(batch, run, base)
    if out is None:
        out = _poison(torch.empty(shape, dtype=torch.float32, device=batch.device))
    else:
        _out_buffer(out, shape, "out")
    if batch.node_tower is None or batch.node_local is None:
        raise ValueError("dropedge_gates needs the batch's node_tower and node_local (the key's tower id and node index)")
    b = batch.cstruct()
    r = run.cstruct()
    flags = (_lib.DROPEDGE_SYMMETRIC if symmetric else 0) | (_lib.DROPEDGE_RESCALE if rescale else 0)
    if per_step:
        st = _lib.lib().spwgnn_dropedge_step_gates(C.byref(b), C.byref(r), rate, flags,
                                                   base.data_ptr() if base is not None else None, base_step,
                                                   out.data_ptr(), slots, _stream(batch.device))
        _lib.check(st, "spwgnn_dropedge_step_gates")
        return out
    st = _lib.lib().spwgnn_dropedge_gates(C.byref(b), C.byref(r), rate, flags,
                                          base.data_ptr() if base is not None else None, out.data_ptr(),
                                          _stream(batch.device))
    _lib.check(st, "spwgnn_dropedge_gates")
    return out


def dropedge_keep_host(key: int, tower: int, a: int, b: int, rate: float, symmetric: bool = True,
                       step: Optional[int] = None) -> bool:
    """Whether DropEdge keeps edge (tower, sender a → receiver b) under `key` (spwgnn_dropedge_keep_host; no device).
    ``step``: the draw of propagation step `step` of a per-step mask (spwgnn_dropedge_keep_host_step; step 0 is the
    shared mask's draw)."""
    flags = _lib.DROPEDGE_SYMMETRIC if symmetric else 0
    if step is None:
        symbol = "spwgnn_dropedge_keep_host"
        st = int(_lib.lib().spwgnn_dropedge_keep_host(int(key) & 0xFFFFFFFFFFFFFFFF, int(tower), int(a), int(b),
                                                      float(rate), flags))
    else:
        if int(step) < 0:
            raise ValueError(f"step must be >= 0 (got {step})")
        symbol = "spwgnn_dropedge_keep_host_step"
        st = int(_lib.lib().spwgnn_dropedge_keep_host_step(int(key) & 0xFFFFFFFFFFFFFFFF, int(tower), int(a), int(b),
                                                           int(step), float(rate), flags))
    if st < 0:
        _lib.check(st, symbol)
    return st == 1


def workspace_bytes(batch: TowerBatch, run: RunConfig) -> int:
    n = int(_lib.lib().spwgnn_workspace_bytes(batch.n_nodes, batch.n_eblocks, run.mp_steps, 1 if run.training else 0))
    if n < 0:
        raise _lib.SpwgnnError("invalid batch shape for workspace")
    return n


def fused_path(batch: TowerBatch, run: RunConfig, gated: bool = False) -> int:
    """The library's own answer to which launches this batch and run take (spwgnn_fused_path): bit 0 =
    the forward's fused small-batch step loop, bit 1 = the backward's. ``gated``: for a call with relation gates
    (spwgnn_fused_path_gated). No device work."""
    b = batch.cstruct()
    r = run.cstruct()
    symbol = "spwgnn_fused_path_gated" if gated else "spwgnn_fused_path"
    st = getattr(_lib.lib(), symbol)(C.byref(b), C.byref(r))
    if st < 0:
        _lib.check(st, symbol)
    return int(st)


def team_max_blocks(set_to: Optional[int] = None) -> int:
    """The library's small-batch limit (spwgnn_team_max_blocks): batches of at most this many 32-row
    blocks run the team kernels, larger ones the wide kernels. With ``set_to`` (>= 0) it is changed for
    the process and the previous limit is returned."""
    return int(_lib.lib().spwgnn_team_max_blocks(-1 if set_to is None else int(set_to)))


class wide_kernels:
    """``with wide_kernels(): ...`` — every call inside plans the wide (large-batch) kernels whatever the
    batch size (team limit 0), then the previous limit is restored."""

    def __enter__(self):
        self._prev = team_max_blocks(0)
        return self

    def __exit__(self, *exc):
        team_max_blocks(self._prev)
        return False


DA_STORED_DEFAULT = 3   # the library's compile-time SPWGNN_DA_STORED


def da_stored_steps(set_to: Optional[int] = None) -> int:
    """The stored steps K of the dA sum on the wide x6 kernels (spwgnn_da_stored_steps): the edge backward
    of the last K steps keeps its dh1pre and the dA kernel reads it back instead of repeating the product
    (bitwise the same gradients at every K; clamped per call to min(4, mp_steps - 1)). With ``set_to``
    (>= 0) it is changed for the process and the previous value is returned."""
    return int(_lib.lib().spwgnn_da_stored_steps(-1 if set_to is None else int(set_to)))


class da_stored:
    """``with da_stored(k): ...`` — every backward planned inside keeps k dh1pre steps (see
    da_stored_steps), then the previous value is restored."""

    def __init__(self, k: int):
        self._k = int(k)

    def __enter__(self):
        self._prev = da_stored_steps(self._k)
        return self

    def __exit__(self, *exc):
        da_stored_steps(self._prev)
        return False


STATE_WIDTH = 100   # the propagation state's features (Networks.py:29)


def _check_dstate(ws: Workspace, batch: TowerBatch, dstate: torch.Tensor) -> torch.Tensor:
    """The state cotangent of `backward`: the library cannot check its contract (spwgnn_backward_state),
    so it is enforced here."""
    if not ws.has_state:
        raise ValueError("backward(dstate=...) needs forward(..., return_state=True) on this workspace: a plain "
                         "forward does not keep the final state on every path")
    if not isinstance(dstate, torch.Tensor) or tuple(dstate.shape) != (batch.n_nodes, STATE_WIDTH):
        raise ValueError(f"dstate must be a ({batch.n_nodes}, {STATE_WIDTH}) tensor in the plan's node order "
                         f"(got {tuple(getattr(dstate, 'shape', ()))})")
    if dstate.dtype != torch.float32:
        raise ValueError(f"dstate must be float32 (got {dstate.dtype})")
    _require_gpu(dstate, "dstate")
    want = torch.device(batch.device)   # "cuda" names the current device: compare the index only when given
    if want.index is not None and dstate.device.index != want.index:
        raise ValueError(f"dstate must be on the batch's device {batch.device} (got {dstate.device})")
    return dstate.contiguous()


def _out_buffer(t: torch.Tensor, shape: tuple, what: str) -> torch.Tensor:
    """A caller's output buffer, validated: on the GPU, fp32, contiguous, of exactly `shape`."""
    _require_gpu(t, what)
    if tuple(t.shape) != tuple(shape) or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous fp32 {tuple(shape)} tensor")
    return t


def _dprop_buffer(batch: TowerBatch, dprop: Optional[torch.Tensor], want_dprop: bool) -> Optional[torch.Tensor]:
    """d/d'propagation' output: the caller's ``dprop`` (it implies want_dprop), a fresh one, or None."""
    if dprop is not None:
        return _out_buffer(dprop, (batch.n_nodes, STATE_WIDTH), "dprop")
    if want_dprop:
        return _poison(torch.empty(batch.n_nodes, STATE_WIDTH, dtype=torch.float32, device=batch.device))
    return None


def _check_params(flat_params: torch.Tensor):
    _require_gpu(flat_params, "params")
    if flat_params.dtype != torch.float32 or not flat_params.is_contiguous() or flat_params.numel() != P.flat_size():
        raise ValueError("params must be a contiguous fp32 flat buffer of spwgnn_param_count() floats")


def _training_forward(ws: Workspace, batch: TowerBatch, run: RunConfig, dstate: Optional[torch.Tensor] = None):
    """The guard of every backward: `ws` holds the training forward of `batch` and `run` (and, for a state
    cotangent, its final state). Returns the checked ``dstate``."""
    if not run.training:
        raise _lib.SpwgnnError("backward needs a training forward on the same workspace")
    if dstate is not None:
        dstate = _check_dstate(ws, batch, dstate)
    if not ws.holds(batch, run):
        # the backward reads what the forward stored (masks, activations, packed weights); the split-
        # bf16 maths do not store z1/zo1 at all, so a mismatched math or step count reads garbage
        raise _lib.SpwgnnError("backward needs the training forward of the same batch and RunConfig "
                               f"on this workspace (stored {ws.fwd_key}, asked {Workspace.key(batch, run)})")
    return dstate


def _check_sums(total3: Optional[torch.Tensor], weights3: Optional[torch.Tensor]):
    """The epoch sums of the accumulating losses: both or neither, float64."""
    if (total3 is None) != (weights3 is None):
        raise ValueError("total3 and weights3 go together")
    if total3 is not None:
        assert total3.dtype == torch.float64 and weights3.dtype == torch.float64


def _forward(symbol: str, takes_state: bool, flat_params, batch, run, ws, out, shape, what, return_state, state,
             gates=None, step_gates=None):
    """`forward` / `forward_steps`: ``out`` (or a fresh buffer) of `shape` written by the library's `symbol`,
    whose argument list has a state pointer when `takes_state` (and, in front of the outputs, a gate pointer
    with ``gates``, or a gate pointer and its row stride with ``step_gates``)."""
    _check_params(flat_params)
    gates, head = _gate_args(batch, run, gates, step_gates)
    buf = ws.get(workspace_bytes(batch, run))
    if out is None:
        out = _poison(torch.empty(shape, dtype=torch.float32, device=batch.device))
    else:
        _out_buffer(out, shape, what)
    if not return_state:
        if state is not None:
            raise ValueError("a state buffer goes with return_state=True")
    elif state is None:
        state = _poison(torch.empty(batch.n_nodes, STATE_WIDTH, dtype=torch.float32, device=batch.device))
    else:
        _out_buffer(state, (batch.n_nodes, STATE_WIDTH), "state")
    b = batch.cstruct()
    r = run.cstruct(with_prologue=True)
    tail = (state.data_ptr() if return_state else None,) if takes_state else ()
    st = getattr(_lib.lib(), symbol)(flat_params.data_ptr(), C.byref(b), C.byref(r), buf.data_ptr(), buf.numel(),
                                     *head, out.data_ptr(), *tail, _stream(batch.device))
    ws.stored(batch, run, st == 0, return_state, gates)
    _lib.check(st, symbol)
    return (out, state) if return_state else out


def forward(flat_params: torch.Tensor, batch: TowerBatch, run: RunConfig, ws: Workspace,
            logits: Optional[torch.Tensor] = None, return_state: bool = False,
            state: Optional[torch.Tensor] = None, gates: Optional[torch.Tensor] = None,
            step_gates: Optional[torch.Tensor] = None):
    """Logits (n_nodes,). With ``return_state`` also the final propagation state P_S, (n_nodes, 100) fp32
    in the plan's node order (spwgnn_forward_state) — what the next call takes as its ``prop`` — as
    ``(logits, state)``; the logits are the same bits either way. ``state``: the buffer to write it to
    (a captured forward's static output, like ``logits``).
    ``gates`` (spwgnn_forward_gated): one relation gate per edge slot, (32·n_eblocks,) fp32 in the plan's
    edge-slot order (`TowerBatch.edge_gates` builds it), any finite values; edge k's message is scaled by
    gates[k] in the receiver sum of Networks.py:88 alone, padding slots are never read. A gated call takes
    the ungated call's launches in their gated forms (`fused_path(gated=True)`; the results are the wide gated
    kernels' bit for bit), in x6, x3 and h3 (`gates_supported`); its backward must be given the same tensor,
    unchanged.
    ``step_gates`` (spwgnn_forward_step_gated; exclusive with ``gates``): one gate per edge slot AND propagation
    step, (mp_steps, 32·n_eblocks) contiguous fp32 (`TowerBatch.edge_step_gates` builds it): step s scales edge k's
    message by step_gates[s, k]. Equal rows give the ``gates=`` call's bits; the same launches, maths and backward
    contract."""
    if step_gates is not None:
        return _forward("spwgnn_forward_step_gated", True, flat_params, batch, run, ws, logits, (batch.n_nodes,),
                        "logits", return_state, state, gates, step_gates)
    if gates is not None:
        return _forward("spwgnn_forward_gated", True, flat_params, batch, run, ws, logits, (batch.n_nodes,), "logits",
                        return_state, state, gates)
    return _forward("spwgnn_forward_state" if return_state else "spwgnn_forward", return_state, flat_params, batch,
                    run, ws, logits, (batch.n_nodes,), "logits", return_state, state)


def forward_steps(flat_params: torch.Tensor, batch: TowerBatch, run: RunConfig, ws: Workspace,
                  step_logits: Optional[torch.Tensor] = None, return_state: bool = False,
                  state: Optional[torch.Tensor] = None):
    """`forward` with every propagation step's logits (spwgnn_forward_steps): (mp_steps, n_nodes) fp32, row
    s = the readout after step s + 1 steps, nodes in the plan's order; the last row holds `forward`'s
    bits. ``step_logits`` / ``state``: the buffers to write to (a captured forward's static outputs).
    With ``return_state`` returns ``(step_logits, state)``."""
    return _forward("spwgnn_forward_steps", True, flat_params, batch, run, ws, step_logits,
                    (int(run.mp_steps), batch.n_nodes), "step_logits", return_state, state)


def _backward(symbol: str, takes_dstate: bool, flat_params, batch, run, ws, dlogits, rows, grads, want_dprop, dstate,
              dprop, gates=None, step_gates=None):
    """`backward` / `backward_steps` through the library's `symbol`, whose argument list has a state
    cotangent when `takes_dstate` (and a gate pointer in front of ``dlogits`` with ``gates``, or a gate pointer
    and its row stride with ``step_gates``). `rows`: the (mp_steps, n_nodes) shape ``dlogits`` must have, or None."""
    gates, head = _gate_args(batch, run, gates, step_gates)
    dstate = _training_forward(ws, batch, run, dstate)
    if ws.gate_key != _gate_key(gates):
        # the library's contract (spwgnn_backward_gated): the backward's gates hold what the forward's held
        raise ValueError("backward needs the relation gates of the forward on this workspace: the same tensor, "
                         f"unchanged since (forward {ws.gate_key}, backward {_gate_key(gates)}; None = ungated)")
    if rows is not None and (not isinstance(dlogits, torch.Tensor) or tuple(dlogits.shape) != rows):
        raise ValueError(f"dstep_logits must be a {rows} tensor: one row of logit cotangents per propagation step "
                         f"(got {tuple(getattr(dlogits, 'shape', ()))})")
    _require_gpu(dlogits, "dstep_logits" if rows is not None else "dlogits")
    dlogits = dlogits.to(torch.float32).contiguous()
    if grads is None:
        grads = _poison(torch.empty_like(flat_params))
    dprop = _dprop_buffer(batch, dprop, want_dprop)
    b = batch.cstruct()
    r = run.cstruct()
    buf = ws.buf
    mid = (dstate.data_ptr() if dstate is not None else None,) if takes_dstate else ()
    st = getattr(_lib.lib(), symbol)(flat_params.data_ptr(), C.byref(b), C.byref(r), buf.data_ptr(), buf.numel(),
                                     *head, dlogits.data_ptr(), *mid, grads.data_ptr(),
                                     dprop.data_ptr() if dprop is not None else None, _stream(batch.device))
    ws.bwd_key = ws.fwd_key if st == 0 else None
    _lib.check(st, symbol)
    return grads, dprop


def backward(flat_params: torch.Tensor, batch: TowerBatch, run: RunConfig, ws: Workspace, dlogits: torch.Tensor,
             grads: Optional[torch.Tensor] = None, want_dprop: bool = False, dstate: Optional[torch.Tensor] = None,
             dprop: Optional[torch.Tensor] = None, gates: Optional[torch.Tensor] = None,
             step_gates: Optional[torch.Tensor] = None):
    """Gradients of Σ dlogits·z — and, with ``dstate`` ((n_nodes, 100) fp32 on the batch's device, plan node
    order), of Σ dlogits·z + Σ dstate·P_S in the same single pass (spwgnn_backward_state); the forward on
    this workspace must then have been ``forward(..., return_state=True)``. A caller with a loss on the
    state alone passes zero ``dlogits``. ``dprop``: the (n_nodes, 100) buffer to write d/d'propagation' to
    (it implies ``want_dprop``). Returns (grads, dprop).
    ``gates`` (spwgnn_backward_gated): the gate tensor the forward on this workspace ran with — the same
    tensor, not written since; other gates, or none after a gated forward (or gates after an ungated one),
    raise ValueError. `backward_relations` then returns the gradient with respect to these gates.
    ``step_gates`` (spwgnn_backward_step_gated): likewise the forward's per-step gate tensor; `backward_relations`'
    ``drel_steps`` is then its gradient, entry by entry."""
    if step_gates is not None:
        return _backward("spwgnn_backward_step_gated", True, flat_params, batch, run, ws, dlogits, None, grads,
                         want_dprop, dstate, dprop, gates, step_gates)
    if gates is not None:
        return _backward("spwgnn_backward_gated", True, flat_params, batch, run, ws, dlogits, None, grads, want_dprop,
                         dstate, dprop, gates)
    return _backward("spwgnn_backward_state" if dstate is not None else "spwgnn_backward", dstate is not None,
                     flat_params, batch, run, ws, dlogits, None, grads, want_dprop, dstate, dprop)


def backward_steps(flat_params: torch.Tensor, batch: TowerBatch, run: RunConfig, ws: Workspace,
                   dstep_logits: torch.Tensor, grads: Optional[torch.Tensor] = None, want_dprop: bool = False,
                   dstate: Optional[torch.Tensor] = None, dprop: Optional[torch.Tensor] = None):
    """Gradients of Σ_s Σ_i dstep_logits[s, i]·z_s[i] (+ Σ dstate·P_S) in one pass over the step loop
    (spwgnn_backward_steps): ``dstep_logits`` is (mp_steps, n_nodes) fp32 in the plan's node order, row s
    the cotangent of step s's logits (`forward_steps`' rows). The forward on this workspace may be any of
    `forward` / `forward_steps`; ``dstate`` needs ``return_state=True`` there. ``dprop`` as in `backward`.
    Returns (grads, dprop)."""
    return _backward("spwgnn_backward_steps", True, flat_params, batch, run, ws, dstep_logits,
                     (int(run.mp_steps), batch.n_nodes), grads, want_dprop, dstate, dprop)


def backward_inputs(flat_params: torch.Tensor, batch: TowerBatch, run: RunConfig, ws: Workspace,
                    dpos: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d(loss)/d(objects) of the last `backward` / `bce_backward` on this workspace (spwgnn_backward_inputs,
    ABI 8): (n_nodes, 3) fp32 — d/d(x, y, width) of the objects rows as the batch holds them (already
    /170) — in the plan's node order (`TowerBatch.to_input_order` for packed plans), a view of the
    library's (n_nodes, 4) output. One extra launch; the gradients `backward` returned are untouched.
    The relation set (a thresholded one included) is a constant of the graph and is not differentiated.
    ``dpos``: the (n_nodes, 4) buffer the library writes to (the returned view is of it)."""
    if not run.training:
        _lib.check(_lib.E_NOTRAIN, "spwgnn_backward_inputs")
    if not ws.holds(batch, run) or ws.bwd_key != ws.fwd_key:
        raise _lib.SpwgnnError("backward_inputs needs the backward of the same batch and RunConfig on this workspace "
                               "(it reads what that backward left there; a new forward discards it)")
    _require_gpu(flat_params, "params")
    if dpos is None:
        dpos = _poison(torch.empty(batch.n_nodes, 4, dtype=torch.float32, device=batch.device))
    else:
        _out_buffer(dpos, (batch.n_nodes, 4), "dpos")
    b = batch.cstruct()
    r = run.cstruct()
    buf = ws.buf
    st = _lib.lib().spwgnn_backward_inputs(flat_params.data_ptr(), C.byref(b), C.byref(r), buf.data_ptr(), buf.numel(),
                                           dpos.data_ptr(), _stream(batch.device))
    _lib.check(st, "spwgnn_backward_inputs")
    return dpos[:, :3]


def backward_relations(flat_params: torch.Tensor, batch: TowerBatch, run: RunConfig, ws: Workspace,
                       drel: Optional[torch.Tensor] = None, per_step: bool = False,
                       drel_steps: Optional[torch.Tensor] = None):
    """d(loss)/d(relation gate) of the last `backward` / `bce_backward` on this workspace
    (spwgnn_backward_relations): (32·n_eblocks,) fp32 in the plan's edge-slot order (``batch.edge_src`` /
    ``edge_dst``'s; `TowerBatch.edges_to_input` maps it back), 0 in padding slots. Entry k is the gradient
    of a scalar gate on edge k in the receiver sum of Networks.py:88 alone, taken at the run's gates (all ones
    after an ungated forward, the ``gates=`` of `forward` / `backward` after a gated one) — in
    reference terms d loss / d receiver_relations[b, dst_k, k] through line 88, not through the gathers of
    lines 33 and 85. One extra launch that only reads the workspace: the
    gradients `backward` returned and `backward_inputs` are untouched, in either call order.
    ``drel``: the buffer to write to. With ``per_step`` returns ``(drel, drel_steps)``, drel_steps
    (mp_steps, 32·n_eblocks) holding each propagation step's share (their sum over steps is drel);
    ``drel_steps``: the buffer for it (it implies ``per_step``)."""
    per_step = per_step or drel_steps is not None
    if not run.training:
        _lib.check(_lib.E_NOTRAIN, "spwgnn_backward_relations")
    if not ws.holds(batch, run) or ws.bwd_key != ws.fwd_key:
        raise _lib.SpwgnnError("backward_relations needs the backward of the same batch and RunConfig on this "
                               "workspace (it reads what that backward left there; a new forward discards it)")
    _check_params(flat_params)
    slots = 32 * batch.n_eblocks
    if drel is None:
        drel = _poison(torch.empty(slots, dtype=torch.float32, device=batch.device))
    else:
        _out_buffer(drel, (slots,), "drel")
    steps = None
    if drel_steps is not None:
        steps = _out_buffer(drel_steps, (int(run.mp_steps), slots), "drel_steps")
    elif per_step:
        steps = _poison(torch.empty(int(run.mp_steps), slots, dtype=torch.float32, device=batch.device))
    b = batch.cstruct()
    r = run.cstruct()
    buf = ws.buf
    st = _lib.lib().spwgnn_backward_relations(flat_params.data_ptr(), C.byref(b), C.byref(r), buf.data_ptr(), buf.numel(),
                                              drel.data_ptr(), steps.data_ptr() if per_step else None,
                                              _stream(batch.device))
    _lib.check(st, "spwgnn_backward_relations")
    return (drel, steps) if per_step else drel


def bce_backward(flat_params: torch.Tensor, batch: TowerBatch, run: RunConfig, ws: Workspace, logits: torch.Tensor,
                 targets: torch.Tensor, scratch: "BceScratch", dlogits: Optional[torch.Tensor] = None,
                 total3: Optional[torch.Tensor] = None, weights3: Optional[torch.Tensor] = None,
                 grads: Optional[torch.Tensor] = None, want_dprop: bool = False,
                 node_weights: Optional[torch.Tensor] = None, norm=None, dprop: Optional[torch.Tensor] = None):
    """bce (or its accumulating form) then backward in one library call (spwgnn_bce_backward, ABI 6):
    bit-identical to the two calls; on the fused small-batch loop the loss needs no launch of its own.
    With `node_weights` / `norm` (see `bce`) the weighted loss (spwgnn_bce_backward_weighted), whose
    loss launch always runs first. ``logits`` holds one value per node of the batch (the folded loss indexes
    it by plan node). ``dprop`` as in `backward`. Returns (out3, dlogits, grads, dprop)."""
    if logits.numel() != batch.n_nodes:
        raise ValueError(f"logits must hold one value per node of the batch ({batch.n_nodes}), got {logits.numel()}")
    _training_forward(ws, batch, run)
    targets = targets.reshape(-1).to(torch.float32).contiguous()
    _require_gpu(logits, "logits")
    if dlogits is None:
        dlogits = _poison(torch.empty_like(logits))
    if grads is None:
        grads = _poison(torch.empty_like(flat_params))
    _check_sums(total3, weights3)
    dprop = _dprop_buffer(batch, dprop, want_dprop)
    b = batch.cstruct()
    r = run.cstruct()
    buf = ws.buf
    args = (flat_params.data_ptr(), C.byref(b), C.byref(r), buf.data_ptr(), buf.numel(), logits.data_ptr(),
            targets.data_ptr(), logits.numel(), scratch.out3.data_ptr(), dlogits.data_ptr(), scratch.scratch.data_ptr(),
            weights3.data_ptr() if weights3 is not None else None, total3.data_ptr() if total3 is not None else None,
            grads.data_ptr(), dprop.data_ptr() if dprop is not None else None)
    if node_weights is None:
        if norm is not None:
            raise ValueError("norm goes with node_weights")
        st = _lib.lib().spwgnn_bce_backward(*args, _stream(batch.device))
        what = "spwgnn_bce_backward"
    else:
        lw, _keep = _loss_weights(node_weights, norm, logits)
        st = _lib.lib().spwgnn_bce_backward_weighted(*args, C.byref(lw), _stream(batch.device))
        what = "spwgnn_bce_backward_weighted"
    ws.bwd_key = ws.fwd_key if st == 0 else None
    _lib.check(st, what)
    return scratch.out3, dlogits, grads, dprop


def _loss_weights(node_weights: torch.Tensor, norm, logits: torch.Tensor):
    """spwgnn_loss_weights of `node_weights` (one fp32 per logit, on the logits' device) and `norm`: a
    number, a one-element device fp32 tensor (read on the device: a replayed step refills it), or None =
    max(#non-zero weights, 1), counted here. Returns the struct and what it points into."""
    _require_gpu(node_weights, "node_weights")
    w = node_weights.reshape(-1)
    if w.dtype != torch.float32 or not w.is_contiguous():
        w = w.to(torch.float32).contiguous()
    if w.numel() != logits.numel() or w.device != logits.device:
        raise ValueError(f"node_weights must hold one weight per logit on {logits.device} "
                         f"(got {w.numel()} on {w.device} for {logits.numel()} logits)")
    lw = _lib.LossWeightsC()
    lw.w = w.data_ptr()
    if norm is None:
        norm = max(int(torch.count_nonzero(w).item()), 1)   # one host sync
    if isinstance(norm, torch.Tensor):
        _require_gpu(norm, "norm")
        if norm.dtype != torch.float32 or norm.numel() != 1 or norm.device != logits.device:
            raise ValueError("a device norm is one fp32 element on the logits' device")
        lw.norm_dev = norm.data_ptr()
    else:
        if not float(norm) > 0:
            raise ValueError(f"norm must be > 0 (got {norm}); pass max(count of non-zero weights, 1)")
        lw.norm = float(norm)
    return lw, (w, norm)


class BceScratch:
    def __init__(self, device):
        n = int(_lib.lib().spwgnn_bce_scratch_bytes(1))
        self.scratch = torch.empty(n, dtype=torch.uint8, device=device)
        self.out3 = torch.empty(3, dtype=torch.float32, device=device)


def bce(logits: torch.Tensor, targets: torch.Tensor, scratch: BceScratch, dlogits: Optional[torch.Tensor] = None,
        total3: Optional[torch.Tensor] = None, weights3: Optional[torch.Tensor] = None,
        node_weights: Optional[torch.Tensor] = None, norm=None):
    """Keras binary_crossentropy (+ binary_accuracy numerator) and d loss / d logit on device.
    Returns out3 = [loss, n_correct, n] (device) and dlogits. With total3/weights3 (float64) the
    same launch also does total3 += out3.double() * weights3 (spwgnn_bce_accumulate).

    `node_weights` (device fp32, one per logit, in the targets' order): the per-node weighted loss of
    Keras 2.x (spwgnn_bce_weighted) — loss = Σ w·bce / norm, dlogits = w·(σ(z) − t) / norm. A zero weight
    masks its node: it adds 0 to the loss, gets dlogit 0 and is not counted, whatever its logit and
    target hold (NaN included). out3 is then [loss, correct among the nodes with w ≠ 0, their number] —
    with zeros an accuracy over the nodes that count, where Keras's `metrics=` stay unweighted.
    `norm`: a number, a one-element device fp32 tensor (read on the device), or None = the number of
    non-zero weights, at least 1, counted here with one host sync. Keras divides by that count itself
    and gives NaN (0/0) for an all-zero batch; here such a batch gives loss 0 and zero gradients.
    `weights3` stays the epoch-sum weights of the accumulating form."""
    targets = targets.reshape(-1).to(torch.float32).contiguous()
    if dlogits is None:
        dlogits = _poison(torch.empty_like(logits))
    _check_sums(total3, weights3)
    if node_weights is not None:
        lw, _keep = _loss_weights(node_weights, norm, logits)
        st = _lib.lib().spwgnn_bce_weighted(
            logits.data_ptr(), targets.data_ptr(), logits.numel(), C.byref(lw), scratch.out3.data_ptr(),
            dlogits.data_ptr(), scratch.scratch.data_ptr(), weights3.data_ptr() if weights3 is not None else None,
            total3.data_ptr() if total3 is not None else None, _stream(logits.device))
        _lib.check(st, "spwgnn_bce_weighted")
        return scratch.out3, dlogits
    if norm is not None:
        raise ValueError("norm goes with node_weights")
    args = (logits.data_ptr(), targets.data_ptr(), logits.numel(), scratch.out3.data_ptr(), dlogits.data_ptr(),
            scratch.scratch.data_ptr())
    if total3 is None:
        st = _lib.lib().spwgnn_bce(*args, _stream(logits.device))
        _lib.check(st, "spwgnn_bce")
    else:
        st = _lib.lib().spwgnn_bce_accumulate(*args, weights3.data_ptr(), total3.data_ptr(), _stream(logits.device))
        _lib.check(st, "spwgnn_bce_accumulate")
    return scratch.out3, dlogits


def check_tower_loss(tower_loss, node_loss=1.0) -> tuple:
    """(mu, alpha) of the tower-level loss L = alpha·L_node + mu·L_tower: mu finite and >= 0 (0 = the
    tower term is off and every front end runs the launches it ran without it), alpha finite and >= 0."""
    mu, alpha = float(tower_loss), float(node_loss)
    if not (0.0 <= mu < float("inf")) or not (0.0 <= alpha < float("inf")):   # False for a NaN
        raise ValueError(f"tower_loss and node_loss must be finite and >= 0 (got {tower_loss}, {node_loss})")
    return mu, alpha


def counted_towers(batch: TowerBatch, node_weights: Optional[torch.Tensor] = None) -> int:
    """The towers of `batch` with at least one counted node — the tower loss's divisor norm_t. Without
    weights a host count; with weights one host sync."""
    if node_weights is None:
        return int((batch.tower_nodes > 0).sum())
    return counted_nodes_towers(batch, node_weights)[1]


def counted_nodes_towers(batch: TowerBatch, node_weights: torch.Tensor) -> tuple:
    """(nodes with a non-zero weight, towers holding one) of `batch`, read with one host sync."""
    nz = (node_weights.reshape(-1) != 0).to(torch.int64)
    on = torch.cat([nz.new_zeros(1), nz.cumsum(0)])
    off = batch.tower_offsets.to(on.device, torch.int64)
    k, t = torch.stack([on[-1], ((on[off[1:]] - on[off[:-1]]) > 0).sum()]).tolist()
    return int(k), int(t)


class TowerLossScratch:
    """The buffers of `bce_tower`: its scratch, out3 = [L, node correct, node count] and out6 = [L_node, node
    correct, node count, L_tower, towers correct, towers counted]; with ``totals`` the fp64 epoch sums
    total6 += out6 · weights6 of the same launch (weights6 preset to ones)."""

    def __init__(self, device, totals: bool = False):
        n = int(_lib.lib().spwgnn_bce_tower_scratch_bytes(1, 1))
        self.scratch = torch.empty(n, dtype=torch.uint8, device=device)
        self.out3 = torch.empty(3, dtype=torch.float32, device=device)
        self.out6 = torch.empty(6, dtype=torch.float32, device=device)
        self.total6 = torch.zeros(6, dtype=torch.float64, device=device) if totals else None
        self.weights6 = torch.ones(6, dtype=torch.float64, device=device) if totals else None


def bce_tower(logits: torch.Tensor, targets: Optional[torch.Tensor], batch: TowerBatch, scratch: TowerLossScratch,
              tower_loss: float = 1.0, node_loss: float = 1.0, tower_targets: Optional[torch.Tensor] = None,
              norm_t=None, dlogits: Optional[torch.Tensor] = None, node_weights: Optional[torch.Tensor] = None,
              norm=None, total6: Optional[torch.Tensor] = None, weights6: Optional[torch.Tensor] = None,
              per_tower: Optional[torch.Tensor] = None, want_dlogits: bool = True):
    """The combined objective L = node_loss·L_node + tower_loss·L_tower and d L / d logit on the device
    (spwgnn_bce_tower; the exact definition is in include/spwgnn.h). L_node is `bce`'s loss (with
    `node_weights` / `norm`, its weighted one); L_tower is the binary cross-entropy of "every counted block of
    the tower stands", P_u = Π σ(z_i), against the tower's label: ``tower_targets`` ((n_towers,) 0/1, in the
    PLAN's tower order: `TowerBatch.towers_to_plan_order`) or, when None, 1 iff every counted node target is 1.
    A zero node weight masks its node out of its tower as well; a tower without a counted node is skipped.
    ``norm_t``: the tower divisor — a number, a one-element device fp32 tensor, or None = the towers with a
    counted node (`counted_towers`; with weights one host sync). ``targets`` may be None for tower-only labels
    (node_loss 0 and tower_targets given). ``logits`` and ``targets`` are in the plan's node order.
    Returns (out3, dlogits); scratch.out6 holds the six parts. ``per_tower``: an (n_towers,) fp32 buffer for
    the per-tower losses. ``want_dlogits`` False: the loss only (evaluation)."""
    _require_gpu(logits, "logits")
    mu, alpha = check_tower_loss(tower_loss, node_loss)
    if not mu > 0:
        raise ValueError("bce_tower needs tower_loss > 0; without the tower term use bce")
    if logits.dim() != 1 or logits.dtype != torch.float32 or not logits.is_contiguous():
        raise ValueError("logits must be a contiguous fp32 (n,) tensor")
    n, T = int(logits.numel()), int(batch.n_towers)
    if n != batch.n_nodes:
        raise ValueError(f"logits must hold one value per node of the batch ({batch.n_nodes}), got {n}")
    if targets is None:
        if alpha != 0 or tower_targets is None:
            raise ValueError("targets may be None only with node_loss == 0 and tower_targets given")
    else:
        targets = targets.reshape(-1).to(torch.float32).contiguous()
        if targets.numel() != n or targets.device != logits.device:
            raise ValueError(f"targets must hold one value per node ({n}) on {logits.device}")
    off = batch.tower_offsets
    if off.device != logits.device or off.dtype != torch.int32 or off.numel() != T + 1:
        raise ValueError("the batch's tower offsets must be (n_towers + 1,) int32 on the logits' device")
    tl = _lib.TowerLossC()
    tl.n_towers, tl.tower_offsets, tl.alpha, tl.mu = T, off.data_ptr(), alpha, mu
    if tower_targets is not None:
        tower_targets = tower_targets.reshape(-1).to(torch.float32).contiguous()
        if tower_targets.numel() != T or tower_targets.device != logits.device:
            raise ValueError(f"tower_targets must hold one value per tower ({T}) on {logits.device}")
        tl.tower_targets = tower_targets.data_ptr()
    lw = keep = None
    if node_weights is not None:
        lw, keep = _loss_weights(node_weights, norm, logits)
    elif norm is not None:
        raise ValueError("norm goes with node_weights")
    if norm_t is None:
        norm_t = max(counted_towers(batch, keep[0] if keep else None), 1)
    if isinstance(norm_t, torch.Tensor):
        if norm_t.dtype != torch.float32 or norm_t.numel() != 1 or norm_t.device != logits.device:
            raise ValueError("a device norm_t is one fp32 element on the logits' device")
        tl.norm_t_dev = norm_t.data_ptr()
    else:
        if not float(norm_t) > 0:
            raise ValueError(f"norm_t must be > 0 (got {norm_t}); pass max(counted towers, 1)")
        tl.norm_t = float(norm_t)
    if (total6 is None) != (weights6 is None):
        raise ValueError("total6 and weights6 go together")
    if total6 is not None:
        assert total6.dtype == torch.float64 and weights6.dtype == torch.float64 and total6.numel() == 6 == weights6.numel()
        tl.total6, tl.weights6 = total6.data_ptr(), weights6.data_ptr()
    if per_tower is not None:
        _out_buffer(per_tower, (T,), "per_tower")
        tl.per_tower = per_tower.data_ptr()
    tl.out6 = scratch.out6.data_ptr()
    if want_dlogits and dlogits is None:
        dlogits = _poison(torch.empty_like(logits))
    st = _lib.lib().spwgnn_bce_tower(
        logits.data_ptr(), targets.data_ptr() if targets is not None else None, n, C.byref(lw) if lw is not None else None,
        C.byref(tl), scratch.out3.data_ptr(), dlogits.data_ptr() if want_dlogits else None, scratch.scratch.data_ptr(),
        _stream(logits.device))
    _lib.check(st, "spwgnn_bce_tower")
    return scratch.out3, (dlogits if want_dlogits else None)


def check_step_weights(step_loss_weights, mp_steps: int):
    """Validates per-step loss weights λ (deep supervision): ``mp_steps`` finite floats >= 0, not all zero
    — the rules spwgnn_bce_steps refuses by. Returns them as a tuple of floats."""
    import math
    lam = tuple(float(x) for x in step_loss_weights)
    if len(lam) != int(mp_steps):
        raise ValueError(f"step_loss_weights needs one weight per propagation step ({mp_steps}), got {len(lam)}")
    if any(not math.isfinite(x) or x < 0.0 for x in lam):
        raise ValueError(f"step_loss_weights must be finite and >= 0 (got {lam})")
    if not any(x != 0.0 for x in lam):
        raise ValueError("step_loss_weights must not be all zero")
    return lam


class BceStepsScratch:
    """Device buffers of `bce_steps` for ``mp_steps`` rows: the partial sums
    (spwgnn_bce_steps_scratch_bytes), out3 (the combined row) and out3s (mp_steps, 3)."""

    def __init__(self, device, mp_steps: int):
        n = int(_lib.lib().spwgnn_bce_steps_scratch_bytes(1, int(mp_steps)))
        if n < 0:
            raise ValueError(f"mp_steps must be in 1..{_lib.MAX_STEPS} (got {mp_steps})")
        self.mp_steps = int(mp_steps)
        self.scratch = torch.empty(n, dtype=torch.uint8, device=device)
        self.out3 = torch.empty(3, dtype=torch.float32, device=device)
        self.out3s = torch.empty(self.mp_steps, 3, dtype=torch.float32, device=device)


def bce_steps(step_logits: torch.Tensor, targets: torch.Tensor, step_weights, scratch: BceStepsScratch,
              dlogits: Optional[torch.Tensor] = None, total3: Optional[torch.Tensor] = None,
              weights3: Optional[torch.Tensor] = None, total3s: Optional[torch.Tensor] = None,
              node_weights: Optional[torch.Tensor] = None, norm=None):
    """The deep-supervision loss Σ_s λ_s·BCE(z_s, t) over the rows of `forward_steps` in one launch
    (spwgnn_bce_steps). ``step_weights``: mp_steps floats λ_s >= 0, not all zero. Returns
    ``(out3, out3s, dlogits)``: out3 = [Σ_s λ_s·loss_s, correct of the last step, n]; out3s (mp_steps, 3) =
    each step's [loss, correct, n] as `bce` computes them; dlogits (mp_steps, n), row s = λ_s · `bce`'s
    dlogits of row s (+0 where λ_s = 0, whatever the row holds) — what `backward_steps` takes. With
    λ = (0, …, 0, 1) out3 and the last dlogits row are `bce`'s bits. ``node_weights`` / ``norm`` as in `bce`;
    ``total3`` / ``weights3`` accumulate out3, ``total3s`` ((mp_steps, 3) float64, with them) out3s."""
    _require_gpu(step_logits, "step_logits")
    if step_logits.dim() != 2 or step_logits.dtype != torch.float32 or not step_logits.is_contiguous():
        raise ValueError("step_logits must be a contiguous fp32 (mp_steps, n) tensor")
    S, n = int(step_logits.shape[0]), int(step_logits.shape[1])
    if S != scratch.mp_steps:
        raise ValueError(f"the scratch was built for {scratch.mp_steps} steps, step_logits holds {S}")
    sw = _lib.StepWeightsC()
    lam = [float(x) for x in step_weights]
    sw.count = len(lam)
    for s, x in enumerate(lam[:_lib.MAX_STEPS]):
        sw.lam[s] = x
    targets = targets.reshape(-1).to(torch.float32).contiguous()
    if targets.numel() != n:
        raise ValueError(f"targets must hold one value per node ({n}), got {targets.numel()}")
    if dlogits is None:
        dlogits = _poison(torch.empty_like(step_logits))
    elif tuple(dlogits.shape) != (S, n) or dlogits.dtype != torch.float32 or not dlogits.is_contiguous():
        raise ValueError(f"dlogits must be a contiguous fp32 ({S}, {n}) tensor")
    _check_sums(total3, weights3)
    if total3s is not None and total3 is None:
        raise ValueError("total3s goes with total3 and weights3")
    for t, shp in ((total3, (3,)), (weights3, (3,)), (total3s, (S, 3))):
        if t is not None and (t.dtype != torch.float64 or tuple(t.shape) != shp or not t.is_contiguous()):
            raise ValueError(f"the epoch sums are contiguous float64 tensors of shape {shp}")
    lw, _keep = (None, None)
    if node_weights is not None:
        lw, _keep = _loss_weights(node_weights, norm, step_logits[0])
    elif norm is not None:
        raise ValueError("norm goes with node_weights")
    st = _lib.lib().spwgnn_bce_steps(
        step_logits.data_ptr(), targets.data_ptr(), n, S, C.byref(sw), C.byref(lw) if lw is not None else None,
        scratch.out3s.data_ptr(), scratch.out3.data_ptr(), dlogits.data_ptr(), scratch.scratch.data_ptr(),
        weights3.data_ptr() if weights3 is not None else None, total3.data_ptr() if total3 is not None else None,
        total3s.data_ptr() if total3s is not None else None, _stream(step_logits.device))
    _lib.check(st, "spwgnn_bce_steps")
    return scratch.out3, scratch.out3s, dlogits


def adam(params: torch.Tensor, grads: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: int, lr=5e-4,
         beta1=0.9, beta2=0.999, eps=1e-7, l2=0.0, grad_scale=1.0):
    st = _lib.lib().spwgnn_adam(params.data_ptr(), grads.data_ptr(), m.data_ptr(), v.data_ptr(), params.numel(),
                                int(step), lr, beta1, beta2, eps, l2, grad_scale, _stream(params.device))
    _lib.check(st, "spwgnn_adam")


def adam_dev(params: torch.Tensor, grads: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step_dev: torch.Tensor,
             lr_table: torch.Tensor, beta1=0.9, beta2=0.999, eps=1e-7, l2=0.0, grad_scale=1.0):
    """Adam with the step count read from the device word `step_dev` ((1,) int32) and lr_t from
    `lr_table` (device fp32, built by `adam_lr_table`): capturable into a replayed hipGraph."""
    st = _lib.lib().spwgnn_adam_dev(params.data_ptr(), grads.data_ptr(), m.data_ptr(), v.data_ptr(), params.numel(),
                                    step_dev.data_ptr(), lr_table.data_ptr(), lr_table.numel(), beta1, beta2, eps, l2,
                                    grad_scale, _stream(params.device))
    _lib.check(st, "spwgnn_adam_dev")


def adam_lr_table(n: int, lr=5e-4, beta1=0.9, beta2=0.999, device="cuda", decay=0.0) -> torch.Tensor:
    """lr_t of steps 0..n-1 (host-built with spwgnn_adam's own expression), on the device. `decay`
    (Keras 2.x Adam's): entry t is built from lr / (1 + decay·(t − 1)) (spwgnn_adam_lr_table_decay); a
    replayed step past the table's last entry keeps that entry, so the decay freezes there."""
    import numpy as np
    out = np.zeros(int(n), np.float32)
    if decay:
        _lib.check(_lib.lib().spwgnn_adam_lr_table_decay(lr, decay, beta1, beta2, int(n), out.ctypes.data),
                   "spwgnn_adam_lr_table_decay")
    else:
        _lib.check(_lib.lib().spwgnn_adam_lr_table(lr, beta1, beta2, int(n), out.ctypes.data), "spwgnn_adam_lr_table")
    return torch.from_numpy(out).to(device)


def adam_lr_decayed(lr: float, decay: float, iterations: int) -> float:
    """Keras 2.x Adam's decayed learning rate lr / (1 + decay·iterations) as the library rounds it to
    fp32 (spwgnn_adam_lr_decayed); `iterations` = the steps already taken, 0 at the first."""
    return float(_lib.lib().spwgnn_adam_lr_decayed(lr, decay, int(iterations)))


def check_clip_options(clipnorm=0.0, clipvalue=0.0, decay=0.0) -> bool:
    """Validates the optimizer options of the front ends (each >= 0 and not NaN; 0 = off). Returns
    whether clipnorm or clipvalue is set."""
    for name, val in (("clipnorm", clipnorm), ("clipvalue", clipvalue), ("decay", decay)):
        if not float(val) >= 0.0:
            raise ValueError(f"{name} must be >= 0 (got {val}); 0 turns it off")
    return bool(clipnorm or clipvalue)


class ClipScratch:
    """Device buffers of a clipped Adam step: the partial sums of Σg'² (spwgnn_clip_scratch_bytes), the
    step's out4 = [norm, scale, skipped, clipped] and, with `totals`, the fp64 sums total4 = [Σ norm over
    the non-skipped steps, Σ clipped, Σ skipped, Σ steps] the update kernel adds to."""

    def __init__(self, device, totals: bool = False):
        n = int(_lib.lib().spwgnn_clip_scratch_bytes())
        self.scratch = torch.empty(n, dtype=torch.uint8, device=device)
        self.out4 = torch.zeros(4, dtype=torch.float32, device=device)
        self.total4 = torch.zeros(4, dtype=torch.float64, device=device) if totals else None

    def cstruct(self, clipnorm, clipvalue, skip_nonfinite, accumulate: bool) -> _lib.ClipC:
        c = _lib.ClipC()
        c.clipnorm, c.clipvalue = float(clipnorm), float(clipvalue)
        c.skip_nonfinite = 1 if skip_nonfinite else 0
        c.out4 = self.out4.data_ptr()
        if accumulate:
            if self.total4 is None:
                raise ValueError("ClipScratch was built without totals")
            c.total4 = self.total4.data_ptr()
        return c


def adam_clipped(params: torch.Tensor, grads: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: int,
                 clip: ClipScratch, lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-7, l2=0.0, grad_scale=1.0,
                 clipnorm=0.0, clipvalue=0.0, skip_nonfinite=False, accumulate=False) -> torch.Tensor:
    """`adam` on g' clipped as Keras 2.x's Optimizer.get_gradients does (spwgnn_adam_clipped): by the
    global norm of g' = grad_scale·grad + 2·l2·param over the real parameters (`clipnorm`), then by value
    (`clipvalue`); `skip_nonfinite`: a step whose Σg'² is not finite leaves params, m and v untouched.
    One launch more than `adam`; `grads` is not modified. `lr` is the step's own (a decayed one comes
    from `adam_lr_decayed`). Returns clip.out4 = [norm, scale, skipped, clipped] (device);
    `accumulate` also adds the step to clip.total4."""
    _require_gpu(params, "params")
    c = clip.cstruct(clipnorm, clipvalue, skip_nonfinite, accumulate)
    st = _lib.lib().spwgnn_adam_clipped(params.data_ptr(), grads.data_ptr(), m.data_ptr(), v.data_ptr(),
                                        params.numel(), int(step), lr, beta1, beta2, eps, l2, grad_scale, C.byref(c),
                                        clip.scratch.data_ptr(), _stream(params.device))
    _lib.check(st, "spwgnn_adam_clipped")
    return clip.out4


def adam_clipped_dev(params: torch.Tensor, grads: torch.Tensor, m: torch.Tensor, v: torch.Tensor,
                     step_dev: torch.Tensor, lr_table: torch.Tensor, clip: ClipScratch, beta1=0.9, beta2=0.999,
                     eps=1e-7, l2=0.0, grad_scale=1.0, clipnorm=0.0, clipvalue=0.0, skip_nonfinite=False,
                     accumulate=False) -> torch.Tensor:
    """`adam_clipped` with the step count read from `step_dev` and lr_t from `lr_table` (`adam_dev`'s
    arguments): capturable into a replayed hipGraph. A skipped step still reads the advanced step word:
    the iteration count moves on whether or not the update was applied."""
    _require_gpu(params, "params")
    c = clip.cstruct(clipnorm, clipvalue, skip_nonfinite, accumulate)
    st = _lib.lib().spwgnn_adam_clipped_dev(params.data_ptr(), grads.data_ptr(), m.data_ptr(), v.data_ptr(),
                                            params.numel(), step_dev.data_ptr(), lr_table.data_ptr(),
                                            lr_table.numel(), beta1, beta2, eps, l2, grad_scale, C.byref(c),
                                            clip.scratch.data_ptr(), _stream(params.device))
    _lib.check(st, "spwgnn_adam_clipped_dev")
    return clip.out4


def step_advance(key_dev: torch.Tensor, step_dev: torch.Tensor, mode: int = _lib.STEP_KEY_COUNTER, seed: int = 0,
                 rank: int = 0):
    """Start a replayable step on the device: step += 1, dropout key moved on (spwgnn.h)."""
    st = _lib.lib().spwgnn_step_advance(key_dev.data_ptr(), step_dev.data_ptr(), int(mode),
                                        int(seed) & 0xFFFFFFFFFFFFFFFF, int(rank), _stream(key_dev.device))
    _lib.check(st, "spwgnn_step_advance")


def accumulate_out3(total3: torch.Tensor, out3: torch.Tensor, weights3: torch.Tensor) -> None:
    """total3 += out3.double() * weights3 (three float64 sums on the device) in one launch."""
    assert total3.dtype == torch.float64 and weights3.dtype == torch.float64 and out3.dtype == torch.float32
    st = _lib.lib().spwgnn_accumulate_out3(out3.data_ptr(), weights3.data_ptr(), total3.data_ptr(), _stream(out3.device))
    _lib.check(st, "spwgnn_accumulate_out3")


def copy_in(host: torch.Tensor, dev: torch.Tensor, nbytes: int, src_dev_ptr: Optional[int] = None) -> None:
    """dev[:nbytes] ← host[:nbytes] by a kernel on the current stream (spwgnn_copy_in): `host` a pinned
    (device-mapped) tensor, read at `src_dev_ptr` (its device address) when given. Captured into a
    graph it is one kernel node, not a DMA copy."""
    if not host.is_pinned():
        raise ValueError("copy_in reads pinned host memory")
    _require_gpu(dev, "copy_in destination")
    if nbytes > host.numel() * host.element_size() or nbytes > dev.numel() * dev.element_size():
        raise ValueError("copy_in beyond a buffer")
    src = src_dev_ptr if src_dev_ptr is not None else host.data_ptr()
    st = _lib.lib().spwgnn_copy_in(src, dev.data_ptr(), int(nbytes), _stream(dev.device))
    _lib.check(st, "spwgnn_copy_in")


def sigmoid(logits: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sigmoid(logits) (spwgnn_sigmoid); ``out``: the buffer to write to, of the logits' shape."""
    if out is None:
        out = torch.empty_like(logits)
    else:
        _out_buffer(out, tuple(logits.shape), "out")
    st = _lib.lib().spwgnn_sigmoid(logits.data_ptr(), out.data_ptr(), logits.numel(), _stream(logits.device))
    _lib.check(st, "spwgnn_sigmoid")
    return out


READOUT_MODES = {"sum_prob": _lib.READOUT_SUM_PROB, "mean_prob": _lib.READOUT_MEAN_PROB,
                 "sum_logit": _lib.READOUT_SUM_LOGIT, "mean_logit": _lib.READOUT_MEAN_LOGIT}


def tower_readout(logits: torch.Tensor, batch: TowerBatch, mode: str = "sum_prob",
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(T,) per-tower reduction of the node logits on device: "sum_prob" is the Σŷ stability score of
    JengaBuilder.remove_to_demolish (JengaBuilder.py:252-256); "mean_prob" the optional GlobalBlock
    mean pool (not in the reference). ``out``: the (n_towers,) buffer to write to."""
    if mode not in READOUT_MODES:
        raise ValueError(f"readout mode must be one of {sorted(READOUT_MODES)}")
    _require_gpu(logits, "logits")
    logits = logits.reshape(-1).contiguous().to(torch.float32)
    if logits.numel() != batch.n_nodes:
        raise ValueError("logits must hold one value per node of the batch")
    if out is None:
        out = torch.empty(batch.n_towers, dtype=torch.float32, device=logits.device)
    else:
        _out_buffer(out, (batch.n_towers,), "out")
    st = _lib.lib().spwgnn_tower_readout(logits.data_ptr(), batch.tower_offsets.data_ptr(), batch.n_towers,
                                         READOUT_MODES[mode], out.data_ptr(), _stream(logits.device))
    _lib.check(st, "spwgnn_tower_readout")
    return out


class EvalTables:
    """The int64 tables spwgnn_eval_metrics adds to (include/spwgnn.h), as views of ONE flat buffer — a
    data-parallel run sums them over the ranks with one all-reduce of `flat`:
      node4   (rows, 4)        TP, TN, FP, FN over the counted nodes
      tower6  (rows, 6)        towers, exact, tTP, tTN, tFP, tFN          (``towers``)
      by_size (rows, 33, 6)    TP, TN, FP, FN, towers, exact per tower size (``towers``)
      hist    (rows, 2, 256)   the logit histogram per class               (``hist``)
    ``rows``: 1, or mp_steps for the rows of `forward_steps`. Any device (the oracle engines of the CPU
    suite keep theirs on the host)."""

    def __init__(self, device, rows: int = 1, towers: bool = True, hist: bool = True):
        if not 1 <= int(rows) <= _lib.MAX_STEPS:
            raise ValueError(f"rows must be in 1..{_lib.MAX_STEPS} (got {rows})")
        self.rows, self.towers, self.has_hist = int(rows), bool(towers), bool(hist)
        shapes = {"node4": (self.rows, 4)}
        if self.towers:
            shapes.update(tower6=(self.rows, 6), by_size=(self.rows, _lib.EVAL_SIZES, 6))
        if self.has_hist:
            shapes["hist"] = (self.rows, 2, _lib.EVAL_BINS)
        sizes = {k: int(torch.Size(s).numel()) for k, s in shapes.items()}
        self.flat = torch.zeros(sum(sizes.values()), dtype=torch.int64, device=device)
        self.tables, at = {}, 0
        for k, s in shapes.items():
            self.tables[k] = self.flat[at:at + sizes[k]].view(s)
            at += sizes[k]
        self.node4 = self.tables["node4"]
        self.tower6, self.by_size, self.hist = (self.tables.get(k) for k in ("tower6", "by_size", "hist"))

    def zero_(self) -> "EvalTables":
        self.flat.zero_()
        return self

    def add_(self, other: "EvalTables") -> "EvalTables":
        if (other.rows, other.towers, other.has_hist) != (self.rows, self.towers, self.has_hist):
            raise ValueError("add_ needs tables of the same rows and parts")
        self.flat.add_(other.flat.to(self.flat.device))
        return self

    def cpu(self) -> dict:
        """{name: numpy int64 array} of the tables held (one device read)."""
        return self.split(self.flat.cpu())

    def split(self, host: torch.Tensor) -> dict:
        """`cpu()` of a host copy of `flat` the caller made (together with other results, in one read)."""
        out, at = {}, 0
        for k, t in self.tables.items():
            out[k] = host[at:at + t.numel()].view(t.shape).numpy().copy()
            at += t.numel()
        return out


def check_threshold(threshold) -> float:
    """The decision threshold of the evaluation calls: a finite float with 0 < tau < 1."""
    tau = float(threshold)
    if not 0.0 < tau < 1.0:   # False for a NaN
        raise ValueError(f"threshold must lie strictly between 0 and 1 (got {threshold})")
    return tau


def eval_metrics(logits: torch.Tensor, targets: torch.Tensor, tables: EvalTables, batch: Optional[TowerBatch] = None,
                 node_weights: Optional[torch.Tensor] = None, threshold: float = 0.5) -> EvalTables:
    """Adds the evaluation counts of ``logits`` against ``targets`` to ``tables`` on the device, in one launch
    and without a host sync (spwgnn_eval_metrics). ``logits``: (n,) or (R, n) contiguous fp32, R =
    tables.rows (the rows of `forward_steps`); ``targets``: one 0/1 value per node, in the logits' order
    (for packed plans the plan's: `TowerBatch.to_plan_order`). ``batch`` gives the tower offsets and is
    required when the tables hold the tower parts. ``node_weights``: one weight per node; a zero masks
    the node out of every table. ``threshold``: the node is predicted stable when sigmoid(z) > threshold."""
    _require_gpu(logits, "logits")
    if logits.dim() not in (1, 2) or logits.dtype != torch.float32 or not logits.is_contiguous():
        raise ValueError("logits must be a contiguous fp32 (n,) or (rows, n) tensor")
    R, n = (1, int(logits.shape[0])) if logits.dim() == 1 else (int(logits.shape[0]), int(logits.shape[1]))
    if not isinstance(tables, EvalTables) or tables.rows != R:
        raise ValueError(f"tables must be EvalTables built for {R} row(s)")
    if tables.flat.device != logits.device:
        raise ValueError(f"the tables must be on the logits' device {logits.device} (got {tables.flat.device})")
    if n < 1:
        raise ValueError("logits holds no node")
    tau = check_threshold(threshold)
    targets = targets.reshape(-1).to(torch.float32).contiguous()
    if targets.numel() != n or targets.device != logits.device:
        raise ValueError(f"targets must hold one value per node ({n}) on {logits.device}, got {targets.numel()} on "
                         f"{targets.device}")
    ev = _lib.EvalC()
    ev.rows, ev.threshold = R, tau
    w = None
    if node_weights is not None:
        _require_gpu(node_weights, "node_weights")
        w = node_weights.reshape(-1).to(torch.float32).contiguous()
        if w.numel() != n or w.device != logits.device:
            raise ValueError(f"node_weights must hold one weight per node ({n}) on {logits.device}")
        ev.w = w.data_ptr()
    off = None
    if tables.towers:
        if batch is None:
            raise ValueError("tables with the tower parts need the batch (its tower offsets)")
        if batch.n_nodes != n:
            raise ValueError(f"the batch holds {batch.n_nodes} nodes, the logits {n}")
        off = batch.tower_offsets
        if off.device != logits.device or off.dtype != torch.int32 or off.numel() != batch.n_towers + 1:
            raise ValueError("the batch's tower offsets must be (n_towers + 1,) int32 on the logits' device")
        ev.n_towers, ev.tower_offsets = int(batch.n_towers), off.data_ptr()
        ev.tower6, ev.by_size = tables.tower6.data_ptr(), tables.by_size.data_ptr()
    ev.node4 = tables.node4.data_ptr()
    if tables.has_hist:
        ev.hist = tables.hist.data_ptr()
    st = _lib.lib().spwgnn_eval_metrics(logits.data_ptr(), targets.data_ptr(), n, C.byref(ev), _stream(logits.device))
    _lib.check(st, "spwgnn_eval_metrics")
    return tables
