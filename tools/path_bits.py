"""Every output of every workspace entry point as bit patterns, on the suite's smallest shapes either side of
each path choice of the host launch code (csrc/path.h), so two builds of the library (SPWGNN_LIB) can be
compared bit for bit with tools/cmp_npz.py. It runs tests/test_gpu_guard.py's call
sequence (_sequence with the engine's own buffers: forward, forward_state, forward_steps, bce_steps,
backward_steps, backward_inputs, the readouts, bce_backward, backward_state, Adam) under the suite's team
limit: every shape in x6 and f32, ALL_MATH_SHAPES in bf16 / x3 / h3, DROPOUT_SHAPES with dropout 0.1, each
at S = 1 and 3. On n6x5 (fused loops) and wide138 (wide kernels), in x6 and bf16, it adds the same sequence
with a null `prop` (the loop-end shortcuts), a backward of a null prop without dprop (step 0's edge
backward left out) and backwards with grads_early_event set (the split order). Arrays are stored as
unsigned integers of their width: a NaN compares equal to the same NaN.
usage: [SPWGNN_LIB=...] python tools/path_bits.py OUT.npz"""
import copy
import os
import sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_gpu_guard as GD
import test_gpu_state as TS
from spwgnn_amd import TowerBatch, engine as E, params as P

out = {}


def put(tag, arrays):
    for k, a in arrays.items():
        if isinstance(a, np.ndarray):
            a = np.ascontiguousarray(a)
            out[f"{tag}/{k}"] = a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def sequence(case, math, S, rate, tag):
    with TS._limit(case.wide):
        put(f"{tag}_{math}_S{S}_d{rate}", GD._sequence(case, math, S, rate, None, weighted=case.name == "n6x5"))


def backwards(case, math, tag):
    """A training forward, the loss, then backwards the sequence does not make: without dprop, and with the
    early-gradient event."""
    S = 3
    with TS._limit(case.wide):
        batch = TowerBatch.from_plan(case.host_plan(), GD.DEV)
        flat = P.to_flat(GD._params(False)).to(GD.DEV)
        tgt = torch.as_tensor(batch.to_plan_order(case.tgt)).to(GD.DEV)
        ev = torch.cuda.Event()
        ev.record()
        for early in (False, True):
            run = E.RunConfig(S, training=True, math=math, dropout=0.1, seed=GD.DROP_SEED,
                              grads_early_event=ev if early else None)
            ws = E.Workspace(GD.DEV)
            z = E.forward(flat, batch, run, ws)
            _, dz = E.bce(z, tgt, E.BceScratch(GD.DEV))
            for want in (False, True):
                g, dp = E.backward(flat, batch, run, ws, dz, want_dprop=want)
                torch.cuda.synchronize()
                put(f"{tag}_{math}_early{int(early)}_dprop{int(want)}", {"z": GD._np(z), "g": GD._np(g), "dprop": GD._np(dp)})
            o3, dzb, g, _ = E.bce_backward(flat, batch, run, ws, z, tgt, E.BceScratch(GD.DEV))
            torch.cuda.synchronize()
            put(f"{tag}_{math}_early{int(early)}_bce", {"out3": GD._np(o3), "dz": GD._np(dzb), "g": GD._np(g)})


for S in (1, 3):
    for name in GD.SHAPES:
        for math in ("x6", "f32"):
            sequence(GD._case(name), math, S, 0.0, name)
    for name in GD.ALL_MATH_SHAPES:
        for math in ("bf16", "x3", "h3"):
            sequence(GD._case(name), math, S, 0.0, name)
    for name in GD.DROPOUT_SHAPES:
        sequence(GD._case(name), "x6", S, 0.1, name)
for name in ("n6x5", "wide138"):
    null_prop = copy.copy(GD._case(name))
    null_prop.prop = None
    for math in ("x6", "bf16"):
        for S in (1, 3):
            sequence(null_prop, math, S, 0.0, name + "_noprop")
        backwards(GD._case(name), math, name)
        backwards(null_prop, math, name + "_noprop")
np.savez(sys.argv[1], **out)
print("dumped", sys.argv[1], len(out))
