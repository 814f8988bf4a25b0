#!/usr/bin/env python
"""Time the `Trainer` step in x6, x3 and bf16 math on one box, in one process, alternating.

Two shapes: the headline (65,536 fully connected six-box towers, S = 5, dropout 0.1: bench.py config 0)
and the reference's batch of 32 such towers. Per shape the maths run in rounds (x6, x3, bf16, x6, x3,
bf16, ...; at least three), each entry `--steps` back-to-back steps between two device events, so a
drift of the box shows as a spread inside every math instead of as a gap between maths. x3 counts as
faster than x6 only if every x3 round beats every x6 round. For x6 and x3 the launches of every
library kernel are then timed through the `prof_kernel` hook (spwgnn_run.prof_kernel), summed per step.

Writes one JSON with every round's numbers (not only the best):

    python tools/math_bench.py --out profiles/x3_bench.json
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from spwgnn_amd import TowerBatch, _lib, data as D, engine as E, params as P  # noqa: E402
from spwgnn_amd.trainer import Trainer  # noqa: E402

MATHS = ("x6", "x3", "bf16")
KERNELS = {"enc_edge": _lib.K_ENC_EDGE, "enc_node": _lib.K_ENC_NODE, "edge_fwd": _lib.K_EDGE_FWD,
           "node_fwd": _lib.K_NODE_FWD, "node_bwd": _lib.K_NODE_BWD, "edge_bwd": _lib.K_EDGE_BWD, "dA": _lib.K_DA,
           "enc_edge_bwd": _lib.K_ENC_EDGE_BWD, "enc_node_bwd": _lib.K_ENC_NODE_BWD, "wgrad_w2": _lib.K_WGRAD_W2,
           "wgrad_ws": _lib.K_WGRAD_WS}
SLOTS = 16   # event pairs per step and kernel (a step launches a kernel at most 2·S + 2 times)


class HipEvents:
    """Raw hipEvent_t pairs for the library's prof_kernel hook (as bench.py's)."""

    def __init__(self, n):
        self.hip = _lib.hip_runtime()
        self.ev = []
        for _ in range(n):
            e = C.c_void_p()
            if self.hip.hipEventCreate(C.byref(e)) != 0:
                raise RuntimeError("hipEventCreate failed")
            self.ev.append(e.value)

    def recorded_ms(self):
        """Times of the pairs the library recorded (the others are skipped and HIP's error cleared)."""
        out = []
        for i in range(len(self.ev) // 2):
            ms = C.c_float()
            s1 = self.hip.hipEventSynchronize(C.c_void_p(self.ev[2 * i + 1]))
            st = self.hip.hipEventElapsedTime(C.byref(ms), C.c_void_p(self.ev[2 * i]), C.c_void_p(self.ev[2 * i + 1]))
            if st != 0 or s1 != 0:
                self.hip.hipGetLastError()
                continue
            out.append(ms.value)
        return out

    def close(self):
        for e in self.ev:
            self.hip.hipEventDestroy(C.c_void_p(e))


def step_ms(trainer, batch, tgt, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        trainer.step(batch, tgt)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def kernel_table(trainer, batch, tgt, steps):
    """{kernel: {"ms_per_step", "launches_per_step"}} through the prof_kernel hook."""
    table = {}
    for name, kid in KERNELS.items():
        ev = HipEvents(2 * SLOTS * steps)
        for k in range(steps):
            trainer.prof_kernel, trainer.prof_events = kid, ev.ev[2 * SLOTS * k: 2 * SLOTS * (k + 1)]
            trainer.step(batch, tgt)
        trainer.prof_kernel, trainer.prof_events = 0, None
        torch.cuda.synchronize()
        ms = ev.recorded_ms()
        ev.close()
        if ms:
            table[name] = {"ms_per_step": round(sum(ms) / steps, 4), "launches_per_step": len(ms) / steps}
    return table


def run_shape(name, towers, args, dev):
    raw = D.synthetic_towers_fast(towers, 6, seed=1000 + 97 * 6)   # bench.py's towers
    batch = TowerBatch.fully_connected((raw / D.RELATION_THRESHOLD).astype(np.float32), device=dev, nw_max=16)
    tgt = torch.from_numpy(np.random.default_rng(17).integers(0, 2, size=batch.n_nodes).astype(np.float32)).to(dev)
    steps = args.steps if towers > 1024 else args.small_steps
    trainers = {m: Trainer(P.to_flat(P.glorot_uniform(0), device=dev), mp_steps=5, dropout=0.1, seed=1, math=m)
                for m in MATHS}
    for m in MATHS:
        for _ in range(args.warmup):
            trainers[m].step(batch, tgt)
    rounds = []
    for _ in range(args.rounds):
        rounds.append({m: round(step_ms(trainers[m], batch, tgt, steps), 4) for m in MATHS})   # x6, x3, bf16 in turn
        print(name, rounds[-1], flush=True)
    ms = {m: [r[m] for r in rounds] for m in MATHS}
    res = {"towers": towers, "nodes_per_tower": 6, "mp_steps": 5, "dropout": 0.1, "n_nodes": batch.n_nodes,
           "n_eblocks": batch.n_eblocks, "steps_per_round_entry": steps, "rounds": rounds,
           "min_ms": {m: min(ms[m]) for m in MATHS}, "max_ms": {m: max(ms[m]) for m in MATHS},
           "x6_spread_ms": round(max(ms["x6"]) - min(ms["x6"]), 4),
           "x3_faster_than_x6_every_round": max(ms["x3"]) < min(ms["x6"]),
           "fused_path": {m: E.fused_path(batch, trainers[m].run_config()) for m in MATHS},
           "kernels": {m: kernel_table(trainers[m], batch, tgt, args.kernel_steps) for m in ("x6", "x3")}}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10, help="steps per round entry at the headline shape")
    ap.add_argument("--small-steps", type=int, default=200, help="... at the batch of 32")
    ap.add_argument("--kernel-steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--towers", type=int, default=65536)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, choices=MATHS,
                    help="no timing: three headline steps in this math alone (the program of a "
                         "counter run, tools/pmc_math.sh)")
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3")
    dev = "cuda:0"
    if args.only:
        raw = D.synthetic_towers_fast(args.towers, 6, seed=1000 + 97 * 6)
        batch = TowerBatch.fully_connected((raw / D.RELATION_THRESHOLD).astype(np.float32), device=dev, nw_max=16)
        tgt = torch.from_numpy(np.random.default_rng(17).integers(0, 2, size=batch.n_nodes).astype(np.float32)).to(dev)
        tr = Trainer(P.to_flat(P.glorot_uniform(0), device=dev), mp_steps=5, dropout=0.1, seed=1, math=args.only)
        for _ in range(3):
            tr.step(batch, tgt)
        torch.cuda.synchronize()
        return
    res = {"tool": "math_bench", "device": torch.cuda.get_device_name(0),
           "mfma_products_per_fp32_product": {m: int(_lib.lib().spwgnn_math_products(E.MATH_MODES[m])) for m in MATHS},
           "shapes": {"headline": run_shape("headline", args.towers, args, dev),
                      "batch32": run_shape("batch32", 32, args, dev)}}
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
