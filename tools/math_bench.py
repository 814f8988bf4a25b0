#!/usr/bin/env python
"""Time the `Trainer` step in x6, x3, h3 and bf16 math on one box, in one process, alternating.

Two shapes: the headline (65,536 fully connected six-box towers, S = 5, dropout 0.1: bench.py config 0)
and the reference's batch of 32 such towers. Per shape the maths run in rounds (x6, x3, h3, bf16, x6,
x3, h3, bf16, ...; at least three), each entry `--steps` back-to-back steps between two device events,
so a drift of the box shows as a spread inside every math instead of as a gap between maths. A math
counts as faster than x6 only if every one of its rounds beats every x6 round by more than x6's own
spread. For x6, x3 and h3 the launches of every library kernel are then timed through the `prof_kernel`
hook (spwgnn_run.prof_kernel), summed per step.

Forward only (inference, `engine.forward` with training=False; "forward" in the JSON): the same
alternation at the headline shape and at a config-5-like shape (towers of 32 boxes, S = 10, fully
connected: a receiver-block plan), x6 / x3 / h3 — h3's backward is x6's, so this is where it differs.

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

MATHS = ("x6", "x3", "h3", "bf16")
FWD_MATHS = ("x6", "x3", "h3")
FWD_KERNELS = ("enc_edge", "enc_node", "edge_fwd", "node_fwd")
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


def forward_ms(flat, batch, run, ws, z, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        E.forward(flat, batch, run, ws, logits=z)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def forward_kernel_table(flat, batch, S, math, ws, z, steps):
    table = {}
    for name in FWD_KERNELS:
        ev = HipEvents(2 * 2 * SLOTS * steps)
        per = 2 * 2 * SLOTS
        for k in range(steps):
            run = E.RunConfig(S, training=False, math=math, prof_kernel=KERNELS[name], prof_events=ev.ev[per * k: per * (k + 1)])
            E.forward(flat, batch, run, ws, logits=z)
        torch.cuda.synchronize()
        ms = ev.recorded_ms()
        ev.close()
        if ms:
            table[name] = {"ms_per_forward": round(sum(ms) / steps, 4), "launches_per_forward": len(ms) / steps}
    return table


def run_forward_shape(name, towers, nodes, S, args, dev):
    """Inference forwards of one batch, x6 / x3 / h3 alternating; every round's ms per forward."""
    raw = D.synthetic_towers_fast(towers, nodes, seed=1000 + 97 * nodes)
    kw = {"nw_max": 16} if nodes <= 16 else {}
    batch = TowerBatch.fully_connected((raw / D.RELATION_THRESHOLD).astype(np.float32), device=dev, **kw)
    flat = P.to_flat(P.glorot_uniform(0), device=dev)
    z = torch.empty(batch.n_nodes, dtype=torch.float32, device=dev)
    runs = {m: E.RunConfig(S, training=False, math=m) for m in FWD_MATHS}
    wss = {m: E.Workspace(dev) for m in FWD_MATHS}
    for m in FWD_MATHS:
        for _ in range(args.warmup):
            E.forward(flat, batch, runs[m], wss[m], logits=z)
    rounds = []
    for _ in range(args.rounds):
        rounds.append({m: round(forward_ms(flat, batch, runs[m], wss[m], z, args.steps), 4) for m in FWD_MATHS})
        print(name, "forward", rounds[-1], flush=True)
    ms = {m: [r[m] for r in rounds] for m in FWD_MATHS}
    spread = max(ms["x6"]) - min(ms["x6"])
    return {"towers": towers, "nodes_per_tower": nodes, "mp_steps": S, "n_nodes": batch.n_nodes, "n_eblocks": batch.n_eblocks,
            "recv_blocks": bool(batch.flags & 1), "forwards_per_round_entry": args.steps, "rounds": rounds,
            "min_ms": {m: min(ms[m]) for m in FWD_MATHS}, "max_ms": {m: max(ms[m]) for m in FWD_MATHS},
            "x6_spread_ms": round(spread, 4),
            "h3_faster_than_x6_every_round_by_more_than_x6_spread": max(ms["h3"]) + spread < min(ms["x6"]),
            "kernels": {m: forward_kernel_table(flat, batch, S, m, wss[m], z, args.kernel_steps) for m in FWD_MATHS}}


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
           "h3_faster_than_x6_every_round": max(ms["h3"]) < min(ms["x6"]),
           "fused_path": {m: E.fused_path(batch, trainers[m].run_config()) for m in MATHS},
           "kernels": {m: kernel_table(trainers[m], batch, tgt, args.kernel_steps) for m in ("x6", "x3", "h3")}}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10, help="steps per round entry at the headline shape")
    ap.add_argument("--small-steps", type=int, default=200, help="... at the batch of 32")
    ap.add_argument("--kernel-steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--towers", type=int, default=65536)
    ap.add_argument("--towers32", type=int, default=2048, help="towers of the 32-box forward-only shape (config 5: 8192)")
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
           "mfma_products_per_fp32_product_bwd": {m: int(_lib.lib().spwgnn_math_products_bwd(E.MATH_MODES[m])) for m in MATHS},
           "shapes": {"headline": run_shape("headline", args.towers, args, dev),
                      "batch32": run_shape("batch32", 32, args, dev)},
           "forward": {"headline": run_forward_shape("headline", args.towers, 6, 5, args, dev),
                       "n32_s10_recv": run_forward_shape("n32_s10_recv", args.towers32, 32, 10, args, dev)}}
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
