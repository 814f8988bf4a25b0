#!/usr/bin/env python
"""Cost of carrying the propagation state through a training step at bench.py's
headline shape: 65,536 fully connected six-box towers, 5 propagation steps, dropout 0.1, x6 math.

Two steps alternate in this one process, `--reps` times, each timed between two device events over
`--calls` calls after a warm-up:
  plain   forward + BCE + backward                         (spwgnn_forward, spwgnn_backward)
  state   forward with the final state + BCE + backward    (spwgnn_forward_state with a buffer,
          with a state cotangent                            spwgnn_backward_state with a dstate)
The difference is the last node forward without its §3zh shortcut, the first node backward seeded
instead of shortened, and the two layout launches.
Prints one JSON line; `--out` also writes it to a file.

    python tools/state_bench.py --out profiles/state_cost.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from spwgnn_amd import TowerBatch, data as D, engine as E, params as P  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--towers", type=int, default=65536)
    ap.add_argument("--nodes", type=int, default=6)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--math", default="x6")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out")
    a = ap.parse_args()

    raw = D.synthetic_towers(a.towers, a.nodes, seed=1)
    batch = TowerBatch.fully_connected((raw / D.RELATION_THRESHOLD).astype(np.float32), device=DEV)
    flat = P.to_flat(P.glorot_uniform(0), device=DEV)
    n = batch.n_nodes
    g = torch.Generator(device=DEV).manual_seed(0)
    tgt = (torch.rand(n, device=DEV, generator=g) > 0.5).float()
    dstate = torch.randn(n, 100, device=DEV, generator=g) / n
    scratch, ws = E.BceScratch(DEV), E.Workspace(DEV)
    logits, dz = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    grads, state = torch.empty_like(flat), torch.empty(n, 100, device=DEV)

    def step(with_state, run):
        if with_state:
            E.forward(flat, batch, run, ws, logits=logits, return_state=True, state=state)
        else:
            E.forward(flat, batch, run, ws, logits=logits)
        E.bce(logits, tgt, scratch, dlogits=dz)
        E.backward(flat, batch, run, ws, dz, grads=grads, dstate=dstate if with_state else None)

    def run_cfg(**kw):
        return E.RunConfig(a.steps, training=True, dropout=0.1, seed=7, math=a.math, **kw)

    def timed(with_state):
        run = run_cfg()
        for _ in range(3):
            step(with_state, run)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.calls):
            step(with_state, run)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.calls

    runs = {"plain": [], "state": []}
    for _ in range(a.reps):
        for k in runs:
            runs[k].append(round(timed(k == "state"), 4))
    med = {k: float(np.median(v)) for k, v in runs.items()}
    res = {"shape": {"towers": a.towers, "nodes_per_tower": a.nodes, "n_nodes": n, "mp_steps": a.steps, "math": a.math,
                     "dropout": 0.1},
           "ms_per_step": runs, "median_ms": med, "state_minus_plain_ms": round(med["state"] - med["plain"], 4),
           "state_over_plain": round(med["state"] / med["plain"], 4),
           "plain_spread_ms": round(max(runs["plain"]) - min(runs["plain"]), 4)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
