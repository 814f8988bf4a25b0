#!/usr/bin/env python
"""Cost of deep supervision in a training step: the same forward + loss + backward with
step_loss_weights = None (spwgnn_forward, spwgnn_bce_backward) and with the uniform λ = 1/S
(spwgnn_forward_steps, spwgnn_bce_steps, spwgnn_backward_steps). Defaults: bench.py's headline shape (65,536
fully connected six-box towers, 5 steps, dropout 0.1, x6); `--towers 32 --steps 1 --threshold` is BASELINE
config 1's shape, `--steps 5` with it the reference's 5 steps at batch 32.

The two steps alternate in this one process, `--reps` times, each timed between two device events over
`--calls` calls after a warm-up. The derived cost is S − 1 logit-row stores, S − 1 row loads and, on the fused
small-batch loop, one loss launch that the plain step folds into its backward.
Prints one JSON line; `--out` also writes it to a file.

    python tools/steps_bench.py --out profiles/steps_cost_headline.json
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
    ap.add_argument("--threshold", action="store_true", help="thresholded relations (BASELINE configs 1, 2)")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out")
    a = ap.parse_args()

    if a.threshold:
        obj, Rs, Rr, _, _ = D.synthetic_batch(a.towers, a.nodes, seed=1, fully_connected=False)
        batch = TowerBatch.from_dense(obj, Rs, Rr, None, device=DEV)
    else:
        raw = D.synthetic_towers(a.towers, a.nodes, seed=1)
        batch = TowerBatch.fully_connected((raw / D.RELATION_THRESHOLD).astype(np.float32), device=DEV)
    flat = P.to_flat(P.glorot_uniform(0), device=DEV)
    n, S = batch.n_nodes, a.steps
    g = torch.Generator(device=DEV).manual_seed(0)
    tgt = (torch.rand(n, device=DEV, generator=g) > 0.5).float()
    lam = [1.0 / S] * S
    scratch, sscratch, ws = E.BceScratch(DEV), E.BceStepsScratch(DEV, S), E.Workspace(DEV)
    logits, dz = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    Z, dZ = torch.empty(S, n, device=DEV), torch.empty(S, n, device=DEV)
    grads = torch.empty_like(flat)
    run = E.RunConfig(S, training=True, dropout=0.1, seed=7, math=a.math)

    def step(deep):
        if deep:
            E.forward_steps(flat, batch, run, ws, step_logits=Z)
            E.bce_steps(Z, tgt, lam, sscratch, dlogits=dZ)
            E.backward_steps(flat, batch, run, ws, dZ, grads=grads)
        else:
            E.forward(flat, batch, run, ws, logits=logits)
            E.bce_backward(flat, batch, run, ws, logits, tgt, scratch, dlogits=dz, grads=grads)

    def timed(deep):
        for _ in range(3):
            step(deep)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.calls):
            step(deep)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.calls

    runs = {"plain": [], "deep": []}
    for _ in range(a.reps):
        for k in runs:
            runs[k].append(round(timed(k == "deep"), 4))
    med = {k: float(np.median(v)) for k, v in runs.items()}
    res = {"shape": {"towers": a.towers, "nodes_per_tower": a.nodes, "n_nodes": n, "mp_steps": S, "math": a.math,
                     "dropout": 0.1, "relations": "threshold" if a.threshold else "full",
                     "fused_path": E.fused_path(batch, run)},
           "ms_per_step": runs, "median_ms": med, "deep_minus_plain_ms": round(med["deep"] - med["plain"], 4),
           "deep_over_plain": round(med["deep"] / med["plain"], 4),
           "plain_spread_ms": round(max(runs["plain"]) - min(runs["plain"]), 4)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
