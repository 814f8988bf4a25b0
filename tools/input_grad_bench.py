#!/usr/bin/env python
"""Time `engine.backward_inputs` (spwgnn_backward_inputs, k_input_bwd) at the headline shape:
65,536 fully connected six-box towers, S = 5, x6 math (bench.py config 0).

One forward and backward, a warm-up, then device events around `--calls` back-to-back calls. Reports
the time per call, the bytes the kernel must move (the dz1 and dzo1 rows once, the index arrays, the
wave-tile table and the output, computed from the shapes), the resulting GB/s against the HBM peak,
and — with `--step-ms`, the training step's time from bench.py on the same box — the call's share of
a step. Prints one JSON line; `--out` also writes it to a file.

    python tools/input_grad_bench.py --step-ms 25.4 --out profiles/input_grad_bench.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from spwgnn_amd import TowerBatch, data as D, engine as E, params as P  # noqa: E402

PEAK_HBM_GBS = 8000.0   # MI355X_MICROARCH.md (bench.py's figure)
CM_BLK_E, CM_BLK_N = 76 * 64, 52 * 64   # floats per 32-row chunk-major block (spwgnn_layout.h)


def kernel_bytes(batch: TowerBatch, math: str) -> dict:
    """What k_input_bwd has to move once: every block of dz1 that holds an edge (bf16 math: 2 bytes per
    element), every 32-node block of dzo1, both index arrays, the wave-tile table, the output rows."""
    esrc = batch.edge_src.cpu().numpy().reshape(-1, 32)
    live = int((esrc >= 0).any(axis=1).sum())
    el = 2 if math == "bf16" else 4
    b = {"dz1": live * CM_BLK_E * el, "dzo1": (batch.n_nodes + 31) // 32 * CM_BLK_N * 4,
         "index": 2 * batch.n_eblocks * 32 * 4, "wtile": batch.n_wtiles * 16, "dpos": batch.n_nodes * 16}
    b["total"] = sum(b.values())
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--towers", type=int, default=65536)
    ap.add_argument("--nodes", type=int, default=6)
    ap.add_argument("--mp-steps", type=int, default=5)
    ap.add_argument("--math", default="x6", choices=sorted(E.MATH_MODES))
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step-ms", type=float, default=None, help="the training step's ms on this box (bench.py)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.calls < 50:
        ap.error("--calls must be at least 50")
    dev = "cuda:0"
    raw = D.synthetic_towers_fast(args.towers, args.nodes, seed=1000 + 97 * args.nodes)   # bench.py's towers
    batch = TowerBatch.fully_connected((raw / D.RELATION_THRESHOLD).astype(np.float32), device=dev, nw_max=16)
    flat = P.to_flat(P.glorot_uniform(0), device=dev)
    run = E.RunConfig(args.mp_steps, training=True, dropout=0.1, seed=1, math=args.math)
    ws = E.Workspace(dev)
    z = E.forward(flat, batch, run, ws)
    tgt = torch.from_numpy(np.random.default_rng(17).integers(0, 2, size=batch.n_nodes).astype(np.float32)).to(dev)
    _, dz = E.bce(z, tgt, E.BceScratch(dev))
    E.backward(flat, batch, run, ws, dz)
    first = E.backward_inputs(flat, batch, run, ws).clone()
    for _ in range(args.warmup):
        E.backward_inputs(flat, batch, run, ws)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(args.calls):
        out = E.backward_inputs(flat, batch, run, ws)
    b.record()
    torch.cuda.synchronize()
    assert torch.equal(out, first) and bool(torch.isfinite(out).all())
    # each call also allocates its (n_nodes, 4) output through the caching allocator (no device work)
    ms = a.elapsed_time(b) / args.calls
    by = kernel_bytes(batch, args.math)
    gbs = by["total"] / (ms * 1e-3) / 1e9
    res = {"tool": "input_grad_bench", "device": torch.cuda.get_device_name(0), "towers": args.towers,
           "nodes_per_tower": args.nodes, "mp_steps": args.mp_steps, "math": args.math, "n_nodes": batch.n_nodes,
           "n_eblocks": batch.n_eblocks, "n_wtiles": batch.n_wtiles, "calls": args.calls,
           "ms_per_call": round(ms, 4), "bytes": by, "gb_per_s": round(gbs, 1),
           "hbm_peak_gb_per_s": PEAK_HBM_GBS, "frac_of_hbm_peak": round(gbs / PEAK_HBM_GBS, 3),
           "streaming_bound_ms": round(by["total"] / (PEAK_HBM_GBS * 1e9) * 1e3, 4),
           "step_ms": args.step_ms, "share_of_step": None if not args.step_ms else round(ms / args.step_ms, 4)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
