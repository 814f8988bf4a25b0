#!/usr/bin/env python
"""Measure the tower-level loss (spwgnn_bce_tower) on the GPU.

  loss   device-event time per call of engine.bce_tower (derived and explicit tower targets, with and without
         per-node weights) against engine.bce with weights (spwgnn_bce_weighted) and without, at the same n:
         65,536 six-block towers (two launches each) and 32 six-block towers (one launch each, latency-bound).
         The variants alternate within each repeat; the medians over the repeats are reported.
  step   the x6 training step (Trainer.step: forward, loss, backward, Adam) at bench.py's headline shape —
         65,536 fully connected six-box towers, S = 5 — with the tower term on and off, alternating.

Prints one JSON line per mode; `--out` appends them to a file.
    python tools/tower_loss_bench.py loss step --out profiles/tower_loss_bench.txt
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from spwgnn_amd import TowerBatch, data as D, engine as E, params as P  # noqa: E402
from spwgnn_amd.trainer import Trainer  # noqa: E402

DEV = "cuda:0"


def timed(fn, calls: int, warmup: int = 10) -> float:
    """µs per call of fn(), device events around `calls` back-to-back calls."""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3


def towers(n_towers: int, nodes: int) -> TowerBatch:
    raw = D.synthetic_towers_fast(n_towers, nodes, seed=1000 + 97 * nodes)   # bench.py's towers
    return TowerBatch.fully_connected((raw / D.RELATION_THRESHOLD).astype(np.float32), device=DEV, nw_max=16)


def loss(args) -> dict:
    res = {"tool": "tower_loss_bench loss", "device": torch.cuda.get_device_name(0), "nodes_per_tower": args.nodes,
           "calls": args.calls, "repeats": args.repeats, "unit": "us per call (median over the repeats)"}
    for T in (args.towers, 32):
        n = T * args.nodes
        rng = np.random.default_rng(17)
        z = torch.from_numpy(rng.normal(2.0, 2.0, n).astype(np.float32)).to(DEV)
        t = torch.from_numpy((rng.random(n) < 0.85).astype(np.float32)).to(DEV)
        w = torch.from_numpy(rng.choice(np.array([0.0, 0.5, 1.0, 2.5], np.float32), n, p=[0.3, 0.25, 0.25, 0.2])).to(DEV)
        tt = torch.from_numpy(rng.integers(0, 2, T).astype(np.float32)).to(DEV)
        b = type("B", (), {})()
        b.n_nodes, b.n_towers, b.tower_nodes = n, T, np.full(T, args.nodes)
        b.tower_offsets = torch.arange(T + 1, dtype=torch.int32, device=DEV) * args.nodes
        dz = torch.empty_like(z)
        bs, ts = E.BceScratch(DEV), E.TowerLossScratch(DEV)
        norm = float(max(int(torch.count_nonzero(w)), 1))
        norm_t = float(E.counted_towers(b, w))
        variants = {
            "bce": lambda: E.bce(z, t, bs, dlogits=dz),
            "bce_weighted": lambda: E.bce(z, t, bs, dlogits=dz, node_weights=w, norm=norm),
            "tower_derived": lambda: E.bce_tower(z, t, b, ts, 1.0, 1.0, norm_t=T, dlogits=dz),
            "tower_explicit": lambda: E.bce_tower(z, t, b, ts, 1.0, 1.0, tower_targets=tt, norm_t=T, dlogits=dz),
            "tower_weighted": lambda: E.bce_tower(z, t, b, ts, 1.0, 1.0, norm_t=norm_t, dlogits=dz, node_weights=w, norm=norm),
            "tower_only_labels": lambda: E.bce_tower(z, None, b, ts, 1.0, 0.0, tower_targets=tt, norm_t=T, dlogits=dz),
        }
        times = {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, fn in variants.items():
                times[k].append(timed(fn, args.calls))
        row = {k: round(float(np.median(v)), 2) for k, v in times.items()}
        row["spread"] = {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()}
        row["tower_weighted_over_bce_weighted"] = round(row["tower_weighted"] / row["bce_weighted"], 3)
        row["tower_derived_over_bce"] = round(row["tower_derived"] / row["bce"], 3)
        res[f"towers_{T}"] = row
    return res


def step(args) -> dict:
    batch = towers(args.towers, args.nodes)
    tgt = torch.from_numpy((np.random.default_rng(17).random(batch.n_nodes) < 0.85).astype(np.float32)).to(DEV)
    batch.tower_offsets   # the device offsets are built on first use: before the timed steps, not inside them
    trainers = {name: Trainer(P.to_flat(P.glorot_uniform(0), device=DEV), mp_steps=args.mp_steps, math=args.math, **kw)
                for name, kw in (("off", {}), ("on", dict(tower_loss=1.0, node_loss=1.0)))}
    times = {k: [] for k in trainers}
    for _ in range(args.repeats):
        for k, tr in trainers.items():
            times[k].append(timed(lambda: tr.step(batch, tgt), args.steps, warmup=5) / 1e3)
    res = {"tool": "tower_loss_bench step", "device": torch.cuda.get_device_name(0), "towers": args.towers,
           "nodes_per_tower": args.nodes, "n_nodes": batch.n_nodes, "mp_steps": args.mp_steps, "math": args.math,
           "steps": args.steps, "repeats": args.repeats, "unit": "ms per Trainer.step (median over the repeats)"}
    for k, v in times.items():
        res[f"step_{k}_ms"] = round(float(np.median(v)), 4)
        res[f"step_{k}_spread_ms"] = [round(min(v), 4), round(max(v), 4)]
    res["on_over_off"] = round(res["step_on_ms"] / res["step_off_ms"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("modes", nargs="+", choices=["loss", "step"])
    ap.add_argument("--towers", type=int, default=65536)
    ap.add_argument("--nodes", type=int, default=6)
    ap.add_argument("--mp-steps", type=int, default=5)
    ap.add_argument("--math", default="x6", choices=sorted(E.MATH_MODES))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    for mode in args.modes:
        line = json.dumps(loss(args) if mode == "loss" else step(args))
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
