#!/usr/bin/env python
"""Measure the evaluation path (spwgnn_eval_metrics, KerasModel.evaluate) on the GPU.

  kernel    at bench.py's headline shape (65,536 fully connected six-box towers, 393,216 nodes, S = 5, x6):
            device-event time per call of the inference forward and of engine.eval_metrics with R = 1 and
            R = 5 rows — all tables, and with the histogram, the tower tables or both left out, to see which
            part the launch's time goes to. Run it under `rocprofv3 --kernel-trace --stats` for the kernel's
            own time (k_eval_metrics) next to the forward's kernels.
  evaluate  wall time (host clock around work that ends in a device read) of KerasModel.evaluate on the same
            towers as dense Keras inputs, against the host route it replaces — model.predict, then the counts
            in numpy — in the same process; both give the same confusion.

Prints one JSON line; `--out` also writes it to a file.
    python tools/eval_bench.py kernel --out profiles/eval_kernel.json
    python tools/eval_bench.py evaluate --out profiles/eval_evaluate.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from spwgnn_amd import GraphNetwork, KerasModel, TowerBatch, data as D, engine as E, params as P  # noqa: E402

DEV = "cuda:0"


def timed(fn, calls: int, warmup: int = 5) -> float:
    """ms per call of fn(), device events around `calls` back-to-back calls."""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def kernel(args) -> dict:
    raw = D.synthetic_towers_fast(args.towers, args.nodes, seed=1000 + 97 * args.nodes)   # bench.py's towers
    batch = TowerBatch.fully_connected((raw / D.RELATION_THRESHOLD).astype(np.float32), device=DEV, nw_max=16)
    flat = P.to_flat(P.glorot_uniform(0), device=DEV)
    run = E.RunConfig(args.mp_steps, math=args.math)
    ws = E.Workspace(DEV)
    n, S = batch.n_nodes, args.mp_steps
    z1 = torch.empty(n, dtype=torch.float32, device=DEV)
    zs = torch.empty(S, n, dtype=torch.float32, device=DEV)
    E.forward_steps(flat, batch, run, ws, step_logits=zs)
    tgt = torch.from_numpy(np.random.default_rng(17).integers(0, 2, size=n).astype(np.float32)).to(DEV)
    batch.tower_offsets   # built before the timed calls
    res = {"tool": "eval_bench kernel", "device": torch.cuda.get_device_name(0), "towers": args.towers,
           "nodes_per_tower": args.nodes, "n_nodes": n, "mp_steps": S, "math": args.math, "calls": args.calls,
           "forward_ms": round(timed(lambda: E.forward(flat, batch, run, ws, logits=z1), args.calls), 4),
           "forward_steps_ms": round(timed(lambda: E.forward_steps(flat, batch, run, ws, step_logits=zs), args.calls), 4)}
    for R, z in ((1, z1), (S, zs)):
        for name, towers, hist in (("all", True, True), ("no_hist", True, False), ("no_towers", False, True),
                                   ("node4_only", False, False)):
            tab = E.EvalTables(DEV, rows=R, towers=towers, hist=hist)
            ms = timed(lambda: E.eval_metrics(z, tgt, tab, batch=batch if towers else None), args.calls)
            res[f"eval_R{R}_{name}_ms"] = round(ms, 4)
            assert int(tab.node4.sum()) == (args.calls + 5) * R * n
        # the bytes one call reads: per row the logits and the targets in the node stream, both again in the
        # tower walk, and the offsets
        res[f"eval_R{R}_all_bytes"] = 4 * R * (4 * n + batch.n_towers + 1)
    res["eval_R1_share_of_forward"] = round(res["eval_R1_all_ms"] / res["forward_ms"], 4)
    res[f"eval_R{S}_share_of_forward_steps"] = round(res[f"eval_R{S}_all_ms"] / res["forward_steps_ms"], 4)
    return res


def evaluate(args) -> dict:
    raw = D.synthetic_towers_fast(args.towers, args.nodes, seed=1000 + 97 * args.nodes)
    Rs, Rr = D.relation_matrices(raw, None)
    x = {"objects": (raw / D.RELATION_THRESHOLD).astype(np.float32), "sender_relations": Rs, "receiver_relations": Rr}
    target = np.random.default_rng(17).integers(0, 2, size=(args.towers, args.nodes)).astype(np.float32)
    model = KerasModel(GraphNetwork(mp_steps=args.mp_steps, seed=0, device=DEV, math=args.math), args.nodes)

    def host_route():
        p = model.predict(x)[..., 0]                      # every probability back on the host
        pred = p > np.float32(0.5)
        ok = pred.astype(np.float32) == target
        return [int((pred & ok).sum()), int((~pred & ok).sum()), int((pred & ~ok).sum()), int((~pred & ~ok).sum())]

    def device_route():
        d = model.evaluate(x, {"target": target}, return_dict=True)
        return [d["tp"], d["tn"], d["fp"], d["fn"]]

    times = {"predict_numpy": [], "evaluate": []}
    for k in range(args.repeats + 1):                     # alternating; the first pair is the warm-up
        for name, fn in (("predict_numpy", host_route), ("evaluate", device_route)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cells = fn()
            torch.cuda.synchronize()
            if k:
                times[name].append((time.perf_counter() - t0) * 1e3)
            times[name + "_cells"] = cells
    assert times["predict_numpy_cells"] == times["evaluate_cells"], (times["predict_numpy_cells"], times["evaluate_cells"])
    return {"tool": "eval_bench evaluate", "device": torch.cuda.get_device_name(0), "towers": args.towers,
            "nodes_per_tower": args.nodes, "mp_steps": args.mp_steps, "math": args.math, "repeats": args.repeats,
            "cells_tp_tn_fp_fn": times["evaluate_cells"],
            "predict_numpy_ms": [round(t, 2) for t in times["predict_numpy"]],
            "evaluate_ms": [round(t, 2) for t in times["evaluate"]],
            "predict_numpy_median_ms": round(float(np.median(times["predict_numpy"])), 2),
            "evaluate_median_ms": round(float(np.median(times["evaluate"])), 2),
            "note": "both routes convert the dense relation matrices and plan the batch on the host first"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "evaluate"])
    ap.add_argument("--towers", type=int, default=65536)
    ap.add_argument("--nodes", type=int, default=6)
    ap.add_argument("--mp-steps", type=int, default=5)
    ap.add_argument("--math", default="x6", choices=sorted(E.MATH_MODES))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    line = json.dumps(kernel(args) if args.mode == "kernel" else evaluate(args))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
