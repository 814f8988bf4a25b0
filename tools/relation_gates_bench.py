#!/usr/bin/env python
"""Time a gated training step's forward + backward (spwgnn_forward_gated / spwgnn_backward_gated)
against the same tree's ungated run, in x6 math:

  * the headline shape (65,536 fully connected six-box towers, S = 5, bench.py config 0): gated with random gates
    against the ungated call, which takes the wide kernels there too — the cost of the gate itself (one multiply per
    h2 and dh2pre element, pointer-form gathers in the gated kernels);
  * batch 32 (the reference's training batch): the gated call's wide kernels against the ungated call's fused
    small-batch path — the cost of the wide fallback.

Alternating rounds (ungated, gated, ungated, …), `--calls` forward + loss-free backward pairs between two device
events per round; reports each variant's per-round milliseconds, their min–max and the ratio of the minima. Prints
one JSON line; `--out` also writes it to a file.

`steps32`: at batch 32, alternating rounds of the forward + backward pair
  * ungated (the fused small-batch loops), gated on the wide kernels (`engine.wide_kernels()`: the launches a gated
    call took before the team / fused kernels were gated) and gated on the team / fused kernels,
and of whole optimizer steps (forward, loss, backward, Adam) of a `Trainer`
  * without and with DropEdge, issued eagerly (`Trainer.step`) and replayed as a hipGraph (`Trainer.replay_step`).

`step_gates` (`--step-gates`, which runs this section alone): at the headline shape and at batch
32, alternating rounds of the forward + backward pair ungated, with one shared gate row (``gates=``) and with a row
per propagation step (``step_gates=``, mp_steps distinct rows) — the cost of the per-step gate loads over the
shared-gate step. `--shared-only` times the ungated and shared-gate pairs alone through the calls every earlier
library has (a same-box A/B of the shared-gate step against another build, SPWGNN_LIB).

    python tools/relation_gates_bench.py --out profiles/relation_gates_bench.json
    python tools/relation_gates_bench.py --step-gates --out profiles/step_gates_bench.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from spwgnn_amd import TowerBatch, data as D, engine as E, params as P  # noqa: E402


def one_shape(args, towers, calls, math="x6"):
    dev, S = "cuda:0", args.mp_steps
    raw = D.synthetic_towers_fast(towers, args.nodes, seed=1000 + 97 * args.nodes)   # bench.py's towers
    batch = TowerBatch.fully_connected((raw / D.RELATION_THRESHOLD).astype(np.float32), device=dev, nw_max=16)
    flat = P.to_flat(P.glorot_uniform(0), device=dev)
    gates = batch.edge_gates(torch.as_tensor(np.random.default_rng(5).uniform(0.25, 1.5, batch.n_edges).astype(np.float32),
                                             device=dev))
    run = E.RunConfig(S, training=True, dropout=0.1, seed=1, math=math)
    dz = torch.as_tensor(np.random.default_rng(17).normal(0, 1e-3, batch.n_nodes).astype(np.float32), device=dev)
    ws = {None: E.Workspace(dev), "gated": E.Workspace(dev)}
    z = torch.empty(batch.n_nodes, dtype=torch.float32, device=dev)
    grads = torch.empty_like(flat)

    def step(kind):
        g = gates if kind else None
        E.forward(flat, batch, run, ws[kind], logits=z, gates=g)
        E.backward(flat, batch, run, ws[kind], dz, grads=grads, gates=g)

    times = {None: [], "gated": []}
    for kind in (None, "gated"):
        for _ in range(args.warmup):
            step(kind)
    for _ in range(args.rounds):
        for kind in (None, "gated"):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(calls):
                step(kind)
            b.record()
            torch.cuda.synchronize()
            times[kind].append(a.elapsed_time(b) / calls)
    assert bool(torch.isfinite(grads).all())
    rnd = lambda xs: [round(x, 4) for x in xs]
    return {"towers": towers, "n_nodes": batch.n_nodes, "n_eblocks": batch.n_eblocks, "math": math, "calls_per_round": calls,
            "ungated_fused_path": E.fused_path(batch, run), "ungated_ms": rnd(times[None]), "gated_ms": rnd(times["gated"]),
            "ungated_min_max": rnd([min(times[None]), max(times[None])]),
            "gated_min_max": rnd([min(times["gated"]), max(times["gated"])]),
            "ratio_of_minima": round(min(times["gated"]) / min(times[None]), 4)}


def _rounds(args, variants, calls):
    """{name: [ms per call, one per round]}: `variants` {name: callable} timed in alternating rounds."""
    times = {k: [] for k in variants}
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    for _ in range(args.rounds):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b) / calls)
    return times


def steps32(args, math="x6"):
    from spwgnn_amd.batch import HostPlan
    from spwgnn_amd.replay import ReplayStep
    from spwgnn_amd.trainer import Trainer
    dev, S, towers, calls = "cuda:0", args.mp_steps, args.small_towers, args.small_calls
    raw = D.synthetic_towers_fast(towers, args.nodes, seed=1000 + 97 * args.nodes)
    obj = (raw / D.RELATION_THRESHOLD).astype(np.float32)
    batch = TowerBatch.fully_connected(obj, device=dev, nw_max=16)
    flat = P.to_flat(P.glorot_uniform(0), device=dev)
    gates = batch.edge_gates(torch.as_tensor(np.random.default_rng(5).uniform(0.25, 1.5, batch.n_edges).astype(np.float32),
                                             device=dev))
    run = E.RunConfig(S, training=True, dropout=0.1, seed=1, math=math)
    dz = torch.as_tensor(np.random.default_rng(17).normal(0, 1e-3, batch.n_nodes).astype(np.float32), device=dev)
    z, grads = torch.empty(batch.n_nodes, dtype=torch.float32, device=dev), torch.empty_like(flat)
    wss = [E.Workspace(dev) for _ in range(3)]

    def pair(ws, g):
        E.forward(flat, batch, run, ws, logits=z, gates=g)
        E.backward(flat, batch, run, ws, dz, grads=grads, gates=g)

    def gated_wide():
        with E.wide_kernels():
            pair(wss[1], gates)

    fb = _rounds(args, {"ungated": lambda: pair(wss[0], None), "gated_wide": gated_wide,
                        "gated_team": lambda: pair(wss[2], gates)}, calls)
    assert bool(torch.isfinite(grads).all())

    # whole optimizer steps: a Trainer without / with DropEdge, eager and replayed
    m, j = np.nonzero(~np.eye(args.nodes, dtype=bool))
    base = (np.arange(towers, dtype=np.int64) * args.nodes)[:, None]
    plan = HostPlan.build(obj.reshape(-1, 3), np.full(towers, args.nodes, np.int32), (base + m).reshape(-1).astype(np.int32),
                          (base + j).reshape(-1).astype(np.int32), np.full(towers, len(m), np.int32),
                          edge_cap=args.nodes * (args.nodes - 1))
    tgt = np.random.default_rng(3).integers(0, 2, plan.n_nodes).astype(np.float32)
    tbatch, ttgt = TowerBatch.from_plan(plan, dev), torch.as_tensor(tgt, device=dev)
    steps = {}
    for name, rate in (("step", 0.0), ("dropedge_step", args.dropedge)):
        te = Trainer(P.to_flat(P.glorot_uniform(0), device=dev), mp_steps=S, dropout=0.1, seed=1, math=math, dropedge=rate)
        tr = Trainer(P.to_flat(P.glorot_uniform(0), device=dev), mp_steps=S, dropout=0.1, seed=1, math=math, dropedge=rate)
        rs = ReplayStep(plan, dev, tr.replay_body(plan.n_nodes))
        steps[name + "_eager"] = lambda te=te: te.step(tbatch, ttgt)
        steps[name + "_replayed"] = lambda tr=tr, rs=rs: tr.replay_step(rs, plan, tgt)
    st = _rounds(args, steps, calls)
    rnd = lambda xs: [round(x, 4) for x in xs]
    out = {"towers": towers, "n_nodes": batch.n_nodes, "n_eblocks": batch.n_eblocks, "math": math, "calls_per_round": calls,
           "fused_path": {"ungated": E.fused_path(batch, run), "gated": E.fused_path(batch, run, gated=True)},
           "dropedge_rate": args.dropedge}
    for k, v in {**fb, **st}.items():
        out[k + "_ms"] = rnd(v)
        out[k + "_min_max"] = rnd([min(v), max(v)])
    out["gated_team_over_ungated"] = round(min(fb["gated_team"]) / min(fb["ungated"]), 4)
    out["gated_wide_over_gated_team"] = round(min(fb["gated_wide"]) / min(fb["gated_team"]), 4)
    return out


def step_gates_cost(args, towers, calls, math="x6", shared_only=False):
    dev, S = "cuda:0", args.mp_steps
    raw = D.synthetic_towers_fast(towers, args.nodes, seed=1000 + 97 * args.nodes)
    batch = TowerBatch.fully_connected((raw / D.RELATION_THRESHOLD).astype(np.float32), device=dev, nw_max=16)
    flat = P.to_flat(P.glorot_uniform(0), device=dev)
    rows = torch.as_tensor(np.random.default_rng(5).uniform(0.25, 1.5, (S, batch.n_edges)).astype(np.float32), device=dev)
    shared = batch.edge_gates(rows[0])
    run = E.RunConfig(S, training=True, dropout=0.1, seed=1, math=math)
    dz = torch.as_tensor(np.random.default_rng(17).normal(0, 1e-3, batch.n_nodes).astype(np.float32), device=dev)
    z, grads = torch.empty(batch.n_nodes, dtype=torch.float32, device=dev), torch.empty_like(flat)
    wss = [E.Workspace(dev) for _ in range(3)]

    def pair(ws, **kw):
        E.forward(flat, batch, run, ws, logits=z, **kw)
        E.backward(flat, batch, run, ws, dz, grads=grads, **kw)

    variants = {"ungated": lambda: pair(wss[0]), "shared": lambda: pair(wss[1], gates=shared)}
    if not shared_only:
        per_step = batch.edge_step_gates(rows)
        variants["per_step"] = lambda: pair(wss[2], step_gates=per_step)
    t = _rounds(args, variants, calls)
    assert bool(torch.isfinite(grads).all())
    rnd = lambda xs: [round(x, 4) for x in xs]
    out = {"towers": towers, "n_nodes": batch.n_nodes, "n_eblocks": batch.n_eblocks, "math": math, "calls_per_round": calls,
           "fused_path_gated": E.fused_path(batch, run, gated=True)}
    for k, v in t.items():
        out[k + "_ms"] = rnd(v)
        out[k + "_min_max"] = rnd([min(v), max(v)])
    out["shared_over_ungated"] = round(min(t["shared"]) / min(t["ungated"]), 4)
    if not shared_only:
        out["per_step_over_shared"] = round(min(t["per_step"]) / min(t["shared"]), 4)
        out["per_step_over_ungated"] = round(min(t["per_step"]) / min(t["ungated"]), 4)
        # the extra gate loads of a per-step call: (S − 1) more rows of 4 bytes per slot, read by the edge forward, the
        # edge backward (or the dA rebuild) and the W2 gradient's staging
        out["extra_gate_bytes_per_reader"] = int((S - 1) * 4 * 32 * batch.n_eblocks)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--towers", type=int, default=65536)
    ap.add_argument("--small-towers", type=int, default=32)
    ap.add_argument("--nodes", type=int, default=6)
    ap.add_argument("--mp-steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--small-calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dropedge", type=float, default=0.25)
    ap.add_argument("--only-steps32", action="store_true", help="the batch-32 step comparison alone")
    ap.add_argument("--step-gates", action="store_true", help="the per-step gate comparison alone (DESIGN.md §3zzc)")
    ap.add_argument("--shared-only", action="store_true", help="with --step-gates: ungated and shared-gate pairs alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step_gates:
        res = {"tool": "relation_gates_bench --step-gates", "device": torch.cuda.get_device_name(0),
               "nodes_per_tower": args.nodes, "mp_steps": args.mp_steps, "rounds": args.rounds,
               "step_gates": [step_gates_cost(args, args.towers, args.calls, shared_only=args.shared_only),
                              step_gates_cost(args, args.small_towers, args.small_calls, shared_only=args.shared_only)]}
        line = json.dumps(res)
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    res = {"tool": "relation_gates_bench", "device": torch.cuda.get_device_name(0), "nodes_per_tower": args.nodes,
           "mp_steps": args.mp_steps, "rounds": args.rounds,
           "runs": [] if args.only_steps32 else [one_shape(args, args.towers, args.calls),
                                                 one_shape(args, args.small_towers, args.small_calls)],
           "steps32": steps32(args)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
