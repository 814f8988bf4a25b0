#!/usr/bin/env python
"""Time `engine.backward_relations` (spwgnn_backward_relations, k_rel_bwd) at the headline shape:
65,536 fully connected six-box towers, S = 5 (bench.py config 0), in x6 and bf16 math.

Per math: a warm forward, then a forward whose S edge-forward launches are bracketed by the library's
timing hook (their sum is what the kernel is compared with: it repeats the edge forward's product per
(block, step) without the one-hot receiver sum), the loss, the backward, a warm-up, then device events
around `--calls` back-to-back relation calls. Reports the time of the one launch, the summed k_edge_fwd
time of the same run, their ratio, and the bf16 MFMA rate the launch reaches. Prints one JSON line;
`--out` also writes it to a file.

    python tools/relation_grad_bench.py --out profiles/relation_grad_bench.json
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


def hip_events(n):
    hip, evs = _lib.hip_runtime(), []
    for _ in range(n):
        e = C.c_void_p()
        if hip.hipEventCreate(C.byref(e)) != 0:
            raise RuntimeError("hipEventCreate failed")
        evs.append(e.value)
    return hip, evs


def pair_ms(hip, evs):
    out = []
    for i in range(len(evs) // 2):
        ms = C.c_float()
        if hip.hipEventSynchronize(C.c_void_p(evs[2 * i + 1])) != 0 or hip.hipEventElapsedTime(
                C.byref(ms), C.c_void_p(evs[2 * i]), C.c_void_p(evs[2 * i + 1])) != 0:
            raise RuntimeError("an edge-forward launch was not recorded")
        out.append(ms.value)
    return out


def one_math(args, batch, flat, tgt, math):
    dev, S = batch.device, args.mp_steps
    ws = E.Workspace(dev)
    run = E.RunConfig(S, training=True, dropout=0.1, seed=1, math=math)
    E.forward(flat, batch, run, ws)   # warm
    hip, evs = hip_events(2 * S)
    prun = E.RunConfig(S, training=True, dropout=0.1, seed=1, math=math, prof_kernel=_lib.K_EDGE_FWD, prof_events=evs)
    z = E.forward(flat, batch, prun, ws)
    torch.cuda.synchronize()
    efwd = pair_ms(hip, evs)
    for e in evs:
        hip.hipEventDestroy(C.c_void_p(e))
    _, dz = E.bce(z, tgt, E.BceScratch(dev))
    E.backward(flat, batch, run, ws, dz)
    drel = torch.empty(32 * batch.n_eblocks, dtype=torch.float32, device=dev)
    first = E.backward_relations(flat, batch, run, ws, drel=drel).clone()
    for _ in range(args.warmup):
        E.backward_relations(flat, batch, run, ws, drel=drel)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(args.calls):
        E.backward_relations(flat, batch, run, ws, drel=drel)
    b.record()
    torch.cuda.synchronize()
    assert torch.equal(drel, first) and bool(torch.isfinite(drel).all())
    ms = a.elapsed_time(b) / args.calls
    products = int(_lib.lib().spwgnn_math_products_bwd(E.MATH_MODES[math]))
    flop = 2.0 * 32 * 160 * 160 * products * batch.n_eblocks * S   # the padded 32×160×160 product per (block, step)
    return {"math": math, "ms_per_call": round(ms, 4), "edge_fwd_ms": [round(x, 4) for x in efwd],
            "edge_fwd_sum_ms": round(sum(efwd), 4), "ratio_to_edge_fwd_sum": round(ms / sum(efwd), 3),
            "mfma_products_per_fp32_product": products, "mfma_tflops": round(flop / (ms * 1e-3) / 1e12, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--towers", type=int, default=65536)
    ap.add_argument("--nodes", type=int, default=6)
    ap.add_argument("--mp-steps", type=int, default=5)
    ap.add_argument("--maths", default="x6,bf16")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    raw = D.synthetic_towers_fast(args.towers, args.nodes, seed=1000 + 97 * args.nodes)   # bench.py's towers
    batch = TowerBatch.fully_connected((raw / D.RELATION_THRESHOLD).astype(np.float32), device=dev, nw_max=16)
    flat = P.to_flat(P.glorot_uniform(0), device=dev)
    tgt = torch.from_numpy(np.random.default_rng(17).integers(0, 2, size=batch.n_nodes).astype(np.float32)).to(dev)
    res = {"tool": "relation_grad_bench", "device": torch.cuda.get_device_name(0), "towers": args.towers,
           "nodes_per_tower": args.nodes, "mp_steps": args.mp_steps, "n_nodes": batch.n_nodes,
           "n_eblocks": batch.n_eblocks, "calls": args.calls,
           "runs": [one_math(args, batch, flat, tgt, m) for m in args.maths.split(",")]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
