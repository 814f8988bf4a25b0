#!/usr/bin/env python
"""Time the device-filled batch plans (k_plan_device: TowerBatch.from_positions / from_dense_device /
refill) at three shapes of 65,536 towers: six-box fully connected, six-box
thresholded (raw-pixel distance < 170, main.py:71-81) and ragged 4-16-box thresholded.

Per shape:
  fill      `--calls` refills between two device events, per source (positions; dense relation
            matrices for the uniform shapes), against the bytes one fill must move — 12 B per edge
            slot written (edge_src, edge_dst, blk_csr), the pos rows, the tower counts; the positions
            or both relation matrices read, plus the static tables — as GB/s and as a fraction of the
            HBM streaming bound DESIGN.md §3zj uses. Each refill also zeroes the 4-byte status word.
  end2end   wall time of "device tensors in → logits out" (inference, x6): GraphNetwork.forward_logits
            with plan="host" (what the library did before: copy to the host, C++ scan, plan, upload)
            against plan="device", alternating in this one process; for the ragged shape the host path
            is TowerBatch.ragged on the positions copied back, the device path forward_positions.
  capacity  blocks of the capacity plan (N(N−1) slots per tower), of a capacity plan sized for the
            largest relation count seen (edge_cap = max), and of the host's actual-count plan, with
            the inference forward's time on each.
Prints one JSON line; `--out` also writes it to a file.

    python tools/plan_device_bench.py --out profiles/plan_device_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from spwgnn_amd import GraphNetwork, TowerBatch, data as D, engine as E  # noqa: E402

PEAK_HBM_GBS = 8000.0   # MI355X_MICROARCH.md (bench.py's figure)
DEV = "cuda:0"


def fill_bytes(batch, source: str) -> dict:
    slots = batch.n_eblocks * 32
    b = {"edge_src_dst": slots * 8, "blk_csr": batch.n_eblocks * 128, "tower_edges": batch.n_towers * 4,
         "static": batch.n_wtiles * 20 + batch.n_nodes * 4}
    if source == "positions":
        b["pos"] = batch.n_nodes * 16
        b["read"] = batch.n_nodes * 12
    else:
        B, N = batch.node_shape
        b["read"] = 2 * B * N * N * (N - 1) * 4
    b["total"] = sum(b.values())
    return b


def events_ms(fn, calls: int, warmup: int = 5) -> float:
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


def wall_ms(fns: dict, reps: int) -> dict:
    """Alternating wall times (ms, median and every run) of callables that end synchronised."""
    runs = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            runs[k].append(round((time.perf_counter() - t) * 1e3, 2))
    return {k: {"median_ms": float(np.median(v)), "runs_ms": v} for k, v in runs.items()}


def fill_report(batch, source, arg, calls) -> dict:
    ms = events_ms(lambda: batch.refill(arg), calls)
    batch.check()
    by = fill_bytes(batch, source)
    gbs = by["total"] / (ms * 1e-3) / 1e9
    return {"ms_per_call": round(ms, 4), "bytes": by, "gb_per_s": round(gbs, 1),
            "streaming_bound_ms": round(by["total"] / (PEAK_HBM_GBS * 1e9) * 1e3, 4),
            "frac_of_hbm_peak": round(gbs / PEAK_HBM_GBS, 3)}


def forward_ms(net, batch, calls=10) -> float:
    flat, run, ws = net.flat.detach(), net.run_config(), E.Workspace(DEV)
    out = torch.empty(batch.n_nodes, dtype=torch.float32, device=DEV)
    return round(events_ms(lambda: E.forward(flat, batch, run, ws, out), calls, warmup=2), 3)


def capacity_report(net, dev_batch, raw_dev, kw, host_batch) -> dict:
    te = dev_batch.tower_edges
    capmax = int(te.max())
    tight = TowerBatch.from_positions(raw_dev, 170.0, nw_max=16, edge_cap=capmax, check=True, **kw)
    rep = {"relations_per_tower": {"min": int(te.min()), "mean": round(float(te.mean()), 2), "max": capmax},
           "plans": {}}
    for name, b in (("capacity_all_slots", dev_batch), ("capacity_max_count", tight), ("actual_count_host", host_batch)):
        rep["plans"][name] = {"n_eblocks": b.n_eblocks, "n_wtiles": b.n_wtiles, "forward_ms": forward_ms(net, b)}
    rep["blocks_ratio_all_slots_over_actual"] = round(dev_batch.n_eblocks / host_batch.n_eblocks, 3)
    return rep


def uniform_shape(net, towers, thr, calls, reps) -> dict:
    raw = D.synthetic_towers_fast(towers, 6, seed=1000 + 97 * 6)   # bench.py's towers
    assert np.array_equal(raw, raw.astype(np.float32))
    raw_dev = torch.from_numpy(raw.astype(np.float32)).to(DEV)
    Rs, Rr = D.relation_matrices(raw, thr)
    obj_dev = torch.from_numpy((raw / 170).astype(np.float32)).to(DEV)
    Rs_dev, Rr_dev = torch.from_numpy(Rs).to(DEV), torch.from_numpy(Rr).to(DEV)
    pb = TowerBatch.from_positions(raw_dev, thr, nw_max=16, check=True)
    db = TowerBatch.from_dense_device(obj_dev, Rs_dev, Rr_dev, nw_max=16, check=True)
    assert torch.equal(pb.edge_src, db.edge_src) and torch.equal(pb.blk_csr, db.blk_csr)
    res = {"towers": towers, "nodes_per_tower": 6, "threshold": thr, "n_nodes": pb.n_nodes, "n_eblocks": pb.n_eblocks,
           "n_wtiles": pb.n_wtiles, "n_edges": pb.n_edges,
           "fill": {"positions": fill_report(pb, "positions", raw_dev, calls),
                    "dense": fill_report(db, "dense", (Rs_dev, Rr_dev), calls)}}
    with torch.no_grad():
        zs = {}
        res["end2end"] = wall_ms({
            "plan_host": lambda: zs.__setitem__("h", net.forward_logits(obj_dev, Rs_dev, Rr_dev, plan="host")),
            "plan_device": lambda: zs.__setitem__("d", net.forward_logits(obj_dev, Rs_dev, Rr_dev, plan="device")),
            "forward_positions": lambda: zs.__setitem__("p", net.forward_positions(raw_dev, thr)),
        }, reps)
        res["end2end"]["max_abs_logit_diff_device_vs_host"] = float((zs["h"] - zs["d"]).abs().max())
        assert torch.equal(zs["d"], zs["p"])
        if thr is not None:
            host = TowerBatch.from_dense(obj_dev, Rs_dev, Rr_dev, device=DEV, nw_max=16)
            res["capacity"] = capacity_report(net, pb, raw_dev, {}, host)
    return res


def ragged_shape(net, towers, calls, reps) -> dict:
    sizes = np.random.default_rng(11).integers(4, 17, towers).astype(np.int32)
    rows = np.zeros((int(sizes.sum()), 3))
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    for n in range(4, 17):
        idx = np.nonzero(sizes == n)[0]
        t = D.synthetic_towers_fast(len(idx), n, seed=2000 + n)
        rows[(starts[idx][:, None] + np.arange(n)[None, :]).reshape(-1)] = t.reshape(-1, 3)
    assert np.array_equal(rows, rows.astype(np.float32))
    raw_dev = torch.from_numpy(rows.astype(np.float32)).to(DEV)
    kw = {"tower_nodes": sizes}
    pb = TowerBatch.from_positions(raw_dev, 170.0, nw_max=16, check=True, **kw)
    res = {"towers": towers, "nodes_per_tower": "4-16", "threshold": 170.0, "n_nodes": pb.n_nodes,
           "n_eblocks": pb.n_eblocks, "n_wtiles": pb.n_wtiles, "n_edges": pb.n_edges,
           "fill": {"positions": fill_report(pb, "positions", raw_dev, calls)}}
    offs = np.concatenate([starts, [len(rows)]])

    def host_batch():
        r = raw_dev.cpu().numpy().astype(np.float64)
        rl = [r[offs[t]:offs[t + 1]] for t in range(towers)]
        return TowerBatch.ragged([x / 170 for x in rl], 170.0, DEV, 16, rl)

    with torch.no_grad():
        zs = {}
        res["end2end"] = wall_ms({
            "ragged_host": lambda: zs.__setitem__("h", net.forward_batch(host_batch())),
            "forward_positions": lambda: zs.__setitem__("p", net.forward_positions(raw_dev, 170.0, nw_max=16, **kw)),
        }, max(2, reps // 3))
        res["end2end"]["max_abs_logit_diff_device_vs_host"] = float((zs["h"] - zs["p"]).abs().max())
        res["capacity"] = capacity_report(net, pb, raw_dev, kw, host_batch())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--towers", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7, help="alternating end-to-end repetitions")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    net = GraphNetwork(seed=0, device=DEV)
    net.eval()
    res = {"tool": "plan_device_bench", "device": torch.cuda.get_device_name(0), "calls": args.calls,
           "hbm_peak_gb_per_s": PEAK_HBM_GBS, "math": net.math,
           "six_box_fully_connected": uniform_shape(net, args.towers, None, args.calls, args.reps),
           "six_box_thresholded": uniform_shape(net, args.towers, 170.0, args.calls, args.reps),
           "ragged_4_16_thresholded": ragged_shape(net, args.towers, args.calls, args.reps)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
