"""How far two clipped training runs drift apart when clipnorm differs by 1e-7 relative, and the device's
gradient norm against torch's fp64 norm over the real parameter ranges on real training gradients
(DESIGN.md §3zq): a train_on_batch loop at batch 32 on 6-block thresholded towers.
usage: python tools/clip_sensitivity.py [steps]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spwgnn_amd import data as D, params as P  # noqa: E402
from spwgnn_amd.batch import TowerBatch  # noqa: E402
from spwgnn_amd.keras_api import CompactDataset, PropagationNetwork  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
n = 1024
obj, Rs, Rr, prop, tgt = D.synthetic_batch(n, 6, seed=3, fully_connected=False)
ds = CompactDataset(obj, Rs, Rr, prop)
real = np.zeros(P.flat_size(), bool)
for _, off, shape in P.layout():
    real[off:off + int(np.prod(shape))] = True
real = torch.tensor(real, device="cuda")
batches = []
for b0 in range(0, n, 32):
    idx = np.arange(b0, b0 + 32)
    batches.append((TowerBatch.from_plan(ds.subset_plan(idx, edge_cap=True), "cuda"),
                    torch.as_tensor(tgt[idx].reshape(-1), device="cuda")))


def run(c):
    m = PropagationNetwork(seed=0, clipnorm=c).getModel(6)
    norms, worst = [], 0.0
    for k in range(steps):
        b, t = batches[k % len(batches)]
        m.train_on_batch(b, t)
        dev = float(m.clip_stats[0])
        ref = float(torch.sqrt((m._grads.double()[real] ** 2).sum()))
        worst = max(worst, abs(dev - ref) / ref)
        norms.append(dev)
    return np.array(norms), worst, m.net.flat.detach().cpu().numpy().copy()


a, wa, pa = run(0.05)
b, wb, pb = run(0.05 * (1 + 1e-7))
a2, _, pa2 = run(0.05)
print(f"device norm vs torch fp64 over the real ranges, worst relative error in {steps} steps: {wa:.3g}, {wb:.3g}")
print("the same clipnorm twice, bitwise equal norms / parameters:", np.array_equal(a, a2), np.array_equal(pa, pa2))
rel = np.abs(a - b) / a
for k in (0, 1, 2, 5, 10, 20, 50, 100, 150, steps - 1):
    if k < steps:
        print(f"step {k + 1}: norm {a[k]:.7g} (clipnorm 0.05) vs {b[k]:.7g} (0.05·(1 + 1e-7)): relative difference {rel[k]:.3g}")
print(f"max |parameter difference| after {steps} steps: {np.abs(pa - pb).max():.3g}")
