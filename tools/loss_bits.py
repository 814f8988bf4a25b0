"""Every output of the loss entry points as bit patterns, so two builds of the library (SPWGNN_LIB) can be
compared bit for bit with tools/cmp_npz.py: spwgnn_bce, _accumulate, _weighted and
spwgnn_bce_steps (plain and with node weights, S = 3, λ = (0.5, 0, 2), NaN logits in the λ = 0 row) at
n = 1, 18, 256, 257, 1000, 70,001, and spwgnn_bce_backward[_weighted] on a 4 × 6 batch (the loss folded
into the backward's launches) and a 64 × 6 one (its own launch). Arrays are stored as unsigned integers
of their width: a NaN compares equal to the same NaN.
usage: [SPWGNN_LIB=...] python tools/loss_bits.py OUT.npz"""
import os
import sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import model as O
from spwgnn_amd import TowerBatch, data as D, engine as E, params as P

F64 = torch.float64
out = {}


def dev(a):
    return torch.tensor(a, device="cuda")


def put(name, **tensors):
    torch.cuda.synchronize()
    for k, t in tensors.items():
        a = t.detach().cpu().numpy().copy()
        out[f"{name}_{k}"] = a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


S, lam = 3, (0.5, 0.0, 2.0)
for n in (1, 18, 256, 257, 1000, 70001):
    rng = np.random.default_rng(n)          # the inputs of tests/test_gpu_steps.py::test_bce_steps_against_fp64
    Z = rng.normal(scale=3.0, size=(S, n)).astype(np.float32)
    Z[0, 0], Z[2, n - 1] = 20.0, -17.5      # one logit beyond each side of the clip
    t = rng.integers(0, 2, n).astype(np.float32)
    w = rng.choice([0.0, 0.5, 1.0, 2.5], size=n).astype(np.float32)
    Zn = Z.copy()
    Zn[1] = np.nan
    w3 = dev(np.array([float(n), 1.0, 1.0]))
    for row in (0, 2):
        o3, dl = E.bce(dev(Z[row]), dev(t), E.BceScratch("cuda"))
        put(f"bce_n{n}_r{row}", out3=o3, dlogits=dl)
        tot = torch.zeros(3, dtype=F64, device="cuda")
        for _ in range(2):                  # two batches into the same sums
            o3, dl = E.bce(dev(Z[row]), dev(t), E.BceScratch("cuda"), total3=tot, weights3=w3)
        put(f"acc_n{n}_r{row}", out3=o3, dlogits=dl, total3=tot)
        tot = torch.zeros(3, dtype=F64, device="cuda")
        for _ in range(2):
            o3, dl = E.bce(dev(Z[row]), dev(t), E.BceScratch("cuda"), total3=tot, weights3=w3, node_weights=dev(w))
        put(f"wgt_n{n}_r{row}", out3=o3, dlogits=dl, total3=tot)
    for name, nw in (("steps", None), ("stepsw", dev(w))):
        tot, tots = torch.zeros(3, dtype=F64, device="cuda"), torch.zeros(S, 3, dtype=F64, device="cuda")
        sc = E.BceStepsScratch("cuda", S)
        for _ in range(2):
            o3, o3s, dl = E.bce_steps(dev(Zn), dev(t), lam, sc, total3=tot, weights3=w3, total3s=tots, node_weights=nw)
        put(f"{name}_n{n}", out3=o3, out3s=o3s, dlogits=dl, total3=tot, total3s=tots)

flat = P.to_flat(O.random_params(7), device="cuda")
for B in (4, 64):                           # 24 nodes: the folded loss row; 384: two loss workgroups, unfolded
    obj, Rs, Rr, prop, tgt = D.synthetic_batch(B, 6, seed=3, fully_connected=True)
    batch = TowerBatch.from_dense(obj, Rs, Rr, prop, device="cuda")
    tg = dev(tgt.reshape(-1).astype(np.float32))
    w = dev(np.random.default_rng(B).choice([0.0, 0.5, 1.0, 2.5], size=batch.n_nodes).astype(np.float32))
    w3 = dev(np.array([float(batch.n_nodes), 1.0, 1.0]))
    for name, nw in (("bwd", None), ("bwdw", w)):
        run = E.RunConfig(5, training=True, math="x6", dropout=0.1, seed=11)
        ws = E.Workspace("cuda")
        z = E.forward(flat, batch, run, ws)
        tot = torch.zeros(3, dtype=F64, device="cuda")
        o3, dl, g, _ = E.bce_backward(flat, batch, run, ws, z, tg, E.BceScratch("cuda"), total3=tot, weights3=w3,
                                      node_weights=nw)
        put(f"{name}_B{B}", logits=z, out3=o3, dlogits=dl, total3=tot, grads=g)
np.savez(sys.argv[1], **out)
print("dumped", sys.argv[1], len(out))
