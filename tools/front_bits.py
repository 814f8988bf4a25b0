"""What the Python front ends compute, as bit patterns, so two trees of the package over ONE built library
(SPWGNN_LIB) can be compared bit for bit with tools/cmp_npz.py. Public API only. On 128
synthetic 6-box towers (thresholded relations):
  fit_<options>_<eager|graph>   the history lists and the final flat weights of fit(batch 32, 2 epochs,
                                validation_split 0.25), options plain, sample_weight, clipnorm 1.0 with
                                decay, step_loss_weights
  eval_/predict_<options>       evaluate(return_dict=True) and predict(return_steps=True) of those models
  step_<one|two>[_weighted]     the params and the returned [loss, correct, n] of three Trainer.step calls on
                                one batch of 32 towers / two micro-batches of 16
  replay                        the params after three Trainer.replay_step calls
Arrays are stored as unsigned integers of their width: a NaN compares equal to the same NaN.
usage: [SPWGNN_LIB=...] python tools/front_bits.py OUT.npz"""
import os
import sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import model as O
from spwgnn_amd import TowerBatch, data as D, params as P
from spwgnn_amd.keras_api import CompactDataset, PropagationNetwork
from spwgnn_amd.replay import ReplayStep
from spwgnn_amd.trainer import Trainer

out = {}
UINT = {4: np.uint32, 8: np.uint64}


def put(name, value):
    if isinstance(value, torch.Tensor):
        torch.cuda.synchronize()
        value = value.detach().cpu().numpy()
    a = np.ascontiguousarray(np.asarray(value))
    if a.dtype.kind not in "fiu":
        a = a.astype(np.float64)
    out[name] = a.reshape(-1).view(UINT[a.dtype.itemsize]) if a.dtype.itemsize in UINT else a.reshape(-1)


def put_dict(name, d):
    for k, v in d.items():
        if isinstance(v, dict):
            put_dict(f"{name}.{k}", v)
        elif isinstance(v, list) and v and isinstance(v[0], dict):
            for i, e in enumerate(v):
                put_dict(f"{name}.{k}{i}", e)
        elif v is not None and not isinstance(v, str):
            put(f"{name}.{k}", v)


B, N = 128, 6
obj, Rs, Rr, prop, tgt = D.synthetic_batch(B, N, seed=3, fully_connected=False)
x = {"objects": obj, "sender_relations": Rs, "receiver_relations": Rr, "propagation": prop}
y = {"target": tgt.reshape(B, N, 1)}
sw = np.random.default_rng(5).choice([0.0, 0.5, 1.0, 2.5], size=(B, N)).astype(np.float32)
OPTIONS = {"plain": ({}, {}), "weighted": ({}, {"sample_weight": sw}),
           "clip": ({"clipnorm": 1.0, "decay": 1e-3}, {}), "steps": ({"step_loss_weights": (0.1, 0.1, 0.1, 0.2, 0.5)}, {})}
for name, (model_kw, fit_kw) in OPTIONS.items():
    for graph in (False, True):
        model = PropagationNetwork(seed=1, **model_kw).getModel(N)
        hist = model.fit(x, y, batch_size=32, epochs=2, validation_split=0.25, verbose=0, graph=graph, **fit_kw)
        tag = f"fit_{name}_{'graph' if graph else 'eager'}"
        put_dict(tag, hist)
        put(f"{tag}.flat", model.net.flat)
    put_dict(f"eval_{name}", model.evaluate(x, y, return_dict=True, batch_size=48, **fit_kw))
    put_dict(f"eval_steps_{name}", {"steps": model.evaluate(x, y, return_steps=True, **fit_kw)})
    put(f"predict_{name}", model.predict(x, return_steps=True))
    put(f"predict_last_{name}", model.predict(x, batch_size=48))

ds = CompactDataset(obj, Rs, Rr, prop)
target = tgt.reshape(B, N).astype(np.float32)


def shard(idx):
    return (TowerBatch.from_plan(ds.subset_plan(idx), "cuda"), torch.as_tensor(target[idx].reshape(-1), device="cuda"),
            torch.as_tensor(sw[idx].reshape(-1), device="cuda"))


def trainer(**kw):
    return Trainer(P.to_flat(O.random_params(7), device="cuda"), mp_steps=5, dropout=0.1, seed=11, **kw)


for name, cuts in (("one", (32,)), ("two", (16, 16))):
    for weighted in (False, True):
        tr = trainer()
        tag = f"step_{name}{'_weighted' if weighted else ''}"
        for step in range(3):
            at = 32 * step + np.concatenate([[0], np.cumsum(cuts)])
            parts = [shard(np.arange(a, b)) for a, b in zip(at[:-1], at[1:])]
            b_, t_, w_ = ([p[k] for p in parts] for k in range(3))
            if len(parts) == 1:
                b_, t_, w_ = b_[0], t_[0], w_[0]
            put(f"{tag}.out3_{step}", tr.step(b_, t_, weights=w_ if weighted else None))
        put(f"{tag}.params", tr.params)
        put(f"{tag}.m", tr.m)

tr = trainer()
plans = [ds.subset_plan(np.arange(32 * k, 32 * k + 32), edge_cap=True) for k in range(3)]
rs = ReplayStep(plans[0], "cuda", tr.replay_body(plans[0].n_nodes))
for k, plan in enumerate(plans):
    tr.replay_step(rs, plan, target[32 * k:32 * k + 32])
put("replay.params", tr.params)
put("replay.v", tr.v)
np.savez(sys.argv[1], **out)
print("dumped", sys.argv[1], len(out))
