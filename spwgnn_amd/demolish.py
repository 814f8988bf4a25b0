"""Batched simulator-side inference and the optional per-tower pooling (row 4).

The reference asks the GNN one B=1 `predict` per candidate:
  * `JengaBuilder.remove_to_demolish` (JengaBuilder.py:236-259): for every box i, the tower with box i
    removed → Σ_objects ŷ; the box whose removal gives the smallest sum is removed;
  * `TowerCreator.drop_to_demolish` (TowerCreator.py:276-307): 100 candidate drop positions →
    Σ ŷ each → argmin.
Here all candidates of a decision form ONE batch: one forward over the candidate towers, the
per-tower Σ sigmoid(z) on device (`spwgnn_tower_readout`), and the argmin.

Inference relations are built exactly as the reference's `predict_stabilities`
(JengaBuilder.py:309-326): coordinates are divided by 170 and then compared against the same
threshold 170, so every pair is related (fully connected towers).
"""
from __future__ import annotations

from typing import Tuple, Union

import numpy as np
import torch

from . import engine as E
from .batch import TowerBatch
from .data import RELATION_THRESHOLD
from .network import GraphNetwork

Net = Union[GraphNetwork, "object"]   # GraphNetwork or a keras_api.KerasModel (uses its .net)


def _graph_net(net) -> GraphNetwork:
    return net if isinstance(net, GraphNetwork) else net.net


def removal_candidates(boxes_raw: np.ndarray) -> np.ndarray:
    """(n, n-1, 3): candidate i is the tower with box i removed, the others in their order
    (JengaBuilder.py:244-249)."""
    boxes_raw = np.asarray(boxes_raw, np.float64)
    n = boxes_raw.shape[0]
    if n < 2:
        raise ValueError("a removal needs at least two boxes")
    keep = ~np.eye(n, dtype=bool)
    return np.stack([boxes_raw[keep[i]] for i in range(n)])


def stability_sums(net: Net, towers_raw: np.ndarray, mode: str = "sum_prob") -> torch.Tensor:
    """(C,) Σ ŷ (or another `tower_readout` mode) of each candidate tower (C, N, 3) in raw pixels,
    one batched inference forward (`predict_stabilities` semantics, JengaBuilder.py:309-329)."""
    g = _graph_net(net)
    towers_raw = np.asarray(towers_raw, np.float64)
    objects = (towers_raw / RELATION_THRESHOLD).astype(np.float32)
    batch = TowerBatch.fully_connected(objects, device=g.device)
    with torch.no_grad():
        z = E.forward(g.flat.detach(), batch, g.run_config(), E.Workspace(g.device))
        return E.tower_readout(z, batch, mode)


def stability_gradients(net: Net, towers_raw: np.ndarray, mode: str = "sum_prob") -> Tuple[torch.Tensor, torch.Tensor]:
    """`stability_sums` plus its derivative: (sums (C,), grads (C, N, 3)) with grads[c, n] =
    d sums[c] / d towers_raw[c, n] in raw-pixel units — which way to move (x, y) or resize (width) each
    box to raise the readout, and which box's position the prediction hangs on. The continuous form of
    the candidate searches above (`drop_to_demolish` refined by a gradient step).

    One training forward with dropout 0 (the inference forward's values, with the activations kept),
    one backward from d readout / d logit (σ'(z) for the "prob" modes, 1 for the "logit" modes, the
    "mean" modes divided by N) and `engine.backward_inputs`; the chain rule through the /170
    normalisation. The relation set is a constant: fully connected at inference, so nothing is lost."""
    if mode not in E.READOUT_MODES:
        raise ValueError(f"readout mode must be one of {sorted(E.READOUT_MODES)}")
    g = _graph_net(net)
    towers_raw = np.asarray(towers_raw, np.float64)
    C_, N = towers_raw.shape[:2]
    objects = (towers_raw / RELATION_THRESHOLD).astype(np.float32)
    batch = TowerBatch.fully_connected(objects, device=g.device)
    flat = g.flat.detach()
    run = g.run_config(True, dropout=0.0)
    ws = E.Workspace(g.device)
    with torch.no_grad():
        z = E.forward(flat, batch, run, ws)
        sums = E.tower_readout(z, batch, mode)
        if mode.endswith("prob"):
            p = E.sigmoid(z)
            dz = p * (1.0 - p)
        else:
            dz = torch.ones_like(z)
        if mode.startswith("mean"):
            dz = dz / N
        E.backward(flat, batch, run, ws, dz)
        dobj = E.backward_inputs(flat, batch, run, ws)
        return sums, (dobj / RELATION_THRESHOLD).reshape(C_, N, 3)


def _readout_cotangent(z: torch.Tensor, mode: str, N: int) -> torch.Tensor:
    """d readout / d logit of a `tower_readout` mode over towers of N boxes."""
    if mode.endswith("prob"):
        p = E.sigmoid(z)
        dz = p * (1.0 - p)
    else:
        dz = torch.ones_like(z)
    return dz / N if mode.startswith("mean") else dz


def relation_gradients(net: Net, towers_raw: np.ndarray, mode: str = "sum_prob") -> Tuple[torch.Tensor, torch.Tensor]:
    """`stability_sums` plus which contact each sum rests on: (sums (C,), rel (C, N, N)) with
    rel[c, s, r] = the gradient of sums[c] with respect to a scalar gate on the relation s → r (sender,
    receiver) of candidate c, in the receiver sum of Networks.py:88 alone and at the all-ones gate
    (`engine.backward_relations`; the diagonal is zero). A large |rel[c, s, r]| says the
    readout hangs on what box s tells box r; deleting that relation and re-running the forward is what it
    replaces to first order. The forward is the one of `stability_gradients`: training mode with dropout
    0 on fully connected towers, the same ``dz`` per readout mode."""
    if mode not in E.READOUT_MODES:
        raise ValueError(f"readout mode must be one of {sorted(E.READOUT_MODES)}")
    g = _graph_net(net)
    towers_raw = np.asarray(towers_raw, np.float64)
    N = towers_raw.shape[1]
    objects = (towers_raw / RELATION_THRESHOLD).astype(np.float32)
    batch = TowerBatch.fully_connected(objects, device=g.device)
    flat = g.flat.detach()
    run = g.run_config(True, dropout=0.0)
    ws = E.Workspace(g.device)
    with torch.no_grad():
        z = E.forward(flat, batch, run, ws)
        sums = E.tower_readout(z, batch, mode)
        E.backward(flat, batch, run, ws, _readout_cotangent(z, mode, N))
        drel = E.backward_relations(flat, batch, run, ws)
    return sums, torch.from_numpy(batch.edges_to_input(drel, dense=True)).to(g.device)


def remove_to_demolish(net: Net, boxes_raw: np.ndarray) -> Tuple[np.ndarray, int]:
    """Batched `JengaBuilder.remove_to_demolish` decision: (box_stabilities (n,), remove_index)."""
    sums = stability_sums(net, removal_candidates(boxes_raw)).cpu().numpy().astype(np.float64)
    return sums, int(np.argmin(sums))


def drop_to_demolish(net: Net, towers_with_drop_raw: np.ndarray) -> Tuple[np.ndarray, int]:
    """Batched `TowerCreator.drop_to_demolish` decision over C candidate towers (object 0 = the
    dropped box at each candidate position): (pos_stability (C,), index_min)."""
    sums = stability_sums(net, towers_with_drop_raw).cpu().numpy().astype(np.float64)
    return sums, int(np.argmin(sums))
