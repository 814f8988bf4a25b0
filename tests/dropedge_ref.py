"""Numpy restatement of the DropEdge mask (spwgnn_dropedge_gates) — TEST INFRASTRUCTURE ONLY, a
plain module like relation_gates_ref.py. Built from `oracle.dropout.mix32` / `row_key` with kind 3:

    keep = mix32(row_key(key, 3, tower, a, b) ^ 0) >= floor(rate·2^32),   (a, b) → (min, max) when symmetric
    gate = base · (keep ? scale : 0),   scale = 1/(1 − rate) in fp32 when rescaled, else 1,   padding slots 0
"""
import numpy as np

from oracle import dropout as DR

KIND = 3


def thresh(rate) -> int:
    """floor(rate·2^32) of the fp32 rate, as the library forms it in double."""
    return min(0xFFFFFFFF, int(np.floor(float(np.float32(rate)) * 4294967296.0)))


def keep(key: int, tower, a, b, rate, symmetric: bool = True) -> np.ndarray:
    """Whether edge (tower, sender's local index a → receiver's local index b) is kept under `key` (bool array)."""
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    if symmetric:
        a, b = np.minimum(a, b), np.maximum(a, b)
    rk = DR.row_key(int(key) & 0xFFFFFFFFFFFFFFFF, KIND, tower, a, b)
    return DR.mix32(rk ^ np.uint64(0)) >= np.uint64(thresh(rate))


def scale(rate, rescale: bool) -> np.float32:
    return np.float32(1.0) / (np.float32(1.0) - np.float32(rate)) if rescale else np.float32(1.0)


def slot_gates(edge_src, edge_dst, node_tower, node_local, key: int, rate, symmetric: bool = True,
               rescale: bool = False, base=None) -> np.ndarray:
    """The (32·n_eblocks,) fp32 gates of a plan's edge-slot arrays: what spwgnn_dropedge_gates writes."""
    es, ed = np.asarray(edge_src, np.int64), np.asarray(edge_dst, np.int64)
    nt, nl = np.asarray(node_tower, np.int64), np.asarray(node_local, np.int64)
    ok = (es >= 0) & (ed >= 0)
    s, d = np.where(ok, es, 0), np.where(ok, ed, 0)
    k = keep(key, nt[s], nl[s], nl[d], rate, symmetric)
    g = np.where(k, scale(rate, rescale), np.float32(0.0)).astype(np.float32)
    if base is not None:
        g = np.asarray(base, np.float32) * g
    return np.where(ok, g, np.float32(0.0)).astype(np.float32)


def batch_gates(batch, key: int, rate, symmetric: bool = True, rescale: bool = False, base=None) -> np.ndarray:
    """`slot_gates` of a TowerBatch (its arrays on any device)."""
    arr = lambda t: t.detach().cpu().numpy()
    return slot_gates(arr(batch.edge_src), arr(batch.edge_dst), arr(batch.node_tower), arr(batch.node_local), key, rate,
                      symmetric, rescale, None if base is None else arr(base))
