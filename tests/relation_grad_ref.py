"""fp64 reference of the relation gradients: `oracle.model.forward_gather` with a scalar gate
per (step, edge) on the messages the receiver sum of Networks.py:88 adds up, and torch autograd with the
gates as leaves. At gate ≡ 1 the forward is forward_gather's, bit for bit (x · 1.0 = x).

r_{k,s} = d loss / d gate_s[k] at gate ≡ 1; r_k = Σ_s r_{k,s} (one gate shared by the steps is the sum of the
per-step gates' gradients, since the gate enters every step's sum linearly and separately).
"""
from typing import Optional

import numpy as np
import torch

from oracle import model as O

F64 = torch.float64


def forward_gather_gated(p, pos, src, dst, prop, mp_steps, gates, drop_r: Optional[torch.Tensor] = None,
                         drop_o: Optional[torch.Tensor] = None, keep: Optional[dict] = None):
    """`O.forward_gather` with gates[s] (Ne,) multiplying step s's messages before the index_add_.
    ``keep``: a dict that receives the per-step messages ("e", detached values) and receiver sums ("agg",
    graph tensors with retain_grad: their .grad after backward is g_s)."""
    diff = pos[dst, 0:2] - pos[src, 0:2]
    obj_vec = pos[:, 1:3]
    c_r = torch.relu(O._mlp(diff, p, "rm"))
    c_o = torch.relu(O._mlp(obj_vec, p, "om"))
    if drop_r is not None:
        c_r = c_r * drop_r
    if drop_o is not None:
        c_o = c_o * drop_o
    P = prop
    x = None
    for s in range(mp_steps):
        x = O._mlp(torch.cat([c_r, P[src], P[dst]], dim=-1), p, "rmp")
        agg = torch.zeros(P.shape[0], x.shape[1], dtype=x.dtype).index_add_(0, dst, x * gates[s][:, None])
        if keep is not None:
            agg.retain_grad()
            keep.setdefault("e", []).append(x.detach())
            keep.setdefault("agg", []).append(agg)
        eff = torch.tanh(agg)
        x = O._mlp(torch.cat([c_o, eff, P], dim=-1), p, "omp")
        P = torch.tanh(x[:, 1:] + P)
    return x[:, 0]


def loss_of(z, tgt, loss: str):
    """"bce": the Keras mean BCE; "sum": Σ z; "sum_prob": Σ sigmoid(z)."""
    if loss == "bce":
        return O.keras_bce_from_logits(z, torch.as_tensor(np.asarray(tgt), dtype=F64).reshape(z.shape))
    if loss == "sum":
        return z.sum()
    if loss == "sum_prob":
        return torch.sigmoid(z).sum()
    raise ValueError(loss)


def relation_grads(params, pos, src, dst, prop, S, tgt=None, loss="bce", drop_r=None, drop_o=None, keep=None):
    """(r (Ne,), r_steps (S, Ne), parameter gradients, logits) in fp64, numpy. pos (Nn, 3), src / dst (Ne,)
    global node ids, prop (Nn, 100) or None."""
    tp = O.to_torch(params, requires_grad=True)
    as64 = lambda a: None if a is None else torch.as_tensor(np.asarray(a), dtype=F64)
    src_t, dst_t = torch.as_tensor(np.asarray(src, np.int64)), torch.as_tensor(np.asarray(dst, np.int64))
    x = as64(np.asarray(pos).reshape(-1, 3))
    pr = torch.zeros(x.shape[0], 100, dtype=F64) if prop is None else as64(np.asarray(prop).reshape(-1, 100))
    gates = [torch.ones(len(src_t), dtype=F64, requires_grad=True) for _ in range(S)]
    z = forward_gather_gated(tp, x, src_t, dst_t, pr, S, gates, as64(drop_r), as64(drop_o), keep)
    loss_of(z, tgt, loss).backward()
    steps = np.stack([g.grad.numpy().copy() if g.grad is not None else np.zeros(len(src_t)) for g in gates])
    return steps.sum(0), steps, {k: v.grad.numpy().copy() for k, v in tp.items()}, z.detach().numpy().copy()
