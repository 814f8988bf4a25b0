"""fp64 reference of the relation gates — TEST INFRASTRUCTURE ONLY, a plain module like
relation_grad_ref.py, whose `forward_gather_gated` is the oracle: `forward` below is that function with ONE gate
tensor shared by the steps and the final state returned beside the logits (tests/test_relation_gates_host.py holds
the two equal bit for bit).

The inputs are the cases of tests/test_gpu_input_grad.py; the gates are `gates_for`: uniform(0.25, 1.5) from
default_rng(seed), the first three set to 0, 1 and −0.5. `gated_margins` is `oracle.model.relu_margins_gather`
under the gated forward: per tower the smallest |pre-activation| of every ReLU and the logit's distance to the BCE
clip. No tower is ever left out: a case whose margin falls below TAU takes the next gate seed.
"""
import numpy as np
import torch

import relation_grad_ref as RR
from oracle import model as O

F64 = torch.float64
TAU = 1e-6          # the project's kink margin (tests/test_gpu_chain_parity.py)
GATE_SEED = 1000


def gates_for(n_edges: int, seed: int = GATE_SEED) -> np.ndarray:
    g = np.random.default_rng(seed).uniform(0.25, 1.5, n_edges).astype(np.float32)
    g[:3] = (0.0, 1.0, -0.5)
    return g


def forward(p, pos, src, dst, prop, mp_steps, gate, drop_r=None, drop_o=None):
    """(logits (Nn,), final state (Nn, 100)): RR.forward_gather_gated with gates[s] = gate for every step."""
    diff = pos[dst, 0:2] - pos[src, 0:2]
    c_r = torch.relu(O._mlp(diff, p, "rm"))
    c_o = torch.relu(O._mlp(pos[:, 1:3], p, "om"))
    if drop_r is not None:
        c_r = c_r * drop_r
    if drop_o is not None:
        c_o = c_o * drop_o
    P, x = prop, None
    for _ in range(mp_steps):
        x = O._mlp(torch.cat([c_r, P[src], P[dst]], dim=-1), p, "rmp")
        agg = torch.zeros(P.shape[0], x.shape[1], dtype=x.dtype).index_add_(0, dst, x * gate[:, None])
        x = O._mlp(torch.cat([c_o, torch.tanh(agg), P], dim=-1), p, "omp")
        P = torch.tanh(x[:, 1:] + P)
    return x[:, 0], P


def _tensors(c):
    src = torch.as_tensor(np.asarray(c["src"], np.int64))
    dst = torch.as_tensor(np.asarray(c["dst"], np.int64))
    return src, dst


def gated_margins(c, gate, sizes=None) -> np.ndarray:
    """Per tower: the smallest ReLU pre-activation distance (and logit-to-clip distance) of the GATED fp64 forward."""
    sizes = np.full(c["B"], c["N"]) if sizes is None else np.asarray(sizes)
    tower = torch.as_tensor(np.repeat(np.arange(len(sizes)), sizes))
    p = O.to_torch(c["params"])
    src, dst = _tensors(c)
    x = torch.as_tensor(np.asarray(c["obj"], np.float64).reshape(-1, 3))
    P = torch.as_tensor(np.asarray(c["prop"], np.float64).reshape(-1, 100))
    w = torch.as_tensor(np.asarray(gate, np.float64))
    et = tower[dst]
    marg = torch.full((len(sizes),), float("inf"), dtype=F64)

    def note(pre, rows_tower):
        marg.scatter_reduce_(0, rows_tower, pre.abs().amin(dim=1), reduce="amin")

    with torch.no_grad():
        h = x[dst, 0:2] - x[src, 0:2]
        for i in range(4):
            h = h @ p[f"rm.{i}.kernel"] + p[f"rm.{i}.bias"]
            note(h, et)
            h = torch.relu(h)
        c_r = h
        h = x[:, 1:3]
        for i in range(2):
            h = h @ p[f"om.{i}.kernel"] + p[f"om.{i}.bias"]
            note(h, tower)
            h = torch.relu(h)
        c_o, z = h, None
        for _ in range(c["S"]):
            h = torch.cat([c_r, P[src], P[dst]], dim=-1)
            for i in range(2):
                h = h @ p[f"rmp.{i}.kernel"] + p[f"rmp.{i}.bias"]
                note(h, et)
                h = torch.relu(h)
            msg = (h @ p["rmp.2.kernel"] + p["rmp.2.bias"]) * w[:, None]
            agg = torch.zeros(len(x), msg.shape[1], dtype=F64).index_add_(0, dst, msg)
            h = torch.cat([c_o, torch.tanh(agg), P], dim=-1) @ p["omp.0.kernel"] + p["omp.0.bias"]
            note(h, tower)
            xo = torch.relu(h) @ p["omp.1.kernel"] + p["omp.1.bias"]
            P = torch.tanh(xo[:, 1:] + P)
            z = xo[:, 0]
        note((z.abs() - O.LOGIT_CLIP)[:, None], tower)
    return marg.numpy()


def pick_gates(c, sizes=None, seed: int = GATE_SEED):
    """(gates, seed): the first seed from `seed` on whose gated margins all exceed TAU (no tower is left out)."""
    for s in range(seed, seed + 40):
        g = gates_for(len(c["src"]), s)
        if np.all(gated_margins(c, g, sizes) > TAU):
            return g, s
    raise AssertionError("no gate seed gives every tower a ReLU margin above TAU")


_REFS = {}


def oracle(c, gate, loss="bce", key=None, dstate=None):
    """fp64 autograd with the parameters, the objects, the propagation input and ONE shared gate tensor as leaves.
    Returns a dict: z, state, g (parameter gradients), dprop, dobj, dgate — numpy. ``dstate`` (Nn, 100): the loss
    gains Σ dstate·P_S."""
    k = None if key is None else (key, loss, dstate is not None)
    if k is not None and k in _REFS:
        return _REFS[k]
    tp = O.to_torch(c["params"], requires_grad=True)
    src, dst = _tensors(c)
    x = torch.tensor(np.asarray(c["obj"], np.float64).reshape(-1, 3), requires_grad=True)
    pr = torch.tensor(np.asarray(c["prop"], np.float64).reshape(-1, 100), requires_grad=True)
    w = torch.tensor(np.asarray(gate, np.float64), requires_grad=True)
    z, state = forward(tp, x, src, dst, pr, c["S"], w)
    L = RR.loss_of(z, c["tgt"], loss)
    if dstate is not None:
        L = L + (torch.as_tensor(np.asarray(dstate, np.float64)) * state).sum()
    L.backward()
    out = dict(z=z.detach().numpy().copy(), state=state.detach().numpy().copy(),
               g={n: v.grad.numpy().copy() for n, v in tp.items()}, dprop=pr.grad.numpy().copy(),
               dobj=x.grad.numpy().copy(), dgate=w.grad.numpy().copy())
    if k is not None:
        _REFS[k] = out
    return out


def soft_threshold_gates(raw_xy, src, dst, threshold: float, tau: float):
    """sigmoid((threshold − ‖raw_src.xy − raw_dst.xy‖) / tau) per edge, torch (any dtype), differentiable in raw_xy."""
    d = (raw_xy[src] - raw_xy[dst]).norm(dim=-1)
    return torch.sigmoid((threshold - d) / tau)
