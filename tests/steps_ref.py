"""The fp64 oracle of per-step logits and of the deep-supervision loss Σ_s λ_s·BCE(z_s, y).

The oracle needs no change for them: step s's logit of an S-step run IS the final logit of the same
network run with s + 1 steps (the step loop of Networks.py:83-91 has no look-ahead), so
    z_s = oracle.model.forward_dense(..., mp_steps = s + 1)
and the gradient of the loss is torch autograd over that sum. `step_logits_from_states` is the check of that
statement (tests/test_steps_host.py): the same rows recomputed from the states one S-step run returns.

A batch is a list of groups (objects (B, N, 3), Rs, Rr) of equal-size towers, node rows concatenated in
group order (the input's node order of tests/test_gpu_state.py's Case)."""
import numpy as np
import torch

from oracle import dropout as DR
from oracle import model as O

F64 = torch.float64


def _masks(drop_seed, rate, t0, B, N):
    if not rate:
        return None, None
    towers = t0 + np.arange(B)
    return (torch.as_tensor(DR.relation_mask_towers(drop_seed, rate, towers, N), dtype=F64),
            torch.as_tensor(DR.object_mask_towers(drop_seed, rate, towers, N), dtype=F64))


def _forward(tp, groups, objs, prop, steps, drop_seed=None, rate=0.0, return_state=False):
    zs, sts, off, t0 = [], [], 0, 0
    for (obj, Rs, Rr), o in zip(groups, objs):
        B, N = obj.shape[:2]
        dr, do = _masks(drop_seed, rate, t0, B, N)
        z, states = O.forward_dense(tp, o, torch.as_tensor(Rs, dtype=F64), torch.as_tensor(Rr, dtype=F64),
                                    prop[off:off + B * N].reshape(B, N, 100), steps, dr, do, return_state=True)
        zs.append(z.reshape(-1))
        sts.append([s.reshape(-1, 100) for s in states])
        off, t0 = off + B * N, t0 + B
    if return_state:
        return torch.cat(zs), [torch.cat([g[k] for g in sts]) for k in range(steps + 1)]
    return torch.cat(zs)


def step_logits(tp, groups, objs, prop, S, drop_seed=None, rate=0.0):
    """(S, n) fp64 torch: row s = the logits of the network run with s + 1 steps (autograd through tp, objs, prop)."""
    return torch.stack([_forward(tp, groups, objs, prop, s + 1, drop_seed, rate) for s in range(S)])


def final_state(tp, groups, objs, prop, S):
    return _forward(tp, groups, objs, prop, S, return_state=True)[1][-1]


def step_logits_from_states(tp, groups, objs, prop, S):
    """The same rows from ONE S-step run: z_s = the logit of one more step started from states[s] = P_s."""
    _, states = _forward(tp, groups, objs, prop, S, return_state=True)
    return torch.stack([_forward(tp, groups, objs, states[s], 1) for s in range(S)])


def bce_row(z, t, w=None, norm=None):
    """Keras binary_crossentropy of one row, torch fp64: mean over n, or Σ w·bce / norm with node weights
    (a zero weight masks its node)."""
    zc = torch.clamp(z, -O.LOGIT_CLIP, O.LOGIT_CLIP)
    per = torch.clamp(zc, min=0) - zc * t + torch.log1p(torch.exp(-torch.abs(zc)))
    if w is None:
        return per.mean()
    return torch.where(w != 0, w * per, torch.zeros_like(per)).sum() / norm


def deep_loss(Z, t, lam, w=None, norm=None):
    """Σ_s λ_s·BCE(Z[s], t); a step of zero weight is left out (not multiplied)."""
    terms = [float(l) * bce_row(Z[s], t, w, norm) for s, l in enumerate(lam) if l != 0]
    return sum(terms[1:], terms[0])


def bce_steps_numpy(Z32, t, lam, w=None, norm=None):
    """What spwgnn_bce_steps returns, in fp64 numpy from fp32 logits: out3s (S, 3), out3 (3,), dlogits (S, n),
    each row through oracle.model.keras_bce_grad (weighted: its expressions times w / norm)."""
    Z = np.asarray(Z32, np.float64)
    t = np.asarray(t, np.float64)
    S, n = Z.shape
    out3s, dl = np.zeros((S, 3)), np.zeros((S, n))
    for s in range(S):
        if w is None:
            loss, g = O.keras_bce_grad(Z[s], t)
            on = np.ones(n, bool)
        else:
            w64 = np.asarray(w, np.float64)
            on = w64 != 0
            z = np.clip(Z[s], -O.LOGIT_CLIP, O.LOGIT_CLIP)
            per = np.maximum(z, 0) - z * t + np.log1p(np.exp(-np.abs(z)))
            loss = float(np.where(on, w64 * per, 0.0).sum() / norm)
            g = np.where(on & (np.abs(Z[s]) < O.LOGIT_CLIP), w64 * (1.0 / (1.0 + np.exp(-Z[s])) - t) / norm, 0.0)
        correct = int((on & ((Z[s] > 0).astype(np.float64) == t)).sum())
        out3s[s] = (loss, correct, int(on.sum()))
        dl[s] = lam[s] * g if lam[s] != 0 else 0.0
    comb = sum(lam[s] * out3s[s, 0] for s in range(S) if lam[s] != 0)
    return out3s, np.array([comb, out3s[-1, 1], out3s[-1, 2]]), dl
