"""fp64 restatement of the tower-level loss (spwgnn_bce_tower, include/spwgnn.h) — TEST
INFRASTRUCTURE ONLY, the role eval_ref.py and steps_ref.py play for their features. numpy for the kernel
tests (per-tower values and the hand-written gradient), torch for the autograd oracle.

The clip edges are the float32 values the header spells (logf(1e-7f), log1pf(−1e-7f)) taken as fp64 numbers:
the reference clips where the kernel clips, and a test leaves out the towers whose s_u lies within
EDGE_MARGIN (relative) of an edge, where the last bits of the fp32 sum decide the side."""
from __future__ import annotations

import numpy as np
import torch

F = np.float32
LO = float(np.log(F(1e-7), dtype=F))
HI = float(np.log1p(F(-1e-7), dtype=F))
LN2 = 0.6931471805599453
EDGE_MARGIN = 1e-3
LOGIT_CLIP = 16.11809565      # loss_blocks.h kLogitClip: the node row's clip


def log1mexp(x):
    x = np.asarray(x, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x > -LN2, np.log(-np.expm1(x)), np.log1p(-np.exp(x)))


def neg_log_sigmoid(z):
    """q = max(−z, 0) + log1p(exp(−|z|)) in fp64."""
    z = np.asarray(z, np.float64)
    return np.maximum(-z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def towers_ref(logits, offsets, targets=None, tower_targets=None, weights=None) -> dict:
    """Per tower (fp64 arrays of length T): counted (nodes), s, T (0/1), inside, loss, g, correct (bool),
    near_edge (bool: |s − edge| <= EDGE_MARGIN·|edge| for either edge). Skipped towers have counted 0 and
    loss 0."""
    z = np.asarray(logits, np.float64).reshape(-1)
    n = z.size
    off = [int(x) for x in offsets]
    T = len(off) - 1
    on = np.ones(n, bool) if weights is None else (np.asarray(weights).reshape(-1) != 0)
    with np.errstate(over="ignore", invalid="ignore"):
        q = neg_log_sigmoid(z)
        pred = 1.0 / (1.0 + np.exp(-z)) > 0.5
    out = {k: np.zeros(T) for k in ("counted", "s", "T", "loss", "g")}
    out.update(inside=np.zeros(T, bool), correct=np.zeros(T, bool), near_edge=np.zeros(T, bool))
    for u in range(T):
        lo, hi = min(max(off[u], 0), n), min(max(off[u + 1], 0), n)
        idx = [i for i in range(lo, hi) if on[i]]
        out["counted"][u] = len(idx)
        if not idx:
            continue
        s = -float(np.sum(q[idx]))
        if tower_targets is not None:
            Tu = float(tower_targets[u]) == 1.0
        else:
            Tu = all(float(targets[i]) == 1.0 for i in idx)
        sc = min(max(s, LO), HI)
        inside = LO < s < HI
        out["s"][u], out["T"][u], out["inside"][u] = s, float(Tu), inside
        out["loss"][u] = -sc if Tu else -float(log1mexp(sc))
        out["g"][u] = (-1.0 if Tu else 1.0 / np.expm1(-s)) if inside else 0.0
        out["correct"][u] = all(pred[i] for i in idx) == Tu
        out["near_edge"][u] = abs(s - LO) <= EDGE_MARGIN * abs(LO) or abs(s - HI) <= EDGE_MARGIN * abs(HI)
    return out


def tower_loss_ref(logits, offsets, targets=None, tower_targets=None, weights=None, mu=1.0, norm_t=None) -> tuple:
    """(L_tower, d_tower (n,), towers_ref's dict): L_tower = Σ loss_u / norm_t, d_tower_i = mu·g_u·σ(−z_i) / norm_t
    for the counted nodes and 0 elsewhere. norm_t None: the counted towers, at least 1."""
    z = np.asarray(logits, np.float64).reshape(-1)
    tw = towers_ref(z, offsets, targets, tower_targets, weights)
    if norm_t is None:
        norm_t = max(int((tw["counted"] > 0).sum()), 1)
    on = np.ones(z.size, bool) if weights is None else (np.asarray(weights).reshape(-1) != 0)
    d = np.zeros(z.size)
    off = [int(x) for x in offsets]
    with np.errstate(over="ignore"):
        sig_neg = 1.0 / (1.0 + np.exp(z))
    for u in range(len(off) - 1):
        lo, hi = min(max(off[u], 0), z.size), min(max(off[u + 1], 0), z.size)
        for i in range(lo, hi):
            if on[i]:
                d[i] = mu * tw["g"][u] * sig_neg[i] / norm_t
    return float(tw["loss"].sum() / norm_t), d, tw


def node_loss_ref(logits, targets, weights=None, norm=None) -> tuple:
    """(L_node, d_node): Keras BCE with the logit clip, the weighted form with `weights` (divisor `norm`,
    default the non-zero count) — the fp64 of spwgnn_bce / spwgnn_bce_weighted."""
    z64 = np.asarray(logits, np.float64).reshape(-1)
    t = np.asarray(targets, np.float64).reshape(-1)
    w = np.ones_like(z64) if weights is None else np.asarray(weights, np.float64).reshape(-1)
    on = w != 0
    if norm is None:
        norm = z64.size if weights is None else max(int(on.sum()), 1)
    z = np.clip(z64, -LOGIT_CLIP, LOGIT_CLIP)
    per = np.maximum(z, 0) - z * t + np.log1p(np.exp(-np.abs(z)))
    loss = float(np.where(on, w * per, 0.0).sum() / norm)
    with np.errstate(over="ignore"):
        g = np.where(on & (np.abs(z64) < LOGIT_CLIP), w * (1.0 / (1.0 + np.exp(-z64)) - t) / norm, 0.0)
    return loss, g


def combined_ref(logits, offsets, targets=None, tower_targets=None, weights=None, alpha=1.0, mu=1.0, norm=None,
                 norm_t=None) -> tuple:
    """(L, dlogits, parts): L = alpha·L_node + mu·L_tower, parts = the out6 of the kernel in fp64."""
    lt, dt, tw = tower_loss_ref(logits, offsets, targets, tower_targets, weights, mu, norm_t)
    n = np.asarray(logits).size
    on = np.ones(n, bool) if weights is None else (np.asarray(weights).reshape(-1) != 0)
    if targets is None:
        assert alpha == 0
        ln, dn = 0.0, np.zeros(n)
    else:
        ln, dn = node_loss_ref(logits, targets, weights, norm)
    counted = tw["counted"] > 0
    parts = [ln, float("nan"), float(on.sum()), lt, float((tw["correct"] & counted).sum()), float(counted.sum())]
    return alpha * ln + mu * lt, alpha * dn + dt, parts


# ------------------------------------------------------------------------------------------ torch (autograd)
def tower_loss_torch(z: torch.Tensor, offsets, targets=None, tower_targets=None, weights=None, norm_t=None) -> torch.Tensor:
    """L_tower of fp64 logits `z` under autograd: the same definition, the clip as a clamp (zero gradient
    outside, as g_u = 0)."""
    off = [int(x) for x in offsets]
    n = z.numel()
    on = torch.ones(n, dtype=torch.bool) if weights is None else (torch.as_tensor(weights).reshape(-1) != 0)
    q = torch.clamp(-z, min=0.0) + torch.log1p(torch.exp(-z.abs()))
    losses = []
    for u in range(len(off) - 1):
        idx = [i for i in range(off[u], off[u + 1]) if bool(on[i])]
        if not idx:
            continue
        s = -q[idx].sum()
        if tower_targets is not None:
            Tu = float(tower_targets[u]) == 1.0
        else:
            Tu = all(float(targets[i]) == 1.0 for i in idx)
        sc = torch.clamp(s, LO, HI)
        if Tu:
            losses.append(-sc)
        elif float(sc.detach()) > -LN2:
            losses.append(-torch.log(-torch.expm1(sc)))
        else:
            losses.append(-torch.log1p(-torch.exp(sc)))
    if norm_t is None:
        norm_t = max(len(losses), 1)
    return torch.stack(losses).sum() / norm_t if losses else z.sum() * 0.0


def node_loss_torch(z: torch.Tensor, targets, weights=None, norm=None) -> torch.Tensor:
    """L_node under autograd (the logit clip as a clamp: zero gradient outside, as bce_dlogit)."""
    t = torch.as_tensor(np.asarray(targets, np.float64)).reshape(-1)
    zc = torch.clamp(z, -LOGIT_CLIP, LOGIT_CLIP)
    per = torch.clamp(zc, min=0.0) - zc * t + torch.log1p(torch.exp(-zc.abs()))
    if weights is None:
        return per.sum() / (norm or z.numel())
    w = torch.as_tensor(np.asarray(weights, np.float64)).reshape(-1)
    on = w != 0
    return torch.where(on, w * per, torch.zeros_like(per)).sum() / (norm or max(int(on.sum()), 1))
