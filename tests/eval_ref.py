"""numpy restatement of spwgnn_eval_metrics (include/spwgnn.h) — TEST INFRASTRUCTURE ONLY, the
role clip_ref.py and steps_ref.py play for their features. float32 for the probability and the bin
expression, exactly as the header spells them; Python ints for the tables (returned as int64 arrays).

The one thing numpy cannot restate bit for bit is expf: the device's may differ from numpy's by an ulp, so
a test's logits keep |sigmoid(z) − tau| >= MARGIN (`margin_ok`) except where p is exactly tau by
construction (z = 0 at tau = 0.5: exp(-0) = 1 and 1/(1 + 1) = 0.5 in any arithmetic)."""
from __future__ import annotations

import numpy as np

BINS, SIZES = 256, 33
MARGIN = 1e-4
F = np.float32


def probability(z) -> np.ndarray:
    """p = 1.f / (1.f + expf(-z)) in float32."""
    z = np.asarray(z, F)
    with np.errstate(over="ignore", invalid="ignore"):
        return (F(1.0) / (F(1.0) + np.exp(-z, dtype=F))).astype(F)


def bins(z) -> np.ndarray:
    """isnan(z) ? 0 : (int)floorf((fminf(fmaxf(z, -16.f), 15.9375f) + 16.f) * 8.f), float32 throughout."""
    z = np.asarray(z, F)
    nan = np.isnan(z)
    c = np.minimum(np.maximum(np.where(nan, F(0.0), z), F(-16.0)), F(15.9375)).astype(F)
    b = np.floor(((c + F(16.0)).astype(F) * F(8.0)).astype(F)).astype(np.int64)
    return np.where(nan, 0, b)


def margin_ok(z, tau: float) -> np.ndarray:
    """Per logit: its verdict at `tau` cannot hinge on the last bit of expf — |sigmoid(z) − tau| >= MARGIN in
    fp64 for a finite logit other than exact 0; ±inf and NaN have a verdict of their own."""
    z = np.asarray(z, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        far = np.abs(1.0 / (1.0 + np.exp(-z)) - tau) >= MARGIN
    return far | ~np.isfinite(z) | ((z == 0) & (tau == 0.5))


def eval_ref(logits, targets, weights=None, offsets=None, threshold=0.5) -> dict:
    """{"node4": (R, 4), "tower6": (R, 6), "by_size": (R, 33, 6), "hist": (R, 2, 256)} int64; the tower tables
    only with `offsets` ((T + 1,) node offsets)."""
    z = np.asarray(logits, F)
    z = z.reshape(1, -1) if z.ndim == 1 else z
    R, n = z.shape
    t = np.asarray(targets, F).reshape(-1)
    assert t.shape == (n,)
    on = np.ones(n, bool) if weights is None else (np.asarray(weights, F).reshape(-1) != 0)
    tau = F(threshold)
    node4 = [[0] * 4 for _ in range(R)]
    hist = [[[0] * BINS for _ in range(2)] for _ in range(R)]
    tower6 = [[0] * 6 for _ in range(R)]
    by_size = [[[0] * 6 for _ in range(SIZES)] for _ in range(R)]
    for r in range(R):
        pred = probability(z[r]) > tau                        # False for a NaN
        ok = np.where(pred, F(1.0), F(0.0)).astype(F) == t
        cell = np.where(pred, np.where(ok, 0, 2), np.where(ok, 1, 3))   # TP, TN, FP, FN
        b = bins(z[r])
        cls = (t == F(1.0)).astype(int)
        for i in np.flatnonzero(on):
            node4[r][cell[i]] += 1
            hist[r][cls[i]][b[i]] += 1
        if offsets is None:
            continue
        off = [int(x) for x in offsets]
        for u in range(len(off) - 1):
            lo, hi = min(max(off[u], 0), n), min(max(off[u + 1], 0), n)
            idx = [i for i in range(lo, hi) if on[i]]
            if not idx:
                continue
            size = off[u + 1] - off[u]
            k = size if 1 <= size <= 32 else 0
            exact = all(ok[i] for i in idx)
            pstable = all(pred[i] for i in idx)
            astable = all(t[i] == F(1.0) for i in idx)
            for i in idx:
                by_size[r][k][cell[i]] += 1
            by_size[r][k][4] += 1
            by_size[r][k][5] += int(exact)
            tower6[r][0] += 1
            tower6[r][1] += int(exact)
            tower6[r][2 + (0 if pstable and astable else 1 if not pstable and not astable else 2 if pstable else 3)] += 1
    out = {"node4": np.array(node4, np.int64), "hist": np.array(hist, np.int64)}
    if offsets is not None:
        out.update(tower6=np.array(tower6, np.int64), by_size=np.array(by_size, np.int64))
    return out
