"""Evaluation metrics from the integer tables of spwgnn_eval_metrics (engine.EvalTables.cpu()): numpy only,
no GPU, no library call.

The tables (include/spwgnn.h), one leading axis of logit rows each:
  node4   (R, 4)       TP, TN, FP, FN over the counted nodes — the reference's per-block score
                       (s > 0.5) == c (JengaBuilder.py:333-346) is binary_accuracy
  tower6  (R, 6)       towers, exact, tTP, tTN, tFP, tFN — "will this tower stand"
  by_size (R, 33, 6)   TP, TN, FP, FN, towers, exact per tower size 1..32 (bucket 0: any other size): the
                       cross-size table of the paper, read from one ragged batch
  hist    (R, 2, 256)  the logit histogram per class: bin b holds the logits in [-16 + b/8, -16 + (b+1)/8),
                       the ends clamped into bins 0 and 255, NaN in bin 0

Everything the histogram yields — the ROC curve, its area, average precision, a confusion at another
threshold — is the exact value for the QUANTISED logits: every logit moved down to its bin's lower edge.
A quantised logit is predicted stable at threshold tau when 1/(1 + exp(-edge)) > tau in fp32, the device's
rule; so at tau = 0.5 the bin [0, 1/8) counts as "not stable", as a logit of exactly 0 does on the device.
A zero denominator gives NaN."""
from __future__ import annotations

import numpy as np

BINS = 256
SIZES = 33
EDGES = (np.arange(BINS, dtype=np.float32) / np.float32(8.0) - np.float32(16.0)).astype(np.float32)   # lower edges, exact
with np.errstate(over="ignore"):
    EDGE_PROBS = (np.float32(1.0) / (np.float32(1.0) + np.exp(-EDGES, dtype=np.float32))).astype(np.float32)


def _div(a, b) -> float:
    return float(a) / float(b) if b else float("nan")


def _confusion(tp: int, tn: int, fp: int, fn: int) -> dict:
    n = tp + tn + fp + fn
    prec, rec = _div(tp, tp + fp), _div(tp, tp + fn)
    return {"tp": tp, "tn": tn, "fp": fp, "fn": fn, "n": n, "binary_accuracy": _div(tp + tn, n), "precision": prec,
            "recall": rec, "specificity": _div(tn, tn + fp), "f1": _div(2 * tp, 2 * tp + fp + fn)}


def _hist2(hist) -> np.ndarray:
    h = np.asarray(hist)
    if h.shape != (2, BINS):
        raise ValueError(f"a histogram is (2, {BINS}): [class][bin] (got {h.shape}); pick a row first")
    return h.astype(np.int64)


def confusion_at(hist, threshold: float) -> dict:
    """{tp, tn, fp, fn} of the quantised logits at the probability ``threshold``: bin b is predicted stable
    when sigmoid(its lower edge) > threshold in fp32. Exact for thresholds on bin edges when no logit lies
    strictly inside the bin that starts at the threshold."""
    h = _hist2(hist)
    tau = float(threshold)
    if not 0.0 < tau < 1.0:
        raise ValueError(f"threshold must lie strictly between 0 and 1 (got {threshold})")
    stable = EDGE_PROBS > np.float32(tau)
    return {"tp": int(h[1][stable].sum()), "tn": int(h[0][~stable].sum()), "fp": int(h[0][stable].sum()),
            "fn": int(h[1][~stable].sum())}


def roc_curve(hist):
    """(fpr, tpr, thresholds) of the quantised logits, 257 points from (0, 0) to (1, 1): point j < 256
    predicts stable the bins above bin 255 − j (thresholds[j] = sigmoid of that bin's lower edge, decreasing);
    the last point predicts everything stable (threshold 0). NaN rates for an empty class."""
    h = _hist2(hist)
    neg, pos = h[0], h[1]
    N, P = int(neg.sum()), int(pos.sum())
    # above[k] = count in bins > k, k = 255 .. 0, then everything
    fp = np.concatenate([(np.cumsum(neg[::-1]) - neg[::-1]), [N]]).astype(np.float64)
    tp = np.concatenate([(np.cumsum(pos[::-1]) - pos[::-1]), [P]]).astype(np.float64)
    thr = np.concatenate([EDGE_PROBS[::-1].astype(np.float64), [0.0]])
    nan = np.full(BINS + 1, np.nan)
    return (fp / N if N else nan), (tp / P if P else nan), thr


def roc_auc(hist) -> float:
    """Σ_b neg_b·(pos_above_b + pos_b / 2) / (P·N): the exact rank AUC of the bin-quantised logits, ties
    inside a bin counting one half. NaN when a class is empty."""
    h = _hist2(hist)
    neg, pos = [int(x) for x in h[0]], [int(x) for x in h[1]]
    P, N = sum(pos), sum(neg)
    if not P or not N:
        return float("nan")
    twice, above = 0, 0   # twice the pair count, in Python ints: exact at any table size
    for b in range(BINS - 1, -1, -1):
        twice += neg[b] * (2 * above + pos[b])
        above += pos[b]
    return twice / (2 * P * N)


def average_precision(hist) -> float:
    """Σ_k (recall_k − recall_{k−1})·precision_k over the bin-edge thresholds, highest first (the step
    definition, no interpolation). NaN without a positive node."""
    h = _hist2(hist)
    P = int(h[1].sum())
    if not P:
        return float("nan")
    tp = np.cumsum(h[1][::-1]).astype(np.float64)   # stable = bins >= b, b = 255 .. 0
    fp = np.cumsum(h[0][::-1]).astype(np.float64)
    rec = tp / P
    with np.errstate(invalid="ignore", divide="ignore"):
        prec = np.where(tp + fp > 0, tp / (tp + fp), 0.0)
    return float(np.sum(np.diff(np.concatenate([[0.0], rec])) * prec))


def best_threshold(hist) -> float:
    """The bin-edge probability (or 0: everything stable) whose confusion has the highest accuracy; among
    equals the one nearest 0.5. NaN for an empty histogram."""
    h = _hist2(hist)
    fpr, tpr, thr = roc_curve(h)
    N, P = int(h[0].sum()), int(h[1].sum())
    if N + P == 0:
        return float("nan")
    tp = tpr * P if P else np.zeros(BINS + 1)
    tn = (1.0 - fpr) * N if N else np.zeros(BINS + 1)
    correct = np.rint(tp + tn)
    best = np.flatnonzero(correct == correct.max())
    return float(thr[best[np.argmin(np.abs(thr[best] - 0.5))]])


def summarize(tables: dict, row: int = -1) -> dict:
    """The metrics of one logit row of ``tables`` (EvalTables.cpu(); the last row by default):
      tp, tn, fp, fn, n, binary_accuracy, precision, recall, specificity, f1     from node4;
      towers, tower_exact_accuracy, tower_tp / _tn / _fp / _fn, tower_accuracy   from tower6, when held;
      by_size {k: the node metrics + towers, tower_exact_accuracy}               the non-empty buckets;
      roc_auc, average_precision, best_threshold                                 from hist, when held.
    Counts are Python ints; a zero denominator gives NaN."""
    out = _confusion(*(int(x) for x in np.asarray(tables["node4"])[row]))
    if tables.get("tower6") is not None:
        towers, exact, ttp, ttn, tfp, tfn = (int(x) for x in np.asarray(tables["tower6"])[row])
        out.update(towers=towers, tower_exact_accuracy=_div(exact, towers), tower_tp=ttp, tower_tn=ttn, tower_fp=tfp,
                   tower_fn=tfn, tower_accuracy=_div(ttp + ttn, towers))
    if tables.get("by_size") is not None:
        out["by_size"] = {}
        for k, cells in enumerate(np.asarray(tables["by_size"])[row]):
            tp, tn, fp, fn, towers, exact = (int(x) for x in cells)
            if towers:
                out["by_size"][k] = dict(_confusion(tp, tn, fp, fn), towers=towers, tower_exact_accuracy=_div(exact, towers))
    if tables.get("hist") is not None:
        h = np.asarray(tables["hist"])[row]
        out.update(roc_auc=roc_auc(h), average_precision=average_precision(h), best_threshold=best_threshold(h))
    return out
