"""fp64 restatement of the clipped Adam step (spwgnn_adam_clipped, include/spwgnn.h) —
TEST INFRASTRUCTURE ONLY.

Keras 2.x Optimizer.get_gradients (clipnorm, then clipvalue) in front of oracle.model.KerasAdam's update,
Adam's `decay`, and the library's own non-finite guard:

  g'   = grad_scale·grad + 2·l2·param
  norm = sqrt(Σ g'²) over the real parameters (the ranges of P.layout(); the padding is left out)
  clipnorm c > 0 and norm ≥ c:  g' ← g'·(c / norm)          (otherwise the scale is exactly 1)
  clipvalue v > 0:              g' ← clamp(g', −v, v)
  lr_eff = lr / (1 + decay·iterations),  iterations = t − 1;  lr_t = lr_eff·sqrt(1 − β2^t) / (1 − β1^t)
  m, v, p as KerasAdam;  skip_nonfinite and Σ g'² not finite: p, m, v unchanged, t still advances.
"""
from __future__ import annotations

import math

import numpy as np

from spwgnn_amd import params as P

KERAS_EPS = 1e-7


def real_mask() -> np.ndarray:
    """Boolean mask over the padded flat buffer: True on the real parameters."""
    mask = np.zeros(P.flat_size(), bool)
    for _, off, shape in P.layout():
        mask[off:off + int(np.prod(shape))] = True
    return mask


def grad_prime(params, grads, l2=0.0, grad_scale=1.0) -> np.ndarray:
    return grad_scale * np.asarray(grads, np.float64) + 2.0 * l2 * np.asarray(params, np.float64)


def global_norm(gp, mask=None) -> float:
    gp = np.asarray(gp, np.float64)
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.sum(np.square(gp if mask is None else gp[mask]))))


def norm_scale(norm: float, clipnorm: float) -> float:
    return clipnorm / norm if (clipnorm > 0 and norm >= clipnorm) else 1.0


def lr_t(lr, decay, beta1, beta2, t) -> float:
    lr_eff = lr * (1.0 / (1.0 + decay * (t - 1))) if decay > 0 else lr
    return lr_eff * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)


def step(params, grads, m, v, t, lr=5e-4, beta1=0.9, beta2=0.999, eps=KERAS_EPS, l2=0.0, grad_scale=1.0,
         clipnorm=0.0, clipvalue=0.0, decay=0.0, skip_nonfinite=False, mask=None, scale=None):
    """One step t >= 1 on fp64 copies. `mask`: the elements the norm covers (None = all). `scale`: use this
    norm scale instead of the restatement's own (a kernel test passes the device's reported one, so that
    the norm's rounding is judged by the norm test alone). Returns (params, m, v, info) with info =
    dict(norm, scale, skipped, clipped)."""
    p = np.asarray(params, np.float64)
    m = np.asarray(m, np.float64)
    v = np.asarray(v, np.float64)
    gp = grad_prime(p, grads, l2, grad_scale)
    norm = global_norm(gp, mask)
    skipped = bool(skip_nonfinite and not np.isfinite(norm * norm))
    own = norm_scale(norm, clipnorm)
    info = dict(norm=norm, scale=own if scale is None else float(scale), skipped=skipped,
                clipped=bool(clipnorm > 0 and norm >= clipnorm) and not skipped)
    if skipped:
        return p.copy(), m.copy(), v.copy(), info
    with np.errstate(all="ignore"):
        g = gp * info["scale"]
        if clipvalue > 0:
            g = np.where(g > clipvalue, clipvalue, np.where(g < -clipvalue, -clipvalue, g))
        m2 = beta1 * m + (1.0 - beta1) * g
        v2 = beta2 * v + (1.0 - beta2) * g * g
        p2 = p - lr_t(lr, decay, beta1, beta2, t) * m2 / (np.sqrt(v2) + eps)
    return p2, m2, v2, info


class ClippedAdam:
    """oracle.model.KerasAdam's interface with the options: `step(params, grads)` → new params (fp64);
    `last` holds the step's info."""

    def __init__(self, lr=5e-4, beta1=0.9, beta2=0.999, eps=KERAS_EPS, l2=0.0, clipnorm=0.0, clipvalue=0.0,
                 decay=0.0, skip_nonfinite=False, mask=None):
        self.kw = dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps, l2=l2, clipnorm=clipnorm, clipvalue=clipvalue,
                       decay=decay, skip_nonfinite=skip_nonfinite, mask=mask)
        self.t = 0
        self.m = self.v = None
        self.last = None

    def step(self, params, grads) -> np.ndarray:
        params = np.asarray(params, np.float64)
        if self.m is None:
            self.m = np.zeros_like(params)
            self.v = np.zeros_like(params)
        self.t += 1   # a skipped step uses its iteration up too
        p, self.m, self.v, self.last = step(params, grads, self.m, self.v, self.t, **self.kw)
        return p
