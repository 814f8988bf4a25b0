"""x3-math emulation (SPWGNN_MATH_X3, include/spwgnn.h) — TEST INFRASTRUCTURE ONLY.

oracle/bf16.py's factored graph with two substitutions, made for the duration of a `with x3():`
block and undone afterwards:

  * OB.b16   x ↦ h + m with h = bf16(x), m = bf16(x − h): the two-part rounding. It is what the
             one-hot products (the receiver sum of h2, the sender / receiver sums of dh1pre) and the
             bias gradients (the ones column) sum, and what rm.0 / om.0's weight gradients multiply.
  * OB._MM   Y  = X_h·W_h + X_h·W_m + X_m·W_h
             dX = G_h·W_hᵀ + G_h·W_mᵀ + G_m·W_hᵀ
             dW = X_hᵀ·G_h + X_hᵀ·G_m + X_mᵀ·G_h      (every product through OB.mm: k-blocks work)

Call the graph with training=False: x3 stores A, U and V in fp32, so they are not rounded.
`MUTANT` removes one product term (the calibration's wrong implementations): "fwd" drops X_m·W_h
from Y, "dw" drops X_mᵀ·G_h from dW.
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from oracle import bf16 as OB
from oracle import model as O
from spwgnn_amd import data as D

MUTANT = None   # None | "fwd" | "dw"

_b16 = OB.b16   # the one-part rounding (identity when OB.ROUND is off)


def split(x):
    """(h, m): the first two parts of the engine's split2 (RNE at each stage)."""
    h = _b16(x)
    return h, _b16(x - h)


def b16x2(x):
    h, m = split(x)
    return h + m


class _MM3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        xh, xm = split(x)
        wh, wm = split(w)
        ctx.save_for_backward(xh, xm, wh, wm)
        y = OB.mm(xh, wh) + OB.mm(xh, wm)
        return y if MUTANT == "fwd" else y + OB.mm(xm, wh)

    @staticmethod
    def backward(ctx, g):
        xh, xm, wh, wm = ctx.saved_tensors
        gh, gm = split(g)
        dx = OB.mm(gh, wh.T) + OB.mm(gh, wm.T) + OB.mm(gm, wh.T)
        dw = OB.mm(xh.T, gh) + OB.mm(xh.T, gm)
        return dx, dw if MUTANT == "dw" else dw + OB.mm(xm.T, gh)


@contextlib.contextmanager
def x3(mutant=None):
    """oracle.bf16 computes the x3 arithmetic inside the block."""
    global MUTANT
    old = (OB.b16, OB._MM, MUTANT)
    OB.b16, OB._MM, MUTANT = b16x2, _MM3, mutant
    try:
        yield
    finally:
        OB.b16, OB._MM, MUTANT = old


def loss_and_grads(params, pos, src, dst, prop, target, S=5, drop_r=None, drop_o=None, mutant=None, **kw):
    with x3(mutant):
        return OB.loss_and_grads(params, pos, src, dst, prop, target, S, drop_r, drop_o, training=False, **kw)


def noise_band(params, pos, src, dst, prop, target, S=5, drop_r=None, drop_o=None):
    """(ref, band) as OB.noise_band gives them, for the x3 arithmetic: ref the fp64 x3 emulator's (loss,
    logits, grads), band the largest distance from it over its fp32 variants (k-blocks of
    OB.NOISE_KBLOCKS) — {"z_rms", "z_max", "loss", "g": {name: relative L2}}."""
    args = (params, pos, src, dst, prop, target, S, drop_r, drop_o)
    ref = loss_and_grads(*args)
    band = {"z_rms": 0.0, "z_max": 0.0, "loss": 0.0, "g": {k: 0.0 for k in ref[2]}}
    for kb in OB.NOISE_KBLOCKS:
        d = distances(loss_and_grads(*args, dtype=torch.float32, kblock=kb), ref)
        for k in ("z_rms", "z_max", "loss"):
            band[k] = max(band[k], d[k])
        for k in d["g"]:
            band["g"][k] = max(band["g"][k], d["g"][k])
    return ref, band


def bf16_ref(params, pos, src, dst, prop, target, S=5, drop_r=None, drop_o=None):
    """The fp64 bf16 emulator on the same batch (training forward: A, U, V stored rounded)."""
    return OB.loss_and_grads(params, pos, src, dst, prop, target, S, drop_r, drop_o)


# ------------------------------------------------------------------------------------ parameter sets
RELU_BIASES = ("rm.0", "rm.1", "rm.2", "rm.3", "om.0", "om.1", "rmp.0", "rmp.1", "omp.0")


def kink_free_params(seed):
    """Random parameters with every kernel × 0.25 and every ReLU layer's bias 0.25·b + 1: the
    pre-activations stay away from 0, so no product rounding flips a ReLU mask."""
    p = {k: np.array(v, copy=True) for k, v in O.random_params(seed).items()}
    for k in p:
        if k.endswith(".kernel"):
            p[k] = p[k] * 0.25
    for name in RELU_BIASES:
        p[name + ".bias"] = 0.25 * p[name + ".bias"] + 1.0
    return p


# ------------------------------------------------------------------------------------------- batches
def dense_case(T, N, fully, seed=2, prop_scale=0.3):
    """(obj, Rs, Rr, prop, tgt, src, dst): a dense batch with a non-zero 'propagation' input
    (prop_scale 0: zeros) and its edge list in the oracle's slot order."""
    obj, Rs, Rr, prop, tgt = D.synthetic_batch(T, N, seed=seed, fully_connected=fully)
    if prop_scale:
        prop = np.random.default_rng(seed + 7).normal(0, prop_scale, prop.shape).astype(np.float32)
    e = np.array(O.dense_to_edges(Rs, Rr), np.int64).reshape(-1, 4)      # (tower, slot, sender, receiver)
    return obj, Rs, Rr, prop, tgt, e[:, 0] * N + e[:, 2], e[:, 0] * N + e[:, 3], e


def emu_args(case, S=5):
    obj, _, _, prop, tgt, src, dst, _ = case
    return (obj.reshape(-1, 3), src, dst, prop.reshape(-1, 100), tgt.reshape(-1), S)


def distances(got, ref):
    """{"z_max", "z_rms", "loss", "g": {name: rel L2}} of (loss, logits, grads) `got` from `ref`."""
    dz = np.asarray(got[1], np.float64).reshape(-1) - ref[1]
    return {"z_max": float(np.abs(dz).max()), "z_rms": float(np.sqrt(np.mean(dz ** 2))),
            "loss": abs(float(got[0]) - ref[0]), "g": {k: OB.rel_l2(got[2][k], r) for k, r in ref[2].items()}}
