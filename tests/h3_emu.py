"""h3-math emulation (SPWGNN_MATH_H3, include/spwgnn.h) — TEST INFRASTRUCTURE ONLY.

oracle/bf16.py's factored graph with three substitutions, made for the duration of a `with h3():`
block and undone afterwards:

  * OB._MM     Y = X_m·W_h + X_h·W_m + X_h·W_h with the two-part fp16 split h = f16(x), m = f16(x − h)
               (RNE, subnormal halves kept, |x| ≥ 65,520 → inf), every product through OB.mm so that
               k-blocks work. The backward takes the UNROUNDED operands, dX = G·Wᵀ, dW = Xᵀ·G: h3's
               backward is x6's, which has no emulator and whose error lies inside the fp32 band.
  * OB._Round  the forward's one rounding outside a product, h2 in the receiver sum: x ↦ h + m (the
               exact one-hot times the two fp16 parts); identity backward, as before.
  * OB.b16     the identity: with _MM and _Round replaced, only backward code still calls it (bias
               gradients, the sender / receiver sums of dh1pre, rm.0 / om.0's weight gradients), and
               h3's backward does not round to 16 bits anywhere x6 does not.

Call the graph with training=False: h3 stores A, U and V in fp32, so they are not rounded.
`MUTANT = "fwd"` drops X_m·W_h from Y (the calibration's wrong implementation).
Batches, parameter sets and distances are x3_emu's.
"""
from __future__ import annotations

import contextlib

import torch

from oracle import bf16 as OB
from x3_emu import dense_case, distances, emu_args, kink_free_params   # noqa: F401  (shared with the tests)

MUTANT = None   # None | "fwd"


def f16(x):
    """Round to IEEE half (RNE, subnormals kept, overflow to inf) and back, in x's dtype; the identity
    when OB.ROUND is off."""
    if not OB.ROUND:
        return x
    return x.to(torch.float32).to(torch.float16).to(x.dtype)


def split(x):
    """(h, m): the engine's two-part fp16 split."""
    h = f16(x)
    return h, f16(x - h)


def f16x2(x):
    h, m = split(x)
    return h + m


class _MMH3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        xh, xm = split(x)
        wh, wm = split(w)
        y = OB.mm(xh, wm) + OB.mm(xh, wh)
        return y if MUTANT == "fwd" else OB.mm(xm, wh) + y

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        return OB.mm(g, w.T), OB.mm(x.T, g)


class _RoundH3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return f16x2(x)

    @staticmethod
    def backward(ctx, g):
        return g


@contextlib.contextmanager
def h3(mutant=None):
    """oracle.bf16 computes the h3 arithmetic inside the block."""
    global MUTANT
    old = (OB.b16, OB._MM, OB._Round, MUTANT)
    OB.b16, OB._MM, OB._Round, MUTANT = (lambda x: x), _MMH3, _RoundH3, mutant
    try:
        yield
    finally:
        OB.b16, OB._MM, OB._Round, MUTANT = old


def loss_and_grads(params, pos, src, dst, prop, target, S=5, drop_r=None, drop_o=None, mutant=None, **kw):
    with h3(mutant):
        return OB.loss_and_grads(params, pos, src, dst, prop, target, S, drop_r, drop_o, training=False, **kw)


def noise_band(params, pos, src, dst, prop, target, S=5, drop_r=None, drop_o=None):
    """(ref, band) as x3_emu.noise_band gives them, for the h3 arithmetic: ref the fp64 h3 emulator's
    (loss, logits, grads), band the largest distance from it over its fp32 variants (k-blocks of
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
