"""What every front end's optimizer step is made of: the loss path (the last step's BCE or deep
supervision, decided once) and the Adam update (plain or clipped, at a host count or a device word).

The engine protocol
-------------------
`Trainer` drives any object with these methods (the product engine is `trainer.HipEngine`; the CPU suite
plugs in fp64 oracles). "logits" is whatever `forward` returned, handed through untouched.

Required:
  forward(params, batch, run) -> logits
  loss(logits, target) -> (out3, dlogits)            out3 = [loss, correct, n], a buffer the next call reuses
  backward(params, batch, run, dlogits) -> grads     one persistent flat buffer
  adam(params, grads, m, v, step, lr, b1, b2, eps, l2, gscale)
Optional (asked for only by the feature that needs it):
  loss_weighted(logits, target, weights, norm) -> (out3, dlogits)      step(weights=), evaluate(weights=)
  adam_clipped(params, grads, m, v, step, lr, b1, b2, eps, l2, gscale, clipnorm, clipvalue, skip_nonfinite)
      -> out4                                                          clipnorm / clipvalue / decay / skip_nonfinite
  early_event() -> event                                               the overlapped two-piece all-reduce
  set_step_loss_weights(weights, mp_steps)                             step_loss_weights
  eval_metrics(logits, target, tables, batch, weights, threshold)      evaluate
  loss_tower(logits, target, batch, tower_targets, weights, norm, norm_t, tower_loss, node_loss, want_dlogits=True)
      -> (out6, dlogits)                                               Trainer(tower_loss=): step, evaluate
      out6 = [L_node, node correct, node count, L_tower, towers correct, towers counted]; target may be None
      (node_loss 0), tower_targets None (derived), weights / norm None (unweighted). norm is the micro-batch's own
      node divisor (node_loss arrives scaled by its share of the global batch), norm_t the GLOBAL tower divisor;
      dlogits is the gradient of node_loss·L_node + tower_loss·L_tower with them, summed over ranks with weight 1
      (None with want_dlogits False: evaluate, which passes the micro-batch's own tower count as norm_t)
  dropedge_gates(batch, run, rate, symmetric=True, rescale=False, base=None) -> gates
      Trainer(dropedge=): one relation gate per edge slot of the plan ((32·n_eblocks,), 0 = dropped), drawn from
      run.seed as engine.dropedge_gates draws it, `base` (a slot tensor or None) multiplied in; with
      Trainer(dropedge_per_step=True) the call carries per_step=True and returns (mp_steps, 32·n_eblocks), a row per
      propagation step, which the gated calls below then receive as their ``gates=`` (a 2-D tensor: the loss paths
      hand it to the engine's ``step_gates=``)
  forward(params, batch, run, gates=gates) / backward(params, batch, run, dlogits, gates=gates)
      Trainer(dropedge=) and step(relation_weights=): the gated calls (engine.forward / backward's ``gates=``); the
      backward receives the tensor the forward of the same micro-batch ran with. Without DropEdge and without
      relation weights neither call is ever given the keyword.

Relation gates on the loss paths: `forward`, `backward` and `loss_backward` take ``gates=``. With gates,
`loss_backward` is the loss launch followed by `engine.backward(gates=)` — spwgnn_bce_backward takes no gates, so
the fused loss of the small-batch loop is not used. Per-step logits are not gated: `DeepLossPath` raises.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import engine as E


def gate_kw(gates) -> dict:
    """The keyword `engine.forward` / `backward` take a gate tensor under: a 2-D one, (mp_steps, slots), holds one
    gate per edge slot and step (``step_gates=``, layer-wise DropEdge); a 1-D one is shared by the steps."""
    return {"step_gates" if gates.dim() == 2 else "gates": gates}


class LossPath:
    """The plain loss path — `engine.forward`, `bce`, `backward`, fused as `bce_backward` — with its
    BceScratch. `loss_path` picks this or `DeepLossPath` once; the callers never ask which they hold.
    The engine functions are looked up on the module at each call (the CPU suite replaces them)."""

    lam = None       # the per-step loss weights of deep supervision
    out3s = None     # the last loss's per-step [loss, correct, n] rows (deep supervision)

    def __init__(self, device, mp_steps: int):
        self.device, self.mp_steps = torch.device(device), int(mp_steps)
        self.scratch = E.BceScratch(self.device)

    def for_replay(self) -> "LossPath":
        """The path a replayed geometry's body holds: one that may own static rows of that geometry."""
        return self

    def forward(self, params, batch, run, ws, out=None, gates=None):
        """The logits the loss takes; ``out``: a replayed step's static (n,) logits buffer."""
        if gates is not None:
            return E.forward(params, batch, run, ws, logits=out, **gate_kw(gates))
        return E.forward(params, batch, run, ws, logits=out)

    def loss(self, logits, target, total3=None, weights3=None, total3s=None, node_weights=None, norm=None):
        """(out3, dlogits); the epoch sums, ``node_weights`` and ``norm`` as `engine.bce` takes them."""
        return E.bce(logits, target, self.scratch, total3=total3, weights3=weights3, node_weights=node_weights,
                     norm=norm)

    def backward(self, params, batch, run, ws, dlogits, grads, gates=None):
        if gates is not None:
            return E.backward(params, batch, run, ws, dlogits, grads=grads, **gate_kw(gates))[0]
        return E.backward(params, batch, run, ws, dlogits, grads=grads)[0]

    def loss_backward(self, params, batch, run, ws, logits, target, scratch, dlogits, grads, total3=None,
                      weights3=None, total3s=None, node_weights=None, norm=None, gates=None):
        """A replayed step's loss and backward on its static buffers: one library call here
        (spwgnn_bce_backward: no loss launch of its own on the fused small-batch loop). With ``gates`` the loss
        launch (into this path's scratch) and then the gated backward."""
        if gates is not None:
            _, dz = E.bce(logits, target, scratch, dlogits=dlogits, total3=total3, weights3=weights3,
                          node_weights=node_weights, norm=norm)
            E.backward(params, batch, run, ws, dz, grads=grads, **gate_kw(gates))
            return
        E.bce_backward(params, batch, run, ws, logits, target, scratch, dlogits=dlogits, total3=total3,
                       weights3=weights3, grads=grads, node_weights=node_weights, norm=norm)

    def last(self, logits):
        """The last propagation step's logits (n,) of what `forward` returned."""
        return logits


class DeepLossPath(LossPath):
    """Deep supervision: every step's logits (`engine.forward_steps`), the loss Σ_s λ_s·BCE(z_s)
    (`bce_steps`, its own launch) and one `backward_steps` over the step loop. A replayed geometry's
    (mp_steps, n) rows and their cotangents live here, made by its first (eager) run."""

    def __init__(self, device, mp_steps: int, step_loss_weights):
        self.device, self.mp_steps = torch.device(device), int(mp_steps)
        self.lam = E.check_step_weights(step_loss_weights, mp_steps)
        self.scratch = E.BceStepsScratch(self.device, mp_steps)
        self.rows = self.drows = None

    def for_replay(self) -> "DeepLossPath":
        return DeepLossPath(self.device, self.mp_steps, self.lam)

    @staticmethod
    def _ungated(gates):
        if gates is not None:
            raise ValueError("step_loss_weights and relation gates (DropEdge, relation_weights) do not combine: "
                             "gated per-step logits are not built")

    def forward(self, params, batch, run, ws, out=None, gates=None):
        self._ungated(gates)
        if out is not None:   # a replayed step: the static rows in place of its (n,) buffer
            if self.rows is None:
                self.rows = torch.empty(self.mp_steps, batch.n_nodes, dtype=torch.float32, device=out.device)
                self.drows = torch.empty_like(self.rows)
            out = self.rows
        return E.forward_steps(params, batch, run, ws, step_logits=out)

    def loss(self, logits, target, total3=None, weights3=None, total3s=None, node_weights=None, norm=None):
        out3, self.out3s, dlogits = E.bce_steps(
            logits, target, self.lam, self.scratch, dlogits=self.drows if logits is self.rows else None,
            total3=total3, weights3=weights3, total3s=total3s, node_weights=node_weights, norm=norm)
        return out3, dlogits

    def backward(self, params, batch, run, ws, dlogits, grads, gates=None):
        self._ungated(gates)
        return E.backward_steps(params, batch, run, ws, dlogits, grads=grads)[0]

    def loss_backward(self, params, batch, run, ws, logits, target, scratch, dlogits, grads, total3=None,
                      weights3=None, total3s=None, node_weights=None, norm=None, gates=None):
        self._ungated(gates)
        _, dlogits = self.loss(logits, target, total3, weights3, total3s, node_weights, norm)
        E.backward_steps(params, batch, run, ws, dlogits, grads=grads)

    def last(self, logits):
        return logits[self.mp_steps - 1]


class TowerLossPath(LossPath):
    """The tower-level loss: L = node_loss·L_node + tower_loss·L_tower from one launch of its
    own (`engine.bce_tower`, two past 256 nodes or towers) in place of `bce`, then the plain `backward` — the
    backward is linear in dlogits, so nothing else changes. The loss needs the batch (its tower offsets):
    `loss` and `loss_backward` take it, with the tower targets and the tower divisor, as keyword arguments.
    `tower.out6` holds the last loss's six parts; with ``totals`` every loss launch also adds out6·weights6
    to `tower.total6` (fit's epoch sums; the caller sets weights6)."""

    needs_towers = True   # a replayed step uploads the plan's tower offsets and their divisor (replay.StaticBatch)

    def __init__(self, device, mp_steps: int, tower_loss: float, node_loss: float = 1.0, totals: bool = False):
        super().__init__(device, mp_steps)
        self.mu, self.alpha = E.check_tower_loss(tower_loss, node_loss)
        if not self.mu > 0:
            raise ValueError("a TowerLossPath needs tower_loss > 0")
        self.tower = E.TowerLossScratch(self.device, totals=totals)

    def loss(self, logits, target, total3=None, weights3=None, total3s=None, node_weights=None, norm=None, *,
             batch=None, tower_targets=None, norm_t=None, node_loss=None, dlogits=None, want_dlogits=True):
        """(out3, dlogits) with out3 = [L, node correct, node count]. ``batch`` is required. ``node_loss``
        overrides the path's (0 for tower-only labels: `target` may then be None)."""
        if batch is None:
            raise ValueError("the tower loss needs batch= (its tower offsets)")
        if total3 is not None or total3s is not None:
            raise ValueError("the tower loss keeps its epoch sums in tower.total6")
        t = self.tower
        return E.bce_tower(logits, target, batch, t, self.mu, self.alpha if node_loss is None else node_loss,
                           tower_targets=tower_targets, norm_t=norm_t, dlogits=dlogits, node_weights=node_weights,
                           norm=norm, total6=t.total6, weights6=t.weights6, want_dlogits=want_dlogits)

    def loss_backward(self, params, batch, run, ws, logits, target, scratch, dlogits, grads, total3=None,
                      weights3=None, total3s=None, node_weights=None, norm=None, gates=None, *, tower_targets=None,
                      norm_t=None, node_loss=None):
        """The loss launch followed by `engine.backward`. A replayed step derives its tower targets from the node
        targets; its tower offsets and its divisor (`norm_t`, a device float) come with the batch upload, since
        plans of one geometry may cut their nodes into different towers. total3 / weights3 of the plain paths
        are not taken (tower.total6 holds the sums)."""
        _, dz = self.loss(logits, target, node_weights=node_weights, norm=norm, batch=batch,
                          tower_targets=tower_targets, norm_t=norm_t, node_loss=node_loss, dlogits=dlogits)
        if gates is not None:
            E.backward(params, batch, run, ws, dz, grads=grads, **gate_kw(gates))
        else:
            E.backward(params, batch, run, ws, dz, grads=grads)


def loss_path(device, mp_steps: int, step_loss_weights=None, *, tower_loss: float = 0.0, node_loss: float = 1.0,
              totals: bool = False) -> LossPath:
    """The loss path of a front end: chosen here, once, not per step."""
    mu, alpha = E.check_tower_loss(tower_loss, node_loss)
    if mu > 0:
        if step_loss_weights is not None:
            raise ValueError("tower_loss and step_loss_weights do not combine (the tower term on per-step rows "
                             "is not built)")
        return TowerLossPath(device, mp_steps, mu, alpha, totals=totals)
    if step_loss_weights is None:
        return LossPath(device, mp_steps)
    return DeepLossPath(device, mp_steps, step_loss_weights)


class AdamUpdate:
    """The optimizer of a front end: Adam's hyperparameters, the Keras 2.x options (0 / False = off) and,
    once one of those is set, the ClipScratch of the clipped update (one launch more). The attributes may
    be changed between steps."""

    def __init__(self, device, lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-7, l2=0.0, clipnorm=0.0, clipvalue=0.0,
                 decay=0.0, skip_nonfinite=False, totals: bool = False):
        E.check_clip_options(clipnorm, clipvalue, decay)
        self.device, self.totals = device, totals
        self.lr, self.beta1, self.beta2, self.eps, self.l2 = lr, beta1, beta2, eps, l2
        self.clipnorm, self.clipvalue, self.decay = float(clipnorm), float(clipvalue), float(decay)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.scratch: Optional[E.ClipScratch] = None

    def clip_on(self) -> bool:
        return bool(self.clipnorm or self.clipvalue or self.decay or self.skip_nonfinite)

    def clip_scratch(self) -> E.ClipScratch:
        if self.scratch is None:
            self.scratch = E.ClipScratch(self.device, totals=self.totals)
        return self.scratch

    def update(self, params, grads, m, v, iterations: int):
        """The update of step `iterations` (counted from 1), at the decayed lr. Returns the clipped
        update's out4 = [norm, scale, skipped, clipped] (device), None for the plain one."""
        if not self.clip_on():
            E.adam(params, grads, m, v, iterations, self.lr, self.beta1, self.beta2, self.eps, self.l2)
            return None
        lr = E.adam_lr_decayed(self.lr, self.decay, iterations - 1) if self.decay else self.lr
        return E.adam_clipped(params, grads, m, v, iterations, self.clip_scratch(), lr, self.beta1, self.beta2,
                              self.eps, self.l2, 1.0, self.clipnorm, self.clipvalue, self.skip_nonfinite)

    def update_dev(self, params, grads, m, v, ctr, accumulate: bool = False):
        """The update at the device step word of `ctr` (replay.DeviceCounters), lr_t — the decay in it —
        from its table: a replayed step's. `accumulate`: the clipped update adds to the scratch's totals."""
        if not self.clip_on():
            E.adam_dev(params, grads, m, v, ctr.step, ctr.lr_table, self.beta1, self.beta2, self.eps, self.l2)
        else:
            E.adam_clipped_dev(params, grads, m, v, ctr.step, ctr.lr_table, self.clip_scratch(), self.beta1,
                               self.beta2, self.eps, self.l2, 1.0, self.clipnorm, self.clipvalue,
                               self.skip_nonfinite, accumulate=accumulate)


def delegated(owner: str, name: str) -> property:
    """A read/write attribute of a front end that lives on its `owner` attribute (the AdamUpdate)."""
    return property(lambda self: getattr(getattr(self, owner), name),
                    lambda self, value: setattr(getattr(self, owner), name, value))
