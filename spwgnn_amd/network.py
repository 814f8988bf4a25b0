"""GraphNetwork: the reference's propagation network as a torch module backed by libspwgnn_hip.

Reference graph: src/Networks.py:16-104 (PropagationNetwork.getModel) over the MLP blocks of
src/Blocks.py:12-91. Inputs and output keep the reference layout: objects (B,N,3), sender/receiver
relations (B,N,E), propagation (B,N,100) → per-object stability probability (B,N,1).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from . import engine as E
from . import params as P
from .batch import TowerBatch


class _PropagationFn(torch.autograd.Function):
    """Forward/backward of the whole graph through the C-ABI; gradients w.r.t. the flat parameter
    buffer, the propagation input and the objects (the (n_nodes, 3) rows in the plan's node order;
    the relation set is a constant of the graph and is not differentiated) — and, with ``gates`` (one relation
    gate per edge slot, `engine.forward`'s), the gates: d loss / d gate comes from `engine.backward_relations`
    after the gated backward. With ``want_state`` a second
    output, the final state (n_nodes, 100), whose gradient enters the same backward pass as ``dstate``.
    With ``want_steps`` the first output is every step's logits (mp_steps, n_nodes) (`engine.forward_steps`)
    and its gradient goes back through `engine.backward_steps`, still one pass over the step loop.
    A 2-D ``gates`` ((mp_steps, slots), `engine.forward`'s ``step_gates``) holds one gate per edge slot and step;
    its gradient is `engine.backward_relations`' ``drel_steps``."""

    @staticmethod
    def forward(ctx, flat, prop_dummy, obj_dummy, batch: TowerBatch, run: E.RunConfig, ws: E.Workspace,
                want_state: bool = False, want_steps: bool = False, gates: Optional[torch.Tensor] = None):
        ctx.batch, ctx.run, ctx.ws = batch, run, ws
        ctx.gated = gates is not None
        ctx.save_for_backward(*((flat, gates) if ctx.gated else (flat,)))
        ctx.want_prop = prop_dummy.requires_grad
        ctx.want_obj = obj_dummy.requires_grad
        ctx.want_state = want_state
        ctx.want_steps = want_steps
        ctx.set_materialize_grads(False)   # an unused output's gradient arrives as None, not as zeros
        ctx.gate_kw = "step_gates" if ctx.gated and gates.dim() == 2 else "gates"
        if ctx.gated:   # forward_batch refuses gates with want_steps
            return E.forward(flat, batch, run, ws, return_state=want_state, **{ctx.gate_kw: gates})
        return (E.forward_steps if want_steps else E.forward)(flat, batch, run, ws, return_state=want_state)

    @staticmethod
    def backward(ctx, dlogits, dstate=None):
        flat, gates = ctx.saved_tensors if ctx.gated else (*ctx.saved_tensors, None)
        if dstate is not None:
            dstate = dstate.to(torch.float32).contiguous()
        if dlogits is None:   # a loss on the state alone: the library still takes a dlogits array
            shape = (ctx.run.mp_steps, ctx.batch.n_nodes) if ctx.want_steps else (ctx.batch.n_nodes,)
            dlogits = torch.zeros(shape, dtype=torch.float32, device=flat.device)
        if ctx.gated:
            grads, dprop = E.backward(flat, ctx.batch, ctx.run, ctx.ws, dlogits, want_dprop=ctx.want_prop, dstate=dstate,
                                      **{ctx.gate_kw: gates})
        else:
            grads, dprop = (E.backward_steps if ctx.want_steps else E.backward)(
                flat, ctx.batch, ctx.run, ctx.ws, dlogits, want_dprop=ctx.want_prop, dstate=dstate)
        dobj = E.backward_inputs(flat, ctx.batch, ctx.run, ctx.ws) if ctx.want_obj else None
        # d loss / d gate at the run's gates, 0 in padding slots (one more launch that only reads the workspace)
        dgates = None
        if ctx.gated and ctx.needs_input_grad[8]:
            dgates = E.backward_relations(flat, ctx.batch, ctx.run, ctx.ws, per_step=ctx.gate_kw == "step_gates")
            if ctx.gate_kw == "step_gates":   # (drel, drel_steps): the per-step gates' gradient is drel_steps
                dgates = dgates[1]
        return grads, dprop, dobj, None, None, None, None, None, dgates


class _TowerLossFn(torch.autograd.Function):
    """`tower_bce`: the loss launch of `engine.bce_tower` in the forward, which also writes d L / d logit;
    the backward scales that stored dlogits by the incoming gradient."""

    @staticmethod
    def forward(ctx, logits, targets, batch, scratch, tower_loss, node_loss, tower_targets, node_weights, norm, norm_t):
        out3, dz = E.bce_tower(logits.detach().reshape(-1).to(torch.float32).contiguous(), targets, batch, scratch,
                               tower_loss, node_loss, tower_targets=tower_targets, norm_t=norm_t,
                               node_weights=node_weights, norm=norm)
        ctx.save_for_backward(dz)
        ctx.shape, ctx.dtype = logits.shape, logits.dtype
        return out3[0].clone()

    @staticmethod
    def backward(ctx, grad):
        (dz,) = ctx.saved_tensors
        return (grad * dz).reshape(ctx.shape).to(ctx.dtype), *([None] * 9)


def tower_bce(logits: torch.Tensor, targets: Optional[torch.Tensor], batch: TowerBatch, tower_loss: float = 1.0,
              node_loss: float = 1.0, tower_targets: Optional[torch.Tensor] = None,
              node_weights: Optional[torch.Tensor] = None, norm=None, norm_t=None,
              scratch: Optional["E.TowerLossScratch"] = None) -> torch.Tensor:
    """The scalar L = node_loss·L_node + tower_loss·L_tower of `engine.bce_tower` as a
    differentiable function of ``logits`` — what `GraphNetwork.forward_batch` returned for ``batch``, in the
    plan's node order, as ``targets`` (`TowerBatch.to_plan_order`) and ``tower_targets``
    (`TowerBatch.towers_to_plan_order`) are. ``scratch.out6`` (pass your own `engine.TowerLossScratch` to
    read it) holds the six parts of the last call."""
    if scratch is None:
        scratch = E.TowerLossScratch(logits.device)
    return _TowerLossFn.apply(logits, targets, batch, scratch, tower_loss, node_loss, tower_targets, node_weights,
                              norm, norm_t)


class GraphNetwork(nn.Module):
    """Propagation network (rm, om, rmp, omp) with shared weights across sizes and steps.

    ``mp_steps`` defaults to the reference's 5 (Networks.py:83); ``dropout`` to its 0.1 on the
    two encodings (Networks.py:77-78), active only in training mode. ``math`` ("x6" by default, the
    fp32-class parity path; "h3", "x3", "bf16", "f32": `engine.MATH_MODES`) is the arithmetic of the matrix
    products in training, inference and `forward_pooled`.

    ``dropedge`` (a rate in [0, 1)): in train mode under autograd every forward drops a random
    subset of the relations — `engine.dropedge_gates` with the step's dropout key, multiplied into the call's
    ``relation_weights`` in torch, so the chain rule to a weights leaf stays autograd's. ``dropedge_symmetric``:
    both directions of a contact share the draw; ``dropedge_rescale``: kept relations weigh 1/(1 − rate).
    `eval()` and no-grad calls draw nothing. 0 = off. ``dropedge_per_step`` (layer-wise DropEdge, §3zzc; active
    only with ``dropedge`` > 0): a fresh subset at every propagation step instead of one for all of them.
    """

    def __init__(self, mp_steps: int = E.REF_MP_STEPS, dropout: float = E.REF_DROPOUT, seed: int = 0,
                 device="cuda", params: Optional[Dict[str, np.ndarray]] = None, math: str = "x6",
                 dropedge: float = 0.0, dropedge_symmetric: bool = True, dropedge_rescale: bool = False,
                 dropedge_per_step: bool = False):
        super().__init__()
        if math not in E.MATH_MODES:
            raise ValueError(f"math must be one of {sorted(E.MATH_MODES)}")
        self.dropedge = E.check_dropedge(dropedge)
        self.dropedge_symmetric, self.dropedge_rescale = bool(dropedge_symmetric), bool(dropedge_rescale)
        self.dropedge_per_step = bool(dropedge_per_step)
        if self.dropedge > 0 and not E.gates_supported(math):
            raise ValueError(f'dropedge is not supported in math "{math}" (x6, x3 and h3 take relation gates)')
        self.math = math          # the matrix-product arithmetic of every run this network builds (engine.RunConfig.math)
        self.mp_steps = mp_steps
        self.dropout = dropout
        init = params if params is not None else P.glorot_uniform(seed)
        self.flat = nn.Parameter(P.to_flat(init, device=device))
        self._step_seed = seed * 1000003 + 17

    @property
    def device(self):
        return self.flat.device

    def keras_weights(self) -> Dict[str, np.ndarray]:
        return P.from_flat(self.flat)

    def load_keras_weights(self, params: Dict[str, np.ndarray]):
        with torch.no_grad():
            self.flat.copy_(P.to_flat(params, device=self.flat.device))

    def run_config(self, training: bool = False, **kw) -> E.RunConfig:
        """A `RunConfig` of this network's step count and math (the front ends build theirs with it)."""
        return E.RunConfig(self.mp_steps, training=training, math=self.math, **kw)

    def _run(self, input_grad: bool = False) -> E.RunConfig:   # input_grad: an input (objects, prop) wants a gradient
        need_grad = torch.is_grad_enabled() and (self.flat.requires_grad or input_grad)
        drop = self.training and self.dropout > 0 and need_grad
        seed = 0
        if drop or (self.training and self.dropedge > 0 and need_grad):   # a step that draws: the next key
            self._step_seed += 1
            seed = self._step_seed
        return E.RunConfig(self.mp_steps, training=need_grad, dropout=self.dropout if drop else 0.0, seed=seed,
                           math=self.math)

    def forward_batch(self, batch: TowerBatch, prop: Optional[torch.Tensor] = None,
                      objects: Optional[torch.Tensor] = None, return_state: bool = False, return_steps: bool = False,
                      relation_weights: Optional[torch.Tensor] = None,
                      relation_step_weights: Optional[torch.Tensor] = None):
        """Logits (n_nodes,) for a compact batch (the reference returns sigmoid of these).

        ``relation_step_weights`` (exclusive with ``relation_weights``): one gate per active
        relation AND propagation step, as `TowerBatch.edge_step_gates` takes them — (S, B, N, N) indexed [step,
        tower, sender, receiver], or (S, E) in the input's edge order. Step s scales relation k's message by its
        step-s gate; everything else as ``relation_weights``, the gradient of a leaf included.

        ``relation_weights``: soft relations — one gate per active relation, as
        `TowerBatch.edge_gates` takes them: a dense (B, N, N) tensor indexed [tower, sender, receiver] for towers
        of one size, or a 1-D tensor in the input's edge order. Relation k's message is scaled by its gate in the
        receiver sum of Networks.py:88 alone (the gathers of lines 33 and 85 stay ungated); any finite value,
        0 and negative ones included. Autograd reaches the weights, ``prop``, ``objects`` AND the gates (the gate
        gradient is `engine.backward_relations` after the gated backward). Runs the wide kernels at every batch
        size, in x6, x3 and h3; combines with ``return_state``, not with ``return_steps``.

        ``return_steps``: instead of the last step's logits, every step's, (mp_steps, n_nodes) — row s is
        the readout after s + 1 propagation steps (the network's column 0 at that step, Networks.py:89-94),
        the last row the logits this call returns otherwise, bit for bit. The rows are in the INPUT's node
        order (a packed plan's rows are put back with `TowerBatch.to_input_order`; every other plan keeps
        the input's order anyway). Differentiable in the weights, ``prop`` and ``objects`` like the logits:
        a loss Σ_s λ_s·L(z_s) — deep supervision — takes one backward pass. Combines with ``return_state``.

        ``return_state``: return ``(logits, state)`` — state (n_nodes, 100) is the propagation state after
        the last step, P_S = tanh(x[:, 1:] + P_{S-1}) (Networks.py:91), in the plan's node order like the
        logits, differentiable like them. Feed it to the next call as ``prop`` to carry the state on
        (`rollout`); a state that carries a gradient makes that next call differentiate with respect to it.

        ``objects``: the torch tensor the batch's node rows were built from (n_nodes·3 elements, the
        input's node order, any device / float dtype). The forward reads the batch's own copy; when
        the tensor requires grad, backward also returns d/d objects into it (one extra launch,
        `engine.backward_inputs`), in its own shape, device and dtype. The relation set — a
        thresholded one included — is held constant: it is not differentiated."""
        want_obj = objects is not None and torch.is_grad_enabled() and objects.requires_grad
        # a carried state that has a gradient path needs this call's backward even under frozen weights
        want_prop = return_state and prop is not None and torch.is_grad_enabled() and prop.requires_grad
        gates = None
        if relation_step_weights is not None:
            if relation_weights is not None:
                raise ValueError("relation_weights and relation_step_weights are mutually exclusive")
            if return_steps:
                raise ValueError("relation_step_weights do not combine with return_steps (per-step logits are not gated)")
            if not E.gates_supported(self.math):
                raise ValueError(f'relation_step_weights are not supported in math "{self.math}" (x6, x3 and h3 take '
                                 "them)")
            if int(relation_step_weights.shape[0]) != int(self.mp_steps):
                raise ValueError(f"relation_step_weights needs one leading row per propagation step ({self.mp_steps}), "
                                 f"got {tuple(relation_step_weights.shape)}")
            gates = batch.edge_step_gates(relation_step_weights)   # torch indexing: autograd reaches the leaf
        if relation_weights is not None:
            if return_steps:
                raise ValueError("relation_weights do not combine with return_steps (per-step logits are not gated)")
            if not E.gates_supported(self.math):
                raise ValueError(f'relation_weights are not supported in math "{self.math}" (x6, x3 and h3 take them)')
            gates = batch.edge_gates(relation_weights)   # torch indexing: autograd reaches relation_weights
        want_rel = gates is not None and torch.is_grad_enabled() and gates.requires_grad
        run = self._run(want_obj or want_prop or want_rel)
        if self.dropedge > 0 and self.training and run.training:
            if return_steps:
                raise ValueError("dropedge does not combine with return_steps (per-step logits are not gated)")
            mask = E.dropedge_gates(batch, run, self.dropedge, symmetric=self.dropedge_symmetric,
                                    rescale=self.dropedge_rescale, per_step=self.dropedge_per_step)
            # in torch: autograd carries the mask to the weights leaf (a shared weight row under a per-step mask
            # broadcasts over the steps; per-step weights under a shared mask likewise)
            gates = mask if gates is None else (gates * mask).contiguous()
        ws = E.Workspace(self.device)
        if prop is not None:
            batch = batch.with_prop(prop)
            # the backward returns dprop as (n_nodes, 100): autograd maps it back through the reshape
            # to whatever layout the caller passed ((B, N, 100) in the reference)
            dummy = prop.reshape(batch.n_nodes, 100)
        else:
            dummy = torch.zeros(0, device=self.device)
        if want_obj:
            # d/d objects arrives as (n_nodes, 3) in plan order: autograd maps it back through the
            # gather (TowerBatch.to_input_order for packed plans), the device / dtype move and the reshape
            odummy = batch.to_plan_order(objects.reshape(batch.n_nodes, 3).to(self.device, torch.float32))
        else:
            odummy = dummy.new_zeros(0)
        if not run.training:
            with torch.no_grad():
                if gates is not None:
                    out = E.forward(self.flat.detach(), batch, run, ws, return_state=return_state,
                                    **{"step_gates" if gates.dim() == 2 else "gates": gates})
                else:
                    out = (E.forward_steps if return_steps else E.forward)(self.flat.detach(), batch, run, ws,
                                                                           return_state=return_state)
        else:
            out = _PropagationFn.apply(self.flat, dummy, odummy, batch, run, ws, return_state, return_steps, gates)
        if return_steps and batch.node_perm is not None:   # rows of a packed plan back in the input's node order
            steps = batch.to_input_order((out[0] if return_state else out).t()).t()
            return (steps, out[1]) if return_state else steps
        return out

    def rollout(self, batches: Sequence[TowerBatch], prop: Optional[torch.Tensor] = None,
                objects: Optional[Sequence[Optional[torch.Tensor]]] = None) -> Tuple[List[torch.Tensor], torch.Tensor]:
        """The network over the frames of a trajectory, the belief state carried from frame to frame as
        BRDPN's propagation input is (Blocks.py is "directly taken from" it): ``batches`` holds one
        `TowerBatch` per frame, the same nodes in the same plan order in each (positions and relation sets
        may differ); frame k's final state is frame k + 1's ``prop``, frame 0 takes ``prop`` (None = zero).
        Returns (the per-frame logits, the final state). Autograd flows through all frames — weights, the
        initial ``prop`` and, with ``objects`` (one tensor or None per frame, as in `forward_batch`), the
        positions; each frame keeps its own workspace until its backward has run."""
        batches = list(batches)
        if not batches:
            raise ValueError("rollout needs at least one frame")
        if any(b.n_nodes != batches[0].n_nodes for b in batches):
            raise ValueError("rollout frames must hold the same nodes (n_nodes differs)")
        if objects is not None and len(objects) != len(batches):
            raise ValueError("objects must give one entry (or None) per frame")
        logits, state = [], prop
        for k, batch in enumerate(batches):
            z, state = self.forward_batch(batch, state, objects[k] if objects is not None else None, return_state=True)
            logits.append(z)
        return logits, state

    def _dense_batch(self, objects, sender_relations, receiver_relations, propagation, plan: str) -> TowerBatch:
        if plan == "host":
            return TowerBatch.from_dense(objects, sender_relations, receiver_relations, propagation, device=self.device)
        if plan != "device":
            raise ValueError('plan must be "host" or "device"')
        return TowerBatch.from_dense_device(objects, sender_relations, receiver_relations, propagation)

    def forward_logits(self, objects, sender_relations, receiver_relations, propagation=None,
                       plan: str = "host", return_state: bool = False, return_steps: bool = False,
                       relation_weights: Optional[torch.Tensor] = None,
                       relation_step_weights: Optional[torch.Tensor] = None):
        """``relation_weights``: a (B, N, N) [tower, sender, receiver] tensor of relation gates (soft relations:
        see `forward_batch`); entries without a relation are not read. Autograd reaches it.
        ``relation_step_weights``: (S, B, N, N), one such tensor per propagation step (see `forward_batch`).
        ``return_steps``: (S, B, N) — every step's logits (see `forward_batch`) in place of the last step's.
        (B, N) logits; with ``return_state`` ``(logits, state)``, state (B, N, 100) (see `forward_batch`). A torch ``objects`` that requires grad receives d/d objects (B, N, 3) on
        backward (see `forward_batch`; the relations are constants).
        ``plan``: "host" converts the relation matrices on the host (`TowerBatch.from_dense`: a copy to
        the host, a C++ scan, an upload); "device" needs all inputs on the device and converts them there
        (`TowerBatch.from_dense_device`: one kernel, no host round trip, no synchronisation). The two
        plans order a tile's edges alike but pad differently, so the logits agree within the engine's
        position-independence bound (DESIGN.md §3 "Determinism"), not bit for bit in every math."""
        batch = self._dense_batch(objects, sender_relations, receiver_relations, None, plan)
        prop = None
        if propagation is not None:
            prop = torch.as_tensor(propagation, dtype=torch.float32, device=self.device).reshape(batch.n_nodes, 100)
        z = self.forward_batch(batch, prop, objects if isinstance(objects, torch.Tensor) else None,
                               return_state=return_state, return_steps=return_steps, relation_weights=relation_weights,
                               relation_step_weights=relation_step_weights)
        shape = (self.mp_steps, *batch.node_shape) if return_steps else batch.node_shape
        if return_state:
            z, state = z
            return z.reshape(shape), state.reshape(*batch.node_shape, E.STATE_WIDTH)
        return z.reshape(shape)

    def forward(self, objects, sender_relations, receiver_relations, propagation=None, plan: str = "host",
                return_state: bool = False, return_steps: bool = False,
                relation_weights: Optional[torch.Tensor] = None,
                relation_step_weights: Optional[torch.Tensor] = None):
        """(B, N, 1) probabilities: sigmoid(x[:, :, :1]) of the last step (Networks.py:93-96);
        differentiable in a torch ``objects`` like `forward_logits` (``plan``, ``relation_weights`` and
        ``relation_step_weights`` as there). With
        ``return_state`` ``(probabilities, state)``, state (B, N, 100). With ``return_steps`` the
        probabilities of every step, (S, B, N, 1): how the predicted stabilities settle over the steps."""
        z = self.forward_logits(objects, sender_relations, receiver_relations, propagation, plan, return_state,
                                return_steps, relation_weights, relation_step_weights)
        if return_state:
            return torch.sigmoid(z[0])[..., None], z[1]
        return torch.sigmoid(z)[..., None]

    def relation_gradients(self, objects, sender_relations, receiver_relations, propagation=None, dlogits=None,
                           loss=None) -> torch.Tensor:
        """Which relation a prediction rests on: a tensor shaped like ``receiver_relations`` (B, N, E) that
        holds r_k at [b, dst_k, k] for every active relation column k of tower b and zero elsewhere
        (`engine.backward_relations`). r_k is the gradient of a scalar gate on relation k in
        the receiver sum of Networks.py:88 ALONE, at the all-ones gate: d L / d receiver_relations[b, dst_k, k]
        through line 88, not through the gathers of lines 33 and 85 that read the same tensors. (The gradient at
        other gates is the ``.grad`` of a ``relation_weights`` leaf of `forward_logits`.)
        L is Σ dlogits·z for a ``dlogits`` (B, N) tensor, or ``loss(z)`` for a callable taking the (B, N)
        logits and returning a scalar (its d/dz by torch autograd), or — neither given — Σ sigmoid(z), the
        stability readout. One training forward with dropout 0 (the inference values, activations kept),
        one backward, one more launch. Inputs as `forward_logits` takes them (host plan)."""
        if dlogits is not None and loss is not None:
            raise ValueError("give dlogits or loss, not both")
        to_np = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        Rs, Rr = to_np(sender_relations), to_np(receiver_relations)
        batch = self._dense_batch(objects, sender_relations, receiver_relations, None, "host")
        if propagation is not None:
            batch = batch.with_prop(torch.as_tensor(propagation, dtype=torch.float32, device=self.device)
                                    .reshape(batch.n_nodes, 100))
        B, N = batch.node_shape
        flat = self.flat.detach()
        run = self.run_config(True, dropout=0.0)
        ws = E.Workspace(self.device)
        with torch.no_grad():
            z = E.forward(flat, batch, run, ws)
        if dlogits is not None:
            dz = torch.as_tensor(dlogits, dtype=torch.float32, device=self.device).reshape(-1)
        else:
            with torch.enable_grad():
                zz = z.detach().reshape(B, N).requires_grad_(True)
                L = torch.sigmoid(zz).sum() if loss is None else loss(zz)
                (dz,) = torch.autograd.grad(L, zz)
            dz = dz.reshape(-1)
        with torch.no_grad():
            E.backward(flat, batch, run, ws, dz.contiguous())
            drel = E.backward_relations(flat, batch, run, ws)
        dense = batch.edges_to_input(drel, dense=True)   # (B, N, N) [sender, receiver]
        out = np.zeros(Rr.shape, np.float32)
        for b in range(B):
            cols = np.nonzero((Rr[b] != 0).any(0) & (Rs[b] != 0).any(0))[0]
            s, r = Rs[b][:, cols].argmax(0), Rr[b][:, cols].argmax(0)
            out[b, r, cols] = dense[b, s, r]
        return torch.from_numpy(out).to(self.device)

    def forward_pooled(self, objects, sender_relations, receiver_relations, propagation=None,
                       mode: str = "mean_prob", plan: str = "host") -> torch.Tensor:
        """(B,) per-tower pooled output — the optional GlobalBlock-style readout (not in the
        reference): "mean_prob" / "sum_prob" (Σŷ of JengaBuilder.py:252-256) /
        "mean_logit" / "sum_logit", reduced on device. Inference only (no autograd, a torch
        ``objects`` included; `demolish.stability_gradients` gives d(readout)/d objects).
        ``plan`` as in `forward_logits`."""
        batch = self._dense_batch(objects, sender_relations, receiver_relations, propagation, plan)
        with torch.no_grad():
            z = E.forward(self.flat.detach(), batch, self.run_config(), E.Workspace(self.device))
            return E.tower_readout(z, batch, mode)

    def forward_positions(self, raw: torch.Tensor, threshold: Optional[float] = 170.0, divisor: float = 170.0,
                          tower_nodes=None, nw_max: Optional[int] = None, edge_cap=None, tower_ids=None,
                          propagation: Optional[torch.Tensor] = None, check: bool = False, return_state: bool = False,
                          soft_tau: Optional[float] = None):
        """Logits from raw-pixel positions on the device, (B, N) for ``raw`` (B, N, 3) or (n_nodes,) for
        ragged towers ((n_nodes, 3) with ``tower_nodes``): the relation set (raw-pixel distance <
        ``threshold``, main.py:71-81) and the objects rows raw / ``divisor`` (main.py:91) are built on
        the device by `TowerBatch.from_positions`, whose other arguments these are.
        A ``raw`` that requires grad receives d/d raw = (d/d objects) / divisor on backward. The relation
        set is a CONSTANT of the graph: it is not differentiated, although it was computed from ``raw`` —
        the gradient is that of the network on the relation set the positions select, and it does not
        see a relation appear or vanish as a box crosses the threshold.
        ``soft_tau`` > 0 (raw pixels; equal towers, ``raw`` (B, N, 3)) makes the relation set of main.py:71-81
        differentiable: the plan is fully connected and relation s → r carries the gate
        sigmoid((threshold − ‖raw_s.xy − raw_r.xy‖) / soft_tau), computed in torch from ``raw`` — close to 1 well
        inside the threshold, 1/2 on it, close to 0 far outside (as τ → 0 the hard relation set, up to the
        gathers of Networks.py:33 and :85, which stay ungated). d/d raw then flows through the gates as well as
        through the object rows."""
        soft = soft_tau is not None and float(soft_tau) > 0.0
        gates = None
        if soft:
            if threshold is None or raw.dim() != 3 or tower_nodes is not None:
                raise ValueError("soft_tau needs a threshold and equal towers: raw (B, N, 3)")
            xy = raw[..., :2].to(self.device, torch.float32)
            d2 = ((xy[:, :, None, :] - xy[:, None, :, :]) ** 2).sum(-1)    # (B, N, N) [sender, receiver]
            pos = d2 > 0   # the diagonal (and coincident boxes): sqrt has no derivative at 0; the diagonal is never read
            dist = torch.where(pos, torch.sqrt(torch.where(pos, d2, torch.ones_like(d2))), torch.zeros_like(d2))
            gates = torch.sigmoid((float(threshold) - dist) / float(soft_tau))
        batch = TowerBatch.from_positions(raw, None if soft else threshold, divisor, tower_nodes, nw_max, edge_cap,
                                          tower_ids, None, check)
        prop = None
        if propagation is not None:
            prop = torch.as_tensor(propagation, dtype=torch.float32, device=self.device).reshape(batch.n_nodes, 100)
        objects = None
        if torch.is_grad_enabled() and raw.requires_grad:
            # the forward reads the batch's own rows (the kernel's raw / divisor); this node only carries
            # d/d objects back to raw through the division
            objects = raw.reshape(batch.n_nodes, raw.shape[-1])[:, :3] / divisor
        z = self.forward_batch(batch, prop, objects, return_state=return_state, relation_weights=gates)
        if return_state:
            z, state = z
            if batch.node_shape is None:
                return z, state
            return z.reshape(batch.node_shape), state.reshape(*batch.node_shape, E.STATE_WIDTH)
        return z.reshape(batch.node_shape) if batch.node_shape is not None else z
