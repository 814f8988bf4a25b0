"""Keras-shaped front end: PropagationNetwork.getModel(...) → model.fit / model.predict.

Mirrors the reference call sites one-to-one so a driver written against the reference drops in:
  * PropagationNetwork().getModel(n_objects, object_dim=3, relation_dim=1)  — Networks.py:12-104
    (one model per n_objects, cached at Networks.py:17-18,103; all models share rm/om/rmp/omp weights, :40-56)
  * model.fit(x_dict, {'target': y}, batch_size=32, epochs=10, validation_split=0.2, shuffle=True,
    verbose=1)                                                            — main.py:92-98
  * model.predict(x_dict) → (B, N, 1) probabilities                       — JengaBuilder.py:328-329
Compile semantics (Networks.py:101-102): Adam(lr=5e-4, decay=0) per model, binary_crossentropy,
binary_accuracy. Every step runs through libspwgnn_hip (forward, BCE, backward, Adam).
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib
from . import engine as E
from . import params as P
from .batch import HostPlan, TowerBatch
from .network import GraphNetwork
from .replay import DeviceCounters, ReplayCache, step_body
from .step import AdamUpdate, DeepLossPath, LossPath, TowerLossPath, delegated


def node_weights(target, sample_weight=None, class_weight=None) -> np.ndarray:
    """Per-node loss weights (B, N) float32 of Keras's `sample_weight` / `class_weight` for a (B, N[, 1])
    0/1 target (pure numpy; model.fit's arguments, main.py:92-98).

    `sample_weight`: (B,) — one weight per tower, repeated over its N nodes (with Keras 2.x's
    weighted_masked_objective that is the same loss) — or (B, N), Keras's sample_weight_mode='temporal'.
    `class_weight`: {0: a, 1: b}, applied per node by its target: an extension, Keras refuses
    class_weight for 3-D targets. Both given: their product. A weight of 0 masks the node."""
    t = np.asarray(target)
    if t.ndim == 3 and t.shape[-1] == 1:
        t = t[..., 0]
    if t.ndim != 2:
        raise ValueError("target must be (B, N) or (B, N, 1)")
    w = np.ones(t.shape, np.float64)
    if sample_weight is not None:
        sw = np.asarray(sample_weight, np.float64)
        if sw.shape == t.shape[:1]:
            sw = sw[:, None]
        elif sw.shape != t.shape:
            raise ValueError(f"sample_weight must be (B,) or (B, N) = {t.shape} (got {sw.shape})")
        w = w * sw
    if class_weight is not None:
        if set(class_weight) != {0, 1}:
            raise ValueError("class_weight must be {0: a, 1: b}")
        w = w * np.where(t == 1, float(class_weight[1]), float(class_weight[0]))
    return w.astype(np.float32)


class CompactDataset:
    """Host-side compact copy of a dense dataset: per-tower node rows and active edges."""

    def __init__(self, objects, Rs, Rr, propagation=None):
        objects = np.asarray(objects, np.float32)
        self.B, self.N = objects.shape[:2]
        full = TowerBatch.from_dense(objects[:1], np.asarray(Rs)[:1], np.asarray(Rr)[:1], device="cpu")  # validates layout
        del full
        # one C++ conversion for the whole set
        import ctypes as C
        from . import _lib
        Rs = np.ascontiguousarray(Rs, np.float32)
        Rr = np.ascontiguousarray(Rr, np.float32)
        E_ = self.N * (self.N - 1)
        cap = self.B * E_
        src = np.zeros(max(cap, 1), np.int32)
        dst = np.zeros(max(cap, 1), np.int32)
        tec = np.zeros(self.B, np.int32)
        ne = C.c_int64(0)
        _lib.check(_lib.lib().spwgnn_dense_to_edges(Rs.ctypes.data, Rr.ctypes.data, self.B, self.N, src.ctypes.data,
                                                    dst.ctypes.data, None, cap, C.byref(ne), tec.ctypes.data),
                   "dense_to_edges")
        n = int(ne.value)
        self.objects = objects
        self.src = src[:n] - np.repeat(np.arange(self.B, dtype=np.int32) * self.N, tec)   # tower-local
        self.dst = dst[:n] - np.repeat(np.arange(self.B, dtype=np.int32) * self.N, tec)
        self.edge_off = np.concatenate([[0], np.cumsum(tec)]).astype(np.int64)
        self.tower_edges = tec
        self.prop = None if propagation is None or not np.any(np.asarray(propagation)) else \
            np.asarray(propagation, np.float32)

    def subset(self, idx: np.ndarray, device) -> TowerBatch:
        return TowerBatch.from_plan(self.subset_plan(idx), device)

    def subset_plan(self, idx: np.ndarray, edge_cap: bool = False) -> HostPlan:
        """Host plan of the towers `idx`; `edge_cap`: blocks sized for all N(N−1) relation slots
        per tower, so every batch of len(idx) towers has one geometry (replayed steps)."""
        idx = np.asarray(idx)
        n = len(idx)
        # the towers' edge ranges gathered in one vectorised pass (tower k of the batch: node ids + k·N)
        cnt = self.tower_edges[idx].astype(np.int64)
        tot = int(cnt.sum())
        first = np.cumsum(cnt) - cnt                         # batch position of each tower's first edge
        gidx = np.arange(tot, dtype=np.int64) + np.repeat(self.edge_off[idx] - first, cnt)
        shift = np.repeat(np.arange(n, dtype=np.int32) * self.N, cnt)
        src = (self.src[gidx] + shift).astype(np.int32)
        dst = (self.dst[gidx] + shift).astype(np.int32)
        prop = None if self.prop is None else self.prop[idx].reshape(n * self.N, 100)
        return HostPlan.build(self.objects[idx].reshape(n * self.N, 3), np.full(n, self.N, np.int32), src, dst,
                              self.tower_edges[idx], prop, node_shape=(n, self.N),
                              edge_cap=self.N * (self.N - 1) if edge_cap else None)


class KerasModel:
    """One compiled per-N model of the reference (Networks.py:99-104); weights shared via ``net``."""

    def __init__(self, net: GraphNetwork, n_objects: int, object_dim: int = 3, lr: float = 5e-4,
                 l2: float = 0.0, clipnorm: float = 0.0, clipvalue: float = 0.0, decay: float = 0.0,
                 skip_nonfinite: bool = False, step_loss_weights=None, tower_loss: float = 0.0, node_loss: float = 1.0,
                 dropedge: float = 0.0, dropedge_symmetric: bool = True, dropedge_rescale: bool = False,
                 dropedge_per_step: bool = False):
        if object_dim != 3:
            # Networks.py:70-73 + main.py:28-31/59-63: the object_dim=2 path of the reference is
            # broken (om gets 1 feature, boxes[...,2] is out of range); only the Jenga layout runs.
            raise ValueError("only object_dim=3 ([x, y, width]) is supported, as in the working reference path")
        self.net = net
        self.n_objects = n_objects
        dev = net.device
        # Keras 2.x Adam(lr, decay, clipnorm, clipvalue) and the non-finite guard (0 / False = off): with
        # any of them set every step's update is engine.adam_clipped(_dev), one launch more
        self.opt = AdamUpdate(dev, lr, l2=l2, clipnorm=clipnorm, clipvalue=clipvalue, decay=decay,
                              skip_nonfinite=skip_nonfinite, totals=True)
        # deep supervision: None (the reference's loss on the last step, exactly the launches of before) or
        # mp_steps weights λ_s >= 0, not all zero — every step then trains on Σ_s λ_s·BCE(z_s, y)
        self._plain = LossPath(dev, net.mp_steps)
        self._path = self._plain if step_loss_weights is None else DeepLossPath(dev, net.mp_steps, step_loss_weights)
        self._rows: Optional[DeepLossPath] = None
        # the tower-level loss: tower_loss > 0 trains on node_loss·L_node + tower_loss·L_tower; 0 =
        # off, exactly the launches of before (node_loss is then not read)
        self.tower_loss, self.node_loss = E.check_tower_loss(tower_loss, node_loss)
        if self.tower_loss > 0:
            if step_loss_weights is not None:
                raise ValueError("tower_loss and step_loss_weights do not combine (the tower term on per-step rows "
                                 "is not built)")
            self._path = TowerLossPath(dev, net.mp_steps, self.tower_loss, self.node_loss, totals=True)
        self.step_loss_weights = self._path.lam
        # DropEdge: every training step (train_on_batch, fit) drops a random subset of the
        # relations, drawn from the step's dropout key; predict and evaluate draw nothing. 0 = off, the calls of before
        self.dropedge = E.check_dropedge(dropedge)
        self.dropedge_symmetric, self.dropedge_rescale = bool(dropedge_symmetric), bool(dropedge_rescale)
        # layer-wise DropEdge (§3zzc; active only with dropedge > 0): a fresh subset at every propagation step
        self.dropedge_per_step = bool(dropedge_per_step)
        if self.dropedge > 0:
            if not E.gates_supported(net.math):
                raise ValueError(f"dropedge needs a math that takes relation gates (x6, x3, h3), not {net.math}")
            if self.step_loss_weights is not None:
                raise ValueError("dropedge and step_loss_weights do not combine (gated per-step logits are not built)")
        self._tot_s = None if step_loss_weights is None else torch.zeros(net.mp_steps, 3, dtype=torch.float64, device=dev)
        self.m = torch.zeros_like(net.flat.data)
        self.v = torch.zeros_like(net.flat.data)
        self.iterations = 0
        self._ws = E.Workspace(dev)
        self._grads = torch.empty_like(net.flat.data)
        self.history: Dict[str, List[float]] = {}
        # replayed fit steps (spwgnn_amd/replay.py): device step words, per-geometry graphs, epoch sums
        self._ctr: Optional[DeviceCounters] = None
        self._replays: Optional[ReplayCache] = None
        self._replay_graph: Optional[tuple] = None   # (graph, weighted, clip options) of the cache in _replays
        self._tot = torch.zeros(3, dtype=torch.float64, device=dev)
        self._w3: Dict[int, torch.Tensor] = {}

    lr, l2, beta1, beta2, eps = (delegated("opt", k) for k in ("lr", "l2", "beta1", "beta2", "eps"))
    clipnorm, clipvalue, decay, skip_nonfinite = (delegated("opt", k) for k in
                                                  ("clipnorm", "clipvalue", "decay", "skip_nonfinite"))
    step_out3 = property(lambda self: self._path.out3s)   # the last loss's (S, 3) per-step rows (step_loss_weights)

    def _dropedge_options(self):
        """(rate, symmetric, rescale) of a DropEdge model — with a fourth entry True when the mask is drawn per
        propagation step — None without it (replay.step_body's argument)."""
        if not self.dropedge > 0:
            return None
        return (self.dropedge, self.dropedge_symmetric, self.dropedge_rescale) + ((True,) if self.dropedge_per_step else ())

    def _dropedge_gates(self, batch, run):
        """A training step's DropEdge mask as relation gates, {} without DropEdge (the calls of before)."""
        if not self.dropedge > 0:
            return {}
        return {"gates": E.dropedge_gates(batch, run, self.dropedge, symmetric=self.dropedge_symmetric,
                                          rescale=self.dropedge_rescale, per_step=self.dropedge_per_step)}

    def _every_step(self) -> DeepLossPath:
        """A path over every step's rows whatever the model trains on: λ = e_{S−1} gives the plain loss's bits."""
        if self._path.lam is not None:
            return self._path
        if self._rows is None:
            self._rows = DeepLossPath(self.net.device, self.net.mp_steps, (0.0,) * (self.net.mp_steps - 1) + (1.0,))
        return self._rows

    def _weights3(self, towers: int) -> torch.Tensor:
        """The epoch sums' fp64 weights [towers of the batch, 1, 1] (fit's convention), cached."""
        if towers not in self._w3:
            self._w3[towers] = torch.tensor([float(towers), 1.0, 1.0], dtype=torch.float64, device=self.net.device)
        return self._w3[towers]

    def _dense_slices(self, x: Dict[str, np.ndarray], batch_size: int):
        """(slice, TowerBatch) over the towers of a dense input dict, `batch_size` at a time: predict's
        batches (the plan fit's validation batch has)."""
        objects = np.asarray(x["objects"], np.float32)
        Rs, Rr, prop = np.asarray(x["sender_relations"]), np.asarray(x["receiver_relations"]), x.get("propagation")
        for b0 in range(0, objects.shape[0], batch_size):
            sl = slice(b0, min(objects.shape[0], b0 + batch_size))
            yield sl, TowerBatch.from_dense(objects[sl], Rs[sl], Rr[sl], None if prop is None else np.asarray(prop)[sl],
                                            device=self.net.device)

    # ---------------------------------------------------------------- inference
    def predict(self, x: Dict[str, np.ndarray], batch_size: int = 32768, return_steps: bool = False) -> np.ndarray:
        """(B, N, 1) probabilities; ``return_steps``: (B, N, S), the probabilities read out after each of
        the S propagation steps (the last column is the plain prediction)."""
        B, N = np.shape(x["objects"])[:2]
        path, R = (self._every_step(), self.net.mp_steps) if return_steps else (self._plain, 1)
        out = np.zeros((B, N, R), np.float32)
        run = self.net.run_config()
        for sl, batch in self._dense_slices(x, batch_size):
            with torch.no_grad():
                z = path.forward(self.net.flat.detach(), batch, run, self._ws)
                out[sl] = E.sigmoid(z.reshape(-1)).reshape(R, -1, N).permute(1, 2, 0).cpu().numpy()
        return out

    # ---------------------------------------------------------------- training
    def train_on_batch(self, batch: TowerBatch, target: torch.Tensor, node_weights=None, tower_targets=None):
        """One Keras step: forward (dropout on), BCE, backward, Adam. Returns out3 = [loss, correct, n]
        (device). `node_weights` (one per node, in the targets' order): the weighted loss of engine.bce
        with the divisor max(#non-zero weights, 1) (one host sync to count them). With step_loss_weights
        out3 = [Σ_s λ_s·loss_s, the last step's correct, n] and `step_out3` holds the (S, 3) per-step rows.
        With tower_loss the loss is node_loss·L_node + tower_loss·L_tower (`loss_parts`: its six parts);
        `tower_targets`: (n_towers,) 0/1 labels, None = derived from the node targets; a `target` of None
        (tower-only labels) drops the node term."""
        net, path = self.net, self._path
        net._step_seed += 1
        run = net.run_config(True, dropout=net.dropout, seed=net._step_seed)
        gated = self._dropedge_gates(batch, run)
        z = path.forward(net.flat.data, batch, run, self._ws, **gated)
        if self.tower_loss > 0:
            out3, dz = path.loss(z, target, node_weights=self._dev_weights(node_weights), batch=batch,
                                 tower_targets=self._dev_weights(tower_targets),
                                 node_loss=0.0 if target is None else None)
        else:
            if tower_targets is not None:
                raise ValueError("tower_targets need a model with tower_loss > 0")
            out3, dz = path.loss(z, target, node_weights=self._dev_weights(node_weights))
        path.backward(net.flat.data, batch, run, self._ws, dz, self._grads, **gated)
        self.iterations += 1
        self.opt.update(net.flat.data, self._grads, self.m, self.v, self.iterations)
        return out3

    def _clip_on(self) -> bool:
        return self.opt.clip_on()

    def _clip_scratch(self) -> E.ClipScratch:   # with totals: the epoch's clip sums
        return self.opt.clip_scratch()

    @property
    def clip_stats(self) -> Optional[torch.Tensor]:
        """The last clipped step's [norm, scale, skipped, clipped] (device tensor), None before one."""
        return None if self.opt.scratch is None else self.opt.scratch.out4

    @property
    def loss_parts(self) -> Optional[torch.Tensor]:
        """The last tower loss's [L_node, node correct, node count, L_tower, towers correct, towers counted]
        (device tensor), None without tower_loss."""
        return self._path.tower.out6 if self.tower_loss > 0 else None

    def _dev_weights(self, node_weights) -> Optional[torch.Tensor]:
        if node_weights is None:
            return None
        return torch.as_tensor(node_weights, dtype=torch.float32, device=self.net.device).reshape(-1).contiguous()

    def _replay_body(self):
        """One fit step's launches for a replayed geometry: the same sequence as train_on_batch
        (key + 1, forward, BCE, backward, Adam at the incremented step) with the per-step scalars
        read from the device, and the epoch sums accumulated on the device."""
        net = self.net
        return step_body(net.flat.data, self._grads, self.m, self.v, self._path, self.opt, self._ctr,
                         lambda **kw: net.run_config(True, dropout=net.dropout, **kw), _lib.STEP_KEY_COUNTER,
                         sums=(self._tot, self._tot_s, self._w3), dropedge=self._dropedge_options())

    def evaluate_batch(self, batch: TowerBatch, target: torch.Tensor, node_weights=None, norm=None, tower_targets=None):
        """out3 = [loss, correct, n] of an inference forward ([Σ_s λ_s·loss_s, the last step's correct, n] with
        step_loss_weights); `node_weights` / `norm` as engine.bce takes them (norm None: the non-zero weights
        are counted, one host sync). With tower_loss: [node_loss·L_node + tower_loss·L_tower, node correct, n],
        the six parts in `loss_parts`; `tower_targets` and a `target` of None as in `train_on_batch`."""
        z = self._path.forward(self.net.flat.data, batch, self.net.run_config(), self._ws)
        if self.tower_loss > 0:
            return self._tower_eval(z, batch, target, self._dev_weights(node_weights), norm,
                                    self._dev_weights(tower_targets))
        return self._path.loss(z, target, node_weights=self._dev_weights(node_weights), norm=norm)[0]

    def _tower_eval(self, z, batch, target, w, norm, tower_targets, sums: bool = False):
        """The tower loss of inference logits, no gradient; `sums`: added to the path's epoch sums (else those
        are left alone)."""
        t = self._path.tower
        return E.bce_tower(z, target, batch, t, self.tower_loss, 0.0 if target is None else self.node_loss,
                           tower_targets=tower_targets, node_weights=w, norm=norm,
                           total6=t.total6 if sums else None, weights6=t.weights6 if sums else None,
                           want_dlogits=False)[0]

    def evaluate(self, x: Dict[str, np.ndarray], y, batch_size: int = 32768, sample_weight=None,
                 threshold: float = 0.5, return_dict: bool = False, return_steps: bool = False):
        """Keras evaluate: ``[loss, binary_accuracy]`` of the model on (x, y) — y the fit's {'target': ...} or
        the array itself — counted on the device (engine.eval_metrics): per batch the inference forward, the
        accumulating loss (fp64 sums with weights (towers of the batch, 1, 1), fit's convention: the loss
        is the tower-weighted mean of the batch losses) and the metrics launch; the host reads the device
        once, after the last batch.

        ``return_dict``: metrics.summarize of the tables (node, tower and per-tower-size confusion, ROC area,
        average precision, best threshold) plus ``loss``. ``threshold``: a node is predicted stable when its
        probability exceeds it (0.5: the reference's, JengaBuilder.py:343); the loss does not depend on it.
        ``sample_weight`` ((B,) or (B, N)) as in `fit`: the loss is weighted per batch by Σ w·bce / #{w ≠ 0} and
        a zero weight masks its node out of every count. ``return_steps``: a list of mp_steps summaries, the
        logits read out after each propagation step scored against the same targets (with or without
        step_loss_weights); entry s carries that step's own ``loss``, and the last entry is the plain summary.
        With step_loss_weights the model's loss is Σ_s λ_s·loss_s, as in `fit`: it is the last entry's ``loss``,
        and every entry carries its own as ``step_loss``."""
        from . import metrics as M
        if self.tower_loss > 0:
            return self._evaluate_tower(x, y, batch_size, sample_weight, threshold, return_dict, return_steps)
        if isinstance(y, dict) and "tower_target" in y:
            raise ValueError("y['tower_target'] needs a model with tower_loss > 0")
        objects = np.asarray(x["objects"], np.float32)
        B = objects.shape[0]
        target = np.asarray(y["target"] if isinstance(y, dict) else y, np.float32).reshape(B, -1)
        tau = E.check_threshold(threshold)
        W = node_weights(target, sample_weight) if sample_weight is not None else None
        dev, net, S = self.net.device, self.net, self.net.mp_steps
        lam = self.step_loss_weights
        # return_steps: every step's loss rides in the one loss launch, whatever the model trains on
        path = self._every_step() if return_steps else self._path
        by_steps = path.lam is not None
        tot_s = torch.zeros(S, 3, dtype=torch.float64, device=dev) if by_steps else None
        tables = E.EvalTables(dev, rows=S if return_steps else 1)
        tot = torch.zeros(3, dtype=torch.float64, device=dev)
        run = net.run_config()
        for idx, batch in self._dense_slices(x, batch_size):
            tgt = torch.as_tensor(target[idx], device=dev).reshape(-1).contiguous()
            w = self._dev_weights(W[idx]) if W is not None else None
            norm = max(int(np.count_nonzero(W[idx])), 1) if W is not None else None   # counted on the host
            z = path.forward(net.flat.data, batch, run, self._ws)
            path.loss(z, tgt, total3=tot, weights3=self._weights3(batch.n_towers), total3s=tot_s, node_weights=w,
                      norm=norm)
            E.eval_metrics(z if return_steps else path.last(z), tgt, tables, batch=batch, node_weights=w, threshold=tau)
        # the one device read: the integer tables and the bits of the fp64 loss sums in one copy
        sums = [tot.view(torch.int64)] + ([tot_s.reshape(-1).view(torch.int64)] if by_steps else [])
        host = torch.cat([tables.flat] + sums).cpu()
        nt = tables.flat.numel()
        counts = tables.split(host[:nt])
        loss = float(host[nt:nt + 3].view(torch.float64)[0]) / max(B, 1)
        if not return_steps:
            out = dict(M.summarize(counts), loss=loss)
            return out if return_dict else [loss, out["binary_accuracy"]]
        step_loss = (host[nt + 3:].view(torch.float64).reshape(S, 3)[:, 0] / max(B, 1)).tolist()
        outs = [dict(M.summarize(counts, row=s), loss=step_loss[s]) for s in range(S)]
        if lam is not None:
            for s in range(S):
                outs[s]["step_loss"] = step_loss[s]
            outs[-1]["loss"] = loss
        return outs

    def fit(self, x: Dict[str, np.ndarray], y: Dict[str, np.ndarray], batch_size: int = 32, epochs: int = 10,
            validation_split: float = 0.0, shuffle: bool = True, verbose: int = 1, seed: int = 0,
            graph: bool = False, sample_weight=None, class_weight=None):
        """Keras fit (main.py:92-98). Each training step is the replayable step of
        spwgnn_amd/replay.py — forward, BCE, backward and Adam per batch geometry on static buffers
        refilled by the step's first launch — issued eagerly (`graph=True`: the same step captured
        once and replayed as a hipGraph; bit-identical results; on the MI355X host eager issue is the
        faster, 0.270 vs 0.277 ms per step at batch 32); batches are planned with
        N(N−1) relation slots per tower.

        `sample_weight` ((B,) per tower or (B, N) per node) and `class_weight` ({0: a, 1: b}, per node by
        its target — an extension, Keras refuses it for 3-D targets) weight the loss as Keras 2.x does
        (`node_weights`): each batch's loss is Σ w·bce / #{w ≠ 0}. They are computed before the validation
        split and split with it, and weight val_loss too. A zero weight masks its node; a batch whose
        weights are all zero gives loss 0 and no gradient, where Keras gives NaN (0/0). The accuracies
        count the nodes with w ≠ 0 only — with zero weights a deviation from Keras, whose `metrics=` stay
        unweighted; with none it is Keras's. With neither argument the steps are exactly the unweighted
        ones.

        With clipnorm, clipvalue, decay or skip_nonfinite set on the model the history gains, per epoch,
        `grad_norm` (the mean global gradient norm over the epoch's non-skipped steps), `clipped_steps` and
        `skipped_steps`, from one fp64 device accumulator read where the loss sums are read.

        With step_loss_weights set on the model `loss` / `val_loss` are Σ_s λ_s·loss_s, `binary_accuracy` stays
        the last step's, and the history gains `step_loss` and `step_binary_accuracy`: per epoch a list of S
        values, each step's own loss and accuracy, summed on the device in the loss launch."""
        if self.tower_loss > 0:
            return self._fit_tower(x, y, batch_size, epochs, validation_split, shuffle, verbose, seed, graph,
                                   sample_weight, class_weight)
        if "tower_target" in y:
            raise ValueError("y['tower_target'] needs a model with tower_loss > 0")
        if "relation_weights" in x:
            raise ValueError("x['relation_weights'] is not part of fit (replayed steps carry no base weights); "
                             "Trainer.step(relation_weights=) and GraphNetwork take them")
        objects = np.asarray(x["objects"], np.float32)
        target = np.asarray(y["target"], np.float32).reshape(objects.shape[0], -1)
        B = objects.shape[0]
        weighted = sample_weight is not None or class_weight is not None
        W = node_weights(target, sample_weight, class_weight) if weighted else None
        n_tr = keras_split_at(B, validation_split)
        n_val = B - n_tr
        ds = CompactDataset(objects, x["sender_relations"], x["receiver_relations"], x.get("propagation"))
        rng = np.random.default_rng(seed)
        dev = self.net.device
        hist = {"loss": [], "binary_accuracy": []}
        clip_on = self._clip_on()
        if clip_on:
            hist.update({"grad_norm": [], "clipped_steps": [], "skipped_steps": []})
            clip = self._clip_scratch()
        lam = self.step_loss_weights
        if lam is not None:
            hist.update({"step_loss": [], "step_binary_accuracy": []})
        if n_val:
            hist.update({"val_loss": [], "val_binary_accuracy": []})
            vbatch = ds.subset(np.arange(n_tr, B), dev)
            vtgt = torch.as_tensor(target[n_tr:], device=dev).reshape(-1).contiguous()
            vw = self._dev_weights(W[n_tr:]) if weighted else None
            vnorm = max(int(np.count_nonzero(W[n_tr:])), 1) if weighted else None   # counted once, on the host
        # every step runs as a replayed hipGraph per batch geometry (graph=False: the same launches
        # eagerly); the device words start from the host counters and the host mirrors each step
        if self._ctr is None:
            self._ctr = DeviceCounters(dev, self.net._step_seed, self.iterations, self.lr, self.beta1,
                                       self.beta2, decay=self.decay)
        else:
            self._ctr.set(key=self.net._step_seed, step=self.iterations, lr=self.lr, beta1=self.beta1,
                          beta2=self.beta2, decay=self.decay)
        # the clip options are baked into a geometry's launches (and its captured graph)
        opts = (graph, weighted, self.clipnorm, self.clipvalue, self.skip_nonfinite, clip_on, self._dropedge_options())
        if lam is not None:
            opts += (lam,)
        if self._replays is None or self._replay_graph != opts:
            self._replays = ReplayCache(dev, self._replay_body, graph=graph, weighted=weighted)
            self._replay_graph = opts
        # per-epoch sums stay on the device (stream-ordered copies) and are read once after the last
        # epoch — with verbose=0 the host never waits for the GPU between epochs (a sync per epoch
        # drained the pipeline: ≈ 8 µs per step at batch 32); verbose > 0 reads them per epoch to print
        ep_tot = torch.zeros(epochs, 3, dtype=torch.float64, device=dev)
        ep_val = torch.zeros(epochs, 3, dtype=torch.float32, device=dev)
        ep_clip = torch.zeros(epochs, 4, dtype=torch.float64, device=dev) if clip_on else None
        ep_steps = torch.zeros(epochs, len(lam), 3, dtype=torch.float64, device=dev) if lam is not None else None

        def record(ep):
            tot_l, tot_c, tot_n = ep_tot[ep].tolist()
            hist["loss"].append(tot_l / max(n_tr, 1))
            hist["binary_accuracy"].append(tot_c / max(tot_n, 1))
            if lam is not None:
                rows = ep_steps[ep].tolist()
                hist["step_loss"].append([r[0] / max(n_tr, 1) for r in rows])
                hist["step_binary_accuracy"].append([r[1] / max(r[2], 1) for r in rows])
            if clip_on:
                c_norm, c_clipped, c_skipped, c_steps = ep_clip[ep].tolist()
                hist["grad_norm"].append(c_norm / max(c_steps - c_skipped, 1.0))
                hist["clipped_steps"].append(int(c_clipped))
                hist["skipped_steps"].append(int(c_skipped))
            if n_val:
                vl, vc, vn = ep_val[ep].tolist()
                hist["val_loss"].append(vl)
                hist["val_binary_accuracy"].append(vc / max(vn, 1))

        for ep in range(epochs):
            order = rng.permutation(n_tr) if shuffle else np.arange(n_tr)
            # (Σ loss·batch, Σ correct, Σ nodes) on the device: no host sync per batch, so the host
            # builds the next batch while the GPU runs this one
            self._tot.zero_()
            if lam is not None:
                self._tot_s.zero_()
            if clip_on:
                clip.total4.zero_()
            for b0 in range(0, n_tr, batch_size):
                idx = order[b0:b0 + batch_size]
                self._weights3(len(idx))
                self._replays(ds.subset_plan(idx, edge_cap=True), target[idx], W[idx] if weighted else None)
                self.net._step_seed += 1
                self.iterations += 1
            ep_tot[ep].copy_(self._tot)
            if lam is not None:
                ep_steps[ep].copy_(self._tot_s)
            if clip_on:
                ep_clip[ep].copy_(clip.total4)
            if n_val:
                ep_val[ep].copy_(self.evaluate_batch(vbatch, vtgt, vw, vnorm))
            if verbose:
                record(ep)
                msg = f"Epoch {ep + 1}/{epochs} - loss: {hist['loss'][-1]:.4f} - binary_accuracy: {hist['binary_accuracy'][-1]:.4f}"
                if n_val:
                    msg += f" - val_loss: {hist['val_loss'][-1]:.4f} - val_binary_accuracy: {hist['val_binary_accuracy'][-1]:.4f}"
                print(msg)
        if not verbose:
            for ep in range(epochs):
                record(ep)
        for k, v in hist.items():
            self.history.setdefault(k, []).extend(v)
        return hist


    # ---------------------------------------------------------------- the tower-level loss
    def _tower_labels(self, x, y, sample_weight, class_weight=None):
        """(B, N, node targets (B, N) or None, tower targets (B,) or None, node weights (B, N) or None) of a
        fit / evaluate call on a tower-loss model. Without 'target' the node term is off (node_loss 0)."""
        B, N = np.shape(x["objects"])[:2]
        y = y if isinstance(y, dict) else {"target": y}
        target = np.asarray(y["target"], np.float32).reshape(B, -1) if "target" in y else None
        tt = np.asarray(y["tower_target"], np.float32).reshape(-1) if "tower_target" in y else None
        if target is None and tt is None:
            raise ValueError("y needs 'target', 'tower_target' or both")
        if tt is not None and tt.shape != (B,):
            raise ValueError(f"y['tower_target'] must hold one label per tower ({B},), got {tt.shape}")
        W = None
        if sample_weight is not None or class_weight is not None:
            if target is None and class_weight is not None:
                raise ValueError("class_weight goes by the node targets: it needs y['target']")
            W = node_weights(target if target is not None else np.zeros((B, N), np.float32), sample_weight, class_weight)
        return B, N, target, tt, W

    def _tower_step(self, batch, target, w, tt):
        """One eager fit step with the tower loss: the replayed step's launches (spwgnn_amd/replay.py step_body)
        with this batch's own buffers — the key/step advance, the forward, the loss launch and the backward,
        Adam at the device step word. Explicit tower targets and weighted batches take it: their labels and
        the tower divisor, a per-batch count, are not part of a replayed geometry's static block."""
        net, path, ctr = self.net, self._path, self._ctr
        E.step_advance(ctr.key, ctr.step, _lib.STEP_KEY_COUNTER, 0, 0)
        run = net.run_config(True, dropout=net.dropout, seed_dev=ctr.key)
        gated = self._dropedge_gates(batch, run)
        z = path.forward(net.flat.data, batch, run, self._ws, **gated)
        path.loss_backward(net.flat.data, batch, run, self._ws, z, target, None, None, self._grads, node_weights=w,
                           tower_targets=tt, node_loss=0.0 if target is None else None, **gated)
        self.opt.update_dev(net.flat.data, self._grads, self.m, self.v, ctr, self.opt.totals)

    def _fit_tower(self, x, y, batch_size, epochs, validation_split, shuffle, verbose, seed, graph, sample_weight,
                   class_weight):
        """`fit` with tower_loss > 0. y: {'target': (B, N[, 1])} (tower labels derived: a tower stands iff every
        counted node target is 1), {'tower_target': (B,)} alone (tower-only labels: node_loss is forced to 0) or
        both. Derived labels without weights run the replayed step (`graph` as in `fit`); explicit tower
        targets or weights run the same launches eagerly per batch (`_tower_step`). The history holds `loss`
        (= node_loss·L_node + tower_loss·L_tower), `binary_accuracy`, `tower_loss` (L_tower) and
        `tower_accuracy`, with `val_` forms under validation_split — batch means weighted by the batch's
        towers, as `fit`'s — and the clip statistics of `fit`. Each batch's L_tower divides by its own
        counted towers."""
        B, N, target, tt, W = self._tower_labels(x, y, sample_weight, class_weight)
        alpha = self.node_loss if target is not None else 0.0
        weighted = W is not None
        replayed = tt is None and not weighted
        n_tr = keras_split_at(B, validation_split)
        n_val = B - n_tr
        ds = CompactDataset(np.asarray(x["objects"], np.float32), x["sender_relations"], x["receiver_relations"],
                            x.get("propagation"))
        rng = np.random.default_rng(seed)
        dev, path = self.net.device, self._path
        tot6, w6 = path.tower.total6, path.tower.weights6
        hist = {"loss": [], "binary_accuracy": [], "tower_loss": [], "tower_accuracy": []}
        clip_on = self._clip_on()
        if clip_on:
            hist.update({"grad_norm": [], "clipped_steps": [], "skipped_steps": []})
            clip = self._clip_scratch()
        if n_val:
            hist.update({"val_" + k: [] for k in ("loss", "binary_accuracy", "tower_loss", "tower_accuracy")})
            vbatch = ds.subset(np.arange(n_tr, B), dev)
            vtgt = None if target is None else torch.as_tensor(target[n_tr:], device=dev).reshape(-1).contiguous()
            vw = self._dev_weights(W[n_tr:]) if weighted else None
            vnorm = max(int(np.count_nonzero(W[n_tr:])), 1) if weighted else None
            vtt = self._dev_weights(tt[n_tr:]) if tt is not None else None
        if self._ctr is None:
            self._ctr = DeviceCounters(dev, self.net._step_seed, self.iterations, self.lr, self.beta1,
                                       self.beta2, decay=self.decay)
        else:
            self._ctr.set(key=self.net._step_seed, step=self.iterations, lr=self.lr, beta1=self.beta1,
                          beta2=self.beta2, decay=self.decay)
        if "relation_weights" in x:
            raise ValueError("x['relation_weights'] is not part of fit (replayed steps carry no base weights)")
        opts = (graph, "tower", self.tower_loss, alpha, self.clipnorm, self.clipvalue, self.skip_nonfinite, clip_on,
                self._dropedge_options())
        if replayed and (self._replays is None or self._replay_graph != opts):
            net = self.net
            self._replays = ReplayCache(dev, lambda: step_body(
                net.flat.data, self._grads, self.m, self.v, path, self.opt, self._ctr,
                lambda **kw: net.run_config(True, dropout=net.dropout, **kw), _lib.STEP_KEY_COUNTER,
                dropedge=self._dropedge_options()), graph=graph)
            self._replay_graph = opts
        ep_tot = torch.zeros(epochs, 6, dtype=torch.float64, device=dev)
        ep_val = torch.zeros(epochs, 6, dtype=torch.float32, device=dev)
        ep_clip = torch.zeros(epochs, 4, dtype=torch.float64, device=dev) if clip_on else None
        mu = self.tower_loss

        def record(ep):
            t = ep_tot[ep].tolist()
            hist["loss"].append((alpha * t[0] + mu * t[3]) / max(n_tr, 1))
            hist["binary_accuracy"].append(t[1] / max(t[2], 1))
            hist["tower_loss"].append(t[3] / max(n_tr, 1))
            hist["tower_accuracy"].append(t[4] / max(t[5], 1))
            if clip_on:
                c_norm, c_clipped, c_skipped, c_steps = ep_clip[ep].tolist()
                hist["grad_norm"].append(c_norm / max(c_steps - c_skipped, 1.0))
                hist["clipped_steps"].append(int(c_clipped))
                hist["skipped_steps"].append(int(c_skipped))
            if n_val:
                v = ep_val[ep].tolist()
                hist["val_loss"].append(alpha * v[0] + mu * v[3])
                hist["val_binary_accuracy"].append(v[1] / max(v[2], 1))
                hist["val_tower_loss"].append(v[3])
                hist["val_tower_accuracy"].append(v[4] / max(v[5], 1))

        for ep in range(epochs):
            order = rng.permutation(n_tr) if shuffle else np.arange(n_tr)
            tot6.zero_()
            if clip_on:
                clip.total4.zero_()
            for b0 in range(0, n_tr, batch_size):
                idx = order[b0:b0 + batch_size]
                w6.copy_(self._weights6(len(idx)))          # stream-ordered: the step's loss launch reads it
                plan = ds.subset_plan(idx, edge_cap=True)
                if replayed:
                    self._replays(plan, target[idx])
                else:
                    self._tower_step(TowerBatch.from_plan(plan, dev),
                                     None if target is None else torch.as_tensor(target[idx], device=dev).reshape(-1).contiguous(),
                                     self._dev_weights(W[idx]) if weighted else None,
                                     self._dev_weights(tt[idx]) if tt is not None else None)
                self.net._step_seed += 1
                self.iterations += 1
            ep_tot[ep].copy_(tot6)
            if clip_on:
                ep_clip[ep].copy_(clip.total4)
            if n_val:
                self.evaluate_batch(vbatch, vtgt, vw, vnorm, vtt)
                ep_val[ep].copy_(path.tower.out6)
            if verbose:
                record(ep)
                msg = (f"Epoch {ep + 1}/{epochs} - loss: {hist['loss'][-1]:.4f} - binary_accuracy: "
                       f"{hist['binary_accuracy'][-1]:.4f} - tower_loss: {hist['tower_loss'][-1]:.4f} - tower_accuracy: "
                       f"{hist['tower_accuracy'][-1]:.4f}")
                if n_val:
                    msg += (f" - val_loss: {hist['val_loss'][-1]:.4f} - val_tower_loss: {hist['val_tower_loss'][-1]:.4f}"
                            f" - val_tower_accuracy: {hist['val_tower_accuracy'][-1]:.4f}")
                print(msg)
        w6.fill_(1.0)
        if not verbose:
            for ep in range(epochs):
                record(ep)
        for k, v in hist.items():
            self.history.setdefault(k, []).extend(v)
        return hist

    def _weights6(self, towers: int) -> torch.Tensor:
        """The epoch sums' fp64 weights of out6: the two losses times the batch's towers (fit's convention)."""
        key = ("w6", towers)
        if key not in self._w3:
            self._w3[key] = torch.tensor([float(towers), 1.0, 1.0, float(towers), 1.0, 1.0], dtype=torch.float64,
                                         device=self.net.device)
        return self._w3[key]

    def _evaluate_tower(self, x, y, batch_size, sample_weight, threshold, return_dict, return_steps):
        """`evaluate` with tower_loss > 0: [loss, binary_accuracy, tower_loss, tower_accuracy], or with
        ``return_dict`` the summary of `evaluate` plus ``tower_loss`` and ``tower_accuracy`` (at 0.5, against the
        labels the loss uses: y['tower_target'] or the derived ones); ``loss`` is node_loss·L_node +
        tower_loss·L_tower. y as in `fit`."""
        from . import metrics as M
        if return_steps:
            raise ValueError("return_steps is not built for tower-loss models")
        B, N, target, tt, W = self._tower_labels(x, y, sample_weight)
        alpha = self.node_loss if target is not None else 0.0
        tau = E.check_threshold(threshold)
        dev, net, path = self.net.device, self.net, self._path
        tables = E.EvalTables(dev) if target is not None else None
        tot = torch.zeros(6, dtype=torch.float64, device=dev)
        run = net.run_config()
        for idx, batch in self._dense_slices(x, batch_size):
            tgt = None if target is None else torch.as_tensor(target[idx], device=dev).reshape(-1).contiguous()
            w = self._dev_weights(W[idx]) if W is not None else None
            norm = max(int(np.count_nonzero(W[idx])), 1) if W is not None else None
            z = path.forward(net.flat.data, batch, run, self._ws)
            self._tower_eval(z, batch, tgt, w, norm, self._dev_weights(tt[idx]) if tt is not None else None)
            tot += path.tower.out6.double() * self._weights6(batch.n_towers)
            if tables is not None:
                E.eval_metrics(z, tgt, tables, batch=batch, node_weights=w, threshold=tau)
        t = tot.tolist()
        parts = dict(loss=(alpha * t[0] + self.tower_loss * t[3]) / max(B, 1), tower_loss=t[3] / max(B, 1),
                     tower_accuracy=t[4] / max(t[5], 1))
        acc = t[1] / max(t[2], 1)
        if not return_dict:
            return [parts["loss"], acc, parts["tower_loss"], parts["tower_accuracy"]]
        out = dict(M.summarize(tables.cpu())) if tables is not None else {"binary_accuracy": acc}
        out.update(parts)
        return out


def keras_split_at(n_samples: int, validation_split: float) -> int:
    """Number of training samples Keras 2.x keeps for fit(validation_split=v) (main.py:96):
    split_at = int(n · (1 − v)); the validation set is the LAST n − split_at samples, taken before
    shuffling."""
    if not validation_split:
        return int(n_samples)
    if not 0.0 < validation_split < 1.0:
        raise ValueError("validation_split must be in [0, 1)")
    return int(int(n_samples) * (1.0 - validation_split))


class PropagationNetwork:
    """Networks.py:12-104: getModel caches one compiled model per n_objects, all sharing the
    weights of the first one built (set_weights / reuse_model, Networks.py:40-56)."""

    def __init__(self, device="cuda", seed: int = 0, mp_steps: int = E.REF_MP_STEPS, dropout: float = E.REF_DROPOUT,
                 math: str = "x6", clipnorm: float = 0.0, clipvalue: float = 0.0, decay: float = 0.0,
                 skip_nonfinite: bool = False, step_loss_weights=None, tower_loss: float = 0.0, node_loss: float = 1.0,
                 dropedge: float = 0.0, dropedge_symmetric: bool = True, dropedge_rescale: bool = False,
                 dropedge_per_step: bool = False):
        # Networks.py:101 Adam(lr=0.0005, decay=0.0); clipnorm / clipvalue are Keras 2.x Optimizer kwargs
        E.check_clip_options(clipnorm, clipvalue, decay)
        if step_loss_weights is not None:   # deep supervision (KerasModel): one weight per propagation step
            step_loss_weights = E.check_step_weights(step_loss_weights, mp_steps)
        tower_loss, node_loss = E.check_tower_loss(tower_loss, node_loss)   # the tower-level loss (KerasModel); 0 = off
        if tower_loss > 0 and step_loss_weights is not None:
            raise ValueError("tower_loss and step_loss_weights do not combine")
        self._opt = dict(clipnorm=clipnorm, clipvalue=clipvalue, decay=decay, skip_nonfinite=skip_nonfinite,
                         step_loss_weights=step_loss_weights, tower_loss=tower_loss, node_loss=node_loss,
                         dropedge=E.check_dropedge(dropedge), dropedge_symmetric=dropedge_symmetric,
                         dropedge_rescale=dropedge_rescale, dropedge_per_step=bool(dropedge_per_step))
        if math not in E.MATH_MODES:
            raise ValueError(f"math must be one of {sorted(E.MATH_MODES)}")
        if self._opt["dropedge"] > 0:   # DropEdge (KerasModel): refused here, at construction, where it cannot run
            if not E.gates_supported(math):
                raise ValueError(f"dropedge needs a math that takes relation gates (x6, x3, h3), not {math}")
            if step_loss_weights is not None:
                raise ValueError("dropedge and step_loss_weights do not combine")
        self._math = math   # every model's arithmetic (GraphNetwork.math); "x6": the fp32-class default
        self.Nets: Dict[int, KerasModel] = {}
        self.set_weights = False
        self._net: Optional[GraphNetwork] = None
        self._device, self._seed, self._mp, self._drop = device, seed, mp_steps, dropout

    def getModel(self, n_objects: int, object_dim: int = 3, relation_dim: int = 1) -> KerasModel:  # noqa: N802
        if n_objects in self.Nets:
            return self.Nets[n_objects]
        if not self.set_weights:
            self._net = GraphNetwork(self._mp, self._drop, self._seed, device=self._device, math=self._math)
            self.set_weights = True
        model = KerasModel(self._net, n_objects, object_dim, **self._opt)
        self.Nets[n_objects] = model
        return model
