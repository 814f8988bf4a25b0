"""Data-parallel training step: towers sharded over ranks, one RCCL all-reduce of the flat gradient.

The reference trains with Keras fit on one CPU process (src/main.py:92-98; Adam + BCE compiled at
src/Networks.py:101-102). Here every rank owns a shard of the tower batch (towers are independent
graphs, so the shard needs no halo and no data-path collective), runs forward → BCE → backward
through libspwgnn_hip, and the 209,501 fp32 gradients (one flat bucket, 0.84 MB) are summed with
ONE torch.distributed all-reduce (backend "nccl" = RCCL over xGMI on MI355X), then Adam runs on
every rank.

Weighting: the reference's loss is the mean BCE over all B·N nodes of the batch
(src/Networks.py:102). A rank's backward yields the gradient of the mean over ITS nodes, so each
rank scales its gradient by n_local / n_global before the sum; Σ_r (n_r/n)·g_r is then exactly
the gradient of the global mean, for ragged and unequal shards alike (config 4). n_global comes
from the shard plan (`spwgnn_amd/shard.py`) or, when not given, from one 8-byte all-reduce.
Micro-batches (`step` with lists) accumulate their node-weighted gradients before the one
all-reduce and the one Adam update.

Per-node loss weights (`step(..., weights=)`, Keras's sample_weight / class_weight): the loss is
Σ w·bce over the nodes of the global batch divided by the number of its nodes with w ≠ 0
(`norm_global`). Each micro-batch's loss divides by its own non-zero count nnz_i, and its gradient is
scaled by nnz_i / norm_global instead of n_i / n_global: the same sum.

The arithmetic engine is pluggable only so the CPU test-suite can drive this control flow under
gloo with the oracle; the product engine is HipEngine and has no CPU fallback.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.distributed as dist

from . import _lib, engine as E, params as P
from .batch import TowerBatch
from .replay import DeviceCounters, step_body
from .step import AdamUpdate, delegated, loss_path


_M64 = (1 << 64) - 1


def splitmix64(x: int) -> int:
    """One splitmix64 output step (Steele et al.): a bijective 64-bit mix."""
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def dropout_key(seed: int, iteration: int, rank: int, micro: int) -> int:
    """The run's 64-bit dropout key for (seed, optimizer step, rank, micro-batch): each field is
    folded through splitmix64 in turn, so no field overflows into the next (a packed
    ((seed·P + it)·R + rank)·M + micro key collides once rank ≥ R or micro ≥ M)."""
    h = splitmix64(seed & _M64)
    for v in (iteration, rank, micro):
        h = splitmix64(h ^ (v & _M64))
    return h


class HipEngine:
    """The product engine of the protocol (spwgnn_amd/step.py): libspwgnn_hip on one device. With
    step_loss_weights set (deep supervision) "logits" and "dlogits" are the (mp_steps, n) rows of every step
    and the loss is Σ_s λ_s·BCE(z_s); the Trainer's control flow — scaling, all-reduce, the early-gradient
    event — only hands them through, so which loss runs is `path`'s business alone."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.ws = E.Workspace(self.device)
        self.grads: Optional[torch.Tensor] = None
        self._early_ev = self._clip = None
        self.set_step_loss_weights(None, E.REF_MP_STEPS)

    def set_step_loss_weights(self, lam, mp_steps: int):
        self.path = loss_path(self.device, mp_steps, lam)

    def set_tower_loss(self, tower_loss: float, node_loss: float, mp_steps: int):
        """The tower-level loss (step.TowerLossPath) as this engine's path: replayed steps run it too."""
        self.path = loss_path(self.device, mp_steps, None, tower_loss=tower_loss, node_loss=node_loss)

    def loss_tower(self, logits, target, batch, tower_targets, weights, norm, norm_t, tower_loss, node_loss,
                   want_dlogits: bool = True):
        """(out6, dlogits) of engine.bce_tower with the step's coefficients and divisors; out6 is one
        persistent tensor the next call reuses. `want_dlogits` False (evaluate): the loss only, dlogits None."""
        t = self.path.tower
        _, dz = E.bce_tower(logits, target, batch, t, tower_loss, node_loss, tower_targets=tower_targets, norm_t=norm_t,
                            node_weights=weights, norm=norm, want_dlogits=want_dlogits)
        return t.out6, dz

    step_loss_weights = property(lambda self: self.path.lam)
    bce_scratch = property(lambda self: self.path.scratch)
    out3s = property(lambda self: self.path.out3s)   # the last loss's per-step [loss, correct, n] (device, (mp_steps, 3))

    def forward(self, params, batch: TowerBatch, run: E.RunConfig, gates=None):
        return self.path.forward(params, batch, run, self.ws, gates=gates)

    def dropedge_gates(self, batch: TowerBatch, run: E.RunConfig, rate, symmetric=True, rescale=False, base=None,
                       per_step=False):
        """The step's DropEdge mask as relation gates (engine.dropedge_gates), drawn from the run's key."""
        return E.dropedge_gates(batch, run, rate, symmetric=symmetric, rescale=rescale, base=base, per_step=per_step)

    def loss(self, logits, target):
        return self.path.loss(logits, target)

    def loss_weighted(self, logits, target, weights, norm):
        return self.path.loss(logits, target, node_weights=weights, norm=norm)

    def backward(self, params, batch, run, dlogits, gates=None):
        if self.grads is None or self.grads.numel() != params.numel():
            self.grads = torch.empty_like(params)
        return self.path.backward(params, batch, run, self.ws, dlogits, self.grads, gates=gates)

    def eval_metrics(self, logits, target, tables, batch, weights=None, threshold=0.5):
        """The evaluation counts of `logits` (the rows `forward` returned) added to `tables` on the device
        (engine.eval_metrics)."""
        return E.eval_metrics(logits, target, tables, batch=batch, node_weights=weights, threshold=threshold)

    def early_event(self):
        """The event the library records once the early gradient range is final
        (spwgnn_run.grads_early_event); created (recorded once) on first use."""
        if self._early_ev is None:
            self._early_ev = torch.cuda.Event()
            self._early_ev.record(torch.cuda.current_stream(self.device))   # creates the underlying hipEvent_t
        return self._early_ev

    def adam(self, params, grads, m, v, step, lr, b1, b2, eps, l2, gscale):
        E.adam(params, grads, m, v, step, lr, b1, b2, eps, l2, gscale)

    def clip_scratch(self) -> "E.ClipScratch":
        if self._clip is None:
            self._clip = E.ClipScratch(self.device)
        return self._clip

    def adam_clipped(self, params, grads, m, v, step, lr, b1, b2, eps, l2, gscale, clipnorm, clipvalue,
                     skip_nonfinite):
        """`adam` on the clipped gradient (engine.adam_clipped); returns out4 = [norm, scale, skipped,
        clipped], a device tensor the next step overwrites."""
        return E.adam_clipped(params, grads, m, v, step, self.clip_scratch(), lr, b1, b2, eps, l2, gscale,
                              clipnorm, clipvalue, skip_nonfinite)


def _micro_batches(batches, targets, weights):
    """`step`'s and `evaluate`'s arguments as lists of equal length, one entry per micro-batch."""
    batches = batches if isinstance(batches, (list, tuple)) else [batches]
    targets = targets if isinstance(targets, (list, tuple)) else [targets]
    if len(batches) != len(targets) or not batches:
        raise ValueError("one target per micro-batch")
    if weights is not None:
        weights = weights if isinstance(weights, (list, tuple)) else [weights]
        if len(weights) != len(batches):
            raise ValueError("one weight tensor per micro-batch")
    return batches, targets, weights


def _nonzero(weights) -> int:
    return int(torch.count_nonzero(torch.as_tensor(weights)).item())   # one host sync


class Trainer:
    """Keras-semantics training step (dropout 0.1, BCE, Adam lr=5e-4 eps=1e-7) with optional DP."""

    def __init__(self, params: torch.Tensor, engine=None, mp_steps: int = E.REF_MP_STEPS,
                 dropout: float = E.REF_DROPOUT, seed: int = 0, lr: float = 5e-4, beta1: float = 0.9,
                 beta2: float = 0.999, eps: float = 1e-7, l2: float = 0.0, group=None, math: str = "x6",
                 buckets: int = 1, overlap: bool = True, clipnorm: float = 0.0, clipvalue: float = 0.0,
                 decay: float = 0.0, skip_nonfinite: bool = False, step_loss_weights=None, tower_loss: float = 0.0,
                 node_loss: float = 1.0, dropedge: float = 0.0, dropedge_symmetric: bool = True,
                 dropedge_rescale: bool = False, dropedge_per_step: bool = False):
        # dropedge_per_step (layer-wise DropEdge; active only with dropedge > 0): a fresh subset at
        # every propagation step — the step's gates are (mp_steps, slots) and go to the engine as step_gates.
        # dropedge (a rate in [0, 1)): every training step drops a random subset of the relations —
        # gate 0 in the receiver sum, or 1/(1 − rate) on a kept one with dropedge_rescale — drawn from the step's
        # dropout key with a kind of its own; dropedge_symmetric: both directions of a contact share the draw.
        # Training only (`evaluate` draws nothing). 0: exactly the steps of before, no gated call.
        # tower_loss (mu > 0): the objective is node_loss·L_node + tower_loss·L_tower, L_tower the tower-level
        # BCE of engine.bce_tower; `step` then takes tower_targets= and sets `loss_parts`.
        # 0: exactly the steps of before (node_loss is then not read).
        # step_loss_weights (None, or mp_steps floats >= 0, not all zero): deep supervision — the loss is
        # Σ_s λ_s·BCE(z_s, y) over every propagation step's logits instead of the last step's BCE; `step`
        # then returns [that sum, the last step's correct count, n]. None: exactly the steps of before.
        # Keras 2.x optimizer arguments (0 = off) and the non-finite guard: with any of them set the
        # update is engine.adam_clipped — the global norm of the all-reduced gradient, one launch more —
        # instead of engine.adam; with none, exactly the launches of before
        # (the eager `step` goes through the engine protocol; `opt` itself runs the replayed steps' update)
        self.opt = AdamUpdate(params.device, lr, beta1, beta2, eps, l2, clipnorm, clipvalue, decay, skip_nonfinite)
        self.params = params
        self.engine = engine if engine is not None else HipEngine(params.device)
        if self.opt.clip_on() and not hasattr(self.engine, "adam_clipped"):
            raise ValueError("clipnorm / clipvalue / decay / skip_nonfinite need an engine with adam_clipped("
                             "params, grads, m, v, step, lr, b1, b2, eps, l2, gscale, clipnorm, clipvalue, "
                             "skip_nonfinite) (the engine protocol: spwgnn_amd/step.py)")
        self.step_loss_weights = None if step_loss_weights is None else E.check_step_weights(step_loss_weights, mp_steps)
        if self.step_loss_weights is not None:
            if not hasattr(self.engine, "set_step_loss_weights"):
                raise ValueError("step_loss_weights needs an engine with set_step_loss_weights(weights, mp_steps) "
                                 "(the engine protocol: spwgnn_amd/step.py)")
            self.engine.set_step_loss_weights(self.step_loss_weights, mp_steps)
        self.tower_loss, self.node_loss = E.check_tower_loss(tower_loss, node_loss)
        self.loss_parts = None    # the last tower-loss step's six numbers for this rank's shard (device, fp32)
        if self.tower_loss > 0:
            if self.step_loss_weights is not None:
                raise ValueError("tower_loss and step_loss_weights do not combine (the tower term on per-step rows "
                                 "is not built)")
            if not hasattr(self.engine, "loss_tower"):
                raise ValueError("tower_loss needs an engine with loss_tower(logits, target, batch, tower_targets, "
                                 "weights, norm, norm_t, tower_loss, node_loss) (the engine protocol: "
                                 "spwgnn_amd/step.py)")
            if hasattr(self.engine, "set_tower_loss"):
                self.engine.set_tower_loss(self.tower_loss, self.node_loss, mp_steps)
        self.dropedge = E.check_dropedge(dropedge)
        self.dropedge_symmetric, self.dropedge_rescale = bool(dropedge_symmetric), bool(dropedge_rescale)
        self.dropedge_per_step = bool(dropedge_per_step)
        if self.dropedge > 0:
            if not E.gates_supported(math):
                raise ValueError(f"dropedge needs a math that takes relation gates (spwgnn_gates_supported: x6, x3 and "
                                 f"h3 do, {math} does not)")
            if self.step_loss_weights is not None:
                raise ValueError("dropedge and step_loss_weights do not combine (gated per-step logits are not built)")
            if not hasattr(self.engine, "dropedge_gates"):
                raise ValueError("dropedge needs an engine with dropedge_gates(batch, run, rate, symmetric, rescale, "
                                 "base) and gates= on forward / backward (the engine protocol: spwgnn_amd/step.py)")
        self._rel = None          # the current step's relation weights, one per micro-batch (step(relation_weights=))
        self.clip_stats = None    # the last clipped step's [norm, scale, skipped, clipped] (device tensor)
        self.m = torch.zeros_like(params)
        self.v = torch.zeros_like(params)
        self.mp_steps, self.dropout, self.seed, self.math = mp_steps, dropout, seed, math
        self.iterations = 0
        self.group = group
        self.distributed = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(group) if self.distributed else 1
        self.rank = dist.get_rank(group) if self.distributed else 0
        self.prof_kernel = 0
        self.prof_events = None
        # gradient all-reduce: `buckets` contiguous 64-float-aligned pieces of the flat gradient, each
        # its own async all-reduce (all in flight together, waited before Adam); ar_events: an optional
        # (start, end) torch.cuda.Event pair recorded around the all-reduce (bench.py's allreduce_ms)
        self.buckets = max(1, int(buckets))
        self.ar_events = None
        # overlap (N > 1, an engine with early_event): the backward records an event once the gradients
        # of the flat range [rmp.1.kernel, end) are final (spwgnn_run.grads_early_event); that range is
        # all-reduced on a side stream while dA, the encoder backward and the encoder-side gradients run
        # (SURVEY §8e), the rest after the backward. ar_early_events: an optional (start, end) event
        # pair recorded on the side stream around the early all-reduce (bench.py's rehearsal trace)
        self.overlap = overlap
        self.ar_early_events = None
        self._side = None
        self._early_lo = next(off for name, off, _ in P.layout() if name == "rmp.1.kernel")
        self._ctr = None          # replayed steps' device counters (replay_body)
        self._ctr_at = 0          # the host iteration count the device step word holds
        self._w3 = {}             # (count, 1, 1) fp64 weights of a micro-batch's [loss, correct, n]
        self._acc = None          # the micro-batches' gradient sum (the engine reuses its own buffer)

    lr, b1, b2, eps, l2 = (delegated("opt", k) for k in ("lr", "beta1", "beta2", "eps", "l2"))
    clipnorm, clipvalue, decay, skip_nonfinite = (delegated("opt", k) for k in
                                                  ("clipnorm", "clipvalue", "decay", "skip_nonfinite"))

    def _adam(self, acc):
        """The update of step `iterations` (already advanced) from the reduced gradient `acc`: after the
        all-reduce, so every rank clips by the same norm and takes the same skip decision."""
        o = self.opt
        if not o.clip_on():
            self.engine.adam(self.params, acc, self.m, self.v, self.iterations, o.lr, o.beta1, o.beta2, o.eps, o.l2, 1.0)
            return
        lr = E.adam_lr_decayed(o.lr, o.decay, self.iterations - 1) if o.decay else o.lr
        self.clip_stats = self.engine.adam_clipped(self.params, acc, self.m, self.v, self.iterations, lr, o.beta1,
                                                   o.beta2, o.eps, o.l2, 1.0, o.clipnorm, o.clipvalue, o.skip_nonfinite)

    def _early(self, run):
        """Overlapped steps: the engine's early-gradient event, handed to the backward through `run`."""
        if not self._split():
            return None
        ev = self.engine.early_event()
        run.grads_early_event = ev
        return ev

    def run_config(self, micro: int = 0) -> E.RunConfig:
        # distinct dropout keys per step, per rank and per micro-batch (different towers)
        key = dropout_key(self.seed, self.iterations, self.rank, micro)
        return E.RunConfig(self.mp_steps, training=True, dropout=self.dropout, seed=key, math=self.math,
                           prof_kernel=self.prof_kernel, prof_events=self.prof_events)

    def _sync_counters(self):
        """Device step word and lr table ← the host's iteration count and (lr, β1, β2, decay), when they
        differ (a step() or an lr / decay change since the last replay)."""
        if self._ctr is None:
            self._ctr = DeviceCounters(self.params.device, 0, self.iterations, self.lr, self.b1, self.b2,
                                       decay=self.decay)
        elif (self._ctr_at != self.iterations or self._ctr.hyper != (float(self.lr), float(self.b1), float(self.b2))
              or self._ctr.decay != float(self.decay)):
            self._ctr.set(step=self.iterations, lr=self.lr, beta1=self.b1, beta2=self.b2, decay=self.decay)
        self._ctr_at = self.iterations

    def replay_body(self, n_nodes: int, n_global: Optional[int] = None, weighted: bool = False):
        """The launches of one single-batch `step` for spwgnn_amd.replay.ReplayStep (hipGraph
        replay): the dropout key and Adam step are device words (spwgnn_step_advance in the
        Trainer's splitmix key mode, spwgnn_adam_dev), so every replay is the next optimizer step
        with the masks `step` would draw. Single process only (no all-reduce inside a graph).

        Run each step through `replay_step(rs, plan, target)`: a replay advances the device words
        only, and replay_step keeps `iterations` (the host counter `step` reads) in step with them.

        `weighted`: a body for ReplayStep(..., weighted=True) — it takes the step's per-node loss
        weights and their divisor (the batch's own non-zero count, a device float) as `weights=` and
        `norm=`; `replay_step(rs, plan, target, weights)` uploads them. Whole-batch steps only (no
        n_global: the gradient scale nnz / norm_global would be a per-step host value)."""
        if self.world > 1:
            raise ValueError("replayed steps are single-process; DP steps use step()")
        if not isinstance(self.engine, HipEngine):
            raise ValueError("replayed steps need the HIP engine")
        self._sync_counters()
        if weighted and n_global not in (None, n_nodes):
            raise ValueError("weighted replayed steps cover the whole batch (no n_global)")
        if self.tower_loss > 0 and (weighted or n_global not in (None, n_nodes)):
            # the tower divisor of a weighted step is a per-step count, and a shard's needs the global one
            raise ValueError("replayed tower-loss steps are unweighted whole-batch steps with derived tower targets; "
                             "use step() otherwise")
        E.check_clip_options(self.clipnorm, self.clipvalue, self.decay)
        if self.opt.clip_on():
            self.clip_stats = self.opt.clip_scratch().out4

        def make_run(**kw):
            return E.RunConfig(self.mp_steps, training=True, dropout=self.dropout, math=self.math, **kw)
        return step_body(self.params, torch.empty_like(self.params), self.m, self.v, self.engine.path, self.opt,
                         self._ctr, make_run, _lib.STEP_KEY_SPLITMIX, self.seed, self.rank,
                         grad_scale=n_nodes / (n_global or n_nodes), dropedge=self._dropedge_options())

    def bucket_bounds(self, n: int):
        """[(start, end)) of the gradient buckets over a flat buffer of n floats (64-float aligned)."""
        k = min(self.buckets, max(1, n // 64))
        cuts = [0] + [min(n, (n * i // k + 63) // 64 * 64) for i in range(1, k)] + [n]
        return [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]

    def allreduce(self, acc: torch.Tensor):
        """Σ over ranks of the node-weighted flat gradient (RCCL over xGMI with backend nccl). With
        buckets > 1 the pieces are issued as async all-reduces, all in flight before the first wait."""
        ev = self.ar_events
        if ev is not None:
            ev[0].record()
        if self.buckets == 1:
            dist.all_reduce(acc, op=dist.ReduceOp.SUM, group=self.group)
        else:
            works = [dist.all_reduce(acc[a:b], op=dist.ReduceOp.SUM, group=self.group, async_op=True)
                     for a, b in self.bucket_bounds(acc.numel())]
            for w in works:
                w.wait()
        if ev is not None:
            ev[1].record()

    def _split(self) -> bool:
        # any process group (a one-rank group included: its all-reduce is the identity, the choreography
        # of events, side stream and collectives is the same as at N > 1)
        return self.distributed and self.overlap and hasattr(self.engine, "early_event")

    def _combine(self, acc, g, w, sl, first):
        """acc[sl] ← w·g[sl] (first micro-batch) or acc[sl] + w·g[sl]; acc may be g itself; sl None: all of it."""
        a, b = (acc, g) if sl is None else (acc[sl], g[sl])
        if not first:
            a.add_(b, alpha=w)
        elif acc is not g:
            torch.mul(b, w, out=a)
        elif w != 1.0:
            a.mul_(w)

    def reduce_split(self, acc, g, w, first, ev):
        """The last backward's gradient `g` folded into `acc` (weight w) and the sum over ranks, in two
        pieces: the early range [rmp.1.kernel, end) on a side stream that waits for `ev` (the library
        records it mid-backward), issued before the late range [0, rmp.1.kernel) on the step's stream.
        Elementwise the same arithmetic as `allreduce` after the whole backward."""
        lo = self._early_lo
        early, late = slice(lo, acc.numel()), slice(0, lo)
        cuda = acc.is_cuda
        cur = torch.cuda.current_stream(acc.device) if cuda else None
        if cuda:
            if self._side is None:
                # high priority: a stream of its own on the device's hardware queues, so its wait on the
                # mid-backward event is not queued behind the step stream's remaining kernels
                self._side = torch.cuda.Stream(acc.device, priority=-1)
            self._side.wait_event(ev)
            ctx = torch.cuda.stream(self._side)
        else:
            import contextlib
            ctx = contextlib.nullcontext()
        with ctx:
            if self.ar_early_events is not None:
                self.ar_early_events[0].record()
            self._combine(acc, g, w, early, first)
            work = dist.all_reduce(acc[early], op=dist.ReduceOp.SUM, group=self.group, async_op=True)
            if self.ar_early_events is not None:   # timing: the side stream waits for the early piece
                work.wait()
                self.ar_early_events[1].record()
        self._combine(acc, g, w, late, first)
        if self.ar_events is not None:
            self.ar_events[0].record()
        dist.all_reduce(acc[late], op=dist.ReduceOp.SUM, group=self.group)
        work.wait()   # the step's stream (CUDA) / the host (CPU tensors) waits for the early piece
        if cuda:
            cur.wait_stream(self._side)
        if self.ar_events is not None:
            self.ar_events[1].record()

    def replay_step(self, rs, plan, target, weights=None):
        """One replayed optimizer step (rs: a ReplayStep/ReplayCache over `replay_body`): the
        device words are first brought to the host's counters (a `step()` may have run in
        between), the step runs, and the host counter advances with the device one. `weights`: the
        per-node loss weights of a weighted step (host array, one per node)."""
        self._sync_counters()
        out = rs(plan, target) if weights is None else rs(plan, target, weights)
        self.iterations += 1
        self._ctr_at = self.iterations
        return out

    def _count_global(self, n_local: float) -> int:
        """Σ over ranks of a per-rank count (one 8-byte all-reduce)."""
        if self.world <= 1:
            return int(n_local)
        t = torch.tensor([float(n_local)], dtype=torch.float64,
                         device=self.params.device if dist.get_backend(self.group) != "gloo" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return int(t.item())

    def _sum_ranks(self, t: torch.Tensor) -> torch.Tensor:
        """t ← Σ over ranks of t, in place (one all-reduce; the identity without a process group)."""
        if not self.distributed:
            return t
        if t.is_cuda and dist.get_backend(self.group) == "gloo":
            h = t.cpu()
            dist.all_reduce(h, op=dist.ReduceOp.SUM, group=self.group)
            return t.copy_(h)
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return t

    def evaluate(self, batches, targets, weights=None, threshold: float = 0.5, *, tower_targets=None) -> dict:
        """The model's metrics over the GLOBAL evaluation set, of which `batches` / `targets` (one or a list:
        micro-batches) are this rank's shard: an inference run (no dropout, nothing stored, no step taken)
        whose integer tables (engine.EvalTables) are filled on the device and summed over the ranks with one
        all-reduce; the fp64 pair [Σ loss·n, n] takes a second. Returns metrics.summarize of the summed tables
        plus ``loss`` (the node-weighted mean of the micro-batch losses) — the same dict on every rank.

        `weights` (one per micro-batch, a weight per node): the weighted loss of `step`, each micro-batch's
        divided by its own non-zero count, which is also its n in the pair; a zero weight masks its node out
        of every count. `threshold`: a node is predicted stable when its probability exceeds it. With
        step_loss_weights the engine's (mp_steps, n) rows are all scored: the dict describes the last step,
        ``loss`` is Σ_s λ_s·loss_s and ``steps`` lists every step's summary. The engine needs
        `eval_metrics(logits, target, tables, batch, weights, threshold)`.

        With tower_loss > 0 the loss launch is the tower loss's (no gradient written): ``loss`` is
        node_loss·L_node + tower_loss·L_tower over the global set, and the dict gains ``tower_loss`` (L_tower, the
        mean over the counted towers) and ``tower_accuracy`` (at 0.5, against `tower_targets` — one tensor per
        micro-batch, plan order — or the derived labels; it replaces the table's, which is the derived one at
        `threshold`). A `targets` entry of None (tower-only labels) drops that micro-batch's node term and, as
        the tables need node targets, the summary: the dict then holds the three loss entries only."""
        from . import metrics as M
        batches, targets, weights = _micro_batches(batches, targets, weights)
        if self.tower_loss > 0:
            return self._evaluate_tower(batches, targets, weights, E.check_threshold(threshold), tower_targets)
        if tower_targets is not None:
            raise ValueError("tower_targets need Trainer(tower_loss > 0)")
        if not hasattr(self.engine, "eval_metrics"):
            raise ValueError("evaluate needs an engine with eval_metrics(logits, target, tables, batch, weights, threshold) "
                             "(the engine protocol: spwgnn_amd/step.py)")
        tau = E.check_threshold(threshold)
        rows = self.mp_steps if self.step_loss_weights is not None else 1
        run = E.RunConfig(self.mp_steps, training=False, dropout=0.0, math=self.math)
        tables = E.EvalTables(self.params.device, rows=rows)
        sums = torch.zeros(2, dtype=torch.float64, device=self.params.device)   # Σ loss·n, n
        for i, (b, tg) in enumerate(zip(batches, targets)):
            z = self.engine.forward(self.params, b, run)
            if weights is None:
                wt = None
                out3, _ = self.engine.loss(z, tg)
            else:
                wt = weights[i]
                out3, _ = self.engine.loss_weighted(z, tg, wt, max(_nonzero(wt), 1))
            n_i = out3[2].to(sums)           # the nodes that count: all of them, or those with w ≠ 0
            sums += torch.stack([out3[0].to(sums) * n_i, n_i])   # before the engine reuses its out3 buffer
            self.engine.eval_metrics(z, tg, tables, b, wt, tau)
        self._sum_ranks(tables.flat)
        self._sum_ranks(sums)
        counts = tables.cpu()
        loss_n, n = sums.tolist()
        out = dict(M.summarize(counts), loss=loss_n / n if n else float("nan"))
        if rows > 1:
            out["steps"] = [M.summarize(counts, row=s) for s in range(rows)]
        return out

    def _evaluate_tower(self, batches, targets, weights, tau, tower_targets) -> dict:
        """`evaluate` of a tower-loss trainer: per micro-batch the inference forward, the tower loss with the
        micro-batch's own divisors (no dlogits) and the metrics launch; Σ L_node_i·k_i, Σ L_tower_i·t_i and the
        counts are summed over the ranks with the tables."""
        from . import metrics as M
        tower_targets = self._tower_lists(batches, tower_targets)
        if not hasattr(self.engine, "eval_metrics"):
            raise ValueError("evaluate needs an engine with eval_metrics(logits, target, tables, batch, weights, threshold) "
                             "(the engine protocol: spwgnn_amd/step.py)")
        run = E.RunConfig(self.mp_steps, training=False, dropout=0.0, math=self.math)
        tables = E.EvalTables(self.params.device)
        sums = torch.zeros(7, dtype=torch.float64, device=self.params.device)   # the six parts' sums, micro-batches without node targets
        for i, (b, tg) in enumerate(zip(batches, targets)):
            wt = None if weights is None else weights[i]
            k, t = (b.n_nodes, E.counted_towers(b)) if wt is None else E.counted_nodes_towers(b, torch.as_tensor(wt))
            z = self.engine.forward(self.params, b, run)
            out6, _ = self.engine.loss_tower(z, tg, b, None if tower_targets is None else tower_targets[i], wt,
                                             None if wt is None else max(k, 1), max(t, 1), self.tower_loss,
                                             self.node_loss if tg is not None else 0.0, want_dlogits=False)
            sums[:6] += out6.to(sums) * self._weights6(k, max(t, 1), out6).to(sums)
            if tg is None:
                sums[6] += 1.0
            else:
                self.engine.eval_metrics(z, tg, tables, b, wt, tau)
        self._sum_ranks(tables.flat)
        self._sum_ranks(sums)
        lp = self._tower_parts(sums[:6]).tolist()
        out = dict(M.summarize(tables.cpu())) if sums[6].item() == 0 else {}
        out.update(loss=self.node_loss * lp[0] + self.tower_loss * lp[3], tower_loss=lp[3],
                   tower_accuracy=lp[4] / lp[5] if lp[5] else float("nan"))
        return out

    def _dropedge_options(self):
        """(rate, symmetric, rescale) of a DropEdge trainer — with a fourth entry True when the mask is drawn per
        propagation step — None without it."""
        if not self.dropedge > 0:
            return None
        return (self.dropedge, self.dropedge_symmetric, self.dropedge_rescale) + ((True,) if self.dropedge_per_step else ())

    def _gates(self, i: int, b, run):
        """Micro-batch i's relation gates: its relation weights (a slot tensor, or what `TowerBatch.edge_gates`
        takes) with the step's DropEdge mask multiplied in; None without either."""
        base = None if self._rel is None else self._rel[i]
        if base is not None and not (isinstance(base, torch.Tensor) and tuple(base.shape) == (32 * b.n_eblocks,)):
            base = b.edge_gates(base)
        if self.dropedge > 0:
            kw = {"per_step": True} if self.dropedge_per_step else {}   # the shared mask: the call of before
            return self.engine.dropedge_gates(b, run, self.dropedge, symmetric=self.dropedge_symmetric,
                                              rescale=self.dropedge_rescale, base=base, **kw)
        return base

    def _accumulate_and_update(self, batches, loss_of):
        """The micro-batch loop of `step`: forward, `loss_of(i, logits, batch) -> (dlogits, gradient weight)`,
        backward, the weighted gradient sum (the last one in two pieces when overlapped), the all-reduce and
        the Adam update."""
        single = len(batches) == 1
        acc = None
        for i, b in enumerate(batches):
            run = self.run_config(micro=i)
            gates = self._gates(i, b, run)
            kw = {} if gates is None else {"gates": gates}   # an ungated step: the calls of before
            z = self.engine.forward(self.params, b, run, **kw)
            dz, w = loss_of(i, z, b)
            ev = self._early(run) if i == len(batches) - 1 else None
            g = self.engine.backward(self.params, b, run, dz, **kw)
            if acc is None:
                # one batch: the engine's own buffer (HipEngine.grads), scaled in place; micro-batches: the
                # engine writes every backward into that buffer, so the sum lives in the Trainer's accumulator
                acc = g if single else self._accumulator(g)
            if ev is not None:   # the last micro-batch: accumulate and reduce in two pieces
                self.reduce_split(acc, g, w, i == 0, ev)
            else:
                self._combine(acc, g, w, None, i == 0)
        if self.distributed and not self._split():   # any process group (one rank: the identity, through the collective)
            self.allreduce(acc)
        self.iterations += 1
        self._adam(acc)

    def _tower_lists(self, batches, tower_targets):
        if tower_targets is not None:
            tower_targets = tower_targets if isinstance(tower_targets, (list, tuple)) else [tower_targets]
            if len(tower_targets) != len(batches):
                raise ValueError("one tower target tensor per micro-batch")
        return tower_targets

    def _tower_parts(self, parts):
        """The shard's six numbers from Σ L_node_i·k_i, Σ L_tower_i·(its divisor) and the counts (fp64)."""
        return torch.stack([parts[0] / parts[2].clamp(min=1.0), parts[1], parts[2],
                            parts[3] / parts[5].clamp(min=1.0), parts[4], parts[5]])

    def _tower_out3(self, lp):
        """[node_loss·L_node + tower_loss·L_tower, node correct, node count] in fp64 with the coefficients as the
        fp32 values the loss launch takes: for one whole batch the bits of its own out3."""
        lp = lp.double()
        a, m = (float(torch.tensor(c, dtype=torch.float32)) for c in (self.node_loss, self.tower_loss))
        return torch.stack([a * lp[0] + m * lp[3], lp[1], lp[2]]).float()

    def _step_tower(self, batches, targets, weights, counts, towers, total, tower_targets, towers_global):
        """`step` with the tower term (tower_loss > 0). The node term of micro-batch i keeps its own divisor
        k_i and enters with node_loss·k_i / total, as its gradient does without the tower term; tower counts
        do not scale with node counts for ragged towers, so the tower term takes the GLOBAL divisor — the
        counted towers of the whole batch, `towers_global` or all-reduced — inside the loss, and the
        gradients are summed with weight 1."""
        tower_targets = self._tower_lists(batches, tower_targets)
        t_total = max(int(towers_global if towers_global is not None else self._count_global(sum(towers))), 1)
        whole = len(batches) == 1 and self.world == 1 and towers_global is None
        acc = [None]

        def loss_of(i, z, b):
            tg, k = targets[i], counts[i]
            alpha = self.node_loss * (k / total) if tg is not None else 0.0
            out6, dz = self.engine.loss_tower(z, tg, b, None if tower_targets is None else tower_targets[i],
                                              None if weights is None else weights[i],
                                              None if weights is None else max(k, 1), t_total, self.tower_loss, alpha)
            # the engine's out6 is one persistent tensor: Σ L_node_i·k_i, Σ L_tower_i·t_total and the counts, in fp64
            # (one batch that is the whole global batch: out6 itself — k / k and t_total / t_total change nothing)
            if whole:
                acc[0] = out6.clone()
            else:
                p = out6.double() * self._weights6(k, t_total, out6)
                acc[0] = p if acc[0] is None else acc[0] + p
            return dz, 1.0

        self._accumulate_and_update(batches, loss_of)
        lp = acc[0] if whole else self._tower_parts(acc[0])
        self.loss_parts = lp.float()
        return self._tower_out3(lp)

    def step(self, batch, target, n_global: Optional[int] = None, weights=None, norm_global: Optional[int] = None, *,
             tower_targets=None, towers_global: Optional[int] = None, relation_weights=None):
        """One optimizer step. `batch`/`target` may be lists (micro-batches of this rank's shard);
        `n_global` = nodes in the whole global batch (all ranks, all micro-batches). Returns one
        [loss, correct, n] device tensor for this rank's shard: the node-weighted mean BCE over its
        micro-batches, the binary_accuracy numerator and the node count.

        `weights` (one tensor per micro-batch, a weight per node in the targets' order): the weighted
        loss of engine.bce — Σ w·bce over the global batch / `norm_global`, the number of nodes with
        w ≠ 0 in the whole global batch (all-reduced when None, as n_global is; at least 1). Zero
        weights mask their nodes. Counting each micro-batch's non-zero weights is one host sync. The
        result is then [loss over this rank's counted nodes, correct among them, their number]. The
        engine needs `loss_weighted(logits, target, weights, norm)`.

        With tower_loss > 0 the objective is node_loss·L_node + tower_loss·L_tower.
        `tower_targets`: one (n_towers,) 0/1 tensor per micro-batch in the plan's tower order, or None = a
        tower's label is "every counted node target is 1". A `target` of None (tower-only labels) drops the
        node term of that micro-batch. `towers_global`: the counted towers of the whole global batch
        (all-reduced when None). The result is [node_loss·L_node + tower_loss·L_tower, node correct, node
        count] of this rank's shard, and `loss_parts` holds its [L_node, node correct, node count, L_tower,
        towers correct, towers counted]. The engine needs `loss_tower` (spwgnn_amd/step.py).

        `relation_weights` (one per micro-batch): relation gates of the step (engine.forward's ``gates=``) — a
        (32·n_eblocks,) tensor in the plan's edge-slot order, or what `TowerBatch.edge_gates` takes (one value per
        active relation in the input's edge order, or (B, N, N)). With Trainer(dropedge=) the step's mask is
        multiplied into them. Not differentiated here (`GraphNetwork` carries the chain rule to a weights leaf)."""
        batches, targets, weights = _micro_batches(batch, target, weights)
        if relation_weights is not None:
            relation_weights = relation_weights if isinstance(relation_weights, (list, tuple)) else [relation_weights]
            if len(relation_weights) != len(batches):
                raise ValueError("one relation weight tensor per micro-batch")
            if self.step_loss_weights is not None:
                raise ValueError("relation_weights and step_loss_weights do not combine (gated per-step logits are "
                                 "not built)")
        self._rel = relation_weights
        try:
            return self._step(batches, targets, weights, n_global, norm_global, tower_targets, towers_global)
        finally:
            self._rel = None

    def _step(self, batches, targets, weights, n_global, norm_global, tower_targets, towers_global):
        if self.tower_loss <= 0 and (tower_targets is not None or towers_global is not None):
            raise ValueError("tower_targets / towers_global need Trainer(tower_loss > 0)")
        # micro-batch i counts k_i nodes — all of them, or those with w ≠ 0 — of `total` in the global batch:
        # its loss is the mean over its k_i, its gradient enters the sum scaled by k_i / total
        if weights is None:
            if norm_global is not None:
                raise ValueError("norm_global goes with weights")
            counts = [b.n_nodes for b in batches]
            total = n_global if n_global is not None else self._count_global(sum(counts))
        else:
            if self.tower_loss > 0:   # both counts of every micro-batch in one host sync each
                both = [E.counted_nodes_towers(bt, torch.as_tensor(w)) for bt, w in zip(batches, weights)]
                counts, towers = [c[0] for c in both], [c[1] for c in both]
            else:
                counts = [_nonzero(w) for w in weights]
            total = max(int(norm_global if norm_global is not None else self._count_global(sum(counts))), 1)
        if self.tower_loss > 0:
            if weights is None:
                towers = [E.counted_towers(bt) for bt in batches]
            return self._step_tower(batches, targets, weights, counts, towers, total, tower_targets, towers_global)
        single = len(batches) == 1
        keep = {}

        def loss_of(i, z, b):
            tg, k = targets[i], counts[i]
            if weights is None:
                out3, dz = self.engine.loss(z, tg)
            else:
                out3, dz = self.engine.loss_weighted(z, tg, weights[i], max(k, 1))
            # the engine's out3 is one persistent tensor: kept before the next call reuses it — one batch's as
            # the engine computed it (one copy), micro-batches' as Σ loss_i·k_i, Σ correct_i, Σ n_i in fp64
            if single and weights is None:
                keep["res"] = out3.clone()
            else:
                w3 = out3.double() * self._weights3(k, out3)
                keep["tot3"] = w3 if "tot3" not in keep else keep["tot3"] + w3
            return dz, k / total

        self._accumulate_and_update(batches, loss_of)
        if "tot3" not in keep:
            res = keep["res"]
            return res.float() if res.dtype != torch.float32 else res
        # mean loss over this rank's counted nodes, total correct, total counted (device, fp32)
        tot3 = keep["tot3"]
        n = tot3[2] if weights is None else tot3[2].clamp(min=1.0)
        return torch.stack([tot3[0] / n, tot3[1], tot3[2]]).float()

    def _weights3(self, k: int, out3: torch.Tensor) -> torch.Tensor:
        """The cached fp64 [k, 1, 1] on out3's device (most recent last; ragged micro-batches keep 16)."""
        key = (k, out3.device)
        wt = self._w3.pop(key, None)
        if wt is None:
            wt = out3.new_tensor([float(k), 1.0, 1.0], dtype=torch.float64)
        self._w3[key] = wt
        while len(self._w3) > 16:
            self._w3.pop(next(iter(self._w3)))
        return wt

    def _weights6(self, k: int, towers: int, out6: torch.Tensor) -> torch.Tensor:
        """The cached fp64 [k, 1, 1, towers, 1, 1] on out6's device (`_weights3`'s cache and its bound)."""
        key = (k, towers, out6.device)
        wt = self._w3.pop(key, None)
        if wt is None:
            wt = out6.new_tensor([float(k), 1.0, 1.0, float(towers), 1.0, 1.0], dtype=torch.float64)
        self._w3[key] = wt
        while len(self._w3) > 16:
            self._w3.pop(next(iter(self._w3)))
        return wt

    def _accumulator(self, g: torch.Tensor) -> torch.Tensor:
        if self._acc is None or self._acc.shape != g.shape or self._acc.device != g.device:
            self._acc = torch.empty_like(g)
        return self._acc
