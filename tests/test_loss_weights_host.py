"""CPU: the host side of per-node loss weights (spwgnn_bce_weighted, spwgnn_bce_backward_weighted, added
within ABI 8) — exports, the argument statuses that come back before any device work, keras_api.node_weights
against a literal fp64 restatement of Keras 2.x's weighted_masked_objective, and the data-parallel Trainer
with weights under gloo (the oracle engine) against the single-process step on the full batch.
Reference: model.fit's sample_weight / class_weight (src/main.py:92-98)."""
import ctypes as C
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import model as O
from spwgnn_amd import _lib, data as D, params as P
from spwgnn_amd.batch import TowerBatch
from spwgnn_amd.keras_api import node_weights
from spwgnn_amd.trainer import Trainer

WEIGHT_VALUES = np.array([0.0, 0.5, 1.0, 2.5])


def draw_weights(rng, shape):
    """Weights from {0, 0.5, 1, 2.5}, about 30 % zeros."""
    return rng.choice(WEIGHT_VALUES, size=shape, p=[0.3, 0.25, 0.25, 0.2])


def test_exports_and_struct_size():
    lib = _lib.lib()
    assert hasattr(lib, "spwgnn_bce_weighted") and hasattr(lib, "spwgnn_bce_backward_weighted")
    assert lib.spwgnn_struct_size(4) == C.sizeof(_lib.LossWeightsC) == 24
    assert lib.spwgnn_struct_size(5) == -1
    assert lib.spwgnn_version() == 8 == _lib.ABI_VERSION


def _structs():
    """A well-formed batch / run pair whose pointers are never followed (tests/test_input_grad_host.py)."""
    b = _lib.BatchC()
    b.n_towers, b.n_nodes, b.n_wtiles, b.n_eblocks, b.nw_max, b.flags = 2, 12, 2, 2, 6, 0
    fake = 0x1000
    b.pos = b.node_tower = b.node_local = b.wtile = b.edge_src = b.edge_dst = b.blk_csr = fake
    r = _lib.RunC()
    r.mp_steps, r.training, r.dropout, r.math = 3, 1, 0.0, _lib.MATH_X6
    return b, r, fake


def _lw(w, norm_dev, norm):
    lw = _lib.LossWeightsC()
    lw.w, lw.norm_dev, lw.norm = w, norm_dev, norm
    return lw


def test_statuses_without_a_device():
    lib = _lib.lib()
    b, r, fake = _structs()
    need = lib.spwgnn_workspace_bytes(b.n_nodes, b.n_eblocks, r.mp_steps, 1)

    def bwd(lw, n=b.n_nodes, w3=None, t3=None, nbytes=need):
        return lib.spwgnn_bce_backward_weighted(fake, C.byref(b), C.byref(r), fake, nbytes, fake, fake, n, fake, fake, fake,
                                                w3, t3, fake, None, C.byref(lw) if lw is not None else None, None)

    def bce(lw, w3=None, t3=None):
        return lib.spwgnn_bce_weighted(fake, fake, 12, C.byref(lw) if lw is not None else None, fake, fake, fake, w3, t3,
                                       None)

    good = _lw(fake, None, 12.0)
    for call in (bwd, bce):
        assert call(None) == _lib.E_ARG                          # null lw
        assert call(_lw(None, None, 12.0)) == _lib.E_ARG         # null w
        assert call(_lw(fake, None, 0.0)) == _lib.E_ARG          # norm by value must be > 0
        assert call(_lw(fake, None, -1.0)) == _lib.E_ARG
        assert call(good, w3=fake) == _lib.E_ARG                 # weights3 / total3 go together
        assert call(good, t3=fake) == _lib.E_ARG
    assert bwd(good, n=11) == _lib.E_ARG and bwd(good, n=13) == _lib.E_ARG   # n != n_nodes
    assert bwd(_lw(fake, fake, 0.0), n=11) == _lib.E_ARG         # ... with a device norm too
    # the checks above are the only thing in the way: the same well-formed call gets as far as the
    # workspace size (still before any device work)
    assert bwd(good, nbytes=need - 1) == _lib.E_WORKSPACE
    assert bwd(_lw(fake, fake, 0.0), nbytes=need - 1) == _lib.E_WORKSPACE    # norm_dev set: norm unread


# ---------------------------------------------------------------- node_weights against Keras 2.x
def _keras_weighted_masked_objective(y_true, logits, weights):
    """Keras 2.x training_utils.weighted_masked_objective around binary_crossentropy, literally, in fp64
    (no mask): score per (B, N); reduced to the weights' rank; times the weights; divided by the mean of
    (weights != 0); the mean of that."""
    p = np.clip(1.0 / (1.0 + np.exp(-logits)), O.KERAS_EPS, 1.0 - O.KERAS_EPS)        # K.binary_crossentropy's clip
    bce = -(y_true * np.log(p) + (1.0 - y_true) * np.log(1.0 - p))                     # (B, N, 1)
    score = bce.mean(axis=-1)                                                          # the loss fn: mean over the last axis
    weights = np.asarray(weights, np.float64)
    score = score.mean(axis=tuple(range(weights.ndim, score.ndim))) if weights.ndim < score.ndim else score
    score = score * weights
    score = score / np.mean((weights != 0).astype(np.float64))
    return float(score.mean())


def _per_node(y_true, logits, W):
    """The engine's formula: Σ w·bce / #{w != 0} with the expanded per-node weights."""
    loss, _ = _weighted_bce_grad(logits.reshape(-1), y_true.reshape(-1), W.reshape(-1), max(np.count_nonzero(W), 1))
    return loss


def _weighted_bce_grad(z64, t, w, norm):
    z64, t, w = (np.asarray(a, np.float64) for a in (z64, t, w))
    z = np.clip(z64, -O.LOGIT_CLIP, O.LOGIT_CLIP)
    per = np.maximum(z, 0) - z * t + np.log1p(np.exp(-np.abs(z)))
    on = w != 0
    loss = float(np.where(on, w * per, 0.0).sum() / norm)
    g = np.where(on & (np.abs(z64) < O.LOGIT_CLIP), w * (1.0 / (1.0 + np.exp(-z64)) - t) / norm, 0.0)
    return loss, g


def test_node_weights_equal_keras_weighted_masked_objective():
    B, N = 5, 4
    rng = np.random.default_rng(0)
    y = rng.integers(0, 2, (B, N, 1)).astype(np.float64)
    z = rng.normal(scale=2.0, size=(B, N, 1))
    sw_b = draw_weights(rng, B)
    sw_b[0], sw_b[1] = 0.0, 2.5          # at least one masked and one counted tower
    sw_bn = draw_weights(rng, (B, N))
    sw_bn[0, 0], sw_bn[0, 1] = 0.0, 0.5
    cw = {0: 2.0, 1: 0.5}
    cw_bn = np.where(y[..., 0] == 1, cw[1], cw[0])
    cases = [
        (dict(sample_weight=sw_b), sw_b),                               # Keras: per-sample weights
        (dict(sample_weight=sw_bn), sw_bn),                             # sample_weight_mode='temporal'
        (dict(class_weight=cw), cw_bn),                                 # the extension, as temporal weights
        (dict(sample_weight=sw_b, class_weight=cw), sw_b[:, None] * cw_bn),
        (dict(sample_weight=sw_bn, class_weight=cw), sw_bn * cw_bn),
    ]
    for kw, keras_w in cases:
        W = node_weights(y, **kw)
        assert W.shape == (B, N) and W.dtype == np.float32
        expanded = np.broadcast_to(keras_w[:, None] if keras_w.ndim == 1 else keras_w, (B, N))
        assert np.array_equal(W, expanded.astype(np.float32)), kw      # every value is exact in fp32
        ref = _keras_weighted_masked_objective(y, z, keras_w)
        assert abs(_per_node(y, z, W) - ref) <= 1e-12, kw
    assert np.array_equal(node_weights(y[..., 0]), np.ones((B, N), np.float32))   # (B, N) targets, no weights
    for bad in (dict(sample_weight=np.ones(B + 1)), dict(sample_weight=np.ones((B, N + 1))), dict(class_weight={1: 2.0})):
        try:
            node_weights(y, **bad)
        except ValueError:
            continue
        raise AssertionError(bad)


# ---------------------------------------------------------------- gloo data parallel
class WeightedOracleEngine:
    """fp64 torch-CPU oracle behind the Trainer's engine interface, with `loss_weighted` (tests only)."""

    def __init__(self):
        self._layout = P.layout()

    def _params(self, flat):
        f = flat.detach().to(torch.float64)
        return {n: f[o:o + int(np.prod(s))].reshape(s).clone().requires_grad_(True) for n, o, s in self._layout}

    def forward(self, flat, batch, run):
        self.p = self._params(flat)
        pos = batch.pos[:, :3].to(torch.float64)
        src = torch.as_tensor(batch.src, dtype=torch.long)
        dst = torch.as_tensor(batch.dst, dtype=torch.long)
        prop = torch.zeros(batch.n_nodes, 100, dtype=torch.float64)
        self.z = O.forward_gather(self.p, pos, src, dst, prop, run.mp_steps)
        return self.z.detach()

    def loss(self, logits, target):
        raise AssertionError("a weighted step must call loss_weighted")

    def loss_weighted(self, logits, target, weights, norm):
        loss, g = _weighted_bce_grad(logits.numpy(), target.numpy(), weights.numpy(), norm)
        return torch.tensor([loss, 0.0, float(np.count_nonzero(weights.numpy()))]), torch.tensor(g)

    def backward(self, flat, batch, run, dlogits):
        self.z.backward(dlogits.to(torch.float64))
        g = torch.zeros_like(flat, dtype=torch.float64)
        for n, o, s in self._layout:
            g[o:o + int(np.prod(s))] = self.p[n].grad.reshape(-1)
        return g

    def adam(self, params, grads, m, v, step, lr, b1, b2, eps, l2, gscale):
        g = gscale * grads + 2 * l2 * params.to(torch.float64)
        m.mul_(b1).add_((1 - b1) * g)
        v.mul_(b2).add_((1 - b2) * g * g)
        lr_t = lr * np.sqrt(1 - b2 ** step) / (1 - b1 ** step)
        params.sub_(lr_t * m / (torch.sqrt(v) + eps))


DP_CUTS = [(0, 4), (4, 7)]   # world 2: 4 + 3 towers


def _dp_problem():
    obj, Rs, Rr, prop, tgt = D.synthetic_batch(7, 5, seed=9, fully_connected=False)
    W = draw_weights(np.random.default_rng(3), (7, 5))
    W[5] = 0.0                    # one tower of the smaller shard fully masked
    assert 0 < np.count_nonzero(W[:4]) != np.count_nonzero(W[4:]) > 0
    return obj, Rs, Rr, tgt, W


def _dp_trainer():
    params = P.to_flat(O.random_params(11), dtype=torch.float64)
    tr = Trainer(params, engine=WeightedOracleEngine(), mp_steps=2, dropout=0.0)
    tr.m = torch.zeros_like(params)
    tr.v = torch.zeros_like(params)
    return params, tr


def _dp_single(steps):
    obj, Rs, Rr, tgt, W = _dp_problem()
    batch = TowerBatch.from_dense(obj, Rs, Rr, device="cpu")
    params, tr = _dp_trainer()
    for _ in range(steps):
        out3 = tr.step(batch, torch.tensor(tgt.reshape(-1), dtype=torch.float64), weights=torch.tensor(W.reshape(-1)))
    assert float(out3[2]) == np.count_nonzero(W)
    return params.numpy()


def _dp_worker(rank, world, port, steps, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    obj, Rs, Rr, tgt, W = _dp_problem()
    sh = slice(*DP_CUTS[rank])
    batch = TowerBatch.from_dense(obj[sh], Rs[sh], Rr[sh], device="cpu")
    params, tr = _dp_trainer()
    for _ in range(steps):   # norm_global None: all-reduced, as n_global is
        tr.step(batch, torch.tensor(tgt[sh].reshape(-1), dtype=torch.float64), weights=torch.tensor(W[sh].reshape(-1)))
    if rank == 0:
        np.save(out, params.numpy())
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_dp_gloo_world2_weighted_equals_full_batch(tmp_path):
    """World 2, 4 + 3 towers of 5 boxes, S = 2, weighted (one tower masked): each rank's loss divides by its
    own non-zero count and its gradient is scaled by nnz_rank / norm_global; the parameters after 2 steps equal
    the single-process weighted step on the full batch to tests/test_distributed.py's 1e-9."""
    out = str(tmp_path / "p.npy")
    mp.start_processes(_dp_worker, args=(2, _free_port(), 2, out), nprocs=2, join=True, start_method="spawn")
    dp = np.load(out)
    ref = _dp_single(2)
    assert np.abs(dp - ref).max() < 1e-9
    assert np.abs(ref - P.to_flat(O.random_params(11), dtype=torch.float64).numpy()).max() > 1e-6  # it moved


def test_weighted_micro_batches_equal_full_batch():
    """Single process: the same weighted batch as two micro-batches (4 + 3 towers) accumulates to the
    full-batch step, and all-ones weights give the unweighted step."""
    obj, Rs, Rr, tgt, W = _dp_problem()
    params, tr = _dp_trainer()
    bs = [TowerBatch.from_dense(obj[a:b], Rs[a:b], Rr[a:b], device="cpu") for a, b in DP_CUTS]
    ts = [torch.tensor(tgt[a:b].reshape(-1), dtype=torch.float64) for a, b in DP_CUTS]
    ws = [torch.tensor(W[a:b].reshape(-1)) for a, b in DP_CUTS]
    for _ in range(2):
        tr.step(bs, ts, weights=ws)
    assert np.abs(params.numpy() - _dp_single(2)).max() < 1e-9
    # w ≡ 1 is the unweighted loss
    class OracleEngine(WeightedOracleEngine):
        def loss(self, logits, target):
            loss, g = O.keras_bce_grad(logits.numpy(), target.numpy())
            return torch.tensor([loss, 0.0, float(logits.numel())]), torch.tensor(g)

        loss_weighted = None

    full = TowerBatch.from_dense(obj, Rs, Rr, device="cpu")
    t = torch.tensor(tgt.reshape(-1), dtype=torch.float64)
    pa, ta = _dp_trainer()
    ta.step(full, t, weights=torch.ones(35, dtype=torch.float64))
    pb = P.to_flat(O.random_params(11), dtype=torch.float64)
    tb = Trainer(pb, engine=OracleEngine(), mp_steps=2, dropout=0.0)
    tb.m, tb.v = torch.zeros_like(pb), torch.zeros_like(pb)
    tb.step(full, t)
    assert np.abs(pa.numpy() - pb.numpy()).max() < 1e-12
