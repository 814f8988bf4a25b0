"""CPU: the host side of the tower-level loss (spwgnn_bce_tower, added within ABI 8) — exports,
the struct's size, every argument status that comes back before any device work (fake pointers that are never
followed, as tests/test_loss_weights_host.py does), the loss path `step.loss_path` picks, the fp64 restatement
tests/tower_loss_ref.py against itself (its hand-written gradient == torch autograd), the packed plans' tower
order, and the data-parallel Trainer with the tower term under gloo (an fp64 oracle engine) against the
single-process step on the full batch."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import test_distributed as TD
from test_eval_host import EvalOracleEngine
import tower_loss_ref as TR
from oracle import model as O
from spwgnn_amd import _lib, engine as E, params as P, step as S
from spwgnn_amd.batch import TowerBatch
from spwgnn_amd.trainer import Trainer

FAKE = 0x1000


def test_exports_struct_size_and_argument_counts():
    lib = _lib.lib()
    assert hasattr(lib, "spwgnn_bce_tower") and hasattr(lib, "spwgnn_bce_tower_scratch_bytes")
    assert len(lib.spwgnn_bce_tower.argtypes) == 9 and len(lib.spwgnn_bce_tower_scratch_bytes.argtypes) == 2
    assert lib.spwgnn_struct_size(12) == C.sizeof(_lib.TowerLossC) == 80
    for unused in (5, 8, 11, 13):
        assert lib.spwgnn_struct_size(unused) == -1
    assert lib.spwgnn_version() == 8 == _lib.ABI_VERSION
    assert lib.spwgnn_bce_tower_scratch_bytes(256, 256) > 0
    assert lib.spwgnn_bce_tower_scratch_bytes(1 << 33, 1 << 30) == lib.spwgnn_bce_tower_scratch_bytes(1, 1)
    assert lib.spwgnn_bce_tower_scratch_bytes(0, 1) == -1 and lib.spwgnn_bce_tower_scratch_bytes(1, 0) == -1


def _tl(**kw):
    tl = _lib.TowerLossC()
    tl.n_towers, tl.tower_offsets, tl.alpha, tl.mu, tl.norm_t, tl.out6 = 2, FAKE, 1.0, 1.0, 2.0, FAKE
    for k, v in kw.items():
        setattr(tl, k, v)
    return tl


def _call(tl, logits=FAKE, targets=FAKE, n=12, lw=None, out3=FAKE, dlogits=FAKE, scratch=FAKE):
    return _lib.lib().spwgnn_bce_tower(logits, targets, n, C.byref(lw) if lw is not None else None,
                                       C.byref(tl) if tl is not None else None, out3, dlogits, scratch, None)


def test_every_bad_argument_is_refused_before_device_work():
    bad = [
        dict(tl=None),
        dict(tl=_tl(), logits=None), dict(tl=_tl(), out3=None), dict(tl=_tl(), scratch=None),
        dict(tl=_tl(), targets=None),                                     # derived targets need the node targets
        dict(tl=_tl(tower_targets=FAKE), targets=None),                   # ... and alpha != 0 needs them too
        dict(tl=_tl(alpha=0.0), targets=None),                            # alpha == 0 alone: no tower targets
        dict(tl=_tl(), n=0), dict(tl=_tl(), n=-3),
        dict(tl=_tl(n_towers=0)), dict(tl=_tl(n_towers=-1)),
        dict(tl=_tl(tower_offsets=None)), dict(tl=_tl(out6=None)), dict(tl=_tl(reserved=1)),
        dict(tl=_tl(mu=0.0)), dict(tl=_tl(mu=-1.0)), dict(tl=_tl(mu=math.inf)), dict(tl=_tl(mu=math.nan)),
        dict(tl=_tl(alpha=-0.5)), dict(tl=_tl(alpha=math.inf)), dict(tl=_tl(alpha=math.nan)),
        dict(tl=_tl(norm_t=0.0)), dict(tl=_tl(norm_t=-2.0)), dict(tl=_tl(norm_t=math.nan)),
        dict(tl=_tl(weights6=FAKE)), dict(tl=_tl(total6=FAKE)),           # the totals go together
    ]
    lw_bad = _lib.LossWeightsC()
    lw_bad.w, lw_bad.norm = None, 12.0
    bad.append(dict(tl=_tl(), lw=lw_bad))
    lw_bad2 = _lib.LossWeightsC()
    lw_bad2.w, lw_bad2.norm = FAKE, 0.0
    bad.append(dict(tl=_tl(), lw=lw_bad2))
    for kw in bad:
        assert _call(**kw) == _lib.E_ARG, {k: (v if k != "tl" else None) for k, v in kw.items()}


def test_engine_and_path_checks():
    for args in ((-1.0, 1.0), (math.nan, 1.0), (math.inf, 1.0), (1.0, -1.0), (1.0, math.nan)):
        with pytest.raises(ValueError):
            E.check_tower_loss(*args)
    assert E.check_tower_loss(0, 1) == (0.0, 1.0) and E.check_tower_loss(0.25, 0) == (0.25, 0.0)
    assert type(S.loss_path("cpu", 5)) is S.LossPath
    assert type(S.loss_path("cpu", 5, tower_loss=0.0, node_loss=0.3)) is S.LossPath        # off: today's path
    assert type(S.loss_path("cpu", 5, (0, 0, 0, 0, 1.0))) is S.DeepLossPath
    p = S.loss_path("cpu", 5, tower_loss=0.5, node_loss=0.25)
    assert type(p) is S.TowerLossPath and (p.mu, p.alpha) == (0.5, 0.25) and p.lam is None
    assert p.tower.out6.shape == (6,) and p.tower.total6 is None
    assert S.loss_path("cpu", 5, tower_loss=1.0, totals=True).tower.total6.dtype == torch.float64
    with pytest.raises(ValueError):
        S.loss_path("cpu", 5, (0, 0, 0, 0, 1.0), tower_loss=1.0)
    params = P.to_flat(O.random_params(11), dtype=torch.float64)
    with pytest.raises(ValueError):
        Trainer(params, engine=TowerOracleEngine(), tower_loss=1.0, step_loss_weights=(0, 0, 0, 0, 1.0))
    with pytest.raises(ValueError):
        Trainer(params, engine=TD.OracleEngine(), tower_loss=1.0)                           # no loss_tower
    with pytest.raises(ValueError):
        Trainer(params, engine=TD.OracleEngine()).step(None, None, tower_targets=torch.zeros(1))


# ---------------------------------------------------------------- the reference against itself
def _random_case(seed, T=40, sigma=2.0, shift=3.0):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 33, T)
    off = np.concatenate([[0], np.cumsum(sizes)])
    n = int(off[-1])
    z = rng.normal(shift, sigma, n)
    t = (rng.random(n) < 0.9).astype(np.float64)
    w = rng.choice([0.0, 0.5, 1.0, 2.5], size=n, p=[0.3, 0.25, 0.25, 0.2])
    w[off[3]:off[4]] = 0.0
    tt = rng.integers(0, 2, T).astype(np.float64)
    return z, t, w, off, tt


@pytest.mark.parametrize("weighted,explicit,alpha", [(False, False, 1.0), (True, False, 0.5), (False, True, 0.0),
                                                     (True, True, 1.0)])
def test_reference_gradient_equals_autograd(weighted, explicit, alpha):
    z, t, w, off, tt = _random_case(1)
    w_, tt_ = (w if weighted else None), (tt if explicit else None)
    L, d, parts = TR.combined_ref(z, off, None if alpha == 0 else t, tt_, w_, alpha, 0.7)
    zt = torch.tensor(z, requires_grad=True)
    Lt = 0.7 * TR.tower_loss_torch(zt, off, t, tt_, w_)
    if alpha:
        Lt = Lt + alpha * TR.node_loss_torch(zt, t, w_)
    Lt.backward()
    assert abs(float(Lt) - L) <= 1e-12 * max(1.0, abs(L))
    assert np.abs(zt.grad.numpy() - d).max() <= 1e-12
    tw = TR.towers_ref(z, off, t, tt_, w_)
    assert tw["counted"][3] == 0 or not weighted
    assert parts[5] == (tw["counted"] > 0).sum() and 0 < (tw["T"] == 1).sum() < len(tt)


def test_reference_clip_and_branches():
    """Both log1mexp branches agree where they meet, and a tower outside either clip edge has gradient 0."""
    x = np.array([-TR.LN2 - 1e-9, -TR.LN2 + 1e-9])
    assert abs(np.diff(TR.log1mexp(x))[0]) < 1e-8
    off = [0, 3, 35]
    z = np.concatenate([np.full(3, 25.0), np.full(32, -1.0)])        # s = −3e-11·… > HI;  s = −32·1.313 < LO
    for tt in ([1.0, 1.0], [0.0, 0.0]):
        L, d, tw = TR.tower_loss_ref(z, off, tower_targets=tt)
        assert not tw["inside"].any() and np.all(d == 0) and np.isfinite(L)
    assert abs(TR.tower_loss_ref(z, off, tower_targets=[1.0, 0.0])[0] - (-TR.HI - TR.log1mexp(TR.LO)) / 2) < 1e-12


def test_towers_to_plan_order():
    """A packed plan's tower order, recovered from node_perm: per-tower rows follow the node rows."""
    objs, raws, tgts = TD._ragged_problem()
    b = TowerBatch.ragged(objs, relation_threshold=TD.D.RELATION_THRESHOLD, device="cpu", raw_positions_list=raws)
    assert b.towers_to_plan_order(np.arange(3)) is not None
    sizes = np.array([len(o) for o in objs])
    node_tower = np.repeat(np.arange(len(objs)), sizes)
    from spwgnn_amd.batch import HostPlan
    pos = np.concatenate(objs)
    te = b.tower_edges
    plan = HostPlan.build(pos, sizes, b.src, b.dst, te, pack=True)
    pb = TowerBatch.from_plan(plan, "cpu")
    assert pb.node_perm is not None and not np.array_equal(pb.node_perm, np.arange(len(pos)))
    got = pb.towers_to_plan_order(np.arange(len(objs)))
    want = pb.to_plan_order(node_tower)[np.concatenate([[0], np.cumsum(pb.tower_nodes)[:-1]])]
    assert np.array_equal(got, want) and np.array_equal(sizes[got], pb.tower_nodes)
    assert torch.equal(pb.towers_to_plan_order(torch.arange(len(objs))), torch.as_tensor(want))


# ---------------------------------------------------------------- gloo data parallel
class TowerOracleEngine(EvalOracleEngine):
    """tests/test_distributed.py's fp64 oracle (with tests/test_eval_host.py's `eval_metrics`) and `loss_tower`
    from tests/tower_loss_ref.py (tests only)."""

    def loss_tower(self, logits, target, batch, tower_targets, weights, norm, norm_t, tower_loss, node_loss,
                   want_dlogits=True):
        off = np.concatenate([[0], np.cumsum(batch.tower_nodes)])
        L, d, parts = TR.combined_ref(
            logits.numpy(), off, None if target is None else target.numpy(),
            None if tower_targets is None else np.asarray(tower_targets), None if weights is None else np.asarray(weights),
            node_loss, tower_loss, norm, norm_t)
        parts[1] = 0.0
        return torch.tensor(parts, dtype=torch.float64), (torch.tensor(d) if want_dlogits else None)


MU, ALPHA = 0.6, 0.8


def _dp_problem():
    """11 ragged towers of 3..8 boxes (tests/test_distributed.py), targets mostly 1 so that both tower labels
    occur, per-node weights with one tower fully masked, explicit tower targets."""
    objs, raws, _ = TD._ragged_problem()
    rng = np.random.default_rng(17)
    tgts = [(rng.random(len(o)) < 0.85).astype(np.float64) for o in objs]
    ws = [rng.choice([0.0, 0.5, 1.0, 2.5], size=len(o), p=[0.3, 0.25, 0.25, 0.2]) for o in objs]
    ws[1][:] = 0.0
    tts = rng.integers(0, 2, len(objs)).astype(np.float64)
    derived = [float(all(t == 1)) for t in tgts]
    assert 0 < sum(derived) < len(derived)
    return objs, raws, tgts, ws, tts


def _dp_args(mode, a, b):
    """step()'s (batch, target, kwargs) for the towers [a, b) in `mode`."""
    objs, raws, tgts, ws, tts = _dp_problem()
    batch = TD._ragged_batch(objs, raws, a, b)
    tg = torch.tensor(np.concatenate(tgts[a:b]))
    kw = {}
    if mode in ("weighted", "explicit"):
        kw["weights"] = torch.tensor(np.concatenate(ws[a:b]))
    if mode in ("explicit", "tower_only"):
        kw["tower_targets"] = torch.tensor(tts[a:b])
    if mode == "tower_only":
        tg = None
    return batch, tg, kw


def _dp_trainer():
    params = P.to_flat(O.random_params(11), dtype=torch.float64)
    tr = Trainer(params, engine=TowerOracleEngine(), mp_steps=2, dropout=0.0, tower_loss=MU,
                 node_loss=ALPHA)
    tr.m, tr.v = torch.zeros_like(params), torch.zeros_like(params)
    return params, tr


def _dp_steps(tr, cuts, mode, steps):
    parts = [_dp_args(mode, a, b) for a, b in cuts]
    for _ in range(steps):
        if len(parts) == 1:
            b, tg, kw = parts[0]
            out3 = tr.step(b, tg, **kw)
        else:
            kw = {k: [p[2][k] for p in parts] for k in parts[0][2]}
            out3 = tr.step([p[0] for p in parts], [p[1] for p in parts], **kw)
    return out3


def _dp_single(mode, steps):
    params, tr = _dp_trainer()
    out3 = _dp_steps(tr, [(0, 11)], mode, steps)
    return params.numpy(), out3.numpy(), tr.loss_parts.numpy()


def _dp_worker(rank, world, port, steps, out, mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    params, tr = _dp_trainer()
    cuts = [[(0, 2), (2, 3)], [(3, 7), (7, 9), (9, 11)]][rank]       # 3 + 8 towers, as 2 and 3 micro-batches
    _dp_steps(tr, cuts, mode, steps)
    if rank == 0:
        np.save(out, params.numpy())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["derived", "weighted", "explicit", "tower_only"])
def test_dp_gloo_world2_tower_loss_equals_full_batch(tmp_path, mode):
    """World 2, ragged unequal shards (3 + 8 towers) cut into micro-batches, 3 steps: the tower term divides by
    the all-reduced tower count inside the loss, the node term enters scaled by its node share, the gradients
    are summed with weight 1 — the parameters equal the single-process full-batch step at
    tests/test_distributed.py's 1e-9."""
    out = str(tmp_path / "p.npy")
    mp.start_processes(_dp_worker, args=(2, TD._free_port(), 3, out, mode), nprocs=2, join=True, start_method="spawn")
    ref, _, _ = _dp_single(mode, 3)
    assert np.abs(np.load(out) - ref).max() < 1e-9
    assert np.abs(ref - P.to_flat(O.random_params(11), dtype=torch.float64).numpy()).max() > 1e-6   # it moved


@pytest.mark.parametrize("mode", ["derived", "explicit"])
def test_micro_batches_equal_full_batch_and_loss_parts(mode):
    """Single process: ragged micro-batches accumulate to the full-batch step, and `loss_parts` / the returned
    row describe the whole shard: the same six numbers whichever way it is cut."""
    ref, out3, parts = _dp_single(mode, 2)
    params, tr = _dp_trainer()
    o3 = _dp_steps(tr, [(0, 2), (2, 3), (3, 9), (9, 11)], mode, 2)
    assert np.abs(params.numpy() - ref).max() < 1e-9
    assert np.allclose(tr.loss_parts.numpy(), parts, rtol=1e-6, atol=0) and np.allclose(o3.numpy(), out3, rtol=1e-6)
    assert abs(out3[0] - (ALPHA * parts[0] + MU * parts[3])) <= 1e-6 * abs(out3[0])
    assert parts[5] == (10 if mode == "explicit" else 11) and parts[2] > 0


def test_a_shard_reports_its_own_means():
    """One process stepping a 3-tower shard of the 11-tower batch (n_global and towers_global given): `loss_parts`
    holds the shard's own means — L_node over its nodes, L_tower over its counted towers — not its share."""
    objs, raws, tgts, ws, tts = _dp_problem()
    params, tr = _dp_trainer()
    b, tg, _ = _dp_args("derived", 0, 3)
    z = TowerOracleEngine().forward(params, b, tr.run_config())
    off = np.concatenate([[0], np.cumsum(b.tower_nodes)])
    _, _, parts = TR.combined_ref(z.numpy(), off, tg.numpy(), None, None, ALPHA, MU)
    out3 = tr.step(b, tg, n_global=sum(len(o) for o in objs), towers_global=11)
    lp = tr.loss_parts.numpy()
    assert np.allclose(lp[[0, 3]], [parts[0], parts[3]], rtol=1e-6) and lp[2] == b.n_nodes and lp[5] == 3
    assert abs(float(out3[0]) - (ALPHA * parts[0] + MU * parts[3])) <= 1e-6 * float(out3[0])


# ---------------------------------------------------------------- Trainer.evaluate with the tower term
def _eval_worker(rank, world, port, out, mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    params, tr = _dp_trainer()
    parts = [_dp_args(mode, a, b) for a, b in [[(0, 2), (2, 3)], [(3, 7), (7, 9), (9, 11)]][rank]]
    kw = {k: [p[2][k] for p in parts] for k in parts[0][2]}
    d = tr.evaluate([p[0] for p in parts], [p[1] for p in parts], **kw)
    if rank == 0:
        np.save(out, np.array([d["loss"], d["tower_loss"], d["tower_accuracy"], d.get("n", -1), d.get("towers", -1)]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["derived", "explicit", "tower_only"])
def test_evaluate_with_tower_loss(tmp_path, mode):
    """Trainer(tower_loss=).evaluate: the loss parts of the whole set against tests/tower_loss_ref.py on the full
    batch's logits — one batch, micro-batches, and world 2 under gloo give the same numbers; the summary's counts
    are there unless a micro-batch came without node targets; the parameters do not move."""
    params, tr = _dp_trainer()
    before = params.clone()
    b, tg, kw = _dp_args(mode, 0, 11)
    z = TowerOracleEngine().forward(params, b, tr.run_config())
    off = np.concatenate([[0], np.cumsum(b.tower_nodes)])
    w, tt = kw.get("weights"), kw.get("tower_targets")
    alpha = ALPHA if tg is not None else 0.0
    L, _, parts = TR.combined_ref(z.numpy(), off, None if tg is None else tg.numpy(), None if tt is None else tt.numpy(),
                                  None if w is None else w.numpy(), alpha, MU)
    tw = TR.towers_ref(z.numpy(), off, None if tg is None else tg.numpy(), None if tt is None else tt.numpy(),
                       None if w is None else w.numpy())
    acc = (tw["correct"] & (tw["counted"] > 0)).sum() / (tw["counted"] > 0).sum()
    one = tr.evaluate(b, tg, **kw)
    cuts = [_dp_args(mode, a, c) for a, c in [(0, 2), (2, 3), (3, 9), (9, 11)]]
    many = tr.evaluate([p[0] for p in cuts], [p[1] for p in cuts], **{k: [p[2][k] for p in cuts] for k in cuts[0][2]})
    out = str(tmp_path / "e.npy")
    mp.start_processes(_eval_worker, args=(2, TD._free_port(), out, mode), nprocs=2, join=True, start_method="spawn")
    dp = np.load(out)
    for d in (one, many, dict(loss=dp[0], tower_loss=dp[1], tower_accuracy=dp[2])):
        assert abs(d["loss"] - (alpha * parts[0] + MU * parts[3])) <= 1e-9 and abs(d["tower_loss"] - parts[3]) <= 1e-9
        assert d["tower_accuracy"] == acc
    if mode == "tower_only":
        assert set(one) == {"loss", "tower_loss", "tower_accuracy"} and dp[3] == -1
    else:
        assert one["n"] == many["n"] == dp[3] == parts[2] and one["towers"] == dp[4] == parts[5]
    assert torch.equal(params, before) and tr.iterations == 0
    with pytest.raises(ValueError):
        Trainer(P.to_flat(O.random_params(11), dtype=torch.float64), engine=TowerOracleEngine()).evaluate(
            b, tg if tg is not None else torch.zeros(b.n_nodes), tower_targets=torch.zeros(11))


def test_replayed_block_carries_the_tower_offsets():
    """CPU part of the replay contract: two ragged plans of ONE geometry with different tower sizes exist (the
    GPU suite replays such a pair), and a tower-walking step body asks for the offsets in the static block."""
    from spwgnn_amd.replay import step_body
    pa, pb = same_geometry_plans()
    assert pa.geometry == pb.geometry and not np.array_equal(pa.tower_nodes, pb.tower_nodes)
    path = S.loss_path("cpu", 2, tower_loss=1.0)
    assert step_body(None, None, None, None, path, None, None, None, 0).needs_towers
    assert not step_body(None, None, None, None, S.loss_path("cpu", 2), None, None, None, 0).needs_towers


def same_geometry_plans(sizes=((4, 6, 5, 5, 6, 4, 5, 5), (5, 5, 4, 6, 5, 5, 6, 4))):
    """Fully connected ragged plans with 30 relation slots per tower: the same wave-tiles, blocks and array
    shapes — one replay geometry — over different tower sizes."""
    from spwgnn_amd import data as D
    from spwgnn_amd.batch import HostPlan
    plans = []
    for seed, sz in enumerate(sizes):
        raws = [D.synthetic_towers(1, int(n), seed=seed * 50 + i)[0] for i, n in enumerate(sz)]
        pos = np.concatenate([(r / D.RELATION_THRESHOLD).astype(np.float32) for r in raws])
        src, dst, te, off = [], [], [], 0
        for n in sz:
            m, j = np.nonzero(~np.eye(n, dtype=bool))
            src.append(off + m), dst.append(off + j), te.append(len(m))
            off += n
        plans.append(HostPlan.build(pos, np.array(sz, np.int32), np.concatenate(src), np.concatenate(dst),
                                    np.array(te, np.int32), edge_cap=30))
    return plans
