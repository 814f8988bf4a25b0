"""GPU: the tower-level loss above the kernel — the whole gradient against the fp64 oracle, and
the front ends: Trainer.step against the hand sequence, replayed against eager steps, KerasModel.fit against a
hand loop, tower-only labels, `tower_bce` under autograd, and tower_loss = 0 against the plain model."""
import functools
import os

import numpy as np
import pytest
import torch

import tower_loss_ref as TR
from oracle import model as O
from spwgnn_amd import GraphNetwork, PropagationNetwork, TowerBatch, data as D, engine as E, params as P, tower_bce
from spwgnn_amd.batch import HostPlan
from spwgnn_amd.keras_api import CompactDataset, keras_split_at
from spwgnn_amd.replay import ReplayStep
from spwgnn_amd.trainer import Trainer

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
MU, ALPHA = 0.6, 0.8


def dev(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


# -------------------------------------------------------------------------------- 5. the whole gradient, fp64 oracle
def _golden_plan():
    g = np.load(os.path.join(GOLDEN, "golden_N6_B4_S5_thr.npz"))
    params = dict(np.load(os.path.join(GOLDEN, "golden_params.npz")))
    b = TowerBatch.from_dense(g["objects"], g["Rs"], g["Rr"], g["prop"], device="cpu")
    tgt = np.asarray(g["target"], np.float64).reshape(-1)
    return dict(params=params, S=int(g["mp_steps"]), pos=g["objects"].reshape(-1, 3), sizes=b.tower_nodes, src=b.src,
                dst=b.dst, te=b.tower_edges, prop=g["prop"].reshape(-1, 100), tgt=tgt, tt=np.array([1.0, 0.0, 1.0, 0.0]))


def _ragged_plan():
    """11 towers of 4..9 boxes, thresholded relations (main.py:71-81); targets mostly 1, so derived tower labels of
    both kinds occur."""
    rng = np.random.default_rng(5)
    sizes = rng.integers(4, 10, size=11)
    raws = [D.synthetic_towers(1, int(n), seed=500 + i)[0] for i, n in enumerate(sizes)]
    objs = [(r / D.RELATION_THRESHOLD).astype(np.float32) for r in raws]
    b = TowerBatch.ragged(objs, relation_threshold=D.RELATION_THRESHOLD, device="cpu", raw_positions_list=raws)
    n = int(sizes.sum())
    tgt = (rng.random(n) < 0.85).astype(np.float64)
    tgt[:sizes[0]] = 1.0
    return dict(params=O.random_params(seed=1), S=3, pos=np.concatenate(objs), sizes=b.tower_nodes, src=b.src, dst=b.dst,
                te=b.tower_edges, prop=None, tgt=tgt, tt=rng.integers(0, 2, 11).astype(np.float64))


@functools.lru_cache(maxsize=None)
def _oracle_case(name: str, explicit: bool, weighted: bool, pack: bool):
    """The batch on the GPU and the fp64 reference (loss, per-tensor gradients), built once per case: the oracle
    runs on the plan's own arrays, so a packed plan's node and tower order is the reference's too."""
    c = _golden_plan() if name == "golden" else _ragged_plan()
    plan = HostPlan.build(c["pos"], c["sizes"], c["src"], c["dst"], c["te"], c["prop"], pack=pack)
    batch = TowerBatch.from_plan(plan, DEV)
    assert (batch.node_perm is not None) == pack
    tgt = batch.to_plan_order(c["tgt"])
    tt = batch.towers_to_plan_order(c["tt"]) if explicit else None
    w = None
    if weighted:
        w = batch.to_plan_order(np.random.default_rng(7).choice([0.0, 0.5, 1.0, 2.5], size=len(tgt), p=[0.3, 0.25, 0.25, 0.2]))
    off = np.concatenate([[0], np.cumsum(batch.tower_nodes)])
    tp = O.to_torch(c["params"], requires_grad=True)
    pos = torch.as_tensor(plan.arrays[0][:, :3], dtype=torch.float64)
    prop = torch.zeros(len(tgt), 100, dtype=torch.float64) if c["prop"] is None else \
        torch.as_tensor(batch.to_plan_order(c["prop"]), dtype=torch.float64)
    z = O.forward_gather(tp, pos, torch.as_tensor(batch.src, dtype=torch.long), torch.as_tensor(batch.dst, dtype=torch.long),
                         prop, c["S"])
    loss = ALPHA * TR.node_loss_torch(z, tgt, w) + MU * TR.tower_loss_torch(z, off, tgt, tt, w)
    loss.backward()
    tw = TR.towers_ref(z.detach().numpy(), off, tgt, tt, w)
    assert tw["inside"][tw["counted"] > 0].all() and not tw["near_edge"].any()     # no tower at a clip edge
    ref = {k: v.grad.numpy().copy() for k, v in tp.items()}
    return c, batch, tgt, tt, w, float(loss.detach()), ref, tw


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("math", ["f32", "x6"])
@pytest.mark.parametrize("name,explicit,weighted,pack", [("golden", False, False, False), ("golden", True, False, False),
                                                          ("ragged", False, False, False), ("ragged", True, True, False),
                                                          ("ragged", False, False, True), ("ragged", True, False, True)])
def test_gradients_against_fp64_oracle(name, explicit, weighted, pack, math, wide):
    """forward -> bce_tower -> backward against oracle.forward_gather with tests/tower_loss_ref.py's loss under
    torch autograd: per tensor max|Δ| <= 1e-5·max|ref| + 1e-7 and the loss to 1e-5 — the bounds of
    tests/test_gpu_loss_weights.py's test_weighted_gradients_against_fp64_oracle (the project's fp32 parity
    criterion), on the team kernels and the wide ones, for a plain and a packed plan."""
    c, batch, tgt, tt, w, loss_ref, ref, tw = _oracle_case(name, explicit, weighted, pack)
    flat = P.to_flat(c["params"], device=DEV)
    run = E.RunConfig(c["S"], training=True, math=math)

    def go():
        ws, sc = E.Workspace(DEV), E.TowerLossScratch(DEV)
        z = E.forward(flat, batch, run, ws)
        out3, dz = E.bce_tower(z, dev(tgt), batch, sc, MU, ALPHA, tower_targets=dev(tt), node_weights=dev(w))
        grads, _ = E.backward(flat, batch, run, ws, dz)
        return out3, sc.out6, grads
    if wide:
        with E.wide_kernels():
            out3, out6, grads = go()
    else:
        out3, out6, grads = go()
    torch.cuda.synchronize()
    assert abs(float(out3[0]) - loss_ref) <= 1e-5
    assert float(out6[5]) == (tw["counted"] > 0).sum() and float(out6[4]) == (tw["correct"] & (tw["counted"] > 0)).sum()
    g = P.from_flat(grads)
    for k, r in ref.items():
        err = np.abs(g[k] - r).max()
        assert err <= 1e-5 * np.abs(r).max() + 1e-7, (k, err, np.abs(r).max())


# -------------------------------------------------------------------------------- 6. front ends
def _plans(n=3, B=32, N=6):
    plans, tgts = [], []
    for seed in range(1, n + 1):
        raw = D.synthetic_towers(B, N, seed=seed)
        obj = (raw / D.RELATION_THRESHOLD).astype(np.float32)
        Rs, Rr = D.relation_matrices(raw, D.RELATION_THRESHOLD)
        e = np.array(O.dense_to_edges(Rs, Rr), np.int64).reshape(-1, 4)
        te = np.bincount(e[:, 0], minlength=B).astype(np.int32)
        plans.append(HostPlan.build(obj.reshape(-1, 3), np.full(B, N, np.int32), e[:, 0] * N + e[:, 2],
                                    e[:, 0] * N + e[:, 3], te, edge_cap=N * (N - 1)))
        tgts.append((np.random.default_rng(seed).random(B * N) < 0.85).astype(np.float32))
    return plans, tgts


def test_trainer_step_equals_hand_sequence_and_replay():
    """Trainer(tower_loss=).step == forward, bce_tower, backward, adam by hand, and == the replayed step
    (derived labels), bit for bit over three batches: parameters and both Adam moments; `loss_parts` is the
    loss launch's out6."""
    from spwgnn_amd.trainer import dropout_key
    params = O.random_params(12)
    plans, tgts = _plans()
    ta = Trainer(P.to_flat(params, device=DEV), mp_steps=5, dropout=0.1, seed=11, math="x6", tower_loss=MU, node_loss=ALPHA)
    flat = P.to_flat(params, device=DEV)
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    ws, sc = E.Workspace(DEV), E.TowerLossScratch(DEV)
    for it, (p, t) in enumerate(zip(plans, tgts)):
        b = TowerBatch.from_plan(p, DEV)
        out3 = ta.step(b, dev(t))
        run = E.RunConfig(5, training=True, dropout=0.1, seed=dropout_key(11, it, 0, 0), math="x6")
        z = E.forward(flat, b, run, ws)
        o3, dz = E.bce_tower(z, dev(t), b, sc, MU, ALPHA, norm_t=32)
        g, _ = E.backward(flat, b, run, ws, dz)
        E.adam(flat, g, m, v, it + 1)
        assert torch.equal(ta.loss_parts, sc.out6) and torch.equal(out3, o3)      # the launch's own out3, bits included
    assert torch.equal(ta.params, flat) and torch.equal(ta.m, m) and torch.equal(ta.v, v)
    assert 0 < float(sc.out6[4]) <= float(sc.out6[5]) == 32
    tb = Trainer(P.to_flat(params, device=DEV), mp_steps=5, dropout=0.1, seed=11, math="x6", tower_loss=MU, node_loss=ALPHA)
    rs = ReplayStep(plans[0], DEV, tb.replay_body(plans[0].n_nodes))
    for p, t in zip(plans, tgts):
        tb.replay_step(rs, p, t)
    torch.cuda.synchronize()
    assert rs.replays == 2 and tb.iterations == 3
    assert torch.equal(ta.params, tb.params) and torch.equal(ta.m, tb.m) and torch.equal(ta.v, tb.v)
    with pytest.raises(ValueError):
        tb.replay_body(plans[0].n_nodes, weighted=True)


def test_trainer_tower_only_and_explicit_targets():
    """step(batch, None, tower_targets=): no node targets at all; and explicit targets move the parameters
    differently from the derived ones."""
    params = O.random_params(12)
    (plan,), (t,) = _plans(1)
    b = TowerBatch.from_plan(plan, DEV)
    tt = (np.arange(32) % 2).astype(np.float32)
    out = {}
    for name, kw, tg in (("only", dict(tower_targets=dev(tt)), None), ("explicit", dict(tower_targets=dev(tt)), dev(t)),
                         ("derived", {}, dev(t))):
        tr = Trainer(P.to_flat(params, device=DEV), mp_steps=3, dropout=0.0, tower_loss=1.0, node_loss=1.0)
        o3 = tr.step(b, tg, **kw)
        torch.cuda.synchronize()
        assert torch.isfinite(o3).all() and torch.isfinite(tr.params).all()
        out[name] = (tr.params.clone(), tr.loss_parts.clone())
    assert out["only"][1][:3].tolist() == [0.0, 0.0, 192.0] and out["only"][1][5] == 32
    assert torch.equal(out["only"][1][3:], out["explicit"][1][3:])
    assert not torch.equal(out["only"][0], out["explicit"][0]) and not torch.equal(out["derived"][0], out["explicit"][0])


def test_tower_bce_autograd_equals_engine_steps():
    """tower_bce on GraphNetwork.forward_batch's logits: backward gives the flat gradient of forward ->
    bce_tower -> backward, bit for bit, and scales with the incoming gradient."""
    params = O.random_params(3)
    (plan,), (t,) = _plans(1, B=8, N=5)
    b = TowerBatch.from_plan(plan, DEV)
    net = GraphNetwork(mp_steps=3, dropout=0.0, params=params, math="x6")
    sc = E.TowerLossScratch(DEV)
    L = tower_bce(net.forward_batch(b), dev(t), b, MU, ALPHA, scratch=sc)
    (2.0 * L).backward()
    flat = P.to_flat(params, device=DEV)
    ws, sc2 = E.Workspace(DEV), E.TowerLossScratch(DEV)
    run = E.RunConfig(3, training=True, math="x6")
    o3, dz = E.bce_tower(E.forward(flat, b, run, ws), dev(t), b, sc2, MU, ALPHA)
    g, _ = E.backward(flat, b, run, ws, 2.0 * dz)
    assert float(L.detach()) == float(o3[0]) and torch.equal(sc.out6, sc2.out6)
    assert torch.equal(net.flat.grad, g)


FIT_B, FIT_N, FIT_BATCH, FIT_EPOCHS, FIT_VAL = 40, 5, 16, 2, 0.2


@functools.lru_cache(maxsize=None)
def _fit_data():
    obj, Rs, Rr, prop, tgt = D.synthetic_batch(FIT_B, FIT_N, seed=7, fully_connected=False)
    x = {"objects": obj, "sender_relations": Rs, "receiver_relations": Rr, "propagation": prop}
    tgt = (np.random.default_rng(3).random((FIT_B, FIT_N)) < 0.85).astype(np.float32)
    tt = np.random.default_rng(4).integers(0, 2, FIT_B).astype(np.float32)
    return x, tgt, tt


def _fit(graph, y, fit_kw=None, **model_kw):
    x, _, _ = _fit_data()
    model = PropagationNetwork(seed=4, **model_kw).getModel(FIT_N)
    h = model.fit(x, y, batch_size=FIT_BATCH, epochs=FIT_EPOCHS, validation_split=FIT_VAL, verbose=0, graph=graph,
                  **(fit_kw or {}))
    torch.cuda.synchronize()
    return h, model.net.flat.detach().cpu().numpy().copy(), model


def _hand_loop(y, W=None, **model_kw):
    """fit's batches through train_on_batch / evaluate_batch, the history from `loss_parts`; W: (B, N) node weights."""
    x, _, _ = _fit_data()
    tgt, tt = y.get("target"), y.get("tower_target")
    n_tr = keras_split_at(FIT_B, FIT_VAL)
    ds = CompactDataset(x["objects"], x["sender_relations"], x["receiver_relations"], x["propagation"])
    model = PropagationNetwork(seed=4, **model_kw).getModel(FIT_N)
    mu, alpha = model.tower_loss, (model.node_loss if tgt is not None else 0.0)
    vbatch = ds.subset(np.arange(n_tr, FIT_B), DEV)
    rng = np.random.default_rng(0)
    keys = ("loss", "binary_accuracy", "tower_loss", "tower_accuracy")
    hist = {k: [] for k in keys + tuple("val_" + k for k in keys)}
    sel = lambda a, idx: None if a is None else a[idx]
    for _ in range(FIT_EPOCHS):
        order = rng.permutation(n_tr)
        tot = np.zeros(6)
        for b0 in range(0, n_tr, FIT_BATCH):
            idx = order[b0:b0 + FIT_BATCH]
            batch = TowerBatch.from_plan(ds.subset_plan(idx, edge_cap=True), DEV)
            model.train_on_batch(batch, None if tgt is None else dev(tgt[idx].reshape(-1)), node_weights=sel(W, idx),
                                 tower_targets=sel(tt, idx))
            k = float(len(idx))
            tot += model.loss_parts.double().cpu().numpy() * np.array([k, 1.0, 1.0, k, 1.0, 1.0])
        hist["loss"].append((alpha * tot[0] + mu * tot[3]) / n_tr)
        hist["binary_accuracy"].append(tot[1] / max(tot[2], 1))
        hist["tower_loss"].append(tot[3] / n_tr)
        hist["tower_accuracy"].append(tot[4] / max(tot[5], 1))
        model.evaluate_batch(vbatch, None if tgt is None else dev(tgt[n_tr:].reshape(-1)),
                             node_weights=sel(W, slice(n_tr, None)), tower_targets=sel(tt, slice(n_tr, None)))
        v = model.loss_parts.tolist()
        hist["val_loss"].append(alpha * v[0] + mu * v[3])
        hist["val_binary_accuracy"].append(v[1] / max(v[2], 1))
        hist["val_tower_loss"].append(v[3])
        hist["val_tower_accuracy"].append(v[4] / max(v[5], 1))
    torch.cuda.synchronize()
    return hist, model.net.flat.detach().cpu().numpy().copy()


def test_fit_with_tower_loss_equals_hand_loop_and_replay():
    """Derived labels: the replayed steps, eager and captured, and the hand loop over train_on_batch agree bit for
    bit in the parameters and the history; evaluate returns the validation numbers."""
    x, tgt, _ = _fit_data()
    y = {"target": tgt[..., None]}
    kw = dict(tower_loss=MU, node_loss=ALPHA)
    h_eager, p_eager, model = _fit(False, y, **kw)
    h_graph, p_graph, m_graph = _fit(True, y, **kw)
    assert h_eager == h_graph and np.array_equal(p_eager, p_graph)
    assert sum(s.replays for s in m_graph._replays.steps.values()) == 4 - len(m_graph._replays.steps)
    h_hand, p_hand = _hand_loop({"target": tgt}, **kw)
    assert h_hand == h_eager and np.array_equal(p_hand, p_eager)
    assert set(h_eager) == {"loss", "binary_accuracy", "tower_loss", "tower_accuracy", "val_loss", "val_binary_accuracy",
                            "val_tower_loss", "val_tower_accuracy"}
    assert all(np.isfinite(v).all() for v in h_eager.values()) and 0 <= h_eager["tower_accuracy"][-1] <= 1
    n_tr = keras_split_at(FIT_B, FIT_VAL)
    xv = {k: v[n_tr:] for k, v in x.items()}
    ev = model.evaluate(xv, {"target": tgt[n_tr:]})
    assert ev == [h_eager[k][-1] for k in ("val_loss", "val_binary_accuracy", "val_tower_loss", "val_tower_accuracy")]
    d = model.evaluate(xv, {"target": tgt[n_tr:]}, return_dict=True)
    assert d["tower_loss"] == ev[2] and d["tower_accuracy"] == ev[3] and d["binary_accuracy"] == ev[1]
    assert d["tower_accuracy"] == (d["tower_tp"] + d["tower_tn"]) / d["towers"]      # derived labels: evaluate()'s table


def test_fit_with_explicit_and_tower_only_labels():
    """y['tower_target'] with and without 'target': the eager per-batch steps equal the hand loop bit for bit;
    tower-only labels train (the parameters move, the history is finite) and report a zero node row."""
    x, tgt, tt = _fit_data()
    kw = dict(tower_loss=MU, node_loss=ALPHA)
    for y in ({"target": tgt, "tower_target": tt}, {"tower_target": tt}):
        h, p, model = _fit(False, y, **kw)
        h_hand, p_hand = _hand_loop(y, **kw)
        assert h == h_hand and np.array_equal(p, p_hand)
        assert all(np.isfinite(v).all() for v in h.values()) and h["tower_loss"][-1] > 0
    assert h["binary_accuracy"] == [0.0, 0.0] and h["loss"] == [MU * v for v in h["tower_loss"]]
    p0 = PropagationNetwork(seed=4, **kw).getModel(FIT_N).net.flat.detach().cpu().numpy()
    assert not np.array_equal(p, p0)


def test_tower_loss_zero_is_the_plain_model():
    """tower_loss = 0 (any node_loss): the history and the parameters of today's fit, bit for bit; tower targets
    are refused."""
    x, tgt, tt = _fit_data()
    y = {"target": tgt[..., None]}
    h0, p0, m0 = _fit(False, y)
    h1, p1, m1 = _fit(False, y, tower_loss=0.0, node_loss=0.3)
    assert h0 == h1 and np.array_equal(p0, p1) and m1.loss_parts is None
    assert set(h0) == {"loss", "binary_accuracy", "val_loss", "val_binary_accuracy"}
    with pytest.raises(ValueError):
        m1.fit(x, {"target": tgt, "tower_target": tt}, epochs=1, verbose=0)
    _, p2, _ = _fit(False, y, tower_loss=MU)
    assert not np.array_equal(p0, p2)


def test_weighted_fit_and_evaluate_with_tower_loss():
    """fit(sample_weight=, class_weight=) on a tower-loss model — the eager per-batch steps with weights, the
    weighted validation — equals the hand loop with keras_api.node_weights bit for bit, derived and explicit
    labels; a masked tower leaves the tower count; evaluate(sample_weight=) returns the validation numbers."""
    from spwgnn_amd.keras_api import node_weights
    x, tgt, tt = _fit_data()
    sw = np.random.default_rng(11).choice([0.0, 0.5, 1.0, 2.5], size=FIT_B, p=[0.3, 0.25, 0.25, 0.2])
    sw[0], sw[35] = 0.0, 0.0
    cw = {0: 2.0, 1: 0.5}
    W = node_weights(tgt, sw, cw)
    kw = dict(tower_loss=MU, node_loss=ALPHA)
    n_tr = keras_split_at(FIT_B, FIT_VAL)
    for y in ({"target": tgt}, {"target": tgt, "tower_target": tt}):
        h, p, model = _fit(False, y, dict(sample_weight=sw, class_weight=cw), **kw)
        h_hand, p_hand = _hand_loop(y, W, **kw)
        assert h == h_hand and np.array_equal(p, p_hand)
        assert all(np.isfinite(v).all() for v in h.values())
    assert float(model.loss_parts[5]) == np.count_nonzero(sw[n_tr:]) < FIT_B - n_tr       # the validation towers that count
    h, p, model = _fit(False, {"target": tgt}, dict(sample_weight=sw), **kw)
    xv = {k: v[n_tr:] for k, v in x.items()}
    ev = model.evaluate(xv, {"target": tgt[n_tr:]}, sample_weight=sw[n_tr:])
    assert ev == [h[k][-1] for k in ("val_loss", "val_binary_accuracy", "val_tower_loss", "val_tower_accuracy")]
    with pytest.raises(ValueError):
        model.fit(x, {"tower_target": tt}, class_weight=cw, epochs=1, verbose=0)           # class weights go by node targets


def test_tower_bce_with_weights_targets_and_divisor():
    """tower_bce with node weights, explicit tower targets and a given norm_t: the loss and the flat gradient of
    the engine calls with the same arguments, bit for bit."""
    params = O.random_params(3)
    (plan,), (t,) = _plans(1, B=8, N=5)
    b = TowerBatch.from_plan(plan, DEV)
    w = dev(np.random.default_rng(2).choice([0.0, 0.5, 2.0], size=40))
    tt = dev(np.arange(8) % 2)
    net = GraphNetwork(mp_steps=3, dropout=0.0, params=params, math="x6")
    L = tower_bce(net.forward_batch(b), dev(t), b, MU, ALPHA, tower_targets=tt, node_weights=w, norm=17.0, norm_t=5.0)
    L.backward()
    flat = P.to_flat(params, device=DEV)
    ws, sc = E.Workspace(DEV), E.TowerLossScratch(DEV)
    run = E.RunConfig(3, training=True, math="x6")
    o3, dz = E.bce_tower(E.forward(flat, b, run, ws), dev(t), b, sc, MU, ALPHA, tower_targets=tt, node_weights=w,
                         norm=17.0, norm_t=5.0)
    g, _ = E.backward(flat, b, run, ws, dz)
    assert float(L.detach()) == float(o3[0]) and torch.equal(net.flat.grad, g)


def test_replay_follows_each_plans_own_towers():
    """Two ragged plans of ONE replay geometry with different tower sizes, replayed a, b, a (eager, then the
    captured graphs): the tower loss walks each plan's own towers — offsets and divisor ride in the uploaded
    block — so parameters and moments equal Trainer.step on the same plans, bit for bit."""
    from test_tower_loss_host import same_geometry_plans
    pa, pb = same_geometry_plans()
    assert pa.geometry == pb.geometry and not np.array_equal(pa.tower_nodes, pb.tower_nodes)
    params = O.random_params(12)
    rng = np.random.default_rng(1)
    seq = [(p, (rng.random(p.n_nodes) < 0.85).astype(np.float32)) for p in (pa, pb, pa, pb)]
    ta = Trainer(P.to_flat(params, device=DEV), mp_steps=3, dropout=0.1, seed=5, tower_loss=MU, node_loss=ALPHA)
    parts = []
    for p, t in seq:
        ta.step(TowerBatch.from_plan(p, DEV), dev(t))
        parts.append(ta.loss_parts.clone())
    assert not torch.equal(parts[0], parts[1])
    tb = Trainer(P.to_flat(params, device=DEV), mp_steps=3, dropout=0.1, seed=5, tower_loss=MU, node_loss=ALPHA)
    rs = ReplayStep(pa, DEV, tb.replay_body(pa.n_nodes))
    assert rs.static.towers
    for (p, t), want in zip(seq, parts):
        tb.replay_step(rs, p, t)
        assert torch.equal(tb.engine.path.tower.out6, want)
    torch.cuda.synchronize()
    assert rs.replays == 3
    assert torch.equal(ta.params, tb.params) and torch.equal(ta.m, tb.m) and torch.equal(ta.v, tb.v)


def test_trainer_evaluate_hip_engine_with_tower_loss():
    """Trainer(tower_loss=).evaluate on the HIP engine: two micro-batches, weighted and with explicit tower
    targets, against one engine.bce_tower launch on the whole batch's logits; the parameters do not move."""
    S, cuts = 3, [(0, 4), (4, 7)]
    obj, Rs, Rr, prop, tgt = D.synthetic_batch(7, 5, seed=9, fully_connected=False)
    tgt = (np.random.default_rng(1).random((7, 5)) < 0.85).astype(np.float32)
    flat = P.to_flat(O.random_params(11), device=DEV)
    before = flat.clone()
    full = TowerBatch.from_dense(obj, Rs, Rr, device=DEV)
    batches = [TowerBatch.from_dense(obj[a:b], Rs[a:b], Rr[a:b], device=DEV) for a, b in cuts]
    z = E.forward(flat, full, E.RunConfig(S), E.Workspace(DEV))
    W = np.random.default_rng(2).choice(np.array([0.0, 0.5, 2.0], np.float32), size=(7, 5))
    W[1] = 0.0
    tt = np.array([1, 0, 1, 1, 0, 0, 1], np.float32)
    tr = Trainer(flat, mp_steps=S, dropout=0.0, tower_loss=MU, node_loss=ALPHA)
    for w, t_ in ((None, None), (W, tt)):
        sc = E.TowerLossScratch(DEV)
        E.bce_tower(z, dev(tgt.reshape(-1)), full, sc, MU, ALPHA, tower_targets=dev(t_),
                    node_weights=None if w is None else dev(w.reshape(-1)), want_dlogits=False)
        o = sc.out6.tolist()
        d = tr.evaluate(batches, [dev(tgt[a:b].reshape(-1)) for a, b in cuts],
                        weights=None if w is None else [dev(w[a:b].reshape(-1)) for a, b in cuts],
                        tower_targets=None if t_ is None else [dev(t_[a:b]) for a, b in cuts])
        # fp32 losses of two batches against one: tests/test_gpu_eval.py's 1e-6
        assert abs(d["tower_loss"] - o[3]) <= 1e-6 * o[3] and abs(d["loss"] - (ALPHA * o[0] + MU * o[3])) <= 1e-6 * d["loss"]
        assert d["tower_accuracy"] == o[4] / o[5] and d["n"] == o[2] and d["towers"] == o[5]
        assert d["tp"] + d["tn"] == o[1]
    only = tr.evaluate(batches, [None, None], tower_targets=[dev(tt[a:b]) for a, b in cuts])
    assert set(only) == {"loss", "tower_loss", "tower_accuracy"} and np.isfinite(only["loss"])
    assert torch.equal(flat, before) and tr.iterations == 0
