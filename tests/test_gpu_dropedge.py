"""GPU: DropEdge — `engine.dropedge_gates` (spwgnn_dropedge_gates, k_dropedge) bit for bit against the numpy
restatement of its key (tests/dropedge_ref.py), and the front ends that train with it: `Trainer(dropedge=)` against
the fp64 gated oracle (tests/relation_gates_ref.py) with the restated mask, the replayed step against the eager one,
`fit(graph=True)` against `fit(graph=False)`, and `dropedge=0` against the calls of before.

Criteria of the oracle step (x6): loss |Δ| <= 1e-5·(1 + |L|); every parameter tensor's gradient max|Δ| <= 1e-5·max|ref|
+ 1e-8 (the project's gradient criterion, tests/test_gpu_relation_gates.py). ReLU kinks: the Trainer's seed is picked
on the CPU so that under the step's mask every tower's gated margin exceeds GR.TAU — no tower is left out — and the
mask holds kept and dropped edges."""
import numpy as np
import pytest
import torch

import dropedge_ref as REF
import relation_gates_ref as GR
import test_gpu_input_grad as IG
from oracle import model as O
from spwgnn_amd import GraphNetwork, TowerBatch, _lib, data as D, engine as E, params as P
from spwgnn_amd.batch import HostPlan
from spwgnn_amd.keras_api import PropagationNetwork
from spwgnn_amd.replay import ReplayStep
from spwgnn_amd.trainer import Trainer, dropout_key

pytestmark = pytest.mark.gpu

DEV = "cuda"
RATE = 0.25
KEY = 0x1234_5678_9ABC_DEF1


# ------------------------------------------------------------------------------------ the mask, bit for bit
def _ragged_batch(pack, edge_cap=None):
    sizes = np.array([1, 2, 4, 7, 3], np.int32)
    off = np.concatenate([[0], np.cumsum(sizes)])
    src, dst = [], []
    for t, n in enumerate(sizes):
        m, j = np.nonzero(~np.eye(n, dtype=bool))
        src.append(off[t] + m)
        dst.append(off[t] + j)
    src, dst = np.concatenate(src).astype(np.int32), np.concatenate(dst).astype(np.int32)
    pos = np.random.default_rng(0).random((int(off[-1]), 3)).astype(np.float32)
    plan = HostPlan.build(pos, sizes, src, dst, (sizes * (sizes - 1)).astype(np.int32), pack=pack, edge_cap=edge_cap)
    return TowerBatch.from_plan(plan, DEV)


def _device_batch():
    """A capacity plan filled on the device from positions: thresholded relations, whole blocks of padding."""
    raw = torch.as_tensor(D.synthetic_towers(6, 6, seed=3), dtype=torch.float32, device=DEV)
    return TowerBatch.from_positions(raw, threshold=D.RELATION_THRESHOLD, check=True)


def _mask_batch(kind):
    if kind == "host":
        c = IG._case("team_b")
        return TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], device=DEV)
    if kind == "packed":
        b = _ragged_batch(True)
        assert b.node_perm is not None and not np.array_equal(b.node_perm, np.arange(b.n_nodes))
        return b
    if kind == "capacity":
        return _ragged_batch(False, edge_cap=64)
    return _device_batch()


@pytest.mark.parametrize("kind", ["host", "packed", "capacity", "device"])
def test_mask_equals_the_numpy_restatement(kind):
    batch = _mask_batch(kind)
    pad = ((batch.edge_src < 0) | (batch.edge_dst < 0)).cpu().numpy()
    assert (~pad).sum() > 0
    if kind == "capacity":
        assert pad.reshape(-1, 32).all(axis=1).any()      # an all-padding block
    if kind == "device":
        assert pad.sum() > 32                             # unused capacity
    key_dev = torch.tensor([KEY], dtype=torch.int64, device=DEV)
    base = torch.linspace(-1.0, 2.0, 32 * batch.n_eblocks, device=DEV)
    base[pad] = float("nan")                              # a padding slot is 0 whatever its base holds
    some_dropped = False
    for run, key in ((E.RunConfig(seed=KEY), KEY), (E.RunConfig(seed=5, seed_dev=key_dev), KEY), (E.RunConfig(seed=7), 7)):
        for sym in (True, False):
            for rescale in (False, True):
                got = E.dropedge_gates(batch, run, RATE, symmetric=sym, rescale=rescale).cpu().numpy()
                want = REF.batch_gates(batch, key, RATE, sym, rescale)
                assert np.array_equal(got.view(np.int32), want.view(np.int32)), (kind, key, sym, rescale)
                assert np.all(got[pad].view(np.int32) == 0)
                assert set(np.unique(got[~pad])) <= {np.float32(0), REF.scale(RATE, rescale)}
                some_dropped |= bool((got[~pad] == 0).any()) and bool((got[~pad] != 0).any())
        got = E.dropedge_gates(batch, run, RATE, base=base).cpu().numpy()
        want = REF.batch_gates(batch, key, RATE, True, False, base)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)) and np.all(got[pad].view(np.int32) == 0)
    assert some_dropped
    # rate 0 keeps every edge; the caller's buffer is the one written
    out = torch.full((32 * batch.n_eblocks,), 9.0, device=DEV)
    assert E.dropedge_gates(batch, E.RunConfig(seed=KEY), 0.0, out=out) is out
    assert np.array_equal(out.cpu().numpy(), (~pad).astype(np.float32))


def test_symmetric_mask_is_symmetric_per_contact():
    c = IG._case("wide")
    batch = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], device=DEV)
    g = E.dropedge_gates(batch, E.RunConfig(seed=KEY), 0.5)
    m = batch.edges_to_input(g, dense=True)
    assert np.array_equal(m, np.swapaxes(m, -1, -2)) and 0 < m.sum() < c["B"] * c["N"] * (c["N"] - 1)


def test_errors():
    c = IG._case("team_a")
    batch = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], device=DEV)
    run = E.RunConfig(seed=1)
    for bad in (1.0, -0.5, float("nan")):
        with pytest.raises(ValueError):
            E.dropedge_gates(batch, run, bad)
    with pytest.raises(ValueError):
        E.dropedge_gates(batch, run, RATE, out=torch.empty(7, device=DEV))
    with pytest.raises(ValueError):
        E.dropedge_gates(batch, run, RATE, base=torch.ones(7, device=DEV))
    for make in (lambda: GraphNetwork(device=DEV, math="bf16", dropedge=RATE),
                 lambda: PropagationNetwork(device=DEV, math="f32", dropedge=RATE),
                 lambda: PropagationNetwork(device=DEV, dropedge=RATE, step_loss_weights=(1.0,) * 5),
                 lambda: Trainer(P.to_flat(c["params"], device=DEV), math="bf16", dropedge=RATE)):
        with pytest.raises(ValueError):
            make()
    x = {"objects": c["obj"], "sender_relations": c["Rs"], "receiver_relations": c["Rr"],
         "relation_weights": np.ones((c["B"], c["N"], c["N"]), np.float32)}
    with pytest.raises(ValueError):
        PropagationNetwork(device=DEV, dropedge=RATE).getModel(c["N"]).fit(x, {"target": c["tgt"]}, verbose=0)


# ------------------------------------------------------------------------------------ one Trainer step against the oracle
def _oracle_case():
    """team_a with a zero propagation input (the Trainer's batches carry none) and the first Trainer seed whose
    step-0 mask leaves every tower's gated ReLU margin above TAU and holds kept and dropped edges."""
    c = dict(IG._case("team_a"))
    c["prop"] = np.zeros_like(c["prop"])
    N = c["N"]
    src, dst = np.asarray(c["src"], np.int64), np.asarray(c["dst"], np.int64)
    for seed in range(40):
        w = REF.keep(dropout_key(seed, 0, 0, 0), src // N, src % N, dst % N, RATE, True).astype(np.float32)
        if 0 < w.sum() < len(w) and np.all(GR.gated_margins(c, w) > GR.TAU):
            return c, seed, w
    raise AssertionError("no seed gives every tower a gated ReLU margin above TAU")


def test_trainer_step_against_the_gated_oracle():
    c, seed, w = _oracle_case()
    m = GR.gated_margins(c, w)
    print(f"Trainer seed {seed}: {int(w.sum())} of {len(w)} edges kept, gated ReLU margins min {m.min():.2e}")
    assert m.shape == (c["B"],) and np.all(m > GR.TAU)          # no tower left out
    ref = GR.oracle(c, w, "bce")
    batch = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], device=DEV)
    tr = Trainer(P.to_flat(c["params"], device=DEV), mp_steps=c["S"], dropout=0.0, seed=seed, math="x6", dropedge=RATE)
    out3 = tr.step(batch, torch.as_tensor(c["tgt"].reshape(-1), device=DEV))
    torch.cuda.synchronize()
    loss_ref = float(O.keras_bce_grad(ref["z"], c["tgt"].reshape(-1).astype(np.float64))[0])
    loss = float(out3[0])
    print(f"loss {loss:.7f} (fp64 {loss_ref:.7f})")
    assert abs(loss - loss_ref) <= 1e-5 * (1.0 + abs(loss_ref)) and int(out3[2]) == batch.n_nodes
    g = P.from_flat(tr.engine.grads)          # one whole batch: the engine's buffer holds the step's gradient
    for name in sorted(ref["g"]):
        got, want = np.asarray(g[name], np.float64), ref["g"][name]
        err, scale = np.abs(got - want).max(), np.abs(want).max()
        print(f"{name}: max|Δ| {err:.3e} = {err / scale:.2e} of max|ref|")
        assert err <= 1e-5 * scale + 1e-8, name
    assert tr.iterations == 1


# ------------------------------------------------------------------------------------ replayed == eager
def _xy(n, N, seed):
    obj, Rs, Rr, prop, tgt = D.synthetic_batch(n, N, seed=seed, fully_connected=False)
    return ({"objects": obj, "sender_relations": Rs, "receiver_relations": Rr}, {"target": tgt.reshape(n, N, 1)})


def test_fit_replayed_equals_eager_bitwise():
    """fit for 3 epochs of 2 batches, every step a replayed hipGraph, against the same fit issued eagerly: the final
    weights and the histories, bit for bit; and DropEdge changes them (against the same fit without it)."""
    x, y = _xy(16, 5, 7)
    res = []
    for graph, rate in ((True, RATE), (False, RATE), (False, 0.0)):
        model = PropagationNetwork(device=DEV, seed=0, mp_steps=3, dropedge=rate, dropedge_rescale=True).getModel(5)
        h = model.fit(x, y, batch_size=8, epochs=3, verbose=0, graph=graph, shuffle=False)
        torch.cuda.synchronize()
        res.append((h, model.net.flat.detach().cpu().numpy().copy(), model.iterations, model._replays))
    (ha, wa, ia, ra), (hb, wb, ib, rb), (hc, wc, _, _) = res
    assert ia == ib == 6 and ha == hb and np.array_equal(wa, wb)
    assert sum(s.replays for s in ra.steps.values()) == 6 - len(ra.steps)
    assert all(s.graph is None for s in rb.steps.values())
    assert np.all(np.isfinite(wa)) and not np.array_equal(wa, wc)


def test_fit_steps_equal_train_on_batch():
    """The replayed DropEdge step (device key word) draws the masks train_on_batch draws from the host key."""
    from spwgnn_amd.keras_api import CompactDataset
    x, y = _xy(16, 5, 9)
    ma = PropagationNetwork(device=DEV, seed=3, mp_steps=3, dropedge=RATE).getModel(5)
    ma.fit(x, y, batch_size=8, epochs=1, shuffle=False, verbose=0)
    mb = PropagationNetwork(device=DEV, seed=3, mp_steps=3, dropedge=RATE).getModel(5)
    ds = CompactDataset(x["objects"], x["sender_relations"], x["receiver_relations"], None)
    tgt = y["target"].reshape(16, 5)
    for b0 in (0, 8):
        idx = np.arange(b0, b0 + 8)
        batch = TowerBatch.from_plan(ds.subset_plan(idx, edge_cap=True), DEV)
        mb.train_on_batch(batch, torch.as_tensor(tgt[idx].reshape(-1), device=DEV))
    torch.cuda.synchronize()
    assert np.array_equal(ma.net.flat.detach().cpu().numpy(), mb.net.flat.detach().cpu().numpy())


def _plans(n):
    plans, tgts = [], []
    for seed in range(1, n + 1):
        raw = D.synthetic_towers(8, 6, seed=seed)
        obj = (raw / D.RELATION_THRESHOLD).astype(np.float32)
        Rs, Rr = D.relation_matrices(raw, D.RELATION_THRESHOLD)
        e = np.array(O.dense_to_edges(Rs, Rr), np.int64).reshape(-1, 4)
        te = np.bincount(e[:, 0], minlength=8).astype(np.int32)
        plans.append(HostPlan.build(obj.reshape(-1, 3), np.full(8, 6, np.int32), e[:, 0] * 6 + e[:, 2],
                                    e[:, 0] * 6 + e[:, 3], te, edge_cap=30))
        tgts.append(np.random.default_rng(seed).integers(0, 2, 48).astype(np.float32))
    return plans, tgts


def test_trainer_replay_equals_step():
    """Trainer.replay_body with DropEdge (splitmix key mode, dropout 0.1) replayed over three batches of one
    geometry == Trainer.step on the same batches, bit for bit."""
    plans, tgts = _plans(3)
    params = O.random_params(12)
    kw = dict(mp_steps=3, dropout=0.1, seed=11, math="x6", dropedge=RATE, dropedge_symmetric=False)
    ta = Trainer(P.to_flat(params, device=DEV), **kw)
    for p, t in zip(plans, tgts):
        ta.step(TowerBatch.from_plan(p, DEV), torch.as_tensor(t, device=DEV))
    tb = Trainer(P.to_flat(params, device=DEV), **kw)
    rs = ReplayStep(plans[0], DEV, tb.replay_body(plans[0].n_nodes))
    assert not rs.fold                      # a DropEdge body does not fold the prologue
    for p, t in zip(plans, tgts):
        tb.replay_step(rs, p, t)
    torch.cuda.synchronize()
    assert rs.replays == 2
    assert torch.equal(ta.params, tb.params) and torch.equal(ta.m, tb.m) and torch.equal(ta.v, tb.v)


# ------------------------------------------------------------------------------------ dropedge = 0 is the step of before
def test_dropedge_zero_is_the_plain_step_bitwise():
    """Trainer(dropedge=0) against the calls a step made before DropEdge existed — engine.forward, bce, backward,
    adam with the step's key, no gates anywhere — parameters and moments bit for bit over two steps."""
    plans, tgts = _plans(2)
    params = O.random_params(12)
    tr = Trainer(P.to_flat(params, device=DEV), mp_steps=3, dropout=0.1, seed=11, math="x6", dropedge=0.0)
    flat = P.to_flat(params, device=DEV)
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    ws, scratch = E.Workspace(DEV), E.BceScratch(DEV)
    for it, (p, t) in enumerate(zip(plans, tgts)):
        batch, tgt = TowerBatch.from_plan(p, DEV), torch.as_tensor(t, device=DEV)
        tr.step(batch, tgt)
        run = E.RunConfig(3, training=True, dropout=0.1, seed=dropout_key(11, it, 0, 0), math="x6")
        z = E.forward(flat, batch, run, ws)
        _, dz = E.bce(z, tgt, scratch)
        g, _ = E.backward(flat, batch, run, ws, dz)
        E.adam(flat, g, m, v, it + 1)
    torch.cuda.synchronize()
    assert torch.equal(tr.params, flat) and torch.equal(tr.m, m) and torch.equal(tr.v, v)


# ------------------------------------------------------------------------------------ GraphNetwork under autograd
def test_graph_network_draws_in_train_mode_only():
    """GraphNetwork(dropedge=) in train mode under autograd: the mask of the step's key times the relation weights,
    the gradient of a weights leaf masked with it; eval() and no-grad calls draw nothing."""
    c = IG._case("team_a")
    net = GraphNetwork(c["S"], dropout=0.0, device=DEV, params=c["params"], dropedge=0.5)
    plain = GraphNetwork(c["S"], dropout=0.0, device=DEV, params=c["params"])
    batch = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], device=DEV)
    w = torch.full((batch.n_edges,), 0.75, device=DEV, requires_grad=True)
    net.train()
    key = net._step_seed + 1
    z = net.forward_batch(batch, relation_weights=w)
    assert net._step_seed == key
    _, _, kept = batch.edges_to_input(REF.batch_gates(batch, key, 0.5))   # per relation, the input's edge order
    assert 0 < kept.sum() < len(kept)
    plain.train()
    wk = (w.detach() * torch.as_tensor(kept, device=DEV)).requires_grad_(True)
    want = plain.forward_batch(batch, relation_weights=wk)
    assert torch.equal(z.detach(), want.detach())
    z.sum().backward()
    want.sum().backward()
    gw = w.grad.cpu().numpy()
    assert np.all(gw[kept == 0] == 0) and np.any(gw[kept != 0] != 0)
    assert np.array_equal(gw[kept != 0], wk.grad.cpu().numpy()[kept != 0])
    assert torch.equal(net.flat.grad, plain.flat.grad)
    seed = net._step_seed
    net.eval()                       # eval(): nothing is drawn, under autograd too
    plain.eval()
    assert torch.equal(net.forward_batch(batch).detach(), plain.forward_batch(batch).detach())
    net.train()
    with torch.no_grad():            # no gradient wanted: an inference run
        assert torch.equal(net.forward_batch(batch), plain.forward_batch(batch))
    assert net._step_seed == seed
