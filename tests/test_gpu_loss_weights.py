"""GPU: per-node loss weights — spwgnn_bce_weighted / spwgnn_bce_backward_weighted (added within ABI 8)
through engine.bce / engine.bce_backward, the replayed step and KerasModel.fit.

Keras 2.x weighted_masked_objective with the caller's divisor: loss = Σ w·bce / norm, dlogits =
w·(σ(z) − t) / norm, a zero weight a mask (model.fit's sample_weight / class_weight, src/main.py:92-98;
the loss itself Networks.py:102). Checked: the loss kernels against fp64 at every launch shape; w ≡ 1 with
norm = n against the unweighted calls bit for bit; the one-call form against bce + backward bit for bit; a
device norm against a by-value one; masked nodes (flipped and NaN targets) leaving every output untouched;
the gradients against the fp64 oracle; fit against a hand loop of train_on_batch."""
import functools

import numpy as np
import pytest
import torch

from oracle import model as O
from spwgnn_amd import data as D, engine as E, params as P
from spwgnn_amd.batch import TowerBatch
from spwgnn_amd.keras_api import CompactDataset, PropagationNetwork, keras_split_at, node_weights

pytestmark = pytest.mark.gpu

WEIGHT_VALUES = np.array([0.0, 0.5, 1.0, 2.5], np.float32)


def draw_weights(seed, shape):
    """Weights from {0, 0.5, 1, 2.5}, about 30 % zeros, seeded."""
    return np.random.default_rng(seed).choice(WEIGHT_VALUES, size=shape, p=[0.3, 0.25, 0.25, 0.2]).astype(np.float32)


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def ref_weighted_bce(z32, t, w, norm):
    """fp64: (loss, correct among w != 0, #{w != 0}, dlogits) of the weighted loss on fp32 logits."""
    z64, t, w = np.asarray(z32, np.float64), np.asarray(t, np.float64), np.asarray(w, np.float64)
    z = np.clip(z64, -O.LOGIT_CLIP, O.LOGIT_CLIP)
    per = np.maximum(z, 0) - z * t + np.log1p(np.exp(-np.abs(z)))
    on = w != 0
    loss = np.where(on, w * per, 0.0).sum() / norm
    correct = int((on & ((z64 > 0).astype(np.float64) == t)).sum())
    g = np.where(on & (np.abs(z64) < O.LOGIT_CLIP), w * (1.0 / (1.0 + np.exp(-z64)) - t) / norm, 0.0)
    return float(loss), correct, int(on.sum()), g


# ---------------------------------------------------------------- 1. the loss kernels alone
@pytest.mark.parametrize("n", [18, 256, 257, 70000])
def test_weighted_loss_kernels_against_fp64(n):
    """n = 18 under one wave, 256 one workgroup exactly (the single-launch form), 257 two workgroups with one
    node in the second, 70,000 the 256 capped workgroups with a grid stride. 1e-6: an fp32 emulation of this
    reduction (per-thread strided sums, 256-wide tree, fp64 final) stays within 4e-8 relative at these sizes
    with these weights; expf / log1pf add a few ulp per term. The counts are exact."""
    rng = np.random.default_rng(n)
    z = rng.normal(scale=3.0, size=n).astype(np.float32)
    assert np.abs(z).min() > 1e-6          # sigmoid(z) > 0.5 <=> z > 0 in fp32 too
    t = rng.integers(0, 2, n).astype(np.float32)
    w = draw_weights(n + 1, n)
    norm = max(int(np.count_nonzero(w)), 1)
    loss, correct, count, g = ref_weighted_bce(z, t, w, norm)
    out3, dz = E.bce(dev(z), dev(t), E.BceScratch("cuda"), node_weights=dev(w))   # norm counted
    o, dz = out3.cpu().numpy().astype(np.float64), dz.cpu().numpy().astype(np.float64)
    print(f"n={n}: loss {o[0]:.9g} ref {loss:.9g} rel {abs(o[0] - loss) / max(1, abs(loss)):.2e}; "
          f"dlogits max err {np.abs(dz - g).max():.2e} of {np.abs(g).max():.2e}")
    assert abs(o[0] - loss) <= 1e-6 * max(1.0, abs(loss))
    assert np.abs(dz - g).max() <= 1e-6 * np.abs(g).max()
    assert o[1] == correct and o[2] == count == norm
    assert np.all(dz[w == 0] == 0.0)


@pytest.mark.parametrize("n", [192, 70000])
def test_weighted_accumulate_equals_host_sums(n):
    """The accumulating form (total3 += out3·weights3 in the loss launch) with weights: the same out3 and
    dlogits as without total3, and total3 equal to the host's fp64 Σ out3·weights3 over two batches, bit for
    bit (tests/test_gpu_training.py::test_bce_accumulate_equals_bce_then_accumulate, weighted)."""
    rng = np.random.default_rng(n)
    w3 = torch.tensor([float(n), 1.0, 1.0], dtype=torch.float64, device="cuda")
    tot = torch.zeros(3, dtype=torch.float64, device="cuda")
    host = np.zeros(3)
    for k in range(2):
        z, t = dev(rng.normal(scale=3.0, size=n)), dev(rng.integers(0, 2, n))
        w = dev(draw_weights(n + k, n))
        oa, da = E.bce(z, t, E.BceScratch("cuda"), total3=tot, weights3=w3, node_weights=w)
        ob, db = E.bce(z, t, E.BceScratch("cuda"), node_weights=w)
        torch.cuda.synchronize()
        assert torch.equal(oa, ob) and torch.equal(da, db)
        host += oa.double().cpu().numpy() * w3.cpu().numpy()
    assert np.array_equal(tot.cpu().numpy(), host)


# ---------------------------------------------------------------- shared batches
@functools.lru_cache(maxsize=None)
def _problem(B, N, fully):
    obj, Rs, Rr, prop, tgt = D.synthetic_batch(B, N, seed=5, fully_connected=fully)
    batch = TowerBatch.from_dense(obj, Rs, Rr, prop, device="cuda")
    flat = P.to_flat(O.random_params(2), device="cuda")
    return batch, flat, tgt.reshape(-1).astype(np.float32)


def _run(math, split=False):
    run = E.RunConfig(5, training=True, math=math, dropout=0.1, seed=3)
    if split:
        run.grads_early_event = torch.cuda.Event()
        run.grads_early_event.record()
    return run


def _bce_backward(batch, flat, run, t, B, **kw):
    """forward + bce_backward with the epoch sums and d/d'propagation': every output, cloned."""
    ws, sc = E.Workspace("cuda"), E.BceScratch("cuda")
    tot = torch.zeros(3, dtype=torch.float64, device="cuda")
    w3 = torch.tensor([float(B), 1.0, 1.0], dtype=torch.float64, device="cuda")
    z = E.forward(flat, batch, run, ws)
    o3, dz, g, dp = E.bce_backward(flat, batch, run, ws, z, t, sc, total3=tot, weights3=w3, want_dprop=True, **kw)
    torch.cuda.synchronize()
    return {"out3": o3.clone(), "total3": tot.clone(), "dlogits": dz.clone(), "grads": g.clone(), "dprop": dp.clone()}


def _assert_same(a, b):
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------- 2. w ≡ 1, norm = n: the unweighted bits
@pytest.mark.parametrize("n", [18, 256, 257, 70000])
def test_unit_weights_bce_equals_unweighted_bitwise(n):
    rng = np.random.default_rng(n)
    z, t = dev(rng.normal(scale=3.0, size=n)), dev(rng.integers(0, 2, n))
    oa, da = E.bce(z, t, E.BceScratch("cuda"))
    ob, db = E.bce(z, t, E.BceScratch("cuda"), node_weights=torch.ones(n, device="cuda"), norm=n)
    torch.cuda.synchronize()
    assert torch.equal(oa, ob) and torch.equal(da, db)


@pytest.mark.parametrize("B,N,math", [(32, 6, "x6"), (32, 6, "bf16"), (64, 12, "x6"), (3000, 6, "x6")])
def test_unit_weights_bce_backward_equals_unweighted_bitwise(B, N, math):
    """(32, 6): the unweighted call folds the loss into the fused backward; (64, 12): n = 768, the loss launch
    first; (3000, 6): the wide kernels. out3, the epoch sums, dlogits, every gradient and d/d'propagation'."""
    batch, flat, tgt = _problem(B, N, False)
    t = dev(tgt)
    a = _bce_backward(batch, flat, _run(math), t, B)
    b = _bce_backward(batch, flat, _run(math), t, B, node_weights=torch.ones(B * N, device="cuda"), norm=B * N)
    _assert_same(a, b)


# ---------------------------------------------------------------- 3. one call == bce + backward
@pytest.mark.parametrize("B,N,fully,math,split", [(32, 6, False, "x6", False), (32, 6, False, "bf16", False),
                                                   (40, 6, True, "x6", True), (3000, 6, False, "x6", False),
                                                   (64, 12, True, "x6", False)])
def test_weighted_bce_backward_equals_bce_then_backward(B, N, fully, math, split):
    """The grid of tests/test_gpu_training.py::test_bce_backward_equals_bce_then_backward, weighted."""
    batch, flat, tgt = _problem(B, N, fully)
    t, w = dev(tgt), dev(draw_weights(B, B * N))
    run = _run(math, split)
    one = _bce_backward(batch, flat, run, t, B, node_weights=w)
    ws, sc = E.Workspace("cuda"), E.BceScratch("cuda")
    tot = torch.zeros(3, dtype=torch.float64, device="cuda")
    w3 = torch.tensor([float(B), 1.0, 1.0], dtype=torch.float64, device="cuda")
    z = E.forward(flat, batch, run, ws)
    o3, dz = E.bce(z, t, sc, total3=tot, weights3=w3, node_weights=w)
    g, dp = E.backward(flat, batch, run, ws, dz, want_dprop=True)
    torch.cuda.synchronize()
    _assert_same(one, {"out3": o3, "total3": tot, "dlogits": dz, "grads": g, "dprop": dp})
    assert float(o3[2]) == float(torch.count_nonzero(w)) and float(o3[0]) > 0


# ---------------------------------------------------------------- 4. device norm == by-value norm
@pytest.mark.parametrize("B,N", [(32, 6), (3000, 6)])
def test_device_norm_equals_value_norm_bitwise(B, N):
    batch, flat, tgt = _problem(B, N, False)
    t, w = dev(tgt), dev(draw_weights(B + 1, B * N))
    norm = int(torch.count_nonzero(w))
    a = _bce_backward(batch, flat, _run("x6"), t, B, node_weights=w, norm=norm)
    b = _bce_backward(batch, flat, _run("x6"), t, B, node_weights=w, norm=torch.tensor([float(norm)], device="cuda"))
    c = _bce_backward(batch, flat, _run("x6"), t, B, node_weights=w)   # counted
    _assert_same(a, b)
    _assert_same(a, c)


# ---------------------------------------------------------------- 5. a zero weight is a mask
@pytest.mark.parametrize("B,N", [(32, 6), (3000, 6)])
def test_masked_nodes_reach_nothing(B, N):
    """Targets flipped on half of the zero-weight nodes and NaN on the other half: out3, the epoch sums, every
    gradient and d/d'propagation' keep their bits, dlogits too, and are exactly 0 at the masked nodes."""
    batch, flat, tgt = _problem(B, N, False)
    w = draw_weights(B + 2, B * N)
    masked = np.flatnonzero(w == 0)
    assert len(masked) >= 4
    bad = tgt.copy()
    bad[masked[::2]] = 1.0 - bad[masked[::2]]
    bad[masked[1::2]] = np.nan
    a = _bce_backward(batch, flat, _run("x6"), dev(tgt), B, node_weights=dev(w))
    b = _bce_backward(batch, flat, _run("x6"), dev(bad), B, node_weights=dev(w))
    _assert_same(a, b)
    assert not torch.isnan(b["grads"]).any() and not torch.isnan(b["out3"]).any()
    assert torch.all(b["dlogits"][dev(masked, torch.long)] == 0)
    assert torch.count_nonzero(b["dlogits"]) > 0


# ---------------------------------------------------------------- 6. gradients against the fp64 oracle
@functools.lru_cache(maxsize=None)
def _oracle_case():
    B, N, S = 4, 6, 3
    params = O.random_params(seed=1)
    obj, Rs, Rr, prop, tgt = D.synthetic_batch(B, N, seed=3, fully_connected=False)
    W = draw_weights(7, (B, N))
    W[2] = 0.0                                   # one tower fully masked
    W[0, 0], W[1, 1] = 2.5, 0.5
    norm = float(np.count_nonzero(W))
    tp = O.to_torch(params, requires_grad=True)
    z = O.forward_dense(tp, *(torch.as_tensor(a, dtype=torch.float64) for a in (obj, Rs, Rr, prop)), S)
    t, w = torch.as_tensor(tgt, dtype=torch.float64).reshape(B, N), torch.as_tensor(W, dtype=torch.float64)
    zc = torch.clamp(z, -O.LOGIT_CLIP, O.LOGIT_CLIP)
    per = torch.clamp(zc, min=0) - zc * t + torch.log1p(torch.exp(-torch.abs(zc)))
    loss = torch.where(w != 0, w * per, torch.zeros_like(per)).sum() / norm
    loss.backward()
    ref = {k: v.grad.numpy().copy() for k, v in tp.items()}
    return params, (obj, Rs, Rr, prop), tgt, W, float(loss.detach()), ref


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("math", ["f32", "x6"])
def test_weighted_gradients_against_fp64_oracle(math, wide):
    """B = 4, N = 6, S = 3, thresholded relations, one tower fully masked: the weighted loss written in torch
    fp64 on oracle.forward_dense; max|Δ| <= 1e-5·max|ref| + 1e-7 per tensor and the loss to 1e-5 (the
    project's fp32 parity criterion), on the team kernels and the wide ones."""
    params, dense, tgt, W, loss_ref, ref = _oracle_case()
    batch = TowerBatch.from_dense(*dense, device="cuda")
    flat = P.to_flat(params, device="cuda")
    run = E.RunConfig(3, training=True, math=math)

    def go():
        ws = E.Workspace("cuda")
        z = E.forward(flat, batch, run, ws)
        return E.bce_backward(flat, batch, run, ws, z, dev(tgt.reshape(-1)), E.BceScratch("cuda"),
                              node_weights=dev(W.reshape(-1)))
    if wide:
        with E.wide_kernels():
            out3, dz, grads, _ = go()
    else:
        out3, dz, grads, _ = go()
    torch.cuda.synchronize()
    assert abs(float(out3[0]) - loss_ref) <= 1e-5
    assert float(out3[2]) == np.count_nonzero(W)
    assert torch.all(dz.reshape(4, 6)[2] == 0)
    g = P.from_flat(grads)
    for k, r in ref.items():
        err = np.abs(g[k] - r).max()
        assert err <= 1e-5 * np.abs(r).max() + 1e-7, (k, err, np.abs(r).max())


# ---------------------------------------------------------------- the Trainer's replayed weighted step
def test_trainer_weighted_replay_equals_weighted_step():
    """Trainer.replay_body(weighted=True) replayed over three batches of one geometry (weights and their
    divisor uploaded with the batch, the divisor read from the device) == Trainer.step(weights=) on the same
    batches (the divisor by value, loss then backward), bit for bit: parameters and both Adam moments."""
    from spwgnn_amd.batch import HostPlan
    from spwgnn_amd.replay import ReplayStep
    from spwgnn_amd.trainer import Trainer
    params = O.random_params(12)
    plans, tgts, wts = [], [], []
    for seed in (1, 2, 3):
        raw = D.synthetic_towers(32, 6, seed=seed)
        obj = (raw / D.RELATION_THRESHOLD).astype(np.float32)
        Rs, Rr = D.relation_matrices(raw, D.RELATION_THRESHOLD)
        e = np.array(O.dense_to_edges(Rs, Rr), np.int64).reshape(-1, 4)
        te = np.bincount(e[:, 0], minlength=32).astype(np.int32)
        plans.append(HostPlan.build(obj.reshape(-1, 3), np.full(32, 6, np.int32), e[:, 0] * 6 + e[:, 2],
                                    e[:, 0] * 6 + e[:, 3], te, edge_cap=30))
        tgts.append(np.random.default_rng(seed).integers(0, 2, 192).astype(np.float32))
        wts.append(draw_weights(seed + 20, 192))
    ta = Trainer(P.to_flat(params, device="cuda"), mp_steps=5, dropout=0.1, seed=11, math="x6")
    for p, t, w in zip(plans, tgts, wts):
        out3 = ta.step(TowerBatch.from_plan(p, "cuda"), dev(t), weights=dev(w))
    assert float(out3[2]) == np.count_nonzero(wts[-1])
    tb = Trainer(P.to_flat(params, device="cuda"), mp_steps=5, dropout=0.1, seed=11, math="x6")
    rs = ReplayStep(plans[0], "cuda", tb.replay_body(plans[0].n_nodes, weighted=True), weighted=True)
    for p, t, w in zip(plans, tgts, wts):
        tb.replay_step(rs, p, t, w)
    torch.cuda.synchronize()
    assert rs.replays == 2 and tb.iterations == 3
    assert torch.equal(ta.params, tb.params) and torch.equal(ta.m, tb.m) and torch.equal(ta.v, tb.v)


# ---------------------------------------------------------------- 7. fit
FIT_B, FIT_N, FIT_BATCH, FIT_EPOCHS, FIT_VAL = 40, 5, 16, 2, 0.2
CLASS_WEIGHT = {0: 2.0, 1: 0.5}


@functools.lru_cache(maxsize=None)
def _fit_data():
    obj, Rs, Rr, prop, tgt = D.synthetic_batch(FIT_B, FIT_N, seed=7, fully_connected=False)
    x = {"objects": obj, "sender_relations": Rs, "receiver_relations": Rr, "propagation": prop}
    sw = draw_weights(11, FIT_B)
    sw[0], sw[35] = 0.0, 0.0           # masked towers in the training and the validation part
    return x, {"target": tgt.reshape(FIT_B, FIT_N, 1)}, sw


def _fit(graph, **kw):
    x, y, _ = _fit_data()
    model = PropagationNetwork(seed=4).getModel(FIT_N)
    h = model.fit(x, y, batch_size=FIT_BATCH, epochs=FIT_EPOCHS, validation_split=FIT_VAL, verbose=0, graph=graph, **kw)
    torch.cuda.synchronize()
    return h, model.net.flat.detach().cpu().numpy().copy(), model


def test_weighted_fit_equals_hand_loop_and_replay():
    """fit with sample_weight (B,) and class_weight, validation_split 0.2: history and final parameters equal
    a hand loop of weighted train_on_batch + evaluate_batch over the same batches bit for bit (the comparison
    tests/test_gpu_replay.py makes unweighted), and graph=True equals graph=False."""
    x, y, sw = _fit_data()
    h_eager, p_eager, m_eager = _fit(False, sample_weight=sw, class_weight=CLASS_WEIGHT)
    h_graph, p_graph, m_graph = _fit(True, sample_weight=sw, class_weight=CLASS_WEIGHT)
    assert h_eager == h_graph and np.array_equal(p_eager, p_graph)
    assert sum(s.replays for s in m_graph._replays.steps.values()) == 4 - len(m_graph._replays.steps)
    assert all(s.static.weighted for s in m_graph._replays.steps.values())
    # the hand loop
    tgt = y["target"].reshape(FIT_B, FIT_N)
    W = node_weights(tgt, sw, CLASS_WEIGHT)
    n_tr = keras_split_at(FIT_B, FIT_VAL)
    assert n_tr == 32
    ds = CompactDataset(x["objects"], x["sender_relations"], x["receiver_relations"], x["propagation"])
    model = PropagationNetwork(seed=4).getModel(FIT_N)
    vbatch = ds.subset(np.arange(n_tr, FIT_B), "cuda")
    rng = np.random.default_rng(0)
    hist = {"loss": [], "binary_accuracy": [], "val_loss": [], "val_binary_accuracy": []}
    for _ in range(FIT_EPOCHS):
        order = rng.permutation(n_tr)
        tot = np.zeros(3)
        for b0 in range(0, n_tr, FIT_BATCH):
            idx = order[b0:b0 + FIT_BATCH]
            batch = TowerBatch.from_plan(ds.subset_plan(idx, edge_cap=True), "cuda")
            out3 = model.train_on_batch(batch, dev(tgt[idx].reshape(-1)), node_weights=W[idx])
            tot += out3.double().cpu().numpy() * np.array([float(len(idx)), 1.0, 1.0])
        hist["loss"].append(tot[0] / n_tr)
        hist["binary_accuracy"].append(tot[1] / tot[2])
        vl, vc, vn = model.evaluate_batch(vbatch, dev(tgt[n_tr:].reshape(-1)), node_weights=W[n_tr:]).tolist()
        hist["val_loss"].append(vl)
        hist["val_binary_accuracy"].append(vc / vn)
    torch.cuda.synchronize()
    assert hist == h_eager
    assert np.array_equal(model.net.flat.detach().cpu().numpy(), p_eager)
    assert 0 < hist["binary_accuracy"][0] <= 1


def test_fit_with_unit_sample_weight_equals_fit_without():
    h0, p0, m0 = _fit(False)
    h1, p1, m1 = _fit(False, sample_weight=np.ones(FIT_B))
    assert h0 == h1 and np.array_equal(p0, p1)
    assert not any(s.static.weighted for s in m0._replays.steps.values())
    # and the weights of the other test do change the trajectory
    _, _, sw = _fit_data()
    _, p2, _ = _fit(False, sample_weight=sw, class_weight=CLASS_WEIGHT)
    assert not np.array_equal(p0, p2)
