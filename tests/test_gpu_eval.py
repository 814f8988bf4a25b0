"""GPU: spwgnn_eval_metrics and the evaluate() calls above it. Every table is compared as integers
with the numpy restatement tests/eval_ref.py. numpy's expf may differ from the device's by an ulp, so the cases keep
every finite logit's probability at least eval_ref.MARGIN from the threshold (asserted on the CPU before each launch),
except exact 0 at tau = 0.5, where p is exactly 0.5 in any arithmetic.

Shapes: n in {1, 255, 256, 257, 1000} — one node, either side of one 256-thread workgroup, several workgroups — with
R in {1, 5} rows; ragged towers of 1..32 nodes (all 32 sizes and a 40-node tower for bucket 0 at n = 1000), some
straddling a multiple of 256 nodes, one fully masked; logits 0, ±16, ±16.118, ±inf, NaN, bin edges and their fp32
neighbours, 15.9375 and 15.94; a NaN logit and target under a zero weight; one target that is neither 0 nor 1."""
import functools
import math
import os
import types

import numpy as np
import pytest
import torch

import eval_ref as ER
import guard as G
from spwgnn_amd import GraphNetwork, KerasModel, _lib, engine as E, metrics as M

pytestmark = pytest.mark.gpu

DEV = "cuda"
TAUS = (0.5, 0.3, 0.9)
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
_f = np.float32
_near = lambda e, to: np.nextafter(_f(e), _f(to))
SPECIALS = np.array([0.0, 16.0, -16.0, 16.118, -16.118, np.inf, -np.inf, np.nan,
                     -2.0, -0.125, 0.125, 1.0, 3.375, -15.875, 15.875,                       # bin edges k/8
                     _near(0.125, 1), _near(0.125, -1), _near(1.0, 2), _near(1.0, 0), _near(-15.875, 0), _near(-15.875, -20),
                     _near(-2.0, 0), _near(-2.0, -3), 15.9375, 15.94], np.float32)


def tower_sizes(n: int, rng) -> list:
    """Ragged sizes in 1..32 summing to n; at n >= 1000 every size 1..32 and one 40-node tower (bucket 0)."""
    sizes = [int(s) for s in rng.permutation(np.arange(1, 33))]
    if n >= 1000:
        sizes.insert(7, 40)
    out, left = [], n
    while left:
        s = min(sizes.pop() if sizes else int(rng.integers(1, 33)), left)
        out.append(s)
        left -= s
    return out


@functools.lru_cache(maxsize=None)
def case(n: int, R: int):
    """(logits (R, n), targets, weights, offsets) as numpy arrays; built once per shape and never modified."""
    rng = np.random.default_rng(1000 * n + R)
    z = rng.normal(scale=4.0, size=(R, n)).astype(np.float32)
    for tau in TAUS:                                   # no random logit within the expf margin of a threshold
        z[~ER.margin_ok(z, tau)] = 5.0
    if n >= len(SPECIALS):
        for r in range(R):
            z[r, rng.permutation(n)[:len(SPECIALS)]] = SPECIALS
    else:
        for r in range(R):
            z[r] = SPECIALS[(7 * r + np.arange(n)) % len(SPECIALS)]
    off = np.concatenate([[0], np.cumsum(tower_sizes(n, rng))]).astype(np.int32)
    T = len(off) - 1
    t = rng.integers(0, 2, n).astype(np.float32)
    w = rng.choice(np.array([0.0, 0.5, 1.0, 2.5], np.float32), size=n, p=[0.3, 0.25, 0.25, 0.2])
    if n > 1:
        w[0], w[n - 1] = 1.0, 2.5
    if T > 2:
        u = T - 2                                      # one tower fully masked, a NaN logit and target under it
        w[off[u]:off[u + 1]] = 0.0
        z[:, off[u]] = np.nan
        t[off[u]] = np.nan
        t[n - 1] = 0.5                                 # neither 0 nor 1: wrong on the predicted side
    for a in (z, t, w, off):
        a.setflags(write=False)
    return z, t, w, off


@functools.lru_cache(maxsize=None)
def reference(n: int, R: int, tau: float, weighted: bool = True):
    z, t, w, off = case(n, R)
    for r in range(R):
        assert ER.margin_ok(z[r], tau).all()
    return ER.eval_ref(z, t, w if weighted else None, off, tau)


def fake_batch(off):
    """What engine.eval_metrics reads of a TowerBatch: the node count and the device tower offsets."""
    return types.SimpleNamespace(n_nodes=int(off[-1]), n_towers=len(off) - 1,
                                 tower_offsets=torch.tensor(np.asarray(off), dtype=torch.int32, device=DEV))


def dev(a):
    return torch.tensor(np.asarray(a), device=DEV)


def assert_tables(got: dict, ref: dict, what=""):
    assert set(got) <= set(ref), what
    for k, v in got.items():
        assert v.dtype == np.int64 and v.shape == ref[k].shape, (what, k)
        assert np.array_equal(v, ref[k]), (what, k, np.argwhere(v != ref[k])[:5].tolist())


def test_case_shapes():
    """What the docstring promises of the inputs."""
    z, t, w, off = case(1000, 5)
    sizes = np.diff(off)
    assert set(range(1, 33)) <= set(sizes.tolist()) and 40 in sizes and sizes.sum() == 1000
    for n in (257, 1000):
        o = case(n, 1)[3]
        assert any(a < m < b for a, b in zip(o[:-1], o[1:]) for m in range(256, n, 256)), "a tower straddles a multiple of 256"
    assert (w == 0).sum() > 100 and np.isnan(z).sum() >= 5 and np.isinf(z).sum() >= 5
    u = len(sizes) - 2
    assert not w[off[u]:off[u + 1]].any() and np.isnan(z[:, off[u]]).all()                              # the masked tower
    assert len(case(1, 5)[3]) == 2 and case(1, 5)[0].shape == (5, 1)
    ref = reference(1000, 5, 0.5)
    assert (ref["by_size"][-1, :, 4] > 0).sum() == 33 and 0 < ref["tower6"][-1, 0] < len(sizes)        # every bucket; a tower masked
    assert ref["node4"].min() > 0 and ref["hist"][-1, :, 0].sum() > 0 and ref["hist"][-1, :, 255].sum() > 0


# -------------------------------------------------------------------------------- 1. exact tables
@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_exact_tables(n, R, tau):
    z, t, w, off = case(n, R)
    ref = reference(n, R, tau)
    tab = E.EvalTables(DEV, rows=R)
    zt = dev(z[0]) if R == 1 else dev(z)               # (n,) for one row, (R, n) otherwise
    E.eval_metrics(zt, dev(t), tab, batch=fake_batch(off), node_weights=dev(w), threshold=tau)
    got = tab.cpu()
    assert set(got) == {"node4", "tower6", "by_size", "hist"}
    assert_tables(got, ref, (n, R, tau))
    # without weights, and with the optional tables left out
    ref_u = reference(n, R, tau, weighted=False)
    small = E.EvalTables(DEV, rows=R, towers=False, hist=False)
    E.eval_metrics(zt, dev(t), small, threshold=tau)
    assert_tables(small.cpu(), ref_u, (n, R, tau, "node4 only"))
    nohist = E.EvalTables(DEV, rows=R, hist=False)
    E.eval_metrics(zt, dev(t), nohist, batch=fake_batch(off), threshold=tau)
    assert set(nohist.cpu()) == {"node4", "tower6", "by_size"}
    assert_tables(nohist.cpu(), ref_u, (n, R, tau, "no histogram"))


def test_engine_validation():
    z, t, w, off = case(255, 5)
    tab = E.EvalTables(DEV, rows=5)
    zt, tt, b = dev(z), dev(t), fake_batch(off)
    bad = [lambda: E.eval_metrics(zt, tt, E.EvalTables(DEV, rows=1), batch=b),            # rows
           lambda: E.eval_metrics(zt, tt, tab),                                           # tower tables without a batch
           lambda: E.eval_metrics(zt, tt[:-1], tab, batch=b),                             # one target per node
           lambda: E.eval_metrics(zt, tt, tab, batch=b, node_weights=dev(w)[:-1]),
           lambda: E.eval_metrics(zt, tt, tab, batch=fake_batch(off[:-1])),               # the batch's node count
           lambda: E.eval_metrics(zt.double(), tt, tab, batch=b),
           lambda: E.eval_metrics(zt.t(), tt, tab, batch=b),                              # not contiguous
           lambda: E.eval_metrics(zt, tt, tab, batch=b, threshold=1.0),
           lambda: E.eval_metrics(zt, tt, tab, batch=b, threshold=float("nan")),
           lambda: E.eval_metrics(zt, tt, E.EvalTables("cpu", rows=5), batch=b)]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    assert int(tab.flat.abs().sum()) == 0              # nothing ran


# -------------------------------------------------------------------------------- 2. identity with the loss
@pytest.mark.parametrize("weighted", [False, True])
def test_identity_with_the_loss(weighted):
    rng = np.random.default_rng(3)
    n = 1000
    z = rng.normal(scale=3.0, size=n).astype(np.float32)       # no margin filter: the same expression on the same device
    z[:40] = rng.normal(scale=1e-3, size=40)                    # probabilities next to 0.5
    z[40:44] = [0.0, -0.0, np.inf, -np.inf]
    t = rng.integers(0, 2, n).astype(np.float32)
    w = rng.choice(np.array([0.0, 0.5, 2.5], np.float32), size=n) if weighted else None
    zt, tt = dev(z), dev(t)
    out3, _ = E.bce(zt, tt, E.BceScratch(DEV), node_weights=dev(w) if weighted else None)
    tab = E.EvalTables(DEV, towers=False, hist=False)
    E.eval_metrics(zt, tt, tab, node_weights=dev(w) if weighted else None)
    tp, tn, fp, fn = tab.cpu()["node4"][0].tolist()
    o = out3.tolist()
    assert tp + tn == int(o[1]) and tp + tn + fp + fn == int(o[2]) == (int((w != 0).sum()) if weighted else n)
    assert 0 < tp + tn < n


# -------------------------------------------------------------------------------- 3. sums and accumulation
def test_sums_and_accumulation():
    n, R, tau = 1000, 5, 0.5
    z, t, w, off = case(n, R)
    ref = reference(n, R, tau)
    zt, tt, wt = dev(z), dev(t), dev(w)
    tab = E.EvalTables(DEV, rows=R)
    E.eval_metrics(zt, tt, tab, batch=fake_batch(off), node_weights=wt, threshold=tau)
    got = tab.cpu()
    assert np.array_equal(got["hist"].sum(axis=(1, 2)), got["node4"].sum(axis=1))
    assert np.array_equal(got["by_size"][:, :, :4].sum(axis=1), got["node4"])
    assert np.array_equal(got["by_size"][:, :, 4:].sum(axis=1), got["tower6"][:, :2])
    assert np.array_equal(got["tower6"][:, 2:].sum(axis=1), got["tower6"][:, 0])
    # the two halves, split at a tower boundary, accumulate to the whole
    m = len(off) // 2
    cut = int(off[m])
    halves = E.EvalTables(DEV, rows=R)
    E.eval_metrics(zt[:, :cut].contiguous(), tt[:cut], halves, batch=fake_batch(off[:m + 1]), node_weights=wt[:cut], threshold=tau)
    E.eval_metrics(zt[:, cut:].contiguous(), tt[cut:], halves, batch=fake_batch(off[m:] - cut), node_weights=wt[cut:],
                   threshold=tau)
    assert_tables(halves.cpu(), ref, "halves")
    # a second identical call doubles every entry; add_ and zero_
    E.eval_metrics(zt, tt, tab, batch=fake_batch(off), node_weights=wt, threshold=tau)
    assert_tables(tab.cpu(), {k: 2 * v for k, v in ref.items()}, "twice")
    assert_tables(tab.add_(halves).cpu(), {k: 3 * v for k, v in ref.items()}, "add_")
    assert int(tab.zero_().flat.abs().sum()) == 0


# -------------------------------------------------------------------------------- 4. rows
def test_last_row_equals_the_one_row_call():
    n, S, tau = 257, 5, 0.3
    z, t, w, off = case(n, S)
    all_rows, one = E.EvalTables(DEV, rows=S), E.EvalTables(DEV, rows=1)
    E.eval_metrics(dev(z), dev(t), all_rows, batch=fake_batch(off), node_weights=dev(w), threshold=tau)
    E.eval_metrics(dev(z[S - 1]), dev(t), one, batch=fake_batch(off), node_weights=dev(w), threshold=tau)
    a, b = all_rows.cpu(), one.cpu()
    for k in a:
        assert np.array_equal(a[k][S - 1:], b[k]), k
    assert _same(M.summarize(a), M.summarize(b)) and _same(M.summarize(a, row=S - 1), M.summarize(b, row=0))


# -------------------------------------------------------------------------------- 5. guard bands
@pytest.mark.parametrize("optional", [True, False])
@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("n", [255, 256, 257])
def test_guard_bands(n, R, optional):
    """Every buffer of the call between two 64 KiB sentinel bands at the alignment the header asks for and no more:
    nothing is written outside the four tables, the inputs keep their bits (tests/guard.py)."""
    tau = 0.5
    z, t, w, off = case(n, R)
    arena = G.Arena(DEV)
    zt = arena.put(z.copy(), 4, "logits")              # copies: the cached case is read-only
    tt = arena.put(t.copy(), 4, "targets")
    wt = arena.put(w.copy(), 4, "weights")
    ot = arena.put(off.copy(), 4, "tower_offsets") if optional else None
    shapes = {"node4": (R, 4)}
    if optional:
        shapes.update(tower6=(R, 6), by_size=(R, _lib.EVAL_SIZES, 6), hist=(R, 2, _lib.EVAL_BINS))
    tabs = {k: arena.alloc(s, torch.int64, 8, k).zero_() for k, s in shapes.items()}
    ev = _lib.EvalC()
    ev.rows, ev.threshold, ev.w, ev.node4 = R, tau, wt.data_ptr(), tabs["node4"].data_ptr()
    if optional:
        ev.n_towers, ev.tower_offsets = len(off) - 1, ot.data_ptr()
        ev.tower6, ev.by_size, ev.hist = (tabs[k].data_ptr() for k in ("tower6", "by_size", "hist"))
    st = _lib.lib().spwgnn_eval_metrics(zt.data_ptr(), tt.data_ptr(), n, _lib.C.byref(ev),
                                        torch.cuda.current_stream().cuda_stream)
    assert st == 0
    arena.check(f"eval_metrics n={n} R={R} optional={optional}")
    assert_tables({k: v.cpu().numpy() for k, v in tabs.items()}, reference(n, R, tau), "guarded")


# -------------------------------------------------------------------------------- 6. capture
def test_capture_and_replay():
    n, R, tau = 1000, 5, 0.9
    z, t, w, off = case(n, R)
    zt, tt, wt, b = dev(z), dev(t), dev(w), fake_batch(off)
    tab = E.EvalTables(DEV, rows=R)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # the eager warm-up
        E.eval_metrics(zt, tt, tab, batch=b, node_weights=wt, threshold=tau)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        E.eval_metrics(zt, tt, tab, batch=b, node_weights=wt, threshold=tau)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert_tables(tab.cpu(), {k: 4 * v for k, v in reference(n, R, tau).items()}, "warm-up + 3 replays")


# -------------------------------------------------------------------------------- 7. KerasModel.evaluate, Trainer.evaluate
def _same(a, b) -> bool:
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, float) and math.isnan(a):
        return isinstance(b, float) and math.isnan(b)
    return type(a) is type(b) and a == b


def test_keras_evaluate_on_the_golden_shape():
    g = np.load(os.path.join(GOLDEN, "golden_N6_B4_S5_thr.npz"))
    params = dict(np.load(os.path.join(GOLDEN, "golden_params.npz")))
    S, (B, N) = int(g["mp_steps"]), g["objects"].shape[:2]
    assert (B, N, S) == (4, 6, 5)
    net = GraphNetwork(mp_steps=S, params=params, math="x6")
    model = KerasModel(net, N)
    x = {"objects": g["objects"], "sender_relations": g["Rs"], "receiver_relations": g["Rr"], "propagation": g["prop"]}
    target = np.asarray(g["target"], np.float32).reshape(B, N)
    y = {"target": target}
    off = np.arange(B + 1) * N
    d = model.evaluate(x, y, return_dict=True)
    # the tables are eval_ref's on the network's own logits
    with torch.no_grad():
        z = net.eval().forward_logits(g["objects"], g["Rs"], g["Rr"], g["prop"]).cpu().numpy().reshape(-1)
    assert ER.margin_ok(z, 0.5).all()
    ref = M.summarize(ER.eval_ref(z, target.reshape(-1), None, off, 0.5))
    assert _same({k: v for k, v in d.items() if k != "loss"}, ref)
    assert d["n"] == B * N and d["towers"] == B and set(d["by_size"]) == {N}
    assert abs(d["loss"] - float(g["loss"])) < 1e-5          # tests/test_gpu_parity.py's bound on the x6 loss
    loss, acc = model.evaluate(x, y)
    assert [loss, acc] == [d["loss"], d["binary_accuracy"]] and acc == (d["tp"] + d["tn"]) / (B * N)
    # two batches: the same tables, the tower-weighted mean of the batch losses
    d2 = model.evaluate(x, y, batch_size=3, return_dict=True)
    assert _same({k: v for k, v in d2.items() if k != "loss"}, ref)
    assert abs(d2["loss"] - d["loss"]) <= 1e-7 * abs(d["loss"])
    # every step's summary; the last entry is the plain one
    steps = model.evaluate(x, y, return_steps=True)
    assert len(steps) == S and _same(steps[-1], d)
    with torch.no_grad():
        zs = net.forward_logits(g["objects"], g["Rs"], g["Rr"], g["prop"], return_steps=True).cpu().numpy().reshape(S, -1)
    for s in range(S):
        if ER.margin_ok(zs[s], 0.5).all():
            row = M.summarize(ER.eval_ref(zs[s], target.reshape(-1), None, off, 0.5))
            assert _same({k: v for k, v in steps[s].items() if k != "loss"}, row), s
    # sample_weight: a zero masks its tower out of every count
    sw = np.array([0.0, 1.0, 2.0, 1.0])
    dw = model.evaluate(x, y, sample_weight=sw, return_dict=True)
    refw = M.summarize(ER.eval_ref(z, target.reshape(-1), np.repeat(sw, N), off, 0.5))
    assert _same({k: v for k, v in dw.items() if k != "loss"}, refw) and dw["n"] == 3 * N and dw["towers"] == 3
    # threshold: the counts move, the loss does not
    d9 = model.evaluate(x, y, threshold=0.9, return_dict=True)
    if ER.margin_ok(z, 0.9).all():
        assert _same({k: v for k, v in d9.items() if k != "loss"}, M.summarize(ER.eval_ref(z, target.reshape(-1), None, off, 0.9)))
    assert d9["loss"] == d["loss"]
    # after a one-epoch fit, evaluate of the held-out slice returns the history's validation numbers exactly
    h = model.fit(x, y, batch_size=32, epochs=1, validation_split=0.25, verbose=0)
    xv = {k: v[3:] for k, v in x.items()}
    vl, va = model.evaluate(xv, {"target": target[3:]})
    assert vl == h["val_loss"][-1] and va == h["val_binary_accuracy"][-1]


def test_trainer_evaluate_hip_engine():
    """Trainer.evaluate on the HIP engine, single process: two micro-batches, unweighted, weighted and with
    step_loss_weights, against eval_ref on the whole batch's logits; the parameters do not move."""
    from oracle import model as O
    from spwgnn_amd import TowerBatch, data as D, params as P
    from spwgnn_amd.trainer import Trainer
    S, cuts = 3, [(0, 4), (4, 7)]
    obj, Rs, Rr, prop, tgt = D.synthetic_batch(7, 5, seed=9, fully_connected=False)
    flat = P.to_flat(O.random_params(11), device=DEV)
    before = flat.clone()
    full = TowerBatch.from_dense(obj, Rs, Rr, device=DEV)
    batches = [TowerBatch.from_dense(obj[a:b], Rs[a:b], Rr[a:b], device=DEV) for a, b in cuts]
    targets = [dev(tgt[a:b].reshape(-1)) for a, b in cuts]
    zs = E.forward_steps(flat, full, E.RunConfig(S), E.Workspace(DEV))
    z, t, off = zs.cpu().numpy(), tgt.reshape(-1), np.arange(8) * 5
    assert all(ER.margin_ok(z[s], 0.5).all() for s in range(S))     # micro-batch plans may move a logit's last bits
    out3, _ = E.bce(zs[S - 1].contiguous(), dev(t), E.BceScratch(DEV))
    tr = Trainer(flat, mp_steps=S, dropout=0.0)
    out = tr.evaluate(batches, targets)
    assert _same({k: v for k, v in out.items() if k != "loss"}, M.summarize(ER.eval_ref(z[S - 1], t, None, off, 0.5)))
    assert abs(out["loss"] - float(out3[0])) <= 1e-6 * float(out3[0])   # fp32 losses of two batches against one
    # weights: a zero masks its node; the pair's n is the count of the others
    W = np.random.default_rng(2).choice(np.array([0.0, 0.5, 2.0], np.float32), size=(7, 5))
    W[1] = 0.0
    outw = tr.evaluate(batches, targets, weights=[dev(W[a:b].reshape(-1)) for a, b in cuts], threshold=0.5)
    refw = M.summarize(ER.eval_ref(z[S - 1], t, W.reshape(-1), off, 0.5))
    assert _same({k: v for k, v in outw.items() if k != "loss"}, refw) and outw["n"] == int((W != 0).sum()) and outw["towers"] <= 6
    # deep supervision: the engine's (S, n) rows are all scored
    trs = Trainer(flat, mp_steps=S, dropout=0.0, step_loss_weights=(0.25, 0.25, 1.0))
    outs = trs.evaluate(batches, targets)
    ref_rows = ER.eval_ref(z, t, None, off, 0.5)
    assert len(outs["steps"]) == S and all(_same(outs["steps"][s], M.summarize(ref_rows, row=s)) for s in range(S))
    assert _same({k: v for k, v in outs.items() if k not in ("loss", "steps")}, M.summarize(ref_rows))
    assert torch.equal(flat, before) and tr.iterations == 0 and trs.iterations == 0
