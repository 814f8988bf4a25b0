"""GPU: clipnorm, clipvalue, decay and the non-finite guard of the Adam step (spwgnn_adam_clipped;
DESIGN.md §3zq) — the two kernels on their own, the Trainer's step paths against the fp64 restatement
(tests/clip_ref.py) and the Keras front end's three ways of issuing the same steps.

Kernel-level inputs: the whole flat buffer (n = spwgnn_param_count()), seeded random p and g, non-zero m
and v, and NaN in every padding element of g — the padding must stay out of the norm and of the
finiteness check whatever it holds.
"""
import functools

import numpy as np
import pytest
import torch

import clip_ref as R
from oracle import model as O
from spwgnn_amd import data as D, engine as E, params as P
from spwgnn_amd.batch import HostPlan, TowerBatch
from spwgnn_amd.keras_api import CompactDataset, PropagationNetwork
from spwgnn_amd.replay import ReplayStep
from spwgnn_amd.trainer import Trainer

pytestmark = pytest.mark.gpu

HYP = dict(lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-7, l2=1e-3, grad_scale=0.5)
STEP = 7


@functools.lru_cache(maxsize=None)
def _inputs():
    """(p, g, m, v) fp32 host arrays and the real-parameter mask; g's padding is NaN."""
    n = P.flat_size()
    rng = np.random.default_rng(41)
    mask = R.real_mask()
    p = rng.normal(0, 0.1, n).astype(np.float32)
    g = rng.normal(0, 2e-3, n).astype(np.float32)
    g[rng.integers(0, n, 64)] *= 40.0                       # a few large elements (clipvalue's targets)
    g[~mask] = np.nan
    m = rng.normal(0, 1e-3, n).astype(np.float32)
    v = np.square(rng.normal(0, 2e-3, n)).astype(np.float32)
    for a in (p, g, m, v):
        a.setflags(write=False)
    return p, g, m, v, mask


def _dev(*arrs):
    return [torch.tensor(a, device="cuda") for a in arrs]


def _run_clipped(g=None, dev=False, accumulate=False, clip=None, **opt):
    """One clipped step on fresh device copies → (p, m, v host arrays, out4 host, ClipScratch)."""
    p0, g0, m0, v0, _ = _inputs()
    p, gg, m, v = _dev(p0, g0 if g is None else g, m0, v0)
    g_before = gg.clone()
    clip = clip or E.ClipScratch("cuda", totals=True)
    kw = dict(HYP, **opt)
    if dev:
        lr = kw.pop("lr")
        table = E.adam_lr_table(16, lr, kw["beta1"], kw["beta2"], "cuda")
        word = torch.tensor([STEP], dtype=torch.int32, device="cuda")
        out4 = E.adam_clipped_dev(p, gg, m, v, word, table, clip, accumulate=accumulate, **kw)
    else:
        out4 = E.adam_clipped(p, gg, m, v, STEP, clip, accumulate=accumulate, **kw)
    torch.cuda.synchronize()
    assert torch.equal(gg.view(torch.int32), g_before.view(torch.int32))   # grads are never modified
    return p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), out4.cpu().numpy().copy(), clip


def _run_adam(g=None, **opt):
    p0, g0, m0, v0, _ = _inputs()
    p, gg, m, v = _dev(p0, g0 if g is None else g, m0, v0)
    E.adam(p, gg, m, v, STEP, **dict(HYP, **opt))
    torch.cuda.synchronize()
    return p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()


def _ref_norm(**opt):
    p0, g0, _, _, mask = _inputs()
    kw = dict(HYP, **opt)
    return R.global_norm(R.grad_prime(p0, g0, kw["l2"], kw["grad_scale"]), mask)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_norm_matches_fp64():
    """out4[0] against sqrt(Σ g'²) in fp64 over the real ranges: relative error <= 1e-5.

    Derivation: each block partial is a sum of at most k fp32 operations in a row — the per-thread
    strided sum (13 terms), the 8 levels of the LDS tree, the square and the two roundings of
    g' = gscale·g + 2·l2·p — k <= 128, so its relative error is below γ = k·2⁻²⁴ = 7.6e-6 (every term is
    non-negative: no cancellation). The 64 partials are added in double, which adds nothing visible,
    and the square root halves the relative error and adds one rounding: under 1e-5 with room."""
    _, _, _, out4, _ = _run_clipped(clipnorm=0.0)
    ref = _ref_norm()
    rel = abs(float(out4[0]) - ref) / ref
    print(f"norm {out4[0]:.9g} fp64 {ref:.12g} rel {rel:.3g}")
    assert np.isfinite(out4[0]) and rel <= 1e-5
    assert out4[1] == 1.0 and out4[2] == 0.0 and out4[3] == 0.0


@pytest.mark.parametrize("both", [False, True])
def test_update_matches_fp64_with_device_scale(both):
    """p, m, v after one clipped step (clipnorm = half the fp64 norm; `both`: clipvalue on too, applied
    after the norm scale) against the fp64 restatement evaluated with the device's reported scale. The
    yardstick is spwgnn_adam on the same inputs against its own restatement, measured here: the clipped
    kernel may miss by at most twice that per array — its g' carries one rounding more (the scale)."""
    p0, g0, m0, v0, mask = _inputs()
    kw = {k: v for k, v in HYP.items() if k != "grad_scale"}
    base = _run_adam()
    rb = R.step(p0, g0, m0, v0, STEP, grad_scale=HYP["grad_scale"], **kw)
    yard = [np.abs(a[mask] - b[mask]).max() for a, b in zip(base, rb[:3])]
    c = 0.5 * _ref_norm()
    cv = 0.5 * c / np.sqrt(mask.sum()) * 8 if both else 0.0     # a few rms of the scaled gradient
    p, m, v, out4, _ = _run_clipped(clipnorm=c, clipvalue=cv)
    assert out4[3] == 1.0 and out4[2] == 0.0 and abs(out4[1] - 0.5) < 1e-5
    rc = R.step(p0, g0, m0, v0, STEP, grad_scale=HYP["grad_scale"], clipnorm=c, clipvalue=cv, mask=mask,
                scale=float(out4[1]), **kw)
    if both:   # the value clip really bites, and after the norm scale
        gs = R.grad_prime(p0, g0, HYP["l2"], HYP["grad_scale"])[mask] * float(out4[1])
        assert 0 < (np.abs(gs) > cv).sum() < mask.sum() // 2
    for name, got, ref, y in zip("pmv", (p, m, v), rc[:3], yard):
        d = np.abs(got[mask] - ref[mask]).max()
        print(f"{name}: clipped max|Δ| {d:.3g}  spwgnn_adam's {y:.3g}")
        assert d <= 2.0 * y, name


def test_no_clip_is_spwgnn_adam_bitwise():
    """clipnorm above the norm, clipvalue 0: the scale is exactly 1.0f and p, m, v are spwgnn_adam's bits."""
    base = _run_adam()
    p, m, v, out4, _ = _run_clipped(clipnorm=2.0 * _ref_norm())
    mask = _inputs()[4]
    assert out4[1] == 1.0 and out4[3] == 0.0
    for a, b in zip((p, m, v), base):
        assert np.array_equal(_bits(a)[mask], _bits(b)[mask])
        assert np.array_equal(np.isnan(a), np.isnan(b))


def test_clipvalue_clamps_to_exactly_v():
    """clipvalue below max|g'| (l2 = 0, grad_scale = 1: g' is g itself): every element takes the update
    spwgnn_adam gives for the gradient clamped on the host — those above v the update of exactly ±v."""
    p0, g0, m0, v0, mask = _inputs()
    cv = np.float32(4e-3)
    assert (np.abs(g0[mask]) > cv).sum() > 1000 and (np.abs(g0[mask]) < cv).sum() > 1000
    gc = np.where(g0 > cv, cv, np.where(g0 < -cv, -cv, g0)).astype(np.float32)
    base = _run_adam(g=gc, l2=0.0, grad_scale=1.0)
    p, m, v, out4, _ = _run_clipped(clipvalue=float(cv), l2=0.0, grad_scale=1.0)
    assert out4[1] == 1.0 and out4[3] == 0.0
    for a, b in zip((p, m, v), base):
        assert np.array_equal(_bits(a)[mask], _bits(b)[mask])


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_nonfinite_gradient_skips_the_step(bad):
    p0, g0, m0, v0, mask = _inputs()
    g = g0.copy()
    g[np.flatnonzero(mask)[123457]] = bad
    p, m, v, out4, _ = _run_clipped(g=g, clipnorm=1.0, skip_nonfinite=True)
    assert out4[2] == 1.0 and out4[3] == 0.0
    for a, b in zip((p, m, v), (p0, m0, v0)):
        assert np.array_equal(_bits(a), _bits(b))
    # without the flag the value propagates as in Keras: the step is applied
    p, m, v, out4, _ = _run_clipped(g=g, clipnorm=1.0)
    assert out4[2] == 0.0 and not np.array_equal(_bits(p), _bits(p0))


def test_nan_in_padding_only_does_not_skip():
    p0, _, _, _, mask = _inputs()
    p, m, v, out4, _ = _run_clipped(clipnorm=1.0, skip_nonfinite=True)
    assert out4[2] == 0.0 and np.isfinite(out4[0])
    assert np.isfinite(p[mask]).all() and np.isfinite(m[mask]).all() and np.isfinite(v[mask]).all()
    assert not np.array_equal(_bits(p)[mask], _bits(p0)[mask])


def test_deterministic_and_replayable():
    """Two runs give the same bits; adam_clipped and adam_clipped_dev at the same step and table too; the
    fp64 sums take [norm, clipped, skipped, 1] per step."""
    c = 0.5 * _ref_norm()
    a = _run_clipped(clipnorm=c, clipvalue=3e-3, accumulate=True)
    b = _run_clipped(clipnorm=c, clipvalue=3e-3, accumulate=True, clip=a[4])
    d = _run_clipped(clipnorm=c, clipvalue=3e-3, dev=True)
    for x, y, z in zip(a[:4], b[:4], d[:4]):
        assert np.array_equal(_bits(x), _bits(y)) and np.array_equal(_bits(x), _bits(z))
    tot = a[4].total4.cpu().numpy()
    assert np.array_equal(tot, [2.0 * float(a[3][0]), 2.0, 0.0, 2.0])


# ---------------------------------------------------------------- Trainer
B, N, S = 4, 6, 2


@functools.lru_cache(maxsize=None)
def _problem():
    obj, Rs, Rr, prop, tgt = D.synthetic_batch(B, N, seed=31, fully_connected=False)
    return obj, Rs, Rr, prop, tgt, O.random_params(15)


def _oracle_grad(flat64):
    obj, Rs, Rr, prop, tgt, _ = _problem()
    _, _, g = O.loss_and_grads(P.from_flat(torch.tensor(flat64)), obj, Rs, Rr, prop, tgt, S)
    return P.to_flat(g, dtype=torch.float64).numpy()


@functools.lru_cache(maxsize=None)
def _step1_norm():
    return R.global_norm(_oracle_grad(P.to_flat(_problem()[5], dtype=torch.float64).numpy()), R.real_mask())


@functools.lru_cache(maxsize=None)
def _trajectory(kind):
    """clip_ref's fp64 trajectory over three steps (computed once, shared by the maths): the parameters
    after each step and the step's norm."""
    opt = dict(clip=dict(clipnorm=0.5 * _step1_norm()), decay=dict(decay=0.1))[kind]
    adam = R.ClippedAdam(mask=R.real_mask(), **opt)
    ref = P.to_flat(_problem()[5], dtype=torch.float64).numpy()
    out = []
    for _ in range(3):
        ref = adam.step(ref, _oracle_grad(ref))
        out.append((ref.copy(), adam.last["norm"], adam.last["clipped"]))
    return opt, out


def _trainer(math, **opt):
    obj, Rs, Rr, prop, tgt, params = _problem()
    batch = TowerBatch.from_dense(obj, Rs, Rr, None, device="cuda")
    tr = Trainer(P.to_flat(params, device="cuda"), mp_steps=S, dropout=0.0, math=math, **opt)
    return tr, batch, torch.tensor(tgt.reshape(-1), device="cuda")


@pytest.mark.parametrize("math", ["f32", "x6"])
def test_trainer_three_clipped_steps_match_clip_ref(math):
    """clipnorm = half the oracle's step-1 norm. Parameters within 2e-6 of the fp64 trajectory
    (tests/test_gpu_training.py's bound for three steps: a 1e-5 relative error of the scale moves an Adam
    update by about lr·1e-5); the reported norm within 1.5e-5 relative of the oracle's — GRAD_L2_REL 5e-6
    (the engine's gradients against the oracle's, tests/test_gpu_chain_parity.py) plus the summation bound."""
    opt, traj = _trajectory("clip")
    tr, batch, tgt = _trainer(math, **opt)
    for k, (ref, norm, clipped) in enumerate(traj):
        tr.step(batch, tgt)
        torch.cuda.synchronize()
        stats = tr.clip_stats.cpu().numpy()
        rel = abs(float(stats[0]) - norm) / norm
        print(f"step {k + 1}: norm {stats[0]:.8g} oracle {norm:.10g} rel {rel:.3g} scale {stats[1]:.6g}")
        assert rel <= 1.5e-5 and stats[3] == float(clipped) and stats[2] == 0.0
    assert traj[0][2]                                                   # step 1 is clipped
    assert np.abs(tr.params.cpu().numpy() - traj[-1][0]).max() < 2e-6
    assert tr.iterations == 3


@pytest.mark.parametrize("math", ["f32", "x6"])
def test_trainer_never_clipping_is_the_plain_trainer_bitwise(math):
    ta, batch, tgt = _trainer(math)
    tb, _, _ = _trainer(math, clipnorm=1e30)
    for _ in range(3):
        ta.step(batch, tgt)
        tb.step(batch, tgt)
    torch.cuda.synchronize()
    assert ta.clip_stats is None and float(tb.clip_stats[1]) == 1.0
    for a, b in ((ta.params, tb.params), (ta.m, tb.m), (ta.v, tb.v)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("math", ["f32", "x6"])
def test_trainer_skips_a_nonfinite_step(math):
    """One NaN in the target makes the step's gradient NaN (arithmetic on NaN values): with skip_nonfinite
    the parameters and both moments keep their bits, the iteration count still advances, and the next
    clean step moves the parameters to finite values."""
    tr, batch, tgt = _trainer(math, skip_nonfinite=True)
    tr.step(batch, tgt)                                  # a clean step first: non-zero m and v
    torch.cuda.synchronize()
    before = [t.clone() for t in (tr.params, tr.m, tr.v)]
    bad = tgt.clone()
    bad[5] = float("nan")
    tr.step(batch, bad)
    torch.cuda.synchronize()
    assert float(tr.clip_stats[2]) == 1.0 and tr.iterations == 2
    for a, b in zip((tr.params, tr.m, tr.v), before):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    tr.step(batch, tgt)
    torch.cuda.synchronize()
    assert float(tr.clip_stats[2]) == 0.0 and tr.iterations == 3
    assert torch.isfinite(tr.params).all() and not torch.equal(tr.params, before[0])


@pytest.mark.parametrize("math", ["f32", "x6"])
def test_trainer_decay_matches_clip_ref(math):
    opt, traj = _trajectory("decay")
    tr, batch, tgt = _trainer(math, **opt)
    for _ in traj:
        tr.step(batch, tgt)
    torch.cuda.synchronize()
    assert np.abs(tr.params.cpu().numpy() - traj[-1][0]).max() < 2e-6
    # the decay moved the trajectory by more than the bound
    plain, _, _ = _trainer(math)
    for _ in traj:
        plain.step(batch, tgt)
    assert (plain.params - tr.params).abs().max().item() > 2e-5


def test_trainer_clipped_replay_equals_step():
    """Trainer.replay_body with clipnorm and decay (the clipped update read from the device step word and
    the decayed lr table), replayed over three batches of one geometry == Trainer.step, bit for bit."""
    plans, tgts = [], []
    for seed in (1, 2, 3):
        raw = D.synthetic_towers(B, N, seed=seed)
        obj = (raw / D.RELATION_THRESHOLD).astype(np.float32)
        Rs, Rr = D.relation_matrices(raw, D.RELATION_THRESHOLD)
        e = np.array(O.dense_to_edges(Rs, Rr), np.int64).reshape(-1, 4)
        te = np.bincount(e[:, 0], minlength=B).astype(np.int32)
        plans.append(HostPlan.build(obj.reshape(-1, 3), np.full(B, N, np.int32), e[:, 0] * N + e[:, 2],
                                    e[:, 0] * N + e[:, 3], te, edge_cap=N * (N - 1)))
        tgts.append(np.random.default_rng(seed).integers(0, 2, B * N).astype(np.float32))
    opt = dict(clipnorm=0.05, decay=0.1, skip_nonfinite=True)
    params = _problem()[5]
    ta = Trainer(P.to_flat(params, device="cuda"), mp_steps=S, dropout=0.1, seed=11, **opt)
    for p, t in zip(plans, tgts):
        ta.step(TowerBatch.from_plan(p, "cuda"), torch.as_tensor(t, device="cuda"))
    stats_a = ta.clip_stats.clone()
    tb = Trainer(P.to_flat(params, device="cuda"), mp_steps=S, dropout=0.1, seed=11, **opt)
    rs = ReplayStep(plans[0], "cuda", tb.replay_body(plans[0].n_nodes))
    for p, t in zip(plans, tgts):
        tb.replay_step(rs, p, t)
    torch.cuda.synchronize()
    assert rs.replays == 2
    assert torch.equal(ta.params, tb.params) and torch.equal(ta.m, tb.m) and torch.equal(ta.v, tb.v)
    assert torch.equal(stats_a, tb.clip_stats) and tb.iterations == 3


# ---------------------------------------------------------------- Keras front end
def test_keras_fit_paths_agree_bitwise_and_report_clip_history():
    """8 towers of 6, batch 4, 2 epochs, clipnorm set: fit issued eagerly, fit replayed as hipGraphs and a
    train_on_batch loop give the same parameters bit for bit (tests/test_gpu_replay.py's invariant), and
    the history carries the epoch's clip sums."""
    n, bs, epochs, c = 8, 4, 2, 0.02
    obj, Rs, Rr, prop, tgt = D.synthetic_batch(n, 6, seed=13, fully_connected=False)
    x = {"objects": obj, "sender_relations": Rs, "receiver_relations": Rr, "propagation": prop}
    y = {"target": tgt.reshape(n, 6, 1)}
    flats, hists = [], []
    for graph in (False, True):
        model = PropagationNetwork(seed=3, clipnorm=c).getModel(6)
        hists.append(model.fit(x, y, batch_size=bs, epochs=epochs, shuffle=False, verbose=0, graph=graph))
        torch.cuda.synchronize()
        flats.append(model.net.flat.detach().cpu().numpy().copy())
        assert model.iterations == 4
    mb = PropagationNetwork(seed=3, clipnorm=c).getModel(6)
    ds = CompactDataset(obj, Rs, Rr, prop)
    norms = []
    for _ in range(epochs):
        for b0 in range(0, n, bs):
            idx = np.arange(b0, b0 + bs)
            batch = TowerBatch.from_plan(ds.subset_plan(idx, edge_cap=True), "cuda")
            mb.train_on_batch(batch, torch.as_tensor(tgt[idx].reshape(-1), device="cuda"))
            norms.append(float(mb.clip_stats[0]))
    torch.cuda.synchronize()
    flats.append(mb.net.flat.detach().cpu().numpy().copy())
    assert np.array_equal(_bits(flats[0]), _bits(flats[1])) and np.array_equal(_bits(flats[0]), _bits(flats[2]))
    assert hists[0] == hists[1]
    h = hists[0]
    for key in ("grad_norm", "clipped_steps", "skipped_steps"):
        assert len(h[key]) == epochs, key
    assert h["skipped_steps"] == [0, 0]
    assert h["clipped_steps"] == [sum(v >= c for v in norms[:2]), sum(v >= c for v in norms[2:])]
    assert h["clipped_steps"][0] > 0
    for ep in range(epochs):   # the mean of the steps' fp32 norms, summed in fp64
        assert abs(h["grad_norm"][ep] - np.mean(norms[2 * ep:2 * ep + 2])) <= 1e-12
    plain = PropagationNetwork(seed=3).getModel(6)
    hp = plain.fit(x, y, batch_size=bs, epochs=1, shuffle=False, verbose=0)
    assert "grad_norm" not in hp                       # options off: the history of before
