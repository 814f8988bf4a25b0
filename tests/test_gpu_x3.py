"""GPU: x3 math (SPWGNN_MATH_X3) — two bf16 parts per operand, three bf16 MFMA products
per fp32 product — held to its definition through the fp64 x3 emulator (tests/x3_emu.py).

1. Products (kink-free parameters): the engine lies no further from the emulator than 2.5× the band
   of valid fp32 implementations of the same arithmetic (the factor tests/test_gpu_fullsize.py holds
   bf16 to), on the team / fused path and on the wide kernels. A missing or extra product term lies
   ≥ 55× outside (tests/test_x3_host.py calibrates both).
2. Masks (random parameters): with d_bf16 the distance between the fp64 bf16 and x3 emulators, logits
   within d_bf16 / 32 and each gradient tensor within 0.2 · d_bf16 of the x3 emulator.
3. Not some other math; 4. the bitwise invariants x6 has; 5. d/d objects.
The whole file also passes under SPWGNN_POISON_WORKSPACE=1.
"""
import functools

import numpy as np
import pytest
import torch

import x3_emu as X
from oracle import bf16 as OB
from oracle import dropout as DR
from oracle import model as O
from spwgnn_amd import TowerBatch, data as D, demolish, engine as E, params as P
from spwgnn_amd.batch import HostPlan
from spwgnn_amd.keras_api import PropagationNetwork
from spwgnn_amd.network import GraphNetwork
from spwgnn_amd.replay import ReplayStep
from spwgnn_amd.trainer import Trainer

pytestmark = pytest.mark.gpu

BAND_FACTOR = 2.5
TEAM_LIMIT = 512


def _train(params, batch, tgt, S, math, dropout=0.0, seed=0, want_dprop=False, inputs=False):
    """(loss, logits, grads, dprop, dobj) of one training forward + BCE + backward."""
    flat = P.to_flat(params, device="cuda")
    ws = E.Workspace("cuda")
    run = E.RunConfig(S, training=True, math=math, dropout=dropout, seed=seed)
    z = E.forward(flat, batch, run, ws)
    out3, dz = E.bce(z, torch.as_tensor(np.ascontiguousarray(tgt, np.float32), device="cuda").reshape(-1), E.BceScratch("cuda"))
    g, dp = E.backward(flat, batch, run, ws, dz, want_dprop=want_dprop)
    dobj = E.backward_inputs(flat, batch, run, ws) if inputs else None
    torch.cuda.synchronize()
    return (float(out3[0]), z.cpu().numpy(), P.from_flat(g), None if dp is None else dp.cpu().numpy(),
            None if dobj is None else dobj.cpu().numpy())


class _limit:
    """Team limit `n` inside the block; the previous value is restored."""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        self.prev = E.team_max_blocks(self.n)

    def __exit__(self, *exc):
        E.team_max_blocks(self.prev)


def _batch(case, plan="dense", prop=True):
    obj, Rs, Rr, pr, _ = case[:5]
    pr = pr if prop else None
    if plan == "dense":
        return TowerBatch.from_dense(obj, Rs, Rr, pr, device="cuda")
    dense = TowerBatch.from_dense(obj, Rs, Rr, pr, device="cuda")
    rb = TowerBatch.from_edges(obj.reshape(-1, 3), dense.tower_nodes, dense.src, dense.dst, dense.tower_edges,
                               None if pr is None else pr.reshape(-1, 100), device="cuda", recv_blocks=True)
    assert rb.flags == 1
    return rb


# --------------------------------------------------------------------- 1. products, kink-free set
@functools.lru_cache(maxsize=None)
def _kink_ref(T, N, fully, seed):
    params = X.kink_free_params(seed)
    case = X.dense_case(T, N, fully, seed=seed)
    ref, band = X.noise_band(params, *X.emu_args(case))
    return params, case, ref, band


@pytest.mark.parametrize("wide", [False, True], ids=["team", "wide"])
@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("T,N,fully", [(8, 6, True), (5, 9, False)])
def test_x3_products_against_emulator_kink_free(T, N, fully, seed, wide):
    params, case, ref, band = _kink_ref(T, N, fully, seed)
    # preconditions: a kinked input cannot loosen the test
    assert band["z_max"] <= 2e-5, band["z_max"]
    assert all(v <= 2e-4 for v in band["g"].values()), band["g"]
    batch = _batch(case)
    with _limit(0 if wide else TEAM_LIMIT):
        run = E.RunConfig(5, training=True, math="x3")
        assert not (wide and E.fused_path(batch, run) != 0)           # limit 0: the wide kernels
        assert wide or N != 6 or E.fused_path(batch, run) == 3         # small batch: the fused team loops
        got = _train(params, batch, case[4], 5, "x3")
    d = X.distances(got, ref)
    ratio = {k: d["g"][k] / band["g"][k] for k in d["g"]}
    print(f"x3 kink-free T={T} N={N} fully={fully} seed={seed} {'wide' if wide else 'team'}: "
          f"z_max {d['z_max']:.2e} (band {band['z_max']:.2e}), z_rms {d['z_rms']:.2e} (band {band['z_rms']:.2e}), "
          f"loss {d['loss']:.2e} (band {band['loss']:.2e}); grad rel-L2 / band worst {max(ratio.values()):.2f} "
          f"({max(ratio, key=ratio.get)}); " + " ".join(f"{k}={d['g'][k]:.1e}/{band['g'][k]:.1e}" for k in ratio))
    assert d["z_max"] <= BAND_FACTOR * band["z_max"], ("logit max", d["z_max"], band["z_max"])
    assert d["z_rms"] <= BAND_FACTOR * band["z_rms"], ("logit rms", d["z_rms"], band["z_rms"])
    assert d["loss"] <= BAND_FACTOR * band["loss"], ("loss", d["loss"], band["loss"])
    for k in ratio:
        assert d["g"][k] <= BAND_FACTOR * band["g"][k], (k, d["g"][k], band["g"][k])


# ------------------------------------------------------------------------ 2. masks, random set
#        id            T  N   fully  S  plan    prop   dropout
MASK_CASES = {
    "n6_full":        (8, 6,  True,  5, "dense", True,  0.0),
    "n9_thr":         (5, 9,  False, 5, "dense", True,  0.0),
    "n20_thr":        (3, 20, False, 5, "dense", True,  0.0),     # 17–32-node wave-tiles
    "n12_full_recv":  (4, 12, True,  5, "recv",  True,  0.0),     # receiver-block column sums
    "n6_no_prop":     (8, 6,  True,  5, "dense", False, 0.0),
    "n6_one_step":    (8, 6,  True,  1, "dense", True,  0.0),
    "n6_dropout":     (8, 6,  True,  5, "dense", True,  0.1),
}
DROP_SEED = 77


@functools.lru_cache(maxsize=None)
def _mask_ref(name):
    T, N, fully, S, plan, prop, dropout = MASK_CASES[name]
    params = O.random_params(5)
    case = X.dense_case(T, N, fully, prop_scale=0.3 if prop else 0.0)
    dr = do = None
    if dropout:   # the engine's own masks, restated (oracle/dropout.py)
        e = case[7]
        dr = DR.relation_mask_towers(DROP_SEED, dropout, np.arange(T), N)[e[:, 0], e[:, 1]]
        do = DR.object_mask_towers(DROP_SEED, dropout, np.arange(T), N).reshape(-1, 100)
    args = X.emu_args(case, S)
    ref = X.loss_and_grads(params, *args, drop_r=dr, drop_o=do)
    d_bf16 = X.distances(X.bf16_ref(params, *args, drop_r=dr, drop_o=do), ref)
    return params, case, ref, d_bf16


@pytest.mark.parametrize("wide", [False, True], ids=["default", "wide"])
@pytest.mark.parametrize("name", list(MASK_CASES))
def test_x3_masks_against_emulator_random(name, wide):
    T, N, fully, S, plan, prop, dropout = MASK_CASES[name]
    params, case, ref, d_bf16 = _mask_ref(name)
    batch = _batch(case, plan, prop)
    with _limit(0 if wide else TEAM_LIMIT):
        got = _train(params, batch, case[4], S, "x3", dropout, DROP_SEED)
    d = X.distances(got, ref)
    ratio = {k: d["g"][k] / d_bf16["g"][k] for k in d["g"]}
    print(f"x3 masks {name} {'wide' if wide else 'default'}: z_max {d['z_max']:.2e} = d_bf16 / {d_bf16['z_max'] / d['z_max']:.0f} "
          f"(d_bf16 {d_bf16['z_max']:.2e}); grad rel-L2 / d_bf16 worst {max(ratio.values()):.4f} ({max(ratio, key=ratio.get)}); "
          + " ".join(f"{k}={ratio[k]:.4f}" for k in ratio))
    assert d["z_max"] <= d_bf16["z_max"] / 32, (d["z_max"], d_bf16["z_max"])
    for k in ratio:
        assert d["g"][k] <= 0.2 * d_bf16["g"][k], (k, d["g"][k], d_bf16["g"][k])


# --------------------------------------------------------------------- 3. not some other math
def test_x3_is_not_another_math():
    params = O.random_params(5)
    case = X.dense_case(8, 6, True)
    obj, Rs, Rr, prop, tgt = case[:5]
    _, zref, _ = O.loss_and_grads(params, obj, Rs, Rr, prop, tgt, 5)
    batch = _batch(case)
    z = {m: _train(params, batch, tgt, 5, m)[1] for m in ("x3", "x6", "bf16")}
    assert not np.array_equal(z["x3"], z["x6"]) and not np.array_equal(z["x3"], z["bf16"])
    d = {m: float(np.abs(z[m].astype(np.float64) - zref.reshape(-1)).max()) for m in z}
    print("max |dlogit| from the fp64 oracle:", {m: f"{v:.2e}" for m, v in d.items()}, f"bf16 / x3 = {d['bf16'] / d['x3']:.0f}")
    assert d["x3"] > d["x6"]
    assert 32 * d["x3"] <= d["bf16"]


# ----------------------------------------------------------------------- 4. invariants, bitwise
def _equal(a, b, what):
    np.testing.assert_allclose(a[1], b[1], rtol=0, atol=0, err_msg=f"{what}: logits")
    assert a[0] == b[0], (what, "loss")
    for k in a[2]:
        np.testing.assert_allclose(a[2][k], b[2][k], rtol=0, atol=0, err_msg=f"{what}: {k}")
    for i in (3, 4):
        if a[i] is not None:
            np.testing.assert_allclose(a[i], b[i], rtol=0, atol=0, err_msg=f"{what}: output {i}")


@pytest.fixture(scope="module")
def inv_case():
    case = X.dense_case(8, 6, True)
    return O.random_params(5), case, _batch(case)


def test_x3_two_runs_agree_bitwise(inv_case):
    params, case, batch = inv_case
    a = _train(params, batch, case[4], 5, "x3", 0.1, 3, want_dprop=True, inputs=True)
    b = _train(params, batch, case[4], 5, "x3", 0.1, 3, want_dprop=True, inputs=True)
    _equal(a, b, "two x3 runs")
    assert np.abs(a[3]).max() > 0 and np.abs(a[4]).max() > 0


def test_x3_team_and_wide_kernels_agree_bitwise(inv_case):
    params, case, batch = inv_case
    outs = []
    for limit in (TEAM_LIMIT, 0):
        with _limit(limit):
            assert (E.fused_path(batch, E.RunConfig(5, training=True, math="x3", dropout=0.1, seed=3)) != 0) == (limit > 0)
            outs.append(_train(params, batch, case[4], 5, "x3", 0.1, 3, want_dprop=True))
    _equal(outs[0], outs[1], "team vs wide")


def test_x3_da_stored_steps_agree_bitwise(inv_case):
    params, case, batch = inv_case
    outs = []
    with E.wide_kernels():
        for k in (0, 3):
            with E.da_stored(k):
                assert E.da_stored_steps() == k
                outs.append(_train(params, batch, case[4], 5, "x3", 0.1, 3, want_dprop=True))
    _equal(outs[0], outs[1], "stored dh1pre steps K = 0 vs 3")


def test_x3_inference_forward_equals_training_forward(inv_case):
    params, case, batch = inv_case
    flat = P.to_flat(params, device="cuda")
    for wide in (False, True):
        with _limit(0 if wide else TEAM_LIMIT):
            zt = E.forward(flat, batch, E.RunConfig(5, training=True, math="x3"), E.Workspace("cuda"))
            zi = E.forward(flat, batch, E.RunConfig(5, training=False, math="x3"), E.Workspace("cuda"))
            torch.cuda.synchronize()
        np.testing.assert_allclose(zi.cpu().numpy(), zt.cpu().numpy(), rtol=0, atol=0)


def _plans(n):
    plans, tgts = [], []
    for seed in range(1, n + 1):
        raw = D.synthetic_towers(32, 6, seed=seed)
        obj = (raw / D.RELATION_THRESHOLD).astype(np.float32)
        Rs, Rr = D.relation_matrices(raw, D.RELATION_THRESHOLD)
        e = np.array(O.dense_to_edges(Rs, Rr), np.int64).reshape(-1, 4)
        te = np.bincount(e[:, 0], minlength=32).astype(np.int32)
        plans.append(HostPlan.build(obj.reshape(-1, 3), np.full(32, 6, np.int32), e[:, 0] * 6 + e[:, 2],
                                    e[:, 0] * 6 + e[:, 3], te, edge_cap=30))
        tgts.append(np.random.default_rng(seed).integers(0, 2, 192).astype(np.float32))
    return plans, tgts


def test_x3_trainer_replay_equals_step_bitwise():
    params = O.random_params(12)
    plans, tgts = _plans(3)
    ta = Trainer(P.to_flat(params, device="cuda"), mp_steps=5, dropout=0.1, seed=11, math="x3")
    for p, t in zip(plans, tgts):
        ta.step(TowerBatch.from_plan(p, "cuda"), torch.as_tensor(t, device="cuda"))
    tb = Trainer(P.to_flat(params, device="cuda"), mp_steps=5, dropout=0.1, seed=11, math="x3")
    rs = ReplayStep(plans[0], "cuda", tb.replay_body(plans[0].n_nodes))
    for p, t in zip(plans, tgts):
        tb.replay_step(rs, p, t)
    torch.cuda.synchronize()
    assert rs.replays == 2
    assert torch.equal(ta.params, tb.params) and torch.equal(ta.m, tb.m) and torch.equal(ta.v, tb.v)
    # ... and it is x3 that ran: the same steps in x6 end elsewhere
    tc = Trainer(P.to_flat(params, device="cuda"), mp_steps=5, dropout=0.1, seed=11, math="x6")
    tc.step(TowerBatch.from_plan(plans[0], "cuda"), torch.as_tensor(tgts[0], device="cuda"))
    td = Trainer(P.to_flat(params, device="cuda"), mp_steps=5, dropout=0.1, seed=11, math="x3")
    td.step(TowerBatch.from_plan(plans[0], "cuda"), torch.as_tensor(tgts[0], device="cuda"))
    torch.cuda.synchronize()
    assert not torch.equal(tc.m, td.m)


def test_x3_keras_fit_replayed_equals_eager_bitwise():
    obj, Rs, Rr, prop, tgt = D.synthetic_batch(80, 6, seed=7, fully_connected=False)
    x = {"objects": obj, "sender_relations": Rs, "receiver_relations": Rr, "propagation": prop}
    y = {"target": tgt.reshape(80, 6, 1)}
    res = []
    for graph in (True, False):
        model = PropagationNetwork(seed=0, math="x3").getModel(6)
        h = model.fit(x, y, batch_size=32, epochs=2, validation_split=0.2, verbose=0, graph=graph)
        torch.cuda.synchronize()
        res.append((h, model.net.flat.detach().cpu().numpy().copy()))
    assert res[0][0] == res[1][0]
    np.testing.assert_allclose(res[0][1], res[1][1], rtol=0, atol=0)
    m6 = PropagationNetwork(seed=0).getModel(6)
    h6 = m6.fit(x, y, batch_size=32, epochs=2, validation_split=0.2, verbose=0)
    assert h6 != res[0][0]                                   # the x3 models ran x3


# ------------------------------------------------------------------------------- 5. d/d objects
def _dobj_oracle(params, case, S=5):
    """fp64 autograd through the oracle's gather form with the objects as the leaf, mean BCE — the
    reference tests/test_gpu_input_grad.py builds."""
    obj, _, _, prop, tgt, src, dst, _ = case
    tp = O.to_torch(params)
    x = torch.tensor(obj.reshape(-1, 3), dtype=torch.float64, requires_grad=True)
    z = O.forward_gather(tp, x, torch.as_tensor(src), torch.as_tensor(dst),
                         torch.as_tensor(prop.reshape(-1, 100), dtype=torch.float64), S)
    O.keras_bce_from_logits(z, torch.as_tensor(tgt, dtype=torch.float64).reshape(z.shape)).backward()
    return x.grad.numpy().copy()


def test_x3_input_gradients():
    params = X.kink_free_params(1)
    case = X.dense_case(8, 6, True, seed=1)
    ref = _dobj_oracle(params, case)
    batch = _batch(case)
    d = {m: OB.rel_l2(_train(params, batch, case[4], 5, m, inputs=True)[4], ref) for m in ("x3", "bf16")}
    print(f"d/d objects rel-L2 from fp64: x3 {d['x3']:.2e}, bf16 {d['bf16']:.2e} (ratio {d['bf16'] / d['x3']:.0f})")
    assert 32 * d["x3"] <= d["bf16"]
    # demolish.stability_gradients on an x3 net: runs, and agrees with its x6 value to that distance
    towers = np.asarray(case[0], np.float64) * D.RELATION_THRESHOLD
    out = {}
    for m in ("x3", "x6"):
        net = GraphNetwork(device="cuda", params=params, math=m)
        s, g = demolish.stability_gradients(net, towers)
        torch.cuda.synchronize()
        out[m] = (s.cpu().numpy(), g.cpu().numpy())
    assert out["x3"][1].shape == (8, 6, 3) and np.isfinite(out["x3"][1]).all()
    dg = OB.rel_l2(out["x3"][1], out["x6"][1].astype(np.float64))
    print(f"stability_gradients x3 vs x6 rel-L2 {dg:.2e}")
    assert 32 * dg <= d["bf16"]
    assert not np.array_equal(out["x3"][1], out["x6"][1])
