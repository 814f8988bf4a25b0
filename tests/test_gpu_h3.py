"""GPU: h3 math (SPWGNN_MATH_H3) — the forward's matrix products on two fp16 parts per
operand and three f16 MFMA products per fp32 product, the backward x6's.

1. Logits against the fp64 oracle at x6's criterion, |Δ| ≤ 1e-5 + 1e-5·|z|, training forward and
   inference, S ∈ {1, 5}, with and without a 'propagation' input, on every forward path: the fused
   loops, the per-phase team kernels, 17–32-node tiles, receiver-block plans, the wide kernels (one
   workgroup, and five node blocks in two workgroups with a partial last block) and a packed plan.
2. It is the defined arithmetic: the engine's h3 logits are at least 4× closer to fp64 than the
   engine's x3 logits (the emulators give 21×; bf16 parts, or flushed subnormal low parts — every
   glorot weight's low part is a subnormal half — would fail this by an order of magnitude).
3. Logits against the fp64 h3 emulator (tests/h3_emu.py) on the kink-free sets within 2.5× the band of
   valid fp32 implementations; tests/test_h3_host.py shows a missing product term ≥ 1300× outside it.
   The band is used for the logits only (see that calibration's docstring).
4. Gradients against the fp64 oracle at x6's criterion, 1e-5·max|g| + 1e-7 per tensor — every weight
   tensor, d/d 'propagation', d/d objects, with a cotangent on the final state — on kink-free
   parameters with the oracle's ReLU margin asserted, team and wide kernels.
5. The bitwise invariants x6 has.
Cases, fp64 references and the one-step driver are tests/test_gpu_state.py's (computed once, shared).
The whole file also passes under SPWGNN_POISON_WORKSPACE=1.
"""
import functools

import numpy as np
import pytest
import torch

import h3_emu as H
import test_gpu_state as TS
import x3_emu as X
from oracle import model as O
from spwgnn_amd import TowerBatch, data as D, engine as E, params as P
from spwgnn_amd.batch import HostPlan
from spwgnn_amd.replay import ReplayStep
from spwgnn_amd.trainer import Trainer

pytestmark = pytest.mark.gpu

BAND_FACTOR = 2.5


# ------------------------------------------------------------------------ 1. logits, fp64 oracle
FWD_SHAPES = ["n6_full", "n9_thr_recv", "n20_thr", "n12_recv", "n6_wide8", "n6_wide23", "packed"]


@pytest.mark.parametrize("prop", [True, False], ids=["prop", "noprop"])
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("name", FWD_SHAPES)
def test_h3_logits_against_oracle(name, S, prop):
    case = TS._case(name)
    zref, _ = TS._fwd_ref(name, S, prop)
    flat = P.to_flat(O.random_params(5), device="cuda")
    with TS._limit(case.wide):
        batch = case.batch(prop)
        for training in (True, False):
            run = TS._run(S, "h3", training)
            TS._assert_path(name, batch, run)
            z = E.forward(flat, batch, run, E.Workspace("cuda"))
            torch.cuda.synchronize()
            got = batch.to_input_order(z.cpu().numpy())
            share = float((np.abs(got - zref) / (1e-5 + 1e-5 * np.abs(zref))).max())
            print(f"h3 logits {name} S={S} prop={prop} training={training}: max|dz| {np.abs(got - zref).max():.2e}, "
                  f"{share:.3f} of the criterion")
            assert TS._close(got, zref), share


# ------------------------------------------------------------------- 2. the defined arithmetic
def test_h3_is_fp16_parts_not_another_math():
    params = O.random_params(5)
    case = X.dense_case(8, 6, True)
    obj, Rs, Rr, prop, tgt = case[:5]
    _, zref, _ = O.loss_and_grads(params, obj, Rs, Rr, prop, tgt, 5)
    batch = TowerBatch.from_dense(obj, Rs, Rr, prop, device="cuda")
    flat = P.to_flat(params, device="cuda")
    z = {}
    for m in ("h3", "x3", "x6"):
        z[m] = E.forward(flat, batch, E.RunConfig(5, training=True, math=m), E.Workspace("cuda")).cpu().numpy()
    torch.cuda.synchronize()
    d = {m: float(np.abs(z[m].astype(np.float64) - zref.reshape(-1)).max()) for m in z}
    print("max |dlogit| from the fp64 oracle:", {m: f"{v:.2e}" for m, v in d.items()}, f"x3 / h3 = {d['x3'] / d['h3']:.1f}")
    assert not np.array_equal(z["h3"], z["x3"]) and not np.array_equal(z["h3"], z["x6"])
    assert d["h3"] <= d["x3"] / 4, d


# ------------------------------------------------------------- 3. logits, the fp64 h3 emulator
@functools.lru_cache(maxsize=None)
def _kink_ref(T, N, fully, seed):
    params = X.kink_free_params(seed)
    case = X.dense_case(T, N, fully, seed=seed)
    ref, band = H.noise_band(params, *X.emu_args(case))
    return params, case, ref, band


@pytest.mark.parametrize("wide", [False, True], ids=["team", "wide"])
@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("T,N,fully", [(8, 6, True), (5, 9, False)])
def test_h3_logits_against_emulator_kink_free(T, N, fully, seed, wide):
    params, case, ref, band = _kink_ref(T, N, fully, seed)
    assert band["z_max"] <= 2e-5, band["z_max"]     # precondition: a kinked input cannot loosen the test
    obj, Rs, Rr, prop = case[:4]
    batch = TowerBatch.from_dense(obj, Rs, Rr, prop, device="cuda")
    with TS._limit(wide):
        run = E.RunConfig(5, training=True, math="h3")
        assert (E.fused_path(batch, run) == 0) == wide
        z = E.forward(P.to_flat(params, device="cuda"), batch, run, E.Workspace("cuda"))
        torch.cuda.synchronize()
    dz = z.cpu().numpy().astype(np.float64) - ref[1]
    z_max, z_rms = float(np.abs(dz).max()), float(np.sqrt(np.mean(dz ** 2)))
    print(f"h3 kink-free T={T} N={N} fully={fully} seed={seed} {'wide' if wide else 'team'}: z_max {z_max:.2e} "
          f"(band {band['z_max']:.2e}), z_rms {z_rms:.2e} (band {band['z_rms']:.2e})")
    assert z_max <= BAND_FACTOR * band["z_max"], ("logit max", z_max, band["z_max"])
    assert z_rms <= BAND_FACTOR * band["z_rms"], ("logit rms", z_rms, band["z_rms"])


# --------------------------------------------------------------------- 4. gradients, fp64 oracle
@pytest.mark.parametrize("wide", [False, True], ids=["team", "wide"])
@pytest.mark.parametrize("name", ["n6_full", "n9_thr", "n20_thr"])
def test_h3_gradients_against_oracle(name, wide):
    """L = BCE(z) + Σ w ⊙ P_S (a cotangent on the final state), S = 5: every weight tensor, d/d
    'propagation' and d/d objects at x6's criterion."""
    case = TS._case(name)
    ref_g, ref_dprop, ref_dpos, margin = TS._grad_ref(name, 5, True)
    assert margin >= TS.MIN_RELU_MARGIN, margin
    with TS._limit(wide):
        batch = case.batch(True)
        if wide:
            assert E.fused_path(batch, TS._run(5, "h3")) == 0
        got = TS._step(X.kink_free_params(1), case, 5, "h3", batch=batch, check_path=not wide)
    ref = dict(ref_g, dpos=ref_dpos, dprop=ref_dprop)
    have = dict(got["g"], dpos=got["dpos"], dprop=got["dprop"])
    worst, at = 0.0, None
    for k in ref:
        err, bound = TS._maxabs(have[k], ref[k]), 1e-5 * np.abs(ref[k]).max() + 1e-7
        if err / bound > worst:
            worst, at = err / bound, k
    print(f"h3 gradients {name} {'wide' if wide else 'team'}: ReLU margin {margin:.3f}, worst err / bound {worst:.3f} ({at})")
    for k in ref:
        err, bound = TS._maxabs(have[k], ref[k]), 1e-5 * np.abs(ref[k]).max() + 1e-7
        assert err <= bound, (k, err, bound)


# ----------------------------------------------------------------------- 5. invariants, bitwise
def test_h3_two_runs_agree_bitwise():
    case = TS._case("n6_full")
    params = O.random_params(5)
    a = TS._step(params, case, 5, "h3", dropout=0.1, seed=3)
    b = TS._step(params, case, 5, "h3", dropout=0.1, seed=3)
    TS._bits(a, b, "two h3 runs")
    assert np.isfinite(a["z"]).all() and np.abs(a["dprop"]).max() > 0 and np.abs(a["dpos"]).max() > 0


def test_h3_team_and_wide_kernels_agree_bitwise():
    case = TS._case("n6_full")
    params = O.random_params(5)
    outs = []
    for wide in (False, True):
        with TS._limit(wide):
            batch = case.batch(True)
            assert (E.fused_path(batch, TS._run(5, "h3", dropout=0.1, seed=3)) != 0) == (not wide)
            outs.append(TS._step(params, case, 5, "h3", dropout=0.1, seed=3, batch=batch, check_path=False))
    TS._bits(outs[0], outs[1], "team vs wide")


@pytest.mark.parametrize("name", ["n6_full", "n9_thr_recv", "n6_wide23"])
def test_h3_inference_equals_training_forward_and_state_buffer_changes_nothing(name):
    case = TS._case(name)
    flat = P.to_flat(O.random_params(5), device="cuda")
    with TS._limit(case.wide):
        batch = case.batch(True)
        zs = []
        for training in (True, False):
            run = TS._run(5, "h3", training)
            z0 = E.forward(flat, batch, run, E.Workspace("cuda"))                       # state_out = NULL
            z1, st = E.forward(flat, batch, run, E.Workspace("cuda"), return_state=True)   # a state buffer
            torch.cuda.synchronize()
            assert torch.equal(z0, z1) and torch.isfinite(st).all()
            zs.append(z0)
        assert torch.equal(zs[0], zs[1])


def test_h3_da_stored_steps_agree_bitwise():
    case = TS._case("n6_wide23")
    params = O.random_params(5)
    outs = []
    with E.wide_kernels():
        for k in (0, 3):
            with E.da_stored(k):
                assert E.da_stored_steps() == k
                outs.append(TS._step(params, case, 5, "h3", dropout=0.1, seed=3))
    TS._bits(outs[0], outs[1], "stored dh1pre steps K = 0 vs 3")


def test_h3_trainer_replay_equals_step_bitwise():
    params = O.random_params(12)
    plans, tgts = [], []
    for seed in (1, 2):
        raw = D.synthetic_towers(32, 6, seed=seed)
        obj = (raw / D.RELATION_THRESHOLD).astype(np.float32)
        Rs, Rr = D.relation_matrices(raw, D.RELATION_THRESHOLD)
        e = np.array(O.dense_to_edges(Rs, Rr), np.int64).reshape(-1, 4)
        te = np.bincount(e[:, 0], minlength=32).astype(np.int32)
        plans.append(HostPlan.build(obj.reshape(-1, 3), np.full(32, 6, np.int32), e[:, 0] * 6 + e[:, 2],
                                    e[:, 0] * 6 + e[:, 3], te, edge_cap=30))
        tgts.append(np.random.default_rng(seed).integers(0, 2, 192).astype(np.float32))
    ta = Trainer(P.to_flat(params, device="cuda"), mp_steps=5, dropout=0.1, seed=11, math="h3")
    for p, t in zip(plans, tgts):
        ta.step(TowerBatch.from_plan(p, "cuda"), torch.as_tensor(t, device="cuda"))
    tb = Trainer(P.to_flat(params, device="cuda"), mp_steps=5, dropout=0.1, seed=11, math="h3")
    rs = ReplayStep(plans[0], "cuda", tb.replay_body(plans[0].n_nodes))
    for p, t in zip(plans, tgts):
        tb.replay_step(rs, p, t)
    torch.cuda.synchronize()
    assert rs.replays == 1                                  # the second step is a replay
    assert torch.equal(ta.params, tb.params) and torch.equal(ta.m, tb.m) and torch.equal(ta.v, tb.v)
    # ... and it is h3 that ran: the same first step in x6 ends elsewhere
    tc = Trainer(P.to_flat(params, device="cuda"), mp_steps=5, dropout=0.1, seed=11, math="x6")
    tc.step(TowerBatch.from_plan(plans[0], "cuda"), torch.as_tensor(tgts[0], device="cuda"))
    td = Trainer(P.to_flat(params, device="cuda"), mp_steps=5, dropout=0.1, seed=11, math="h3")
    td.step(TowerBatch.from_plan(plans[0], "cuda"), torch.as_tensor(tgts[0], device="cuda"))
    torch.cuda.synchronize()
    assert not torch.equal(tc.m, td.m)
