"""h3 math (SPWGNN_MATH_H3) without a GPU: the C-ABI's math ids and product counts, the
math mode carried through the Python front ends, the h3 emulator (tests/h3_emu.py) against the fp64
oracle and the x3 emulator, and the calibration of the band tests/test_gpu_h3.py holds the logits to."""
import types

import numpy as np
import pytest
import torch

import h3_emu as H
import x3_emu as X
from oracle import bf16 as OB
from oracle import model as O
from spwgnn_amd import TowerBatch, _lib, demolish, engine as E
from spwgnn_amd.keras_api import KerasModel, PropagationNetwork
from spwgnn_amd.network import GraphNetwork
from spwgnn_amd.trainer import Trainer


# ------------------------------------------------------------------------------------------ C-ABI
def test_math_ids_and_product_counts():
    L = _lib.lib()
    assert L.spwgnn_version() == 8
    assert L.spwgnn_math_products(_lib.MATH_H3) == 3 and L.spwgnn_math_products(99) == -1
    ids = (_lib.MATH_X6, _lib.MATH_X3, _lib.MATH_BF16, _lib.MATH_F32, _lib.MATH_H3, 99)
    assert [L.spwgnn_math_products_bwd(m) for m in ids] == [6, 3, 1, 0, 6, -1]
    assert E.MATH_MODES["h3"] == _lib.MATH_H3 == 4
    assert E.RunConfig(5, math="h3").cstruct().math == 4
    assert E.RunConfig(5).cstruct().math == _lib.MATH_X6          # the default stays x6


# ------------------------------------------------------------------------------- Python front ends
class _Stop(Exception):
    pass


@pytest.fixture
def runs(monkeypatch):
    """Every RunConfig that reaches engine.forward, which stops the call there (no GPU work)."""
    seen = []

    def forward(flat, batch, run, ws, *a, **k):
        seen.append(run)
        raise _Stop

    monkeypatch.setattr(E, "forward", forward)
    return seen


def _inputs(B=2, N=4):
    obj, Rs, Rr, prop, tgt, *_ = X.dense_case(B, N, True)
    x = {"objects": obj, "sender_relations": Rs, "receiver_relations": Rr, "propagation": prop}
    return x, tgt


def test_graph_network_carries_h3(runs):
    net = GraphNetwork(device="cpu", math="h3")
    assert net.math == "h3" and net.run_config().math == "h3" and net.run_config(True, dropout=0.1).math == "h3"
    x, _ = _inputs()
    args = (x["objects"], x["sender_relations"], x["receiver_relations"], x["propagation"])
    with torch.no_grad(), pytest.raises(_Stop):
        net.forward_logits(*args)                       # inference
    with pytest.raises(_Stop):
        net.forward_logits(*args)                       # training (autograd)
    with pytest.raises(_Stop):
        net.forward_pooled(*args)
    assert [r.math for r in runs] == ["h3"] * 3
    assert [r.training for r in runs] == [False, True, False]


def test_keras_model_uses_h3_in_all_four_places(runs):
    model = PropagationNetwork(device="cpu", math="h3").getModel(4)
    assert isinstance(model, KerasModel) and model.net.math == "h3"
    x, tgt = _inputs()
    batch = TowerBatch.from_dense(x["objects"], x["sender_relations"], x["receiver_relations"], x["propagation"], device="cpu")
    t = torch.as_tensor(tgt.reshape(-1))
    with pytest.raises(_Stop):
        model.predict(x)
    with pytest.raises(_Stop):
        model.train_on_batch(batch, t)
    with pytest.raises(_Stop):
        model.evaluate_batch(batch, t)
    model._ctr = types.SimpleNamespace(key=None, step=None)      # the replayed body reads only these here
    model._w3[batch.n_towers] = None
    with pytest.raises(_Stop):
        model._replay_body()(batch, t, None, None, None, None)
    assert [r.math for r in runs] == ["h3"] * 4
    assert [r.training for r in runs] == [False, True, False, True]


def test_demolish_uses_h3(runs):
    net = GraphNetwork(device="cpu", math="h3")
    towers = np.random.default_rng(0).uniform(10, 300, (3, 4, 3))
    with pytest.raises(_Stop):
        demolish.stability_sums(net, towers)
    with pytest.raises(_Stop):
        demolish.stability_gradients(net, towers)
    assert [(r.math, r.training) for r in runs] == [("h3", False), ("h3", True)]


def test_trainer_carries_h3_and_defaults_stay_x6():
    flat = torch.zeros(64)
    run = Trainer(flat, engine=object(), math="h3").run_config()      # (no engine call is made here)
    assert run.math == "h3" and run.training and run.cstruct().math == _lib.MATH_H3
    assert Trainer(flat, engine=object()).run_config().math == "x6"
    assert GraphNetwork(device="cpu").math == "x6"
    assert PropagationNetwork(device="cpu").getModel(4).net.math == "x6"
    assert E.RunConfig(5).math == "x6"
    with pytest.raises(ValueError):
        E.RunConfig(5, math="h4").cstruct()
    with pytest.raises(ValueError):
        GraphNetwork(device="cpu", math="h4")


# ------------------------------------------------------------------------------------ the emulator
def test_h3_split_is_two_part_fp16_rne():
    f16 = lambda t: t.to(torch.float32).to(torch.float16).to(torch.float64)
    x = torch.tensor([0.07, 1 + 2.0 ** -11 + 2.0 ** -21, 6e4, 3.14159265358979, -1e-3], dtype=torch.float64)
    x = x.to(torch.float32).to(torch.float64)            # fp32 values, as the engine's operands are
    h, m = H.split(x)
    assert torch.equal(h, f16(x)) and torch.equal(m, f16(x - h))
    # 0.07: the low part is a subnormal half (below 2^-14) and is kept, not flushed
    assert 0 < abs(float(m[0])) < 2.0 ** -14
    # the two parts carry 22 bits of mantissa (|x − h| ≤ 2^-11·|x|, and m keeps 11 bits of that) down to
    # the floor of half a subnormal ulp, 2^-25 absolute
    err = (x - (h + m)).abs()
    assert float(err[0]) <= 2.0 ** -25
    assert bool((err <= torch.maximum(torch.full_like(x, 2.0 ** -25), 2.0 ** -22 * x.abs())).all())
    # 1 + 2^-11 + 2^-21: just above the tie, so h = 1 + 2^-10 and m = 2^-21 − 2^-11 < 0, nothing lost
    assert float(h[1]) == 1.0 + 2.0 ** -10 and float(m[1]) == 2.0 ** -21 - 2.0 ** -11 and float(err[1]) == 0.0
    # one fp16 alone keeps 11 bits
    assert float(((x - h).abs() / x.abs()).max()) > 2.0 ** -13
    # range: at or above 65,520 the high part is inf (65,504 is the largest half)
    big = torch.tensor([65519.0, 65520.0, 7e4, -1e5], dtype=torch.float64)
    hb, _ = H.split(big)
    assert float(hb[0]) == 65504.0 and torch.isinf(hb[1:]).all() and float(hb[3]) < 0


def test_h3_emulator_is_the_reference_graph_and_is_fp32_class():
    """Rounding off: the h3 emulator equals oracle.model's fp64 loss, logits and gradients to 1e-12.
    Rounding on, (8, 6, full) with random_params(5): its logits are further than 1e-8 from fp64 (it
    does round) and at least 8× closer than the x3 emulator's (measured 21×; 8 is a condition: two
    fp16 parts carry 22 mantissa bits where two bf16 parts carry 16). The backward takes unrounded
    operands, so its gradients differ from fp64 only through the forward's values."""
    params = O.random_params(5)
    case = X.dense_case(8, 6, True)
    obj, Rs, Rr, prop, tgt = case[:5]
    lref, zref, gref = O.loss_and_grads(params, obj, Rs, Rr, prop, tgt, 5)
    zref = zref.reshape(-1)
    try:
        OB.ROUND = False
        l0, z0, g0 = H.loss_and_grads(params, *X.emu_args(case))
    finally:
        OB.ROUND = True
    assert abs(l0 - lref) < 1e-12 and np.abs(z0 - zref).max() < 1e-12
    for k in gref:
        assert np.abs(g0[k] - gref[k]).max() <= 1e-12 * np.abs(gref[k]).max(), k
    _, zh, gh = H.loss_and_grads(params, *X.emu_args(case))
    _, z3, _ = X.loss_and_grads(params, *X.emu_args(case))
    dh, d3 = np.abs(zh - zref).max(), np.abs(z3 - zref).max()
    crit = float((np.abs(zh - zref) / (1e-5 + 1e-5 * np.abs(zref))).max())
    print(f"max |dlogit| from fp64: h3 {dh:.2e} ({crit:.2f} of the 1e-5 criterion), x3 {d3:.2e} (ratio {d3 / dh:.0f})")
    assert dh > 1e-8
    assert 8 * dh <= d3
    assert crit <= 0.5
    assert OB._MM is not H._MMH3 and OB._Round is not H._RoundH3 and OB.b16(torch.tensor([1.001]))[0] != 1.001   # undone


# ------------------------------------------------------------------- calibration of the GPU criteria
BAND_FACTOR = 2.5          # tests/test_gpu_h3.py, as tests/test_gpu_x3.py holds x3
KINK_CASES = [(8, 6, True), (5, 9, False)]


@pytest.mark.parametrize("T,N,fully", KINK_CASES)
@pytest.mark.parametrize("seed", [1, 2])
def test_h3_band_calibration_kink_free(T, N, fully, seed):
    """On the kink-free sets the k-block-8 fp32 variant (not one of the band's own) lies within 1.6× the
    band in the logits, and the emulator with the forward term X_m·W_h removed lies outside 2.5× the
    band in the logits: the band DISCRIMINATES THE LOGITS (max and rms), and the GPU test uses it for
    them. It is not used for the gradients: h3's backward is x6's on unrounded operands, so the
    emulator's gradients are the fp64 oracle's up to the forward's 1e-7-class perturbation and the band
    there is pure fp32 accumulation noise of the emulator's own products, which says nothing about the
    engine's x6 backward — the GPU test holds the gradients to x6's criterion against the oracle."""
    params = X.kink_free_params(seed)
    case = X.dense_case(T, N, fully, seed=seed)
    args = X.emu_args(case)
    ref, band = H.noise_band(params, *args)
    assert band["z_max"] <= 2e-5, band
    alt = X.distances(H.loss_and_grads(params, *args, dtype=torch.float32, kblock=8), ref)
    fwd = X.distances(H.loss_and_grads(params, *args, mutant="fwd"), ref)
    print(f"band z_max {band['z_max']:.2e} z_rms {band['z_rms']:.2e}; k8 / band {alt['z_max'] / band['z_max']:.2f}; "
          f"fwd mutant z_max {fwd['z_max'] / band['z_max']:.0f}x, z_rms {fwd['z_rms'] / band['z_rms']:.0f}x the band")
    assert alt["z_max"] <= 1.6 * band["z_max"] + 1e-9 and alt["z_rms"] <= 1.6 * band["z_rms"] + 1e-9
    assert fwd["z_max"] > BAND_FACTOR * band["z_max"]
    assert fwd["z_rms"] > BAND_FACTOR * band["z_rms"]
