"""x3 math (SPWGNN_MATH_X3) without a GPU: the C-ABI's math ids, the math mode carried
through the Python front ends, the x3 emulator (tests/x3_emu.py) against the fp64 oracle, and the
calibration of the two criteria tests/test_gpu_x3.py holds the engine to."""
import types

import numpy as np
import pytest
import torch

import x3_emu as X
from oracle import bf16 as OB
from oracle import model as O
from spwgnn_amd import TowerBatch, _lib, demolish, engine as E
from spwgnn_amd.keras_api import KerasModel, PropagationNetwork
from spwgnn_amd.network import GraphNetwork


# ------------------------------------------------------------------------------------------ C-ABI
def test_math_products_and_run_config():
    L = _lib.lib()
    assert L.spwgnn_version() == 8
    got = [L.spwgnn_math_products(m) for m in (_lib.MATH_X6, _lib.MATH_X3, _lib.MATH_BF16, _lib.MATH_F32, 99)]
    assert got == [6, 3, 1, 0, -1]
    assert E.MATH_MODES["x3"] == _lib.MATH_X3 == 3
    assert E.RunConfig(5, math="x3").cstruct().math == 3
    assert E.RunConfig(5).cstruct().math == _lib.MATH_X6          # the default stays x6
    with pytest.raises(ValueError):
        E.RunConfig(5, math="x4").cstruct()


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


@pytest.mark.parametrize("math", ["x3", "bf16", "x6"])
def test_graph_network_carries_its_math(runs, math):
    net = GraphNetwork(device="cpu", math=math)
    assert net.math == math and net.run_config().math == math and net.run_config(True, dropout=0.1).math == math
    x, _ = _inputs()
    args = (x["objects"], x["sender_relations"], x["receiver_relations"], x["propagation"])
    with torch.no_grad(), pytest.raises(_Stop):
        net.forward_logits(*args)                       # inference
    with pytest.raises(_Stop):
        net.forward_logits(*args)                       # training (autograd)
    with pytest.raises(_Stop):
        net.forward_pooled(*args)
    assert [r.math for r in runs] == [math] * 3
    assert [r.training for r in runs] == [False, True, False]


def test_graph_network_default_and_unknown_math():
    assert GraphNetwork(device="cpu").math == "x6"
    assert PropagationNetwork(device="cpu").getModel(4).net.math == "x6"
    with pytest.raises(ValueError):
        GraphNetwork(device="cpu", math="fp8")
    with pytest.raises(ValueError):
        PropagationNetwork(device="cpu", math="fp8")


def test_keras_model_uses_its_nets_math_in_all_four_places(runs):
    model = PropagationNetwork(device="cpu", math="x3").getModel(4)
    assert isinstance(model, KerasModel) and model.net.math == "x3"
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
    assert [r.math for r in runs] == ["x3"] * 4
    assert [r.training for r in runs] == [False, True, False, True]


def test_demolish_uses_the_nets_math(runs):
    net = GraphNetwork(device="cpu", math="x3")
    towers = np.random.default_rng(0).uniform(10, 300, (3, 4, 3))
    with pytest.raises(_Stop):
        demolish.stability_sums(net, towers)
    with pytest.raises(_Stop):
        demolish.stability_gradients(net, towers)
    assert [(r.math, r.training) for r in runs] == [("x3", False), ("x3", True)]


# ------------------------------------------------------------------------------------ the emulator
def test_x3_emulator_is_the_reference_graph_and_sits_between_bf16_and_exact():
    """Rounding off: the x3 emulator equals oracle.model's fp64 loss, logits and gradients to 1e-12
    (the bf16 emulator's bound). Rounding on: its logits are further from fp64 than 1e-7 and at least
    32× closer than the bf16 emulator's, on (8, 6, full) with random parameters."""
    params = O.random_params(5)
    case = X.dense_case(8, 6, True)
    obj, Rs, Rr, prop, tgt = case[:5]
    lref, zref, gref = O.loss_and_grads(params, obj, Rs, Rr, prop, tgt, 5)
    zref = zref.reshape(-1)
    try:
        OB.ROUND = False
        l0, z0, g0 = X.loss_and_grads(params, *X.emu_args(case))
    finally:
        OB.ROUND = True
    assert abs(l0 - lref) < 1e-12 and np.abs(z0 - zref).max() < 1e-12
    for k in gref:
        assert np.abs(g0[k] - gref[k]).max() <= 1e-12 * np.abs(gref[k]).max(), k
    _, z3, _ = X.loss_and_grads(params, *X.emu_args(case))
    _, zb, _ = X.bf16_ref(params, *X.emu_args(case))
    d3, db = np.abs(z3 - zref).max(), np.abs(zb - zref).max()
    print(f"max |dlogit| from fp64: x3 {d3:.2e}, bf16 {db:.2e} (ratio {db / d3:.0f})")
    assert d3 > 1e-7
    assert 32 * d3 <= db
    assert OB.b16 is not X.b16x2 and OB._MM is not X._MM3          # the substitutions were undone


def test_x3_split_is_two_part_rne():
    x = torch.tensor([1 + 2.0 ** -8 + 2.0 ** -17, 3.14159265358979, -1e-30, 6e4], dtype=torch.float64)
    h, m = X.split(x)
    assert torch.equal(h, OB.b16(x)) and torch.equal(m, OB.b16(x - h))
    assert float(((x - (h + m)).abs() / x.abs()).max()) <= 2.0 ** -16      # a 16-bit mantissa, no less
    assert float(((x - h).abs() / x.abs()).max()) > 2.0 ** -12             # ... where bf16 keeps 8


# ------------------------------------------------------------------- calibration of the GPU criteria
BAND_FACTOR = 2.5          # tests/test_gpu_x3.py, as tests/test_gpu_fullsize.py holds bf16
KINK_CASES = [(8, 6, True), (5, 9, False)]
FWD_KERNELS = [k for k in O.random_params(1) if k.endswith(".kernel") and k not in ("rm.0.kernel", "om.0.kernel")]


@pytest.mark.parametrize("T,N,fully", KINK_CASES)
@pytest.mark.parametrize("seed", [1, 2])
def test_x3_band_calibration_kink_free(T, N, fully, seed):
    """(a) On the kink-free set the k-block-8 fp32 variant (not one of the band's own) lies within
    1.6× the band; the emulator with one forward product term removed lies outside 2.5× the band in the
    logits and in every kernel gradient, the one with one dW term removed in every kernel gradient it
    touches. The band itself meets the GPU test's preconditions."""
    params = X.kink_free_params(seed)
    case = X.dense_case(T, N, fully, seed=seed)
    args = X.emu_args(case)
    ref, band = X.noise_band(params, *args)
    assert band["z_max"] <= 2e-5 and max(band["g"].values()) <= 2e-4, band
    alt = X.distances(X.loss_and_grads(params, *args, dtype=torch.float32, kblock=8), ref)
    assert alt["z_max"] <= 1.6 * band["z_max"] + 1e-9 and alt["z_rms"] <= 1.6 * band["z_rms"] + 1e-9
    for k in alt["g"]:
        assert alt["g"][k] <= 1.6 * band["g"][k] + 1e-9, (k, alt["g"][k], band["g"][k])
    fwd = X.distances(X.loss_and_grads(params, *args, mutant="fwd"), ref)
    dw = X.distances(X.loss_and_grads(params, *args, mutant="dw"), ref)
    print(f"band z_max {band['z_max']:.2e} worst g {max(band['g'].values()):.2e}; k8/band "
          f"{max(alt['g'][k] / (band['g'][k] + 1e-30) for k in alt['g']):.2f}; fwd mutant z {fwd['z_max'] / band['z_max']:.0f}x, "
          f"min g {min(fwd['g'][k] / band['g'][k] for k in FWD_KERNELS):.0f}x; dW mutant min g "
          f"{min(dw['g'][k] / band['g'][k] for k in FWD_KERNELS):.0f}x")
    assert fwd["z_max"] > BAND_FACTOR * band["z_max"]
    for k in FWD_KERNELS:
        assert fwd["g"][k] > BAND_FACTOR * band["g"][k], ("fwd", k)
        assert dw["g"][k] > BAND_FACTOR * band["g"][k], ("dw", k)


RANDOM_CASES = [(8, 6, True, 5), (5, 9, False, 5), (3, 20, False, 5), (4, 12, True, 5), (8, 6, True, 1)]


@pytest.mark.parametrize("T,N,fully,S", RANDOM_CASES)
def test_x3_mask_thresholds_calibration_random(T, N, fully, S):
    """(b) On the random set every fp32 k-block variant of the x3 emulator lies within half of the GPU
    thresholds (logits d_bf16 / 32, gradients 0.2 · d_bf16 per tensor); the forward mutant exceeds them
    in the logits and in at least one gradient tensor."""
    params = O.random_params(5)
    case = X.dense_case(T, N, fully)
    args = X.emu_args(case, S)
    ref = X.loss_and_grads(params, *args)
    d_bf16 = X.distances(X.bf16_ref(params, *args), ref)
    worst_z, worst_g = 0.0, 0.0
    for kb in OB.NOISE_KBLOCKS + (8,):
        alt = X.distances(X.loss_and_grads(params, *args, dtype=torch.float32, kblock=kb), ref)
        worst_z = max(worst_z, alt["z_max"] / d_bf16["z_max"])
        assert alt["z_max"] <= 0.5 * d_bf16["z_max"] / 32, (kb, alt["z_max"], d_bf16["z_max"])
        for k in alt["g"]:
            worst_g = max(worst_g, alt["g"][k] / d_bf16["g"][k])
            assert alt["g"][k] <= 0.5 * 0.2 * d_bf16["g"][k], (kb, k, alt["g"][k], d_bf16["g"][k])
    fwd = X.distances(X.loss_and_grads(params, *args, mutant="fwd"), ref)
    print(f"valid: z / d_bf16 ≤ 1/{1 / worst_z:.0f}, g / d_bf16 ≤ {worst_g:.3f}; fwd mutant z 1/{d_bf16['z_max'] / fwd['z_max']:.1f}, "
          f"worst g {max(fwd['g'][k] / d_bf16['g'][k] for k in fwd['g']):.2f}")
    assert fwd["z_max"] > d_bf16["z_max"] / 32
    assert any(fwd["g"][k] > 0.2 * d_bf16["g"][k] for k in fwd["g"])
