"""Loop-end shortcuts of the wide split-bf16 kernels: with a null 'propagation'
(P0 = 0) and no d/d'propagation' request the step loop leaves out the work whose operand is exactly
zero or whose result nothing reads — step 0's edge backward, step 0's stages of the W1b / W1c /
omp.0-P weight gradients, P·Wo1p and do1·Wo1pᵀ at step 0, all but the logit's tile of the last
step's o1·Wo2', all but the logit's k-block of the first backward step's dx'·Wo2'ᵀ.

The general path (a zero `prop` array, a dprop request) is the reference: every logit and gradient
of the fast path must equal it value for value (np.array_equal: −0 == +0). Every case runs the wide
kernels on a workspace pre-filled with 0xFF bytes and NaN-filled outputs, so a read of an array the
fast path no longer writes shows up as NaN.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import model as O
from spwgnn_amd import TowerBatch, data as D, engine as E, params as P

gpu = pytest.mark.gpu

SHAPES = ["six", "twelve", "ragged", "box32"]


@functools.lru_cache(maxsize=None)
def _batch(shape: str) -> TowerBatch:
    if shape == "ragged":   # 24 thresholded towers of 4..16 boxes, packed into wave-tiles
        pos, sizes, src, dst, tower_edges, _ = D.ragged_batch(24, 4, 16, seed=7)
        return TowerBatch.from_edges(pos, sizes, src, dst, tower_edges, None, device="cuda")
    # fully connected: 8 six-box towers (12-node wave-tiles, two edge blocks each), 5 twelve-box
    # towers, 3 towers of 32 boxes (the 32-row one-hot path)
    T, N = {"six": (8, 6), "twelve": (5, 12), "box32": (3, 32)}[shape]
    raw = D.synthetic_towers(T, N, seed=4)
    return TowerBatch.fully_connected((raw / D.RELATION_THRESHOLD).astype(np.float32), device="cuda")


@functools.lru_cache(maxsize=None)
def _flat():
    return P.to_flat(O.random_params(seed=29), device="cuda")


def _targets(batch):
    rng = np.random.default_rng(batch.n_nodes)
    return torch.tensor(rng.integers(0, 2, size=batch.n_nodes).astype(np.float32), device="cuda")


def _prop(batch, zero: bool):
    if zero:
        return torch.zeros(batch.n_nodes, 100, device="cuda")
    rng = np.random.default_rng(3)
    return torch.tensor(rng.normal(0, 0.3, size=(batch.n_nodes, 100)).astype(np.float32), device="cuda")


def _poisoned_ws(batch, run):
    """A fresh workspace as SPWGNN_POISON_WORKSPACE fills it: every byte 0xFF (NaN as fp32)."""
    ws = E.Workspace("cuda")
    ws.buf = torch.full((E.workspace_bytes(batch, run),), 0xFF, dtype=torch.uint8, device="cuda")
    return ws


def _forward(batch, run):
    ws = _poisoned_ws(batch, run)
    z = E.forward(_flat(), batch, run, ws, logits=torch.full((batch.n_nodes,), float("nan"), device="cuda"))
    return ws, z


def _train_step(batch, S, math, want_dprop, dropout=0.1):
    """One forward + loss + backward on the wide kernels; (logits, grads, dprop) as numpy arrays."""
    run = E.RunConfig(S, training=True, math=math, dropout=dropout, seed=5)
    with E.wide_kernels():
        assert E.fused_path(batch, run) == 0
        ws, z = _forward(batch, run)
        _, dz = E.bce(z, _targets(batch), E.BceScratch("cuda"))
        g = torch.full_like(_flat(), float("nan"))
        _, dp = E.backward(_flat(), batch, run, ws, dz, grads=g, want_dprop=want_dprop)
        torch.cuda.synchronize()
    return z.cpu().numpy(), g.cpu().numpy(), None if dp is None else dp.cpu().numpy()


@gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("S", [1, 2, 5])   # S = 1: step 0 is both the first and the last step
@pytest.mark.parametrize("math", ["x6", "bf16"])
def test_fast_path_equals_general_path(math, S, shape):
    base = _batch(shape)
    za, ga, _ = _train_step(base, S, math, want_dprop=False)                                  # the fast path
    zb, gb, pb = _train_step(base.with_prop(_prop(base, zero=True)), S, math, want_dprop=True)  # the general path
    zc, gc, pc = _train_step(base, S, math, want_dprop=True)                                  # null prop, dprop asked
    assert np.isfinite(zb).all() and np.isfinite(gb).all() and np.isfinite(pb).all()
    assert np.array_equal(za, zb) and np.array_equal(zc, zb)
    ref = P.from_flat(torch.from_numpy(gb))
    for name, got in (("a", P.from_flat(torch.from_numpy(ga))), ("c", P.from_flat(torch.from_numpy(gc)))):
        for k, r in ref.items():
            assert np.array_equal(got[k], r), (name, k, float(np.abs(got[k] - r).max()))
    assert np.array_equal(ga, gb) and np.array_equal(gc, gb)   # the alignment gaps of the flat buffer too
    assert np.array_equal(pc, pb)


@gpu
@pytest.mark.parametrize("shape,S", [("six", 5), ("six", 1), ("ragged", 2), ("box32", 2)])
@pytest.mark.parametrize("math", ["x6", "bf16"])
def test_nonzero_prop_with_and_without_dprop(math, shape, S):
    """A non-zero prop: only the dP_0 shortcut is active. Step 0's edge backward must still run —
    its dU_0 / dV_0 feed the W1b / W1c gradients (left unwritten they would read 0xFF bytes)."""
    b = _batch(shape)
    b = b.with_prop(_prop(b, zero=False))
    z0, g0, _ = _train_step(b, S, math, want_dprop=False)
    z1, g1, p1 = _train_step(b, S, math, want_dprop=True)
    assert np.isfinite(g0).all() and np.isfinite(g1).all() and np.isfinite(p1).all()
    assert np.array_equal(z0, z1) and np.array_equal(g0, g1)
    w1 = P.from_flat(torch.from_numpy(g0))["rmp.0.kernel"]
    assert np.abs(w1[150:250]).max() > 0 and np.abs(w1[250:]).max() > 0   # W1b, W1c rows: P_0ᵀ·dU_0, P_0ᵀ·dV_0


def _infer(batch, S, math="x6"):
    run = E.RunConfig(S, training=False, math=math)
    with E.wide_kernels():
        assert E.fused_path(batch, run) == 0
        _, z = _forward(batch, run)
        torch.cuda.synchronize()
    return z.cpu().numpy()


@gpu
@pytest.mark.parametrize("shape,S", [("box32", 1), ("box32", 2), ("box32", 10), ("six", 2)])
def test_inference_null_prop_equals_zero_prop(shape, S):
    """training=False: P alternates between two rows (P_at(s & 1)); the dropped P0 and P_S stores
    must not be what a later step reads."""
    b = _batch(shape)
    z_null = _infer(b, S)
    z_zero = _infer(b.with_prop(_prop(b, zero=True)), S)
    assert np.isfinite(z_zero).all()
    assert np.array_equal(z_null, z_zero)


@gpu
def test_inference_null_prop_captured_replay():
    """The fast-path inference forward captured into a hipGraph replays to the general path's logits."""
    b = _batch("box32")
    run = E.RunConfig(10)
    z_zero = _infer(b.with_prop(_prop(b, zero=True)), 10)
    with E.wide_kernels():
        assert E.fused_path(b, run) == 0
        ws = _poisoned_ws(b, run)
        z = torch.full((b.n_nodes,), float("nan"), device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            E.forward(_flat(), b, run, ws, logits=z)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            E.forward(_flat(), b, run, ws, logits=z)
        ws.buf.fill_(0xFF)
        z.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
    assert np.array_equal(z.cpu().numpy(), z_zero)


# ---- oracle parity of the unconditional last-step shortcuts (one output tile of o1·Wo2', one k-block
# of dx'·Wo2'ᵀ, no P_S) on the wide kernels at S = 1, 2: shapes the existing oracle tests run on the
# team kernels only. Criterion: tests/test_gpu_parity.py's (logits 1e-5 + 1e-5·|z|, loss 1e-5,
# gradients 1e-5·max|g| + 1e-7 per tensor).
ORACLE_SEEDS = dict(params=7, towers=2)


@functools.lru_cache(maxsize=None)
def _oracle_case(S):
    params = O.random_params(seed=ORACLE_SEEDS["params"])
    obj, Rs, Rr, prop, tgt = D.synthetic_batch(8, 6, seed=ORACLE_SEEDS["towers"], fully_connected=True)
    loss, z, g = O.loss_and_grads(params, obj, Rs, Rr, prop, tgt, S)
    return params, (obj, Rs, Rr, prop, tgt), float(loss), np.asarray(z), g


@pytest.mark.parametrize("S", [1, 2])
def test_oracle_case_is_finite_and_nonzero(S):
    """(CPU) The fp64 oracle alone: finite, and every gradient tensor non-zero at the chosen seeds."""
    _, _, loss, z, g = _oracle_case(S)
    assert np.isfinite(loss) and np.isfinite(z).all()
    for k, v in g.items():
        assert np.isfinite(v).all() and np.abs(v).max() > 0, k


@gpu
@pytest.mark.parametrize("S", [1, 2])
def test_wide_last_step_shortcuts_match_oracle(S):
    params, (obj, Rs, Rr, prop, tgt), loss_ref, z_ref, g_ref = _oracle_case(S)
    batch = TowerBatch.from_dense(obj, Rs, Rr, prop, device="cuda")
    assert batch.prop is None
    flat = P.to_flat(params, device="cuda")
    run = E.RunConfig(S, training=True, math="x6")
    with E.wide_kernels():
        assert E.fused_path(batch, run) == 0
        ws = _poisoned_ws(batch, run)
        z = E.forward(flat, batch, run, ws, logits=torch.full((batch.n_nodes,), float("nan"), device="cuda"))
        out3, dz = E.bce(z, torch.tensor(tgt, device="cuda").reshape(-1), E.BceScratch("cuda"))
        g = torch.full_like(flat, float("nan"))
        E.backward(flat, batch, run, ws, dz, grads=g)
        torch.cuda.synchronize()
    ref = z_ref.reshape(-1)
    err = np.abs(z.cpu().numpy().reshape(-1) - ref)
    print(f"S={S} max|dz|={err.max():.3e} loss {float(out3[0]):.7f} (oracle {loss_ref:.7f})")
    assert np.all(err <= 1e-5 + 1e-5 * np.abs(ref))
    assert abs(float(out3[0]) - loss_ref) < 1e-5
    got = P.from_flat(g)
    for name, r in g_ref.items():
        scale, e = np.abs(r).max(), np.abs(got[name] - r).max()
        print(f"{name:14s} max|g|={scale:.3e} max|dg|={e:.3e}")
        assert e <= 1e-5 * scale + 1e-7, name


@gpu
@pytest.mark.parametrize("math", ["x6", "bf16"])
def test_fast_path_is_deterministic(math):
    """Two runs of the fast path: bitwise equal logits and gradients."""
    b = _batch("ragged")
    z0, g0, _ = _train_step(b, 5, math, want_dprop=False)
    z1, g1, _ = _train_step(b, 5, math, want_dprop=False)
    assert np.isfinite(g0).all()
    assert np.array_equal(z0.view(np.uint32), z1.view(np.uint32))
    assert np.array_equal(g0.view(np.uint32), g1.view(np.uint32))
