"""Stored dh1pre steps of the dA sum (spwgnn_da_stored_steps): on the wide x6 kernels
the edge backward of the last K steps keeps its masked dh1pre in the (then dead) dz4..dz1 arrays and
k_dA_x6 reads those steps back instead of repeating their W2ᵀ products. The values and the order of
the sum are those of the rebuild, so every K must give K = 0's gradients bit for bit (torch.equal on
each of the 22 tensors, on the whole flat buffer and on d/d'propagation').

Every case runs the wide kernels (team limit 0) on a workspace filled with 0xFF bytes before the
forward and NaN-filled outputs: a slab block that no edge backward wrote, or one read at the wrong
place, shows up as NaN or as a different sum.

Shapes (the smallest at which the scheme can go wrong):
  six     3,000 fully connected 6-box towers, 3,000 edge blocks: two towers per wave-tile, a 28-edge
          second block with padding edges, more than one block per wave of k_dA_x6 and a partial last
          round (checked below against the launch geometry);
  twelve  40 fully connected 12-box towers: five blocks per wave-tile (the last one 4 edges), 200
          blocks, one per wave of k_dA_x6;
  ragged  300 thresholded towers of 4..16 boxes, in input order and in spwgnn_plan_order's packed
          order: partly filled blocks, padding edges, towers without edges.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import model as O
from spwgnn_amd import TowerBatch, data as D, engine as E, params as P

gpu = pytest.mark.gpu

SHAPES = ["six", "twelve", "ragged", "ragged_packed"]
KS = [1, 2, 3, 4]


@functools.lru_cache(maxsize=None)
def _batch(shape: str) -> TowerBatch:
    if shape.startswith("ragged"):
        pos, sizes, src, dst, tower_edges, _ = D.ragged_batch(300, 4, 16, seed=11)
        assert (np.asarray(tower_edges) == 0).any(), "the ragged batch should hold a tower without edges"
        return TowerBatch.from_edges(pos, sizes, src, dst, tower_edges, None, device="cuda", pack=shape == "ragged_packed")
    T, N = {"six": (3000, 6), "twelve": (40, 12)}[shape]
    raw = D.synthetic_towers_fast(T, N, seed=4)
    return TowerBatch.fully_connected((raw / D.RELATION_THRESHOLD).astype(np.float32), device="cuda")


@functools.lru_cache(maxsize=None)
def _flat():
    return P.to_flat(O.random_params(seed=31), device="cuda")


@functools.lru_cache(maxsize=None)
def _targets(n_nodes: int):
    rng = np.random.default_rng(n_nodes)
    return torch.tensor(rng.integers(0, 2, size=n_nodes).astype(np.float32), device="cuda")


@functools.lru_cache(maxsize=None)
def _with_prop(shape: str) -> TowerBatch:
    b = _batch(shape)
    rng = np.random.default_rng(3)
    return b.with_prop(torch.tensor(rng.normal(0, 0.3, size=(b.n_nodes, 100)).astype(np.float32), device="cuda"))


def _poisoned_ws(batch, run):
    ws = E.Workspace("cuda")
    ws.buf = torch.full((E.workspace_bytes(batch, run),), 0xFF, dtype=torch.uint8, device="cuda")
    return ws


def _step(batch, run, ws, want_dprop):
    """One forward + loss + backward on `ws`; (grads, dprop) as device tensors."""
    assert E.fused_path(batch, run) == 0
    z = E.forward(_flat(), batch, run, ws, logits=torch.full((batch.n_nodes,), float("nan"), device="cuda"))
    _, dz = E.bce(z, _targets(batch.n_nodes), E.BceScratch("cuda"))
    g = torch.full_like(_flat(), float("nan"))
    _, dp = E.backward(_flat(), batch, run, ws, dz, grads=g, want_dprop=want_dprop)
    torch.cuda.synchronize()
    return g, dp


def _run_cfg(S, math, split):
    ev = None
    if split:
        ev = torch.cuda.Event()
        ev.record()
    return E.RunConfig(S, training=True, math=math, dropout=0.1, seed=5, grads_early_event=ev)


def _grads_at(k, batch, S, math, general, split, steps=1):
    run = _run_cfg(S, math, split)
    with E.wide_kernels(), E.da_stored(k):
        assert E.da_stored_steps() == k
        ws = _poisoned_ws(batch, run)
        for _ in range(steps):
            out = _step(batch, run, ws, want_dprop=general)
    return out


def _assert_same(ref, got, what):
    (g0, p0), (g, p) = ref, got
    assert torch.isfinite(g0).all(), what
    r, t = P.from_flat(g0), P.from_flat(g)
    assert len(r) == 22
    for name in r:
        assert np.array_equal(r[name], t[name]), (what, name, float(np.abs(r[name] - t[name]).max()))
    assert torch.equal(g0, g), what   # the alignment gaps of the flat buffer too
    if p0 is not None:
        assert torch.isfinite(p0).all() and torch.equal(p0, p), what


@gpu
def test_six_box_shape_sums_several_blocks_per_wave():
    """k_dA_x6's geometry at the 'six' shape: workgroups of 8 waves over contiguous block ranges of
    `perw` blocks (a multiple of 8), wave w taking blocks w, w + 8, …"""
    b = _batch("six")
    assert b.n_eblocks == 3000 and b.n_wtiles == 1500   # 60 edges per tile: a full block and a 28-edge one
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = min((b.n_eblocks + 7) // 8, cus)
    perw = (((b.n_eblocks + grid - 1) // grid) + 7) // 8 * 8
    assert perw >= 16, "a wave must sum more than one block: enlarge the batch"
    assert b.n_eblocks % perw != 0, "the last workgroup's range should be partial"


@gpu
@pytest.mark.parametrize("split", [False, True], ids=["one_group", "early_event"])
@pytest.mark.parametrize("general", [False, True], ids=["fast", "general"])
@pytest.mark.parametrize("S", [1, 2, 5])   # S = 1 clamps K to 0, S = 2 to 1
@pytest.mark.parametrize("shape", SHAPES)
def test_every_k_equals_k0(shape, S, general, split):
    """fast: prop = None, no dprop (step 0's edge backward is not launched); general: a non-zero prop
    with dprop requested (it is, and step 0 is still rebuilt)."""
    batch = _with_prop(shape) if general else _batch(shape)
    ref = _grads_at(0, batch, S, "x6", general, split)
    for k in KS:
        _assert_same(ref, _grads_at(k, batch, S, "x6", general, split), (shape, S, general, split, k))


@gpu
@pytest.mark.parametrize("general", [False, True], ids=["fast", "general"])
@pytest.mark.parametrize("shape", ["six", "ragged_packed"])
def test_second_step_on_the_same_workspace(shape, general):
    """Two steps on one workspace: the second backward's slabs alias the dz arrays the first left full."""
    batch = _with_prop(shape) if general else _batch(shape)
    ref = _grads_at(0, batch, 5, "x6", general, False, steps=2)
    _assert_same(_grads_at(0, batch, 5, "x6", general, False), ref, (shape, general, "k0 step 2 vs step 1"))
    for k in KS:
        _assert_same(ref, _grads_at(k, batch, 5, "x6", general, False, steps=2), (shape, general, k))


@gpu
@pytest.mark.parametrize("shape", ["six", "ragged"])
def test_bf16_math_ignores_k(shape):
    """bf16 math keeps K = 0: the setting changes nothing."""
    batch = _batch(shape)
    ref = _grads_at(0, batch, 5, "bf16", False, False)
    _assert_same(ref, _grads_at(4, batch, 5, "bf16", False, False), (shape, "bf16"))


def test_setter_and_default():
    """(host only) spwgnn_da_stored_steps: the setter returns the previous value, a query changes
    nothing, the default is the compile-time default the binding documents."""
    assert E.da_stored_steps() == E.DA_STORED_DEFAULT
    assert E.da_stored_steps() == E.DA_STORED_DEFAULT   # a query does not change it
    try:
        assert E.da_stored_steps(3) == E.DA_STORED_DEFAULT
        assert E.da_stored_steps() == 3 and E.da_stored_steps(-1) == 3
        assert E.da_stored_steps(9) == 3 and E.da_stored_steps() == 9   # stored as given, clamped per call
        with E.da_stored(1):
            assert E.da_stored_steps() == 1
        assert E.da_stored_steps() == 9
    finally:
        E.da_stored_steps(E.DA_STORED_DEFAULT)
    assert E.da_stored_steps() == E.DA_STORED_DEFAULT
