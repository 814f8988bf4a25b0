"""GPU: the memory contract of spwgnn_backward_relations (include/spwgnn.h) under guard bands (tests/guard.py):
`drel` and `drel_steps` are outputs written in full and nothing past them; params, every batch array and the
WHOLE workspace are inputs that come back bit for bit. Shapes at the block boundary — 32·k and 32·k + 1
active edges — a tower of more than 16 nodes (bf16 math then keeps fp32 rows), the wide kernels (bf16 math
then stores A, U, V and g as bf16), and a capacity-padded plan filled on the device with an all-padding block."""
import contextlib

import numpy as np
import pytest
import torch

import guard as G
from oracle import model as O
from spwgnn_amd import TowerBatch, data as D, engine as E, params as P
from spwgnn_amd.batch import HostPlan

pytestmark = pytest.mark.gpu

DEV = "cuda"
S = 3
#         id          tower sizes   dropped relations   nw_max  wide   active edges
SHAPES = {"e32":     ((4, 5),       0,                  16,     False, 32),
          "e33":     ((4, 5, 2),    1,                  16,     False, 33),
          "e64":     ((4, 5, 4, 5), 0,                  16,     False, 64),
          "e33wide": ((4, 5, 2),    1,                  16,     True,  33),
          "n20":     ((20,),        0,                  None,   False, 380)}
BATCH_ARRAYS = ["pos", "node_tower", "node_local", "wtile", "edge_src", "edge_dst", "blk_csr"]


def _host_plan(name) -> HostPlan:
    sizes, dropped, nw_max, _, active = SHAPES[name]
    src, dst, te, pos, off = [], [], [], [], 0
    for i, n in enumerate(sizes):
        raw = D.synthetic_towers(1, n, seed=31 + i)[0]
        m, j = np.nonzero(~np.eye(n, dtype=bool))
        if i == len(sizes) - 1 and dropped:   # the last tower loses its first relations
            m, j = m[dropped:], j[dropped:]
        src.append(off + m)
        dst.append(off + j)
        te.append(len(m))
        pos.append(raw / D.RELATION_THRESHOLD)
        off += n
    src, dst = np.concatenate(src).astype(np.int32), np.concatenate(dst).astype(np.int32)
    assert len(src) == active
    prop = np.random.default_rng(17).normal(0, 0.3, (off, 100)).astype(np.float32)
    hp = HostPlan.build(np.concatenate(pos).astype(np.float32), np.array(sizes, np.int32), src, dst, np.array(te, np.int32),
                        prop, nw_max=nw_max)
    if name in ("e32", "e33", "e33wide"):   # one wave-tile: a full block, and a full block plus one edge
        assert hp.n_wtiles == 1 and hp.n_eblocks == (active + 31) // 32
    return hp


def _run(arena, batch, math, what):
    """forward, loss, backward on a guarded workspace; then the relations call with everything frozen."""
    n, slots = batch.n_nodes, 32 * batch.n_eblocks
    flat = arena.put(P.to_flat(O.random_params(5)).to(DEV), name="params")
    tgt = torch.as_tensor(np.random.default_rng(3).integers(0, 2, n).astype(np.float32), device=DEV)
    run = E.RunConfig(S, training=True, math=math, dropout=0.1, seed=77)
    ws = E.Workspace(DEV)
    ws.buf = arena.alloc(E.workspace_bytes(batch, run), torch.uint8, align=256, name="workspace")
    ws.buf.fill_(0xFF)
    z = E.forward(flat, batch, run, ws)
    _, dz = E.bce(z, tgt, E.BceScratch(DEV))
    g, dp = E.backward(flat, batch, run, ws, dz, want_dprop=batch.prop is not None)
    torch.cuda.synchronize()
    arena.freeze(ws.buf)
    drel = arena.alloc(slots, torch.float32, align=4, name="drel", written=True)
    steps = arena.alloc((S, slots), torch.float32, align=4, name="drel_steps", written=True)
    g0 = g.clone()
    E.backward_relations(flat, batch, run, ws, drel=drel, drel_steps=steps)
    arena.check(f"{what} {math}: backward_relations")
    assert torch.equal(g, g0)
    pad = (batch.edge_src < 0) | (batch.edge_dst < 0)
    assert bool(torch.isfinite(drel).all()) and bool(torch.isfinite(steps).all())
    assert bool((drel[pad] == 0).all()) and bool((steps[:, pad] == 0).all())
    assert int((drel[~pad] != 0).sum()) > 0
    # without the per-step rows: the same bits, and again nothing else touched
    arena.rearm(drel)
    E.backward_relations(flat, batch, run, ws, drel=drel)
    arena.thaw(steps)
    arena.check(f"{what} {math}: backward_relations (drel alone)")
    assert bool((steps.sum(0) - drel).abs().max() <= 1e-6 * drel.abs().max())
    return drel.clone()


@pytest.mark.parametrize("math", ["x6", "bf16"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_guarded_host_plans(name, math):
    hp = _host_plan(name)
    arena = G.Arena(DEV)
    names = BATCH_ARRAYS + ["prop"]
    with (E.wide_kernels() if SHAPES[name][3] else contextlib.nullcontext()):
        batch = TowerBatch.from_plan(hp, DEV, dev_arrays=[arena.put(torch.as_tensor(a).to(DEV), name="batch." + k)
                                                          for a, k in zip(hp.arrays, names)])
        _run(arena, batch, math, name)


@pytest.mark.parametrize("math", ["x6", "bf16"])
def test_guarded_capacity_plan_with_an_all_padding_block(math):
    """A plan filled on the device from relation matrices (N(N−1) slots per tower whatever is active): two of
    the four towers have no relation at all, so whole blocks are padding; they read no row and get zeros."""
    B, N = 4, 6
    raw = D.synthetic_towers(B, N, seed=9)
    Rs, Rr = O.relation_matrices(raw, None)
    Rs[1:3] = 0.0
    Rr[1:3] = 0.0
    obj = torch.as_tensor((raw / D.RELATION_THRESHOLD).astype(np.float32), device=DEV)
    batch = TowerBatch.from_dense_device(obj, torch.as_tensor(Rs, dtype=torch.float32, device=DEV),
                                         torch.as_tensor(Rr, dtype=torch.float32, device=DEV), check=True)
    blocks = (batch.edge_src.view(-1, 32) >= 0).sum(1)
    assert bool((blocks == 0).any()) and bool((blocks > 0).any()) and int(blocks.sum()) == 2 * N * (N - 1)
    arena = G.Arena(DEV)
    for k in BATCH_ARRAYS:   # the batch's device arrays move between bands
        setattr(batch, k, arena.put(getattr(batch, k), name="batch." + k))
    batch._cstruct = None
    drel = _run(arena, batch, math, "capacity plan")
    assert bool((drel.view(-1, 32)[blocks == 0] == 0).all())
