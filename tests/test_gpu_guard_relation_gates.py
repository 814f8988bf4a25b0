"""GPU: the memory contract of spwgnn_forward_gated / spwgnn_backward_gated (include/spwgnn.h) under guard bands
(tests/guard.py): the gate buffer, params and every batch array are inputs that come back bit for bit; logits,
state, grads and dprop are outputs written in full and nothing past them; a workspace of exactly
spwgnn_workspace_bytes() is enough. The payloads sit at addresses that are multiples of the alignment the header
asks for and not of twice it (gates: 16 bytes). Shapes at the block boundary — 32, 33 and 64 active edges — a
20-node tower (the 17–32-node kernels), and a capacity plan filled on the device with all-padding blocks, in x6."""
import numpy as np
import pytest
import torch

import guard as G
import test_gpu_guard_relations as GRL
from oracle import model as O
from spwgnn_amd import TowerBatch, data as D, engine as E, params as P

pytestmark = pytest.mark.gpu

DEV = "cuda"
S = 3


def _run(arena, batch, what):
    """A gated forward (with the state), the loss, the gated backward (with a state cotangent), then the two
    calls that read what it left — every input frozen, every output between bands. Every arena tensor is
    allocated before the forward: the arena's tensors are views of shared buffers, whose version counter — part
    of what `engine.Workspace` remembers of the forward's gates — an in-place fill of a later allocation would move."""
    n, slots = batch.n_nodes, 32 * batch.n_eblocks
    flat = arena.put(P.to_flat(O.random_params(5)).to(DEV), name="params")
    pad = (batch.edge_src < 0) | (batch.edge_dst < 0)
    gate = torch.as_tensor(np.random.default_rng(11).uniform(-0.5, 1.5, slots).astype(np.float32), device=DEV)
    gate[pad] = float("nan")   # a padding slot's value is never used
    gates = arena.put(gate, align=16, name="gates")
    tgt = torch.as_tensor(np.random.default_rng(3).integers(0, 2, n).astype(np.float32), device=DEV)
    dstate = arena.put(torch.as_tensor(np.random.default_rng(4).normal(0, 0.05, (n, 100)).astype(np.float32)), align=16,
                       name="dstate")
    run = E.RunConfig(S, training=True, math="x6", dropout=0.1, seed=77)
    ws = E.Workspace(DEV)
    ws.buf = arena.alloc(E.workspace_bytes(batch, run), torch.uint8, align=256, name="workspace")
    ws.buf.fill_(0xFF)
    logits = arena.alloc(n, torch.float32, align=4, name="logits", written=True)
    state = arena.alloc((n, 100), torch.float32, align=16, name="state", written=True)
    grads = arena.alloc(flat.numel(), torch.float32, align=4, name="grads", written=True)
    dprop = arena.alloc((n, 100), torch.float32, align=4, name="dprop", written=True) if batch.prop is not None else None
    drel = arena.alloc(slots, torch.float32, align=4, name="drel", written=True)
    dpos = arena.alloc((n, 4), torch.float32, align=16, name="dpos", written=True)
    outputs = {"forward": (logits, state), "backward": (grads, dprop), "after": (drel, dpos)}

    def check(stage, what_):
        """arena.check with only the outputs written so far held to "written in full"."""
        later = [t for k in list(outputs)[list(outputs).index(stage) + 1:] for t in outputs[k] if t is not None]
        for t in later:
            arena._find(t).written = False
        arena.check(what_)
        for t in later:
            arena._find(t).written = True
        for t in later:   # ... and still untouched: every byte the unwritten pattern
            assert bool((t.reshape(-1).view(torch.int32) == G.UNWRITTEN_I32).all()), what_

    E.forward(flat, batch, run, ws, logits=logits, return_state=True, state=state, gates=gates)
    check("forward", f"{what}: forward with gates")
    assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(state).all())
    arena.freeze(logits)
    arena.freeze(state)
    _, dz = E.bce(logits, tgt, E.BceScratch(DEV))
    E.backward(flat, batch, run, ws, dz, grads=grads, dprop=dprop, dstate=dstate, gates=gates)
    check("backward", f"{what}: backward with gates")
    assert bool(torch.isfinite(grads).all()) and float(grads.abs().max()) > 0
    if dprop is not None:
        assert bool(torch.isfinite(dprop).all())
    arena.freeze(grads)
    arena.freeze(ws.buf)
    E.backward_relations(flat, batch, run, ws, drel=drel)
    E.backward_inputs(flat, batch, run, ws, dpos=dpos)
    arena.check(f"{what}: backward_relations / backward_inputs after the gated backward")
    assert bool(torch.isfinite(drel).all()) and bool((drel[pad] == 0).all()) and int((drel[~pad] != 0).sum()) > 0
    return drel.clone()


@pytest.mark.parametrize("name", ["e32", "e33", "e64", "n20"])
def test_guarded_host_plans(name):
    hp = GRL._host_plan(name)
    arena = G.Arena(DEV)
    names = GRL.BATCH_ARRAYS + ["prop"]
    batch = TowerBatch.from_plan(hp, DEV, dev_arrays=[arena.put(torch.as_tensor(a).to(DEV), name="batch." + k)
                                                      for a, k in zip(hp.arrays, names)])
    if name == "n20":
        assert 16 < batch.nw_max <= 32
    _run(arena, batch, name)


def test_guarded_capacity_plan_with_all_padding_blocks():
    """A plan filled on the device from relation matrices: two of the four towers have no relation at all, so
    whole blocks are padding (their gate slots hold NaN); they read no row and their gate gradient is zero."""
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
    for k in GRL.BATCH_ARRAYS:   # the batch's device arrays move between bands
        setattr(batch, k, arena.put(getattr(batch, k), name="batch." + k))
    batch._cstruct = None
    drel = _run(arena, batch, "capacity plan")
    assert bool((drel.view(-1, 32)[blocks == 0] == 0).all())
