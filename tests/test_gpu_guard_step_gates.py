"""GPU: the memory contract of spwgnn_forward_step_gated / spwgnn_backward_step_gated / spwgnn_dropedge_step_gates
(include/spwgnn.h) under guard bands (tests/guard.py): the (S, gate_step) gate buffer, params and every batch array
are inputs that come back bit for bit; logits, state, grads, dprop, drel, drel_steps and the DropEdge rows are outputs
written in full and nothing past them; a workspace of exactly spwgnn_workspace_bytes() is enough. The payloads sit at
addresses that are multiples of the alignment the header asks for and not of twice it (gates: 16 bytes). Shapes at
the block boundary — 32, 33 and 64 active edges — a 20-node tower (the 17–32-node kernels), a capacity plan filled on
the device with all-padding blocks, and rows longer than the plan (gate_step > 32·n_eblocks) whose tails hold NaN on
the way in and are not written by the DropEdge kernel, in x6."""
import ctypes as C

import numpy as np
import pytest
import torch

import guard as G
import test_gpu_guard_relations as GRL
from oracle import model as O
from spwgnn_amd import TowerBatch, _lib, data as D, engine as E, params as P

pytestmark = pytest.mark.gpu

DEV = "cuda"
S = 3


def _gate_rows(batch, width):
    """(S, width) fp32: a different uniform(−0.5, 1.5) row per step, NaN in every padding slot and in the row tail."""
    slots = 32 * batch.n_eblocks
    pad = (batch.edge_src < 0) | (batch.edge_dst < 0)
    g = torch.full((S, width), float("nan"), dtype=torch.float32, device=DEV)
    for s in range(S):
        row = torch.as_tensor(np.random.default_rng(11 + s).uniform(-0.5, 1.5, slots).astype(np.float32), device=DEV)
        row[pad] = float("nan")   # a padding slot's value is never used
        g[s, :slots] = row
    return g, pad


def _run(arena, batch, what):
    """A per-step gated forward (with the state), the loss, the gated backward (with a state cotangent), then the two
    calls that read what it left — every input frozen, every output between bands. Every arena tensor is allocated
    before the forward (the arena's tensors share version counters: tests/test_gpu_guard_relation_gates.py)."""
    n, slots = batch.n_nodes, 32 * batch.n_eblocks
    flat = arena.put(P.to_flat(O.random_params(5)).to(DEV), name="params")
    gate, pad = _gate_rows(batch, slots)
    gates = arena.put(gate, align=16, name="step_gates")
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
    drel_steps = arena.alloc((S, slots), torch.float32, align=4, name="drel_steps", written=True)
    dpos = arena.alloc((n, 4), torch.float32, align=16, name="dpos", written=True)
    outputs = {"forward": (logits, state), "backward": (grads, dprop), "after": (drel, drel_steps, dpos)}

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

    E.forward(flat, batch, run, ws, logits=logits, return_state=True, state=state, step_gates=gates)
    check("forward", f"{what}: forward with step gates")
    assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(state).all())
    arena.freeze(logits)
    arena.freeze(state)
    _, dz = E.bce(logits, tgt, E.BceScratch(DEV))
    E.backward(flat, batch, run, ws, dz, grads=grads, dprop=dprop, dstate=dstate, step_gates=gates)
    check("backward", f"{what}: backward with step gates")
    assert bool(torch.isfinite(grads).all()) and float(grads.abs().max()) > 0
    if dprop is not None:
        assert bool(torch.isfinite(dprop).all())
    arena.freeze(grads)
    arena.freeze(ws.buf)
    E.backward_relations(flat, batch, run, ws, drel=drel, drel_steps=drel_steps)
    E.backward_inputs(flat, batch, run, ws, dpos=dpos)
    arena.check(f"{what}: backward_relations / backward_inputs after the per-step gated backward")
    assert bool(torch.isfinite(drel_steps).all()) and bool((drel_steps[:, pad] == 0).all())
    assert int((drel_steps[:, ~pad] != 0).sum()) > 0
    return dict(z=logits.clone(), state=state.clone(), g=grads.clone(), dp=None if dprop is None else dprop.clone(),
                drel=drel.clone(), drel_steps=drel_steps.clone(), gate=gate)


def _host_batch(arena, name):
    hp = GRL._host_plan(name)
    names = GRL.BATCH_ARRAYS + ["prop"]
    return TowerBatch.from_plan(hp, DEV, dev_arrays=[arena.put(torch.as_tensor(a).to(DEV), name="batch." + k)
                                                     for a, k in zip(hp.arrays, names)])


@pytest.mark.parametrize("name", ["e32", "e33", "e64", "n20"])
def test_guarded_host_plans(name):
    arena = G.Arena(DEV)
    batch = _host_batch(arena, name)
    if name == "n20":
        assert 16 < batch.nw_max <= 32
    _run(arena, batch, name)


def _capacity_batch(arena):
    """A plan filled on the device from relation matrices: two of the four towers have no relation at all, so whole
    blocks are padding (their gate slots hold NaN in every row)."""
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
    for k in GRL.BATCH_ARRAYS:   # the batch's device arrays move between bands
        setattr(batch, k, arena.put(getattr(batch, k), name="batch." + k))
    batch._cstruct = None
    return batch, blocks


def test_guarded_capacity_plan_with_all_padding_blocks():
    arena = G.Arena(DEV)
    batch, blocks = _capacity_batch(arena)
    res = _run(arena, batch, "capacity plan")
    assert bool((res["drel_steps"].view(S, -1, 32)[:, blocks == 0] == 0).all())


@pytest.mark.parametrize("name", ["e33", "capacity"])
def test_rows_longer_than_the_plan(name):
    """gate_step = 32·n_eblocks + 36 through the C ABI: NaN in the row tails and the padding slots changes nothing —
    every output equals the contiguous (S, 32·n_eblocks) call's bit for bit — and every buffer keeps its bands."""
    arena = G.Arena(DEV)
    batch = _host_batch(arena, name) if name != "capacity" else _capacity_batch(arena)[0]
    ref = _run(arena, batch, name)
    n, slots = batch.n_nodes, 32 * batch.n_eblocks
    step = slots + 36
    wide, _ = _gate_rows(batch, step)
    assert torch.equal(wide[:, :slots].contiguous().view(torch.int32), ref["gate"].view(torch.int32))
    assert bool(torch.isnan(wide[:, slots:]).all())
    ar2 = G.Arena(DEV)
    gates = ar2.put(wide, align=16, name="step_gates (gate_step > slots)")
    flat = ar2.put(P.to_flat(O.random_params(5)).to(DEV), name="params")
    dstate = ar2.put(torch.as_tensor(np.random.default_rng(4).normal(0, 0.05, (n, 100)).astype(np.float32)), align=16,
                     name="dstate")
    run = E.RunConfig(S, training=True, math="x6", dropout=0.1, seed=77)
    buf = ar2.alloc(E.workspace_bytes(batch, run), torch.uint8, align=256, name="workspace")
    buf.fill_(0xFF)
    logits = ar2.alloc(n, torch.float32, align=4, name="logits", written=True)
    state = ar2.alloc((n, 100), torch.float32, align=16, name="state", written=True)
    grads = ar2.alloc(flat.numel(), torch.float32, align=4, name="grads", written=True)
    dprop = ar2.alloc((n, 100), torch.float32, align=4, name="dprop", written=True) if batch.prop is not None else None
    drel = ar2.alloc(slots, torch.float32, align=4, name="drel", written=True)
    drel_steps = ar2.alloc((S, slots), torch.float32, align=4, name="drel_steps", written=True)
    tgt = torch.as_tensor(np.random.default_rng(3).integers(0, 2, n).astype(np.float32), device=DEV)
    lib, b, r = _lib.lib(), batch.cstruct(), run.cstruct(with_prologue=True)
    stream = torch.cuda.current_stream().cuda_stream
    st = lib.spwgnn_forward_step_gated(flat.data_ptr(), C.byref(b), C.byref(r), buf.data_ptr(), buf.numel(),
                                       gates.data_ptr(), step, logits.data_ptr(), state.data_ptr(), stream)
    assert st == 0
    _, dz = E.bce(logits, tgt, E.BceScratch(DEV))
    r = run.cstruct()
    st = lib.spwgnn_backward_step_gated(flat.data_ptr(), C.byref(b), C.byref(r), buf.data_ptr(), buf.numel(),
                                        gates.data_ptr(), step, dz.data_ptr(), dstate.data_ptr(), grads.data_ptr(),
                                        dprop.data_ptr() if dprop is not None else None, stream)
    assert st == 0
    st = lib.spwgnn_backward_relations(flat.data_ptr(), C.byref(b), C.byref(r), buf.data_ptr(), buf.numel(),
                                       drel.data_ptr(), drel_steps.data_ptr(), stream)
    assert st == 0
    ar2.check(f"{name}: gate_step {step} > {slots}")
    got = dict(z=logits, state=state, g=grads, dp=dprop, drel=drel, drel_steps=drel_steps)
    for k, t in got.items():
        if t is not None:
            assert torch.equal(t.view(torch.int32), ref[k].view(torch.int32)), k
    # a stride that is no multiple of 4, or shorter than the plan: refused before any device work
    for bad in (slots + 2, slots - 4):
        assert lib.spwgnn_forward_step_gated(flat.data_ptr(), C.byref(b), C.byref(r), buf.data_ptr(), buf.numel(),
                                             gates.data_ptr(), bad, logits.data_ptr(), None, stream) == _lib.E_ARG


@pytest.mark.parametrize("name", ["e32", "e33", "e64", "capacity"])
def test_guarded_dropedge_step_gates(name):
    """spwgnn_dropedge_step_gates with gate_step = 32·n_eblocks + 4 and per-step base rows: every slot of every row
    written, the row tails and everything past the last row's slots left alone, every input frozen."""
    arena = G.Arena(DEV)
    batch = _host_batch(arena, name) if name != "capacity" else _capacity_batch(arena)[0]
    slots = 32 * batch.n_eblocks
    step = slots + 4
    pad = (batch.edge_src < 0) | (batch.edge_dst < 0)
    base = torch.stack([torch.linspace(0.5, 1.5, slots, device=DEV) * (s + 1) for s in range(S)])
    base[:, pad] = float("nan")
    d_base = arena.put(base, align=16, name="base")
    key = arena.put(torch.tensor([0x1234_5678_9ABC_DEF1], dtype=torch.int64, device=DEV), align=8, name="seed_dev")
    rows = arena.alloc((S, step), torch.float32, 16, "gates")
    rows.fill_(-7.0)   # the tails must come back as they went in
    run = E.RunConfig(S, seed=5, seed_dev=key)
    b, r = batch.cstruct(), run.cstruct()
    st = _lib.lib().spwgnn_dropedge_step_gates(C.byref(b), C.byref(r), 0.3, _lib.DROPEDGE_SYMMETRIC, d_base.data_ptr(),
                                               slots, rows.data_ptr(), step, torch.cuda.current_stream().cuda_stream)
    assert st == 0
    arena.check(f"{name}: dropedge_step_gates")
    assert bool((rows[:, slots:] == -7.0).all())
    got = rows[:, :slots].contiguous()
    want = E.dropedge_gates(batch, run, 0.3, base=d_base, per_step=True)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert bool((got[:, pad].view(torch.int32) == 0).all()) and bool((got[:, ~pad] != 0).any()) and bool((got[:, ~pad] == 0).any())
