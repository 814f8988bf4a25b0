"""GPU: per-step relation gates — `engine.forward(..., step_gates=)` / `engine.backward(..., step_gates=)`
(spwgnn_forward_step_gated / spwgnn_backward_step_gated), the (S, E) gate gradient `engine.backward_relations` returns
after them as ``drel_steps``, the autograd path of `GraphNetwork(relation_step_weights=)`, and layer-wise DropEdge
(`engine.dropedge_gates(per_step=True)`, `Trainer(dropedge_per_step=True)`, replayed steps) — DESIGN.md §3zzc.

Reference: fp64 torch autograd through relation_grad_ref.forward_gather_gated with the (S, E) gate tensor, the
parameters, the objects and the propagation input as leaves (tests/step_gates_ref.py). Gates: row s is
relation_gates_ref.gates_for(E, seed + s). tests/test_step_gates_host.py holds, for every case here, every tower's
ReLU / BCE-clip margin above TAU = 1e-6 (no tower is left out) and the two mutants — gate rows rotated by one step,
row 0 at every step — outside these criteria in the logits and in at least one gradient tensor.

Criteria (x6 and h3; those of tests/test_gpu_relation_gates.py): logits |Δ| <= 1e-5 + 1e-5·|z|; every parameter
tensor, d/d'propagation', d/d objects and the (S, E) gate gradient max|Δ| <= 1e-5·max|ref| + 1e-8. x3: at most twice
the error of the same case's UNGATED x3 run on the wide kernels against the ungated oracle, on a gate set that is
no closer to a ReLU kink than the ungated inputs are (`step_gates_ref.pick_x3_gates`).

Shapes: the cases of tests/test_gpu_input_grad.py — team_a (3, 5, 4) and team_b (2, 6, 3) on the fused loops, wide
(4, 6, 5, fully connected) on the wide kernels with K = 0 and K = 3 stored dh1pre steps (S = 5 with K = 3 leaves
steps 1 and 0 to k_dA_x6's rebuild), recv (2, 9, 2) as a receiver-block plan and as an 18-node tile — the packed
ragged batch, and the shapes of tests/test_gpu_gated_team.py: tall (tiles of 5 blocks: the dA rebuild inside the fused
loop), tall_recv (the per-phase team chain), pair16 (one 16-node tile, the LDS dA sums).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import relation_gates_ref as GR
import step_gates_ref as SR
import test_gpu_gated_team as GT
import test_gpu_relation_gates as RG
from oracle import model as O
from spwgnn_amd import GraphNetwork, TowerBatch, _lib, data as D, engine as E, params as P
from spwgnn_amd.batch import HostPlan
from spwgnn_amd.replay import ReplayStep
from spwgnn_amd.trainer import Trainer, dropout_key

pytestmark = pytest.mark.gpu

DEV = "cuda"
SPLIT = ["x6", "x3", "h3"]
EXACT = ["x6", "h3"]


# ------------------------------------------------------------------------------------ inputs
_BUILT = {}


def _batch(name, kind):
    """(case, batch, targets in plan order, gates (S, E) in the case's edge order) of case `name` planned as `kind`."""
    if (name, kind) in _BUILT:
        return _BUILT[name, kind]
    c, sizes, gates, _ = SR.case(name)
    if kind in ("team", "wide16", "recv", "tile32") and name in ("team_a", "team_b", "wide", "recv"):
        batch = RG._batch(c, kind)
    elif kind == "packed":
        batch = TowerBatch.from_edges(c["obj"], sizes, c["src"].astype(np.int32), c["dst"].astype(np.int32), c["tes"],
                                      device=DEV, pack=True)
        assert batch.prop is None and batch.node_perm is not None
    elif kind == "tall":
        batch = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], c["prop"], device=DEV)
        assert batch.n_wtiles == 2 and np.all(batch.wtile.cpu().numpy().reshape(-1, 4)[:, 1] == 5)   # past kTeamDaBlocks
    elif kind == "tall_recv":
        batch = TowerBatch.fully_connected(c["obj"], c["prop"], device=DEV, recv_blocks=True)
        assert batch.flags & _lib.BATCH_RECV_BLOCKS
    elif kind == "pair16":
        batch = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], c["prop"], device=DEV, nw_max=16)
        assert batch.n_wtiles == 1 and batch.n_eblocks == 4 and batch.n_nodes == 16
    else:
        raise ValueError((name, kind))
    tgt = batch.to_plan_order(np.asarray(c["tgt"], np.float32).reshape(-1))
    _BUILT[name, kind] = (c, batch, tgt, gates)
    return _BUILT[name, kind]


def _slots(c, batch, gates, fill=0.0):
    """(S, E) gates in the case's edge order → the (S, 32·n_eblocks) slot tensor."""
    return torch.stack([RG._slot_gates(c, batch, row, fill) for row in gates]).contiguous()


def _to_ref_order(c, batch, slot_rows):
    return np.stack([RG._to_ref_order(c, batch, row) for row in slot_rows])


# ------------------------------------------------------------------------------------ engine
def _run(c, batch, math, step_gates=None, gates=None, loss="bce", tgt=None, state=False, dstate=None, training=True):
    """One step's forward + loss + backward (+ backward_inputs, backward_relations with its per-step rows) with
    per-step `step_gates` (S, slots), shared `gates` (slots,) or neither. Returns a dict of device tensors."""
    flat = P.to_flat(c["params"], device=DEV)
    ws = E.Workspace(DEV)
    run = E.RunConfig(c["S"], training=training, math=math)
    kw = {"step_gates": step_gates} if step_gates is not None else ({"gates": gates} if gates is not None else {})
    out = E.forward(flat, batch, run, ws, return_state=state, **kw)
    z, st = out if state else (out, None)
    res = dict(z=z, state=st)
    if not training:
        torch.cuda.synchronize()
        return res
    if loss == "bce":
        t = torch.as_tensor(np.asarray(c["tgt"] if tgt is None else tgt, np.float32), device=DEV).reshape(-1)
        _, dz = E.bce(z, t, E.BceScratch(DEV))
    elif loss == "sum":
        dz = torch.ones_like(z)
    else:
        p = E.sigmoid(z)
        dz = p * (1.0 - p)
    g, dp = E.backward(flat, batch, run, ws, dz, want_dprop=batch.prop is not None, dstate=dstate, **kw)
    drel, drel_steps = E.backward_relations(flat, batch, run, ws, per_step=True)
    res.update(g=g, dp=dp, dobj=E.backward_inputs(flat, batch, run, ws).clone(), drel=drel, drel_steps=drel_steps)
    torch.cuda.synchronize()
    return res


KEYS = ("z", "g", "dp", "dobj", "drel", "drel_steps", "state")


def _bits_equal(what, a, b, keys=KEYS):
    RG._bits_equal(what, a, b, keys=keys)


def _check(what, c, batch, res, ref, dprop=True, order=None):
    """Every output of `res` against the fp64 oracle `ref` at the module docstring's criteria; the gate gradient is
    `drel_steps`, (S, E), and `drel` its sum over the steps."""
    order = (lambda x: x) if order is None else order
    RG._logits_close(what, order(RG._np(res["z"])), ref["z"])
    g = P.from_flat(res["g"])
    for name in sorted(ref["g"]):
        RG._close(f"{what} {name}", np.asarray(g[name], np.float64), ref["g"][name])
    if dprop:
        RG._close(what + " dprop", order(RG._np(res["dp"])), ref["dprop"])
    RG._close(what + " dobj", order(RG._np(res["dobj"])), ref["dobj"])
    steps = res["drel_steps"]
    pad = (batch.edge_src < 0) | (batch.edge_dst < 0)
    assert steps.shape == (c["S"], 32 * batch.n_eblocks) and bool((steps[:, pad] == 0).all())
    RG._close(what + " dgate (S, E)", _to_ref_order(c, batch, RG._np(steps)), ref["dgate"])
    RG._close(what + " drel = Σ_s", RG._to_ref_order(c, batch, RG._np(res["drel"])), ref["dgate"].sum(0))


class _wide:
    """The wide kernels (spwgnn_team_max_blocks(0)) with K stored dh1pre steps (None: the default) inside the block."""

    def __init__(self, on=True, stored=None):
        self.on, self.stored, self.cms = on, stored, []

    def __enter__(self):
        if self.on:
            self.cms.append(E.wide_kernels())
        if self.stored is not None:
            self.cms.append(E.da_stored(self.stored))
        for cm in self.cms:
            cm.__enter__()

    def __exit__(self, *exc):
        for cm in reversed(self.cms):
            cm.__exit__(*exc)
        return False


# name, kind, wide kernels?, stored steps
PARITY = [("team_a", "team", False, None), ("team_b", "team", False, None), ("wide", "wide16", True, 3),
          ("wide", "wide16", True, 0), ("recv", "recv", False, None), ("recv", "tile32", False, None),
          ("ragged", "packed", False, None), ("tall", "tall", False, None), ("tall", "tall_recv", False, None),
          ("pair16", "pair16", False, None)]


# ------------------------------------------------------------------------------------ 1. parity with the fp64 oracle
@pytest.mark.parametrize("math", EXACT)
@pytest.mark.parametrize("name,kind,wide,stored", PARITY, ids=[f"{n}-{k}-K{s}" for n, k, _, s in PARITY])
def test_oracle_parity(name, kind, wide, stored, math):
    """BCE and Σ sigmoid(z) on every path: the fused loops, the wide kernels with K = 0 and K = 3, a receiver-block
    plan, 18-node tiles, a packed ragged batch with a null propagation input, tiles past the LDS dA sums."""
    c, batch, tgt, gates = _batch(name, kind)
    sg = _slots(c, batch, gates)
    order = batch.to_input_order if batch.node_perm is not None else None
    with _wide(wide, stored):
        run = E.RunConfig(c["S"], training=True, math=math)
        if wide:
            assert E.fused_path(batch, run, gated=True) == 0
            assert E.da_stored_steps() == stored and c["S"] == 5
        elif kind in ("team", "packed", "tall", "pair16"):
            assert E.fused_path(batch, run, gated=True) == 3
        for loss in ("bce", "sum_prob"):
            ref = SR.oracle(c, gates, loss, key=name)
            res = _run(c, batch, math, sg, loss=loss, tgt=tgt)
            _check(f"{name}/{kind} K={stored} {math} {loss}", c, batch, res, ref, dprop=batch.prop is not None, order=order)


@pytest.mark.parametrize("name,kind", [("wide", "wide16"), ("team_a", "team")])
def test_x3_errors_against_the_ungated_x3_run(name, kind):
    """The logit error and each tensor's relative L2 error of the per-step gated x3 run against its oracle are at most
    twice those of the UNGATED x3 run of the same case on the wide kernels against the ungated oracle. The gate set
    is `step_gates_ref.pick_x3_gates`': a comparison of rounding errors needs gated inputs that are no closer to a
    ReLU kink than the ungated inputs are (x3's rounding is not fp32-class: TAU does not cover it). With the parity
    tests' gate set of `wide` (seed 1002: four step-loop units within 3.1e-6 – 6.2e-6 of their kinks, where the
    ungated forward's nearest is 7.4e-6 away) one unit flips under x3 and every gradient tensor moves by 0.6 – 1.2 %
    of its norm, against 2e-5 in the ungated run — the size tests/test_step_gates_host.py finds for that flip in
    fp64 — while the logits keep their ratio (1.33)."""
    c, batch, tgt, _ = _batch(name, kind)
    gates, seed = SR.pick_x3_gates(c, SR.case(name)[1])
    print(f"x3 {name}: gate seed {seed}, kink distances {SR.step_gated_margins(c, gates, SR.case(name)[1], groups=True)}")
    rel = lambda got, want: float(np.linalg.norm(got - want) / np.linalg.norm(want))

    def errors(res, ref, steps):
        out = {"logits": float(np.abs(RG._np(res["z"]) - ref["z"]).max())}
        g = P.from_flat(res["g"])
        for n in sorted(ref["g"]):
            out[n] = rel(np.asarray(g[n], np.float64), ref["g"][n])
        out["dprop"] = rel(RG._np(res["dp"]), ref["dprop"])
        out["dobj"] = rel(RG._np(res["dobj"]), ref["dobj"])
        out["dgate"] = rel(_to_ref_order(c, batch, RG._np(res["drel_steps"])), ref["dgate"])
        return out

    ones = np.ones_like(gates)
    with E.wide_kernels():
        plain = errors(_run(c, batch, "x3"), SR.oracle(c, ones, "bce", key=name + "/ones"), True)
    gated = errors(_run(c, batch, "x3", _slots(c, batch, gates)), SR.oracle(c, gates, "bce", key=name + "/x3"), True)
    for k in plain:
        print(f"x3 {name} {k}: per-step gated {gated[k]:.3e} ungated {plain[k]:.3e} ratio {gated[k] / plain[k]:.2f}")
    for k in plain:
        assert gated[k] <= 2 * plain[k], (k, gated[k], plain[k])


def test_state_and_its_cotangent():
    """`state_out` and a `dstate` cotangent with per-step gates: the loss is BCE + Σ dstate·P_S."""
    c, batch, tgt, gates = _batch("team_b", "team")
    dstate = np.random.default_rng(5).normal(0, 0.05, (batch.n_nodes, 100)).astype(np.float32)
    ref = SR.oracle(c, gates, "bce", dstate=dstate)
    res = _run(c, batch, "x6", _slots(c, batch, gates), state=True, dstate=torch.as_tensor(dstate, device=DEV))
    RG._close("state P_S", RG._np(res["state"]), ref["state"])
    _check("team_b x6 bce + dstate", c, batch, res, ref)


# ------------------------------------------------------------------------------------ 2. bitwise properties
BITS = [("team_a", "team"), ("wide", "wide16"), ("recv", "recv"), ("recv", "tile32"), ("ragged", "packed"),
        ("tall", "tall"), ("tall", "tall_recv"), ("pair16", "pair16")]


@pytest.mark.parametrize("math", SPLIT)
@pytest.mark.parametrize("name,kind", BITS)
def test_equal_rows_are_the_shared_gate_call(name, kind, math):
    """S identical rows: logits, state, gradients, dprop, d/d objects, drel and drel_steps of the shared-gate call,
    bit for bit — on the team / fused kernels and on the wide ones."""
    c, batch, tgt, gates = _batch(name, kind)
    row = RG._slot_gates(c, batch, gates[0])
    rows = row[None].repeat(c["S"], 1).contiguous()
    dstate = torch.as_tensor(np.random.default_rng(3).normal(0, 0.1, (batch.n_nodes, 100)).astype(np.float32), device=DEV)
    for wide in (False, True):
        with _wide(wide):
            shared = _run(c, batch, math, gates=row, tgt=tgt, state=True, dstate=dstate)
            step = _run(c, batch, math, rows, tgt=tgt, state=True, dstate=dstate)
        _bits_equal(f"{name}/{kind} {math} wide={wide}: equal rows vs shared", step, shared)
        assert float(step["g"].abs().max()) > 0 and float(step["drel_steps"].abs().max()) > 0


@pytest.mark.parametrize("math", SPLIT)
@pytest.mark.parametrize("name,kind", [("team_a", "team"), ("team_b", "team"), ("ragged", "packed"), ("tall", "tall"),
                                       ("tall", "tall_recv"), ("pair16", "pair16")])
def test_team_run_is_the_wide_run(name, kind, math):
    """Per-step gates on the team / fused kernels against the wide kernels: every output bit for bit; and the rows
    are read (the result differs from row 0 at every step)."""
    c, batch, tgt, gates = _batch(name, kind)
    sg = _slots(c, batch, gates)
    dstate = torch.as_tensor(np.random.default_rng(3).normal(0, 0.1, (batch.n_nodes, 100)).astype(np.float32), device=DEV)
    team = _run(c, batch, math, sg, tgt=tgt, state=True, dstate=dstate)
    with E.wide_kernels():
        wide = _run(c, batch, math, sg, tgt=tgt, state=True, dstate=dstate)
    _bits_equal(f"{name}/{kind} {math} team vs wide", team, wide)
    again = _run(c, batch, math, sg, tgt=tgt, state=True, dstate=dstate)
    _bits_equal(f"{name}/{kind} {math} two runs", again, team)
    row0 = _run(c, batch, math, sg[:1].repeat(c["S"], 1).contiguous(), tgt=tgt, state=True, dstate=dstate)
    assert not torch.equal(row0["z"], team["z"]) and not torch.equal(row0["g"], team["g"])


def test_stored_steps_do_not_change_the_gradients():
    """K = 0 stored dh1pre steps (every step rebuilt by k_dA_x6<GATE>, a gate per (block, step) pair) against K = 3
    (steps 4, 3, 2 read back from the slabs, 1 and 0 rebuilt) and K = 1 at S = 5; and two runs of the same call."""
    c, batch, tgt, gates = _batch("wide", "wide16")
    assert c["S"] == 5
    sg = _slots(c, batch, gates)
    with E.wide_kernels():
        assert E.da_stored_steps() == E.DA_STORED_DEFAULT == 3
        k3 = _run(c, batch, "x6", sg)
        again = _run(c, batch, "x6", sg)
        with E.da_stored(0):
            k0 = _run(c, batch, "x6", sg)
        with E.da_stored(1):
            k1 = _run(c, batch, "x6", sg)
    _bits_equal("two runs", again, k3)
    _bits_equal("K = 0 against K = 3", k0, k3)
    _bits_equal("K = 1 against K = 3", k1, k3)
    assert float(k3["g"].abs().max()) > 0


@pytest.mark.parametrize("name,kind,wide", [("pair16", "pair16", False), ("wide", "wide16", True), ("recv", "tile32", False)])
def test_inference_forward_is_the_training_forward(name, kind, wide):
    c, batch, tgt, gates = _batch(name, kind)
    sg = _slots(c, batch, gates)
    with _wide(wide):
        train = _run(c, batch, "x6", sg, tgt=tgt, state=True)
        infer = _run(c, batch, "x6", sg, state=True, training=False)
    _bits_equal(f"{name} inference against training at dropout 0", infer, train, keys=("z", "state"))


@pytest.mark.parametrize("name,kind,wide", [("team_a", "team", False), ("team_a", "team", True), ("ragged", "packed", False),
                                            ("tall", "tall_recv", False), ("capacity", None, False)])
def test_nan_in_the_padding_slots_changes_nothing(name, kind, wide):
    if name == "capacity":   # a capacity plan filled on the device: N(N−1) slots per tower whatever is active
        c, _, gates, _ = SR.case("team_a")
        batch = TowerBatch.from_dense_device(*(torch.as_tensor(np.asarray(c[k], np.float32), device=DEV)
                                               for k in ("obj", "Rs", "Rr", "prop")), check=True)
        tgt = None
    else:
        c, batch, tgt, gates = _batch(name, kind)
    pad = (batch.edge_src < 0) | (batch.edge_dst < 0)
    assert int(pad.sum()) > 0
    zero, nan = _slots(c, batch, gates, 0.0), _slots(c, batch, gates, float("nan"))
    assert bool(torch.isnan(nan[:, pad]).all()) and torch.equal(zero[:, ~pad], nan[:, ~pad])
    with _wide(wide):
        a = _run(c, batch, "x6", zero, tgt=tgt, state=True)
        b = _run(c, batch, "x6", nan, tgt=tgt, state=True)
    _bits_equal(f"{name} NaN padding", b, a)
    for k in KEYS:
        assert b[k] is None or bool(torch.isfinite(b[k]).all()), k


# ------------------------------------------------------------------------------------ 3. autograd
def test_relation_step_weights_leaf_through_graph_network():
    """A (S, B, N, N) `relation_step_weights` leaf: its .grad is the engine's drel_steps bit for bit, within criterion
    of the oracle; weights, propagation and objects get their gradients in the same pass."""
    c, batch, tgt, gates = _batch("team_b", "team")
    B, N, S = c["B"], c["N"], c["S"]
    bi, si, di = c["src"] // N, c["src"] % N, c["dst"] % N
    dense = np.zeros((S, B, N, N), np.float32)
    dense[:, bi, si, di] = gates
    net = GraphNetwork(mp_steps=S, dropout=0.0, device=DEV, params=c["params"])
    net.train()
    W = torch.tensor(dense, device=DEV, requires_grad=True)
    obj = torch.tensor(c["obj"], device=DEV, requires_grad=True)
    prop = torch.tensor(c["prop"], device=DEV, requires_grad=True)
    z, state = net.forward_logits(obj, c["Rs"], c["Rr"], prop, relation_step_weights=W, return_state=True)
    assert z.shape == (B, N) and state.shape == (B, N, 100)
    z.sum().backward()
    ref = SR.oracle(c, gates, "sum", key="team_b")
    RG._logits_close("relation_step_weights logits", RG._np(z).reshape(-1), ref["z"])
    got = RG._np(W.grad)
    active = np.zeros((B, N, N), bool)
    active[bi, si, di] = True
    assert np.all(got[:, ~active] == 0)
    RG._close("relation_step_weights .grad", got[:, bi, si, di], ref["dgate"])
    RG._close("objects .grad", RG._np(obj.grad).reshape(-1, 3), ref["dobj"])
    RG._close("propagation .grad", RG._np(prop.grad).reshape(-1, 100), ref["dprop"])
    res = _run(c, batch, "x6", _slots(c, batch, gates), loss="sum", state=True)
    for s in range(S):
        assert np.array_equal(batch.edges_to_input(res["drel_steps"][s].cpu().numpy(), dense=True), W.grad[s].cpu().numpy())
    assert torch.equal(res["g"], net.flat.grad)
    # relation_gradients keeps working after a per-step gated run (its own ungated forward and backward)
    r = net.relation_gradients(c["obj"], c["Rs"], c["Rr"], c["prop"])
    assert r.shape == c["Rr"].shape and bool(torch.isfinite(r).all()) and float(r.abs().max()) > 0
    with pytest.raises(ValueError, match="mutually exclusive"):
        net.forward_logits(obj, c["Rs"], c["Rr"], prop, relation_step_weights=W, relation_weights=W[0])
    with pytest.raises(ValueError, match="return_steps"):
        net.forward_logits(obj, c["Rs"], c["Rr"], prop, relation_step_weights=W, return_steps=True)
    with pytest.raises(ValueError, match="not supported"):
        GraphNetwork(mp_steps=S, device=DEV, params=c["params"], math="bf16").forward_logits(
            obj, c["Rs"], c["Rr"], prop, relation_step_weights=W)
    with pytest.raises(ValueError, match="per propagation step"):
        net.forward_logits(obj, c["Rs"], c["Rr"], prop, relation_step_weights=W[:-1])


def test_errors():
    c, batch, tgt, gates = _batch("team_b", "team")
    flat = P.to_flat(c["params"], device=DEV)
    sg = _slots(c, batch, gates)
    ws, run = E.Workspace(DEV), E.RunConfig(c["S"], training=True)
    z = E.forward(flat, batch, run, ws, step_gates=sg)
    dz = torch.ones_like(z)
    with pytest.raises(ValueError, match="relation gates of the forward"):
        E.backward(flat, batch, run, ws, dz)                               # no gates
    with pytest.raises(ValueError, match="relation gates of the forward"):
        E.backward(flat, batch, run, ws, dz, step_gates=sg.clone())        # other gates
    with pytest.raises(ValueError, match="mutually exclusive"):
        E.backward(flat, batch, run, ws, dz, step_gates=sg, gates=sg[0].contiguous())
    E.backward(flat, batch, run, ws, dz, step_gates=sg)
    z = E.forward(flat, batch, run, ws, step_gates=sg)
    sg.mul_(1.0)                                                           # written since the forward
    with pytest.raises(ValueError, match="relation gates of the forward"):
        E.backward(flat, batch, run, ws, dz, step_gates=sg)
    # the existing gates= validation is untouched: a 2-D tensor passed as gates= still raises
    with pytest.raises(ValueError, match="edge-slot order"):
        E.forward(flat, batch, run, ws, gates=sg)
    for bad in (sg[:-1], sg[0], sg[:, :-1], sg.double(), sg.cpu(), sg.t().contiguous().t()):
        with pytest.raises((ValueError, _lib.SpwgnnError)):
            E.forward(flat, batch, run, ws, step_gates=bad)
    for math in ("f32", "bf16"):   # refused before the call: the workspace is not even sized
        ws2 = E.Workspace(DEV)
        with pytest.raises(ValueError, match="not supported"):
            E.forward(flat, batch, E.RunConfig(c["S"], training=True, math=math), ws2, step_gates=sg)
        assert ws2.buf is None
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------ 4. DropEdge per step
RATE = 0.3
KEY = 0x1234_5678_9ABC_DEF1


def _host_rows(batch, key, rate, steps, symmetric=True):
    """The (S, slots) keep decisions from `engine.dropedge_keep_host(step=s)`, slot by slot (padding: 0)."""
    es, ed = batch.edge_src.cpu().numpy(), batch.edge_dst.cpu().numpy()
    nt, nl = batch.node_tower.cpu().numpy(), batch.node_local.cpu().numpy()
    out = np.zeros((steps, len(es)), np.float32)
    for k in np.nonzero((es >= 0) & (ed >= 0))[0]:
        for s in range(steps):
            out[s, k] = float(E.dropedge_keep_host(key, int(nt[es[k]]), int(nl[es[k]]), int(nl[ed[k]]), rate,
                                                   symmetric=symmetric, step=s))
    return out


@pytest.mark.parametrize("kind", ["host", "packed", "capacity"])
def test_step_masks_equal_the_host_draw(kind):
    """Device rows == dropedge_keep_host(step=s) slot by slot; row 0 == spwgnn_dropedge_gates' mask bit for bit;
    rows differ; padding +0 in every row; a shared base row and per-step base rows are multiplied in."""
    import test_gpu_dropedge as GD
    batch = GD._mask_batch(kind)
    S = 4
    pad = ((batch.edge_src < 0) | (batch.edge_dst < 0)).cpu().numpy()
    slots = 32 * batch.n_eblocks
    key_dev = torch.tensor([KEY], dtype=torch.int64, device=DEV)
    for run, key in ((E.RunConfig(S, seed=KEY), KEY), (E.RunConfig(S, seed=5, seed_dev=key_dev), KEY)):
        for sym in (True, False):
            got = E.dropedge_gates(batch, run, RATE, symmetric=sym, per_step=True)
            assert got.shape == (S, slots)
            want = _host_rows(batch, key, RATE, S, sym)
            assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), (kind, sym)
            assert torch.equal(got[0].view(torch.int32), E.dropedge_gates(batch, run, RATE, symmetric=sym).view(torch.int32))
            assert np.all(got.cpu().numpy()[:, pad].view(np.int32) == 0)
            for s in range(S):
                for t in range(s + 1, S):
                    assert not torch.equal(got[s], got[t])
    run = E.RunConfig(S, seed=KEY)
    keep = _host_rows(batch, KEY, RATE, S)
    base1 = torch.linspace(-1.0, 2.0, slots, device=DEV)
    base1[torch.as_tensor(pad, device=DEV)] = float("nan")            # a padding slot is 0 whatever its base holds
    baseS = torch.stack([base1 * (s + 1) for s in range(S)]).contiguous()
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(RATE))
    for base in (base1, baseS):
        got = E.dropedge_gates(batch, run, RATE, rescale=True, base=base, per_step=True).cpu().numpy()
        bb = np.broadcast_to(base.cpu().numpy(), (S, slots))
        want = np.where(pad[None], np.float32(0), bb * np.where(keep != 0, scale, np.float32(0)).astype(np.float32))
        assert np.array_equal(got.view(np.int32), want.astype(np.float32).view(np.int32))
    out = torch.full((S, slots), 9.0, device=DEV)
    assert E.dropedge_gates(batch, run, 0.0, out=out, per_step=True) is out
    assert np.array_equal(out.cpu().numpy(), np.broadcast_to((~pad).astype(np.float32), (S, slots)))


def test_two_shards_give_the_unsharded_masks():
    """The key names an edge by tower id and local indices: shards cut with `tower_ids` draw, per step, their towers'
    part of the whole batch's masks."""
    c, _, _, _ = SR.case("wide")
    B, N, S = c["B"], c["N"], c["S"]
    run = E.RunConfig(S, seed=KEY)
    whole = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], device=DEV)
    mw = E.dropedge_gates(whole, run, RATE, per_step=True)
    dense_w = np.stack([whole.edges_to_input(mw[s], dense=True) for s in range(S)])
    got = []
    for lo, hi in ((0, 1), (1, B)):
        e = np.array(O.dense_to_edges(c["Rs"][lo:hi], c["Rr"][lo:hi]), np.int64).reshape(-1, 4)
        te = np.bincount(e[:, 0], minlength=hi - lo).astype(np.int32)
        shard = TowerBatch.from_edges(c["obj"][lo:hi].reshape(-1, 3), np.full(hi - lo, N, np.int32),
                                      (e[:, 0] * N + e[:, 2]).astype(np.int32), (e[:, 0] * N + e[:, 3]).astype(np.int32), te,
                                      None, DEV, tower_ids=np.arange(lo, hi))
        ms = E.dropedge_gates(shard, run, RATE, per_step=True)
        got.append(np.stack([shard.edges_to_input(ms[s], dense=True) for s in range(S)]))
    assert np.array_equal(np.concatenate(got, axis=1), dense_w) and 0 < dense_w.sum() < dense_w.size


def _oracle_case():
    """team_a with a zero propagation input (the Trainer's batches carry none) and the first Trainer seed whose
    step-0 masks leave every tower's per-step gated ReLU margin above TAU, hold kept and dropped edges in every row
    and separate the two mutants."""
    c = dict(SR.case("team_a")[0])
    c["prop"] = np.zeros_like(c["prop"])
    N = c["N"]
    src, dst = np.asarray(c["src"], np.int64), np.asarray(c["dst"], np.int64)
    for seed in range(40):
        key = dropout_key(seed, 0, 0, 0)
        w = np.array([[float(E.dropedge_keep_host(key, int(a // N), int(a % N), int(b % N), RATE, step=s))
                       for a, b in zip(src, dst)] for s in range(c["S"])], np.float32)
        if not all(0 < row.sum() < len(row) for row in w) or not np.all(SR.step_gated_margins(c, w) > SR.TAU):
            continue
        true = SR.oracle(c, w, "bce")
        if all(SR.mutant_separated(true, SR.oracle(c, m(w), "bce")) for m in (SR.rotated, SR.row0)):
            return c, seed, w
    raise AssertionError("no seed gives every tower a gated ReLU margin above TAU")


def test_trainer_step_against_the_oracle_and_a_manual_step():
    """`Trainer(dropedge=0.3, dropedge_per_step=True)`: one step within criterion of the fp64 oracle under the
    restated masks, and two steps bit for bit equal to a manual forward / bce / backward / Adam with those gates."""
    c, seed, w = _oracle_case()
    print(f"Trainer seed {seed}: kept per step {[int(r.sum()) for r in w]} of {w.shape[1]}")
    ref = SR.oracle(c, w, "bce")
    batch = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], device=DEV)
    tgt = torch.as_tensor(c["tgt"].reshape(-1), device=DEV)
    kw = dict(mp_steps=c["S"], dropout=0.0, seed=seed, math="x6")
    tr = Trainer(P.to_flat(c["params"], device=DEV), dropedge=RATE, dropedge_per_step=True, **kw)
    out3 = tr.step(batch, tgt)
    torch.cuda.synchronize()
    loss_ref = float(O.keras_bce_grad(ref["z"], c["tgt"].reshape(-1).astype(np.float64))[0])
    assert abs(float(out3[0]) - loss_ref) <= 1e-5 * (1.0 + abs(loss_ref))
    g = P.from_flat(tr.engine.grads)
    for name in sorted(ref["g"]):
        RG._close(f"Trainer per-step DropEdge {name}", np.asarray(g[name], np.float64), ref["g"][name])
    tr.step(batch, tgt)
    # by hand, with the gates of engine.dropedge_gates(per_step=True) under the steps' keys
    flat = P.to_flat(c["params"], device=DEV)
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    ws, scratch = E.Workspace(DEV), E.BceScratch(DEV)
    for it in range(2):
        run = E.RunConfig(c["S"], training=True, dropout=0.0, seed=dropout_key(seed, it, 0, 0), math="x6")
        sg = E.dropedge_gates(batch, run, RATE, per_step=True)
        if it == 0:
            assert np.array_equal(_to_ref_order(c, batch, sg.cpu().numpy()), w)
        z = E.forward(flat, batch, run, ws, step_gates=sg)
        _, dz = E.bce(z, tgt, scratch)
        gg, _ = E.backward(flat, batch, run, ws, dz, step_gates=sg)
        E.adam(flat, gg, m, v, it + 1)
    torch.cuda.synchronize()
    assert torch.equal(tr.params, flat) and torch.equal(tr.m, m) and torch.equal(tr.v, v)
    # and the shared mask trains something else
    t1 = Trainer(P.to_flat(c["params"], device=DEV), dropedge=RATE, **kw)
    t1.step(batch, tgt)
    t1.step(batch, tgt)
    assert not torch.equal(t1.params, tr.params)


def test_trainer_replay_equals_step():
    """Trainer.replay_body with per-step DropEdge replayed over three batches of one geometry == Trainer.step on the
    same batches, bit for bit; micro-batches draw per micro-batch."""
    import test_gpu_dropedge as GD
    plans, tgts = GD._plans(3)
    params = O.random_params(12)
    kw = dict(mp_steps=3, dropout=0.1, seed=11, math="x6", dropedge=RATE, dropedge_symmetric=False, dropedge_per_step=True)
    ta = Trainer(P.to_flat(params, device=DEV), **kw)
    for p, t in zip(plans, tgts):
        ta.step(TowerBatch.from_plan(p, DEV), torch.as_tensor(t, device=DEV))
    tb = Trainer(P.to_flat(params, device=DEV), **kw)
    rs = ReplayStep(plans[0], DEV, tb.replay_body(plans[0].n_nodes))
    for p, t in zip(plans, tgts):
        tb.replay_step(rs, p, t)
    torch.cuda.synchronize()
    assert rs.replays == 2
    assert torch.equal(ta.params, tb.params) and torch.equal(ta.m, tb.m) and torch.equal(ta.v, tb.v)
    tc = Trainer(P.to_flat(params, device=DEV), **dict(kw, dropedge_per_step=False))
    for p, t in zip(plans, tgts):
        tc.step(TowerBatch.from_plan(p, DEV), torch.as_tensor(t, device=DEV))
    assert not torch.equal(ta.params, tc.params)
    td = Trainer(P.to_flat(params, device=DEV), **kw)   # two micro-batches in one step
    td.step([TowerBatch.from_plan(p, DEV) for p in plans[:2]], [torch.as_tensor(t, device=DEV) for t in tgts[:2]])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(td.params).all()) and td.iterations == 1


def test_fit_replayed_equals_eager_bitwise():
    """fit with dropedge_per_step for 2 epochs of 2 batches, every step a replayed graph, against the same fit issued
    eagerly: final weights and histories bit for bit; and the per-step masks change them."""
    import test_gpu_dropedge as GD
    from spwgnn_amd.keras_api import PropagationNetwork
    x, y = GD._xy(16, 5, 7)
    res = []
    for graph, per_step in ((True, True), (False, True), (False, False)):
        model = PropagationNetwork(device=DEV, seed=0, mp_steps=3, dropedge=RATE, dropedge_per_step=per_step).getModel(5)
        h = model.fit(x, y, batch_size=8, epochs=2, verbose=0, graph=graph, shuffle=False)
        torch.cuda.synchronize()
        res.append((h, model.net.flat.detach().cpu().numpy().copy(), model.iterations))
    (ha, wa, ia), (hb, wb, ib), (hc, wc, _) = res
    assert ia == ib == 4 and ha == hb and np.array_equal(wa, wb)
    assert np.all(np.isfinite(wa)) and not np.array_equal(wa, wc)
    with pytest.raises(ValueError):
        xr = dict(x, relation_weights=np.ones((16, 5, 5), np.float32))
        PropagationNetwork(device=DEV, dropedge=RATE, dropedge_per_step=True).getModel(5).fit(xr, y, verbose=0)


def test_graph_network_draws_per_step_in_train_mode_only():
    c, _, _, _ = SR.case("team_a")
    net = GraphNetwork(c["S"], dropout=0.0, device=DEV, params=c["params"], dropedge=0.5, dropedge_per_step=True)
    plain = GraphNetwork(c["S"], dropout=0.0, device=DEV, params=c["params"])
    batch = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], device=DEV)
    w = torch.full((batch.n_edges,), 0.75, device=DEV, requires_grad=True)
    net.train()
    plain.train()
    key = net._step_seed + 1
    z = net.forward_batch(batch, relation_weights=w)           # a shared weight row under the per-step masks
    assert net._step_seed == key
    mask = E.dropedge_gates(batch, E.RunConfig(c["S"], seed=key), 0.5, per_step=True)
    kept = np.stack([batch.edges_to_input(mask[s])[2] for s in range(c["S"])])
    wk = (w.detach()[None] * torch.as_tensor(kept, device=DEV)).requires_grad_(True)
    want = plain.forward_batch(batch, relation_step_weights=wk)
    assert torch.equal(z.detach(), want.detach())
    z.sum().backward()
    want.sum().backward()
    assert torch.equal(net.flat.grad, plain.flat.grad)
    got = w.grad.cpu().numpy()
    ref = (wk.grad.cpu().numpy() * kept).sum(0)                # the chain rule through the masks, summed over the steps
    assert np.allclose(got, ref, rtol=1e-6, atol=1e-9) and np.any(got != 0)
    seed = net._step_seed
    net.eval()
    plain.eval()
    assert torch.equal(net.forward_batch(batch).detach(), plain.forward_batch(batch).detach())
    net.train()
    with torch.no_grad():
        assert torch.equal(net.forward_batch(batch), plain.forward_batch(batch))
    assert net._step_seed == seed
