"""GPU: relation gates — `engine.forward(..., gates=)` / `engine.backward(..., gates=)` (spwgnn_forward_gated /
spwgnn_backward_gated), the gate gradient `engine.backward_relations` returns after them, and the autograd path of
`GraphNetwork` (`relation_weights=`, `forward_positions(soft_tau=)`) — against fp64 torch autograd through the gated
oracle with ONE shared gate tensor, the objects and the propagation input as leaves (tests/relation_gates_ref.py;
DESIGN.md §3zz).

Inputs: the cases of tests/test_gpu_input_grad.py. Gates: default_rng(1000).uniform(0.25, 1.5), the first three set
to 0, 1 and −0.5, in the order of the case's edge list; tests/test_relation_gates_host.py holds every tower's ReLU
margin under the gated forward above TAU = 1e-6, so no tower is left out here.

Criteria (x6 and h3): logits |Δ| <= 1e-5 + 1e-5·|z|; every parameter tensor, d/d'propagation', d/d objects and the
gate gradient max|Δ| <= 1e-5·max|ref| + 1e-8 (the project's gradient criterion). x3: at most twice the error of the
same case's UNGATED x3 run on the wide kernels against the ungated oracle (parent code; the factor is the precedent
of test_gpu_input_grad.py case 6).

Measured on MI355X: see DESIGN.md §3zz.
"""
import numpy as np
import pytest
import torch

import relation_gates_ref as GR
import test_gpu_input_grad as IG
from oracle import model as O
from spwgnn_amd import GraphNetwork, TowerBatch, _lib, data as D, engine as E, params as P

pytestmark = pytest.mark.gpu

DEV = "cuda"
SPLIT = ["x6", "x3", "h3"]
EXACT = ["x6", "h3"]


# ------------------------------------------------------------------------------------ inputs
def _batch(c, kind):
    if kind == "team":      # a small batch: the ungated call would take the team / fused kernels
        b = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], c["prop"], device=DEV)
        assert b.n_eblocks <= E.team_max_blocks() == 512
    elif kind == "wide16":  # two towers per wave-tile, more than one block per tile
        b = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], c["prop"], device=DEV, nw_max=16)
        assert b.n_eblocks > b.n_wtiles
    elif kind == "recv":    # a receiver-block plan: the gated call runs the one-hot edge forward on it
        b = TowerBatch.fully_connected(c["obj"], c["prop"], device=DEV, recv_blocks=True)
        assert b.flags & _lib.BATCH_RECV_BLOCKS
    elif kind == "tile32":  # an ordinary plan whose wave-tiles hold 18 nodes: the 17–32-node kernels
        b = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], c["prop"], device=DEV, nw_max=32)
        assert not b.flags and 16 < b.nw_max <= 32
    else:
        raise ValueError(kind)
    return b


def _edge_pairs(batch):
    """(sender, receiver) of the batch's edges in its input edge order, in the INPUT's node ids."""
    s, d, _ = batch.edges_to_input(np.zeros(32 * batch.n_eblocks))
    return s, d


def _slot_gates(c, batch, gate, fill=0.0):
    """The case's gates (the order of c["src"] / c["dst"]) → the plan's slot tensor, matched by (sender, receiver)."""
    s, d = _edge_pairs(batch)
    nn = batch.n_nodes
    ref_key = np.asarray(c["src"], np.int64) * nn + np.asarray(c["dst"], np.int64)
    order = np.argsort(ref_key, kind="stable")
    pos = order[np.searchsorted(ref_key[order], s * nn + d)]
    assert np.array_equal(ref_key[pos], s * nn + d)
    return batch.edge_gates(torch.as_tensor(np.asarray(gate, np.float32)[pos], device=DEV), fill=fill)


def _to_ref_order(c, batch, slot_values):
    s, d, v = batch.edges_to_input(slot_values)
    nn = batch.n_nodes
    got_key = s * nn + d
    order = np.argsort(got_key, kind="stable")
    ref_key = np.asarray(c["src"], np.int64) * nn + np.asarray(c["dst"], np.int64)
    pos = order[np.searchsorted(got_key[order], ref_key)]
    assert np.array_equal(got_key[pos], ref_key)
    return v[..., pos]


# ------------------------------------------------------------------------------------ engine
def _run(c, batch, math, gates, loss="bce", tgt=None, state=False, dstate=None, training=True):
    """One step's forward + loss + backward (+ backward_inputs, backward_relations) with `gates` (slot order, or
    None: ungated). Returns a dict of device tensors."""
    flat = P.to_flat(c["params"], device=DEV)
    ws = E.Workspace(DEV)
    run = E.RunConfig(c["S"], training=training, math=math)
    out = E.forward(flat, batch, run, ws, return_state=state, gates=gates)
    z, st = out if state else (out, None)
    res = dict(z=z, state=st, flat=flat, ws=ws, run=run)
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
    g, dp = E.backward(flat, batch, run, ws, dz, want_dprop=batch.prop is not None, dstate=dstate, gates=gates)
    res.update(g=g, dp=dp, dobj=E.backward_inputs(flat, batch, run, ws).clone(),
               drel=E.backward_relations(flat, batch, run, ws))
    torch.cuda.synchronize()
    return res


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _close(what, got, ref):
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    msg = f"{what}: max|got - ref| {err:.3e} = {err / scale:.2e} of max|ref| {scale:.3e}"
    print(msg)
    assert err <= 1e-5 * scale + 1e-8, msg


def _logits_close(what, z, z_ref, factor=1.0):
    err = np.abs(z - z_ref)
    print(f"{what}: max|dz| {err.max():.3e} (max|z| {np.abs(z_ref).max():.3e})")
    assert np.all(err <= factor * (1e-5 + 1e-5 * np.abs(z_ref))), (what, err.max())


def _check(what, c, batch, res, ref, dprop=True, order=None):
    """Every output of `res` against the fp64 oracle `ref` at the module docstring's criteria. `order`: maps
    per-node rows from the plan's order to the input's (packed plans)."""
    order = (lambda x: x) if order is None else order
    _logits_close(what, order(_np(res["z"])), ref["z"])
    g = P.from_flat(res["g"])
    for name in sorted(ref["g"]):
        _close(f"{what} {name}", np.asarray(g[name], np.float64), ref["g"][name])
    if dprop:
        _close(what + " dprop", order(_np(res["dp"])), ref["dprop"])
    _close(what + " dobj", order(_np(res["dobj"])), ref["dobj"])
    drel = res["drel"]
    pad = (batch.edge_src < 0) | (batch.edge_dst < 0)
    assert drel.shape == (32 * batch.n_eblocks,) and bool((drel[pad] == 0).all())
    _close(what + " dgate", _to_ref_order(c, batch, _np(drel)), ref["dgate"])


def _bits_equal(what, a, b, keys=("z", "g", "dp", "dobj", "drel", "state")):
    for k in keys:
        if a.get(k) is None and b.get(k) is None:
            continue
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{what}: {k} differs"


# ------------------------------------------------------------------------------------ 1. unit gates are free
@pytest.mark.parametrize("math", SPLIT)
@pytest.mark.parametrize("name,kind", [("wide", "wide16"), ("team_a", "team")])
def test_unit_gates_are_the_ungated_wide_run(name, kind, math):
    """w ≡ 1: logits, state, parameter gradients, dprop (and d/d objects, the gate gradient) are bitwise those of the
    ungated call on the wide kernels (x · 1.0 = x)."""
    c = IG._case(name)
    with E.wide_kernels():
        batch = _batch(c, kind) if kind != "team" else TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], c["prop"], device=DEV)
        plain = _run(c, batch, math, None, state=True)
    ones = batch.edge_gates(torch.ones(batch.n_edges, device=DEV))
    assert E.team_max_blocks() == 512
    gated = _run(c, batch, math, ones, state=True)
    _bits_equal(f"{name} {math} unit gates", gated, plain)
    assert bool(torch.isfinite(gated["z"]).all()) and float(gated["g"].abs().max()) > 0


# ------------------------------------------------------------------------------------ 2. parity with the fp64 oracle
@pytest.mark.parametrize("math", EXACT)
@pytest.mark.parametrize("name,kind", [("team_a", "team"), ("team_b", "team"), ("wide", "wide16"), ("recv", "recv"),
                                       ("recv", "tile32")])
def test_oracle_parity(name, kind, math):
    """BCE and Σ sigmoid(z): small batches (the wide fallback), tiles spanning more than one block, a receiver-block
    plan, and 18-node wave-tiles (the 8-wave edge forward and k_edge_bwd<false, …>)."""
    c = IG._case(name)
    gate = GR.gates_for(len(c["src"]))
    batch = _batch(c, kind)
    gates = _slot_gates(c, batch, gate)
    for loss in ("bce", "sum_prob"):
        ref = GR.oracle(c, gate, loss, key=name)
        _check(f"{name}/{kind} {math} {loss}", c, batch, _run(c, batch, math, gates, loss), ref)


_RAGGED = []


def _ragged():
    if not _RAGGED:
        c, sizes, tes = IG._ragged_case()
        gate, seed = GR.pick_gates(c, sizes)
        print(f"ragged case: gate seed {seed}")
        _RAGGED.append((c, sizes, tes, gate))
    return _RAGGED[0]


@pytest.mark.parametrize("math", EXACT)
def test_oracle_parity_packed_ragged_null_prop(math):
    """Towers of 1, 2, 4, 7 and 3 boxes in a packed plan with a null propagation input (step 0 reads no U, V row):
    the gates go through node_perm (`edge_gates`), results come back through `to_input_order`."""
    c, sizes, tes, gate = _ragged()
    batch = TowerBatch.from_edges(c["obj"], sizes, c["src"].astype(np.int32), c["dst"].astype(np.int32), tes, device=DEV,
                                  pack=True)
    assert batch.prop is None and batch.node_perm is not None
    assert not np.array_equal(batch.node_perm, np.arange(batch.n_nodes))
    gates = _slot_gates(c, batch, gate)
    for loss in ("bce", "sum_prob"):
        ref = GR.oracle(c, gate, loss, key="ragged")
        res = _run(c, batch, math, gates, loss, tgt=batch.to_plan_order(c["tgt"]))
        _check(f"ragged packed {math} {loss}", c, batch, res, ref, dprop=False, order=batch.to_input_order)


# ------------------------------------------------------------------------------------ 3. x3
def _errors(c, batch, res, ref):
    """{name: error}: the largest logit error, and each tensor's relative L2 error."""
    rel = lambda got, want: float(np.linalg.norm(got - want) / np.linalg.norm(want))
    out = {"logits": float(np.abs(_np(res["z"]) - ref["z"]).max())}
    g = P.from_flat(res["g"])
    for name in sorted(ref["g"]):
        out[name] = rel(np.asarray(g[name], np.float64), ref["g"][name])
    out["dprop"] = rel(_np(res["dp"]), ref["dprop"])
    out["dobj"] = rel(_np(res["dobj"]), ref["dobj"])
    out["dgate"] = rel(_to_ref_order(c, batch, _np(res["drel"])), ref["dgate"])
    return out


@pytest.mark.parametrize("name,kind", [("wide", "wide16"), ("team_a", "team")])
def test_x3_errors_against_the_ungated_x3_run(name, kind):
    """The logit error and each tensor's relative L2 error of the gated x3 run against the gated oracle are at most
    twice those of the UNGATED x3 run of the same case on the wide kernels against the ungated oracle."""
    c = IG._case(name)
    gate = GR.gates_for(len(c["src"]))
    with E.wide_kernels():
        batch = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], c["prop"], device=DEV, nw_max=16 if kind == "wide16" else None)
        plain = _errors(c, batch, _run(c, batch, "x3", None), GR.oracle(c, np.ones(len(c["src"])), "bce", key=name + "/ones"))
    gated = _errors(c, batch, _run(c, batch, "x3", _slot_gates(c, batch, gate)), GR.oracle(c, gate, "bce", key=name))
    worst = max(gated[k] / plain[k] for k in plain)
    for k in plain:
        print(f"x3 {name} {k}: gated {gated[k]:.3e} ungated {plain[k]:.3e} ratio {gated[k] / plain[k]:.2f}")
    print(f"x3 {name}: largest ratio {worst:.2f}")
    for k in plain:
        assert gated[k] <= 2 * plain[k], (k, gated[k], plain[k])


# ------------------------------------------------------------------------------------ 4. gate 0 is deletion
@pytest.mark.parametrize("math", EXACT)
def test_gate_zero_against_a_batch_without_the_edges(math):
    """Gates 0 on a third of `wide`'s edges (1 elsewhere) against an UNGATED batch built without those edges: both
    sit within the logit criterion of the same exact value, so within twice it of each other."""
    c = IG._case("wide")
    keep = np.arange(len(c["src"])) % 3 != 0
    batch = _batch(c, "wide16")
    z_gated = _np(_run(c, batch, math, _slot_gates(c, batch, keep.astype(np.float32)), training=False)["z"])
    te = np.bincount(c["src"][keep] // c["N"], minlength=c["B"]).astype(np.int32)
    cut = TowerBatch.from_edges(c["obj"].reshape(-1, 3), np.full(c["B"], c["N"], np.int32), c["src"][keep].astype(np.int32),
                                c["dst"][keep].astype(np.int32), te, c["prop"].reshape(-1, 100), device=DEV, nw_max=16)
    assert cut.n_edges == int(keep.sum()) < batch.n_edges
    z_cut = _np(_run(c, cut, math, None, training=False)["z"])
    tp = O.to_torch(c["params"])
    with torch.no_grad():
        z_ref = O.forward_gather(tp, torch.as_tensor(c["obj"].reshape(-1, 3), dtype=GR.F64),
                                 torch.as_tensor(c["src"][keep]), torch.as_tensor(c["dst"][keep]),
                                 torch.as_tensor(c["prop"].reshape(-1, 100), dtype=GR.F64), c["S"]).numpy()
    _logits_close(f"gate 0 {math}: gated against the exact value", z_gated, z_ref)
    _logits_close(f"gate 0 {math}: gated against the cut batch", z_gated, z_cut, factor=2.0)


# ------------------------------------------------------------------------------------ 5. bitwise properties
def test_inference_forward_is_the_training_forward():
    c = IG._case("wide")
    batch = _batch(c, "wide16")
    gates = _slot_gates(c, batch, GR.gates_for(len(c["src"])))
    train = _run(c, batch, "x6", gates, state=True)
    infer = _run(c, batch, "x6", gates, state=True, training=False)
    _bits_equal("inference against training at dropout 0", infer, train, keys=("z", "state"))


def test_stored_steps_do_not_change_the_gated_gradients():
    """K = 0 stored dh1pre steps (every step rebuilt by k_dA_x6<GATE>) against K = 3 (read back from the gated edge
    backward's slabs) at S = 5; and two runs of the same call."""
    c = IG._case("wide")
    assert c["S"] == 5
    batch = _batch(c, "wide16")
    gates = _slot_gates(c, batch, GR.gates_for(len(c["src"])))
    assert E.da_stored_steps() == E.DA_STORED_DEFAULT == 3
    k3 = _run(c, batch, "x6", gates)
    again = _run(c, batch, "x6", gates)
    with E.da_stored(0):
        k0 = _run(c, batch, "x6", gates)
    _bits_equal("two runs", again, k3)
    _bits_equal("K = 0 against K = 3", k0, k3)
    assert float(k3["g"].abs().max()) > 0


@pytest.mark.parametrize("kind", ["team", "capacity"])
def test_nan_in_the_padding_slots_changes_nothing(kind):
    c = IG._case("team_a")
    gate = GR.gates_for(len(c["src"]))
    if kind == "team":
        batch = _batch(c, "team")
    else:   # a capacity plan filled on the device: N(N−1) slots per tower whatever is active
        batch = TowerBatch.from_dense_device(*(torch.as_tensor(np.asarray(c[k], np.float32), device=DEV)
                                               for k in ("obj", "Rs", "Rr", "prop")), check=True)
    pad = (batch.edge_src < 0) | (batch.edge_dst < 0)
    assert int(pad.sum()) > 0
    zero, nan = _slot_gates(c, batch, gate, 0.0), _slot_gates(c, batch, gate, float("nan"))
    assert bool(torch.isnan(nan[pad]).all()) and torch.equal(zero[~pad], nan[~pad])
    a, b = _run(c, batch, "x6", zero, state=True), _run(c, batch, "x6", nan, state=True)
    _bits_equal("NaN padding", b, a)
    for k in ("z", "g", "dp", "dobj", "drel", "state"):
        assert bool(torch.isfinite(b[k]).all()), k


# ------------------------------------------------------------------------------------ 6. state
def test_state_and_its_cotangent():
    """`state_out` and a `dstate` cotangent with gates: the loss is BCE + Σ dstate·P_S."""
    c = IG._case("team_b")
    gate = GR.gates_for(len(c["src"]))
    batch = _batch(c, "team")
    dstate = np.random.default_rng(5).normal(0, 0.05, (batch.n_nodes, 100)).astype(np.float32)
    ref = GR.oracle(c, gate, "bce", dstate=dstate)
    res = _run(c, batch, "x6", _slot_gates(c, batch, gate), state=True, dstate=torch.as_tensor(dstate, device=DEV))
    _close("state P_S", _np(res["state"]), ref["state"])
    _check("team_b x6 bce + dstate", c, batch, res, ref)


# ------------------------------------------------------------------------------------ 7. autograd
def test_relation_weights_leaf_through_graph_network():
    """A (B, N, N) `relation_weights` leaf: its .grad is the engine's gate gradient bit for bit, within criterion of
    the oracle; weights, propagation and objects get their gradients in the same pass."""
    c = IG._case("team_b")
    B, N = c["B"], c["N"]
    gate = GR.gates_for(len(c["src"]))
    dense = np.zeros((B, N, N), np.float32)
    dense[c["src"] // N, c["src"] % N, c["dst"] % N] = gate
    net = GraphNetwork(mp_steps=c["S"], dropout=0.0, device=DEV, params=c["params"])
    net.train()
    W = torch.tensor(dense, device=DEV, requires_grad=True)
    obj = torch.tensor(c["obj"], device=DEV, requires_grad=True)
    prop = torch.tensor(c["prop"], device=DEV, requires_grad=True)
    z, state = net.forward_logits(obj, c["Rs"], c["Rr"], prop, relation_weights=W, return_state=True)
    assert z.shape == (B, N) and state.shape == (B, N, 100)
    z.sum().backward()
    ref = GR.oracle(c, gate, "sum", key="team_b")
    _logits_close("relation_weights logits", _np(z).reshape(-1), ref["z"])
    got = _np(W.grad)
    mask = dense != 0
    mask[c["src"] // N, c["src"] % N, c["dst"] % N] = True
    assert np.all(got[~mask] == 0)
    _close("relation_weights .grad", got[c["src"] // N, c["src"] % N, c["dst"] % N], ref["dgate"])
    _close("objects .grad", _np(obj.grad).reshape(-1, 3), ref["dobj"])
    _close("propagation .grad", _np(prop.grad).reshape(-1, 100), ref["dprop"])
    # the engine's own gate gradient for the same gates and dlogits = 1
    batch = _batch(c, "team")
    res = _run(c, batch, "x6", _slot_gates(c, batch, gate), loss="sum", state=True)
    assert np.array_equal(batch.edges_to_input(res["drel"].cpu().numpy(), dense=True), W.grad.cpu().numpy())
    assert torch.equal(res["g"], net.flat.grad)
    with pytest.raises(ValueError, match="return_steps"):
        net.forward_logits(obj, c["Rs"], c["Rr"], prop, relation_weights=W, return_steps=True)
    with pytest.raises(ValueError, match="not supported"):
        GraphNetwork(mp_steps=c["S"], device=DEV, params=c["params"], math="bf16").forward_logits(
            obj, c["Rs"], c["Rr"], prop, relation_weights=W)


SOFT_SEED, SOFT_TAU = 23, 20.0   # the seed whose gated ReLU margins exceed TAU (asserted below)


def _soft_case():
    """Two five-box towers, fully connected, gates = sigmoid((170 − distance) / 20) of the raw positions."""
    B, N = 2, 5
    raw = D.synthetic_towers(B, N, seed=SOFT_SEED).astype(np.float32)
    m, j = np.nonzero(~np.eye(N, dtype=bool))
    src = np.concatenate([b * N + m for b in range(B)]).astype(np.int64)
    dst = np.concatenate([b * N + j for b in range(B)]).astype(np.int64)
    c = dict(params=O.random_params(2), obj=(raw / np.float32(D.RELATION_THRESHOLD)).astype(np.float32),
             prop=np.zeros((B * N, 100), np.float32), tgt=None, src=src, dst=dst, S=5, B=B, N=N)
    return c, raw


def test_forward_positions_soft_threshold():
    """`forward_positions(soft_tau=20)`: d Σ sigmoid(z) / d raw flows through the object rows AND through the gates;
    against fp64 autograd of the same composition with raw as the leaf."""
    c, raw = _soft_case()
    raw64 = torch.tensor(raw.reshape(-1, 3), dtype=GR.F64, requires_grad=True)
    src, dst = torch.as_tensor(c["src"]), torch.as_tensor(c["dst"])
    w = GR.soft_threshold_gates(raw64[:, :2], src, dst, float(D.RELATION_THRESHOLD), SOFT_TAU)
    m = GR.gated_margins(c, w.detach().numpy())
    print(f"soft threshold: gates {float(w.min()):.3f} .. {float(w.max()):.3f}, gated ReLU margins min {m.min():.2e}")
    assert np.all(m > GR.TAU), m
    z64, _ = GR.forward(O.to_torch(c["params"]), raw64 / float(D.RELATION_THRESHOLD), src, dst,
                        torch.zeros(len(raw64), 100, dtype=GR.F64), c["S"], w)
    torch.sigmoid(z64).sum().backward()
    net = GraphNetwork(mp_steps=c["S"], dropout=0.0, device=DEV, params=c["params"])
    net.train()
    raw_t = torch.tensor(raw, device=DEV, requires_grad=True)
    z = net.forward_positions(raw_t, float(D.RELATION_THRESHOLD), float(D.RELATION_THRESHOLD), soft_tau=SOFT_TAU)
    assert z.shape == (c["B"], c["N"])
    torch.sigmoid(z).sum().backward()
    _logits_close("soft threshold logits", _np(z).reshape(-1), z64.detach().numpy())
    _close("soft threshold d/d raw", _np(raw_t.grad).reshape(-1, 3), raw64.grad.numpy())
    # the part that flows through the gates is not small: without it the criterion is missed
    hard = torch.tensor(raw, device=DEV, requires_grad=True)
    torch.sigmoid(net.forward_positions(hard, None, float(D.RELATION_THRESHOLD))).sum().backward()
    assert float((hard.grad - raw_t.grad).abs().max()) > 1e-3 * float(raw_t.grad.abs().max())


# ------------------------------------------------------------------------------------ 8. errors
def test_errors():
    c = IG._case("team_b")
    batch = _batch(c, "team")
    flat = P.to_flat(c["params"], device=DEV)
    gates = _slot_gates(c, batch, GR.gates_for(len(c["src"])))
    ws, run = E.Workspace(DEV), E.RunConfig(c["S"], training=True)
    z = E.forward(flat, batch, run, ws, gates=gates)
    dz = torch.ones_like(z)
    with pytest.raises(ValueError, match="relation gates of the forward"):
        E.backward(flat, batch, run, ws, dz)                            # no gates
    with pytest.raises(ValueError, match="relation gates of the forward"):
        E.backward(flat, batch, run, ws, dz, gates=gates.clone())       # other gates
    E.backward(flat, batch, run, ws, dz, gates=gates)
    E.backward_relations(flat, batch, run, ws)
    z = E.forward(flat, batch, run, ws, gates=gates)
    gates.mul_(1.0)                                                     # written since the forward
    with pytest.raises(ValueError, match="relation gates of the forward"):
        E.backward(flat, batch, run, ws, dz, gates=gates)
    E.forward(flat, batch, run, ws)                                     # an ungated forward takes no gates back
    with pytest.raises(ValueError, match="relation gates of the forward"):
        E.backward(flat, batch, run, ws, dz, gates=gates)
    for bad in (gates[:-1], torch.cat([gates, gates[:1]]), gates.reshape(-1, 32), gates.double(), gates.cpu()):
        with pytest.raises((ValueError, _lib.SpwgnnError)):
            E.forward(flat, batch, run, ws, gates=bad)
    with pytest.raises(ValueError, match="16-byte"):
        E.forward(flat, batch, run, ws, gates=torch.cat([gates[:1], gates])[1:])
    for math in ("f32", "bf16"):   # refused before the call: the workspace is not even sized
        ws2 = E.Workspace(DEV)
        with pytest.raises(ValueError, match="not supported"):
            E.forward(flat, batch, E.RunConfig(c["S"], training=True, math=math), ws2, gates=gates)
        assert ws2.buf is None
    torch.cuda.synchronize()
