"""GPU: relation sets outside the symmetric family (tests/topology_ref.py) on every path — directed,
uneven-degree, receiver-major and shuffled edge lists, repeated pairs, a→a — one training step each (forward, BCE,
backward, backward_inputs, backward_relations) against fp64 torch autograd (`relation_gates_ref.oracle`).

The reference sums a repeated pair's two messages and an a→a message like any other (Networks.py:84-88 multiplies
by the relation matrices, whatever their columns hold), so the engine must too.

Criteria (f32, x6, h3): logits |Δ| <= 1e-5 + 1e-5·|z|; every parameter gradient, d/d'propagation', d/d objects, the
relation (gate) gradient and the state, per tensor, max|Δ| <= 1e-5·max|ref| + 1e-8; padding slots of the relation
gradient exactly 0. x3 and bf16: the bounds of test_gpu_relation_grad.py::test_lower_precision_maths (relation
gradient: relative L2 error at most 2× the same run's rmp.1.kernel gradient's) and of test_gpu_x3.py (logits and
d/d objects: 32 × the x3 error <= the bf16 error of the same case and path).

Every case asserts its towers' ReLU margins (TAU = 1e-6, none left out) in `topology_ref.case`; the gated variants
theirs in `topology_ref.gates`. tests/test_topology_host.py shows that each case separates a swapped, a dropped and
a reordered edge by more than 100× these criteria. The whole file also passes under SPWGNN_POISON_WORKSPACE=1.

Measured on MI355X: DESIGN.md §6d.
"""
import contextlib

import numpy as np
import pytest
import torch

import dropedge_ref as DREF
import test_gpu_relation_gates as TG
import topology_ref as T
from spwgnn_amd import TowerBatch, _lib, engine as E, params as P

pytestmark = pytest.mark.gpu

DEV = "cuda"


# ------------------------------------------------------------------------------------ batches
def _batch(c, kind):
    nn = int(c["sizes"].sum())
    args = (c["obj"].reshape(nn, 3), c["sizes"], c["src"].astype(np.int32), c["dst"].astype(np.int32), c["te"],
            c["prop"].reshape(nn, 100))
    if kind == "default":     # a small batch, one tower per wave-tile of at most 16 nodes: the team / fused kernels
        b = TowerBatch.from_edges(*args, device=DEV, recv_blocks=False)
        assert b.nw_max <= 16 and b.n_eblocks <= 512 and E.team_max_blocks() in (0, 512)   # 0: inside wide_kernels()
    elif kind == "packed":
        b = TowerBatch.from_edges(*args, device=DEV, recv_blocks=False, pack=True)
        assert b.node_perm is not None and not np.array_equal(b.node_perm, np.arange(nn))
    elif kind == "tile32":    # an ordinary plan of whole towers: above 16 nodes the 8-wave edge forward and the csr walk
        b = TowerBatch.from_edges(*args, device=DEV, nw_max=32, recv_blocks=False)
        assert not b.flags and b.nw_max == int(c["sizes"].max())
    elif kind == "recv":
        b = TowerBatch.from_edges(*args, device=DEV, recv_blocks=True)
        assert b.flags & _lib.BATCH_RECV_BLOCKS and b.n_eblocks == nn
    elif kind == "capacity":
        full = (c["sizes"].astype(np.int64) * (c["sizes"] - 1)).astype(np.int32)
        b = TowerBatch.from_edges(*args, device=DEV, edge_cap=full)
    else:
        raise ValueError(kind)
    return b


def _edge_maps(c, batch):
    """(to_case, to_batch): values in the batch's edge order [to_case] are in the case's order, and the reverse. The
    two lists hold the same pairs (node ids through node_perm); the k-th occurrence of a repeated pair in one is the
    k-th in the other, since plans move towers as wholes and keep the order inside a tower."""
    s, d, _ = batch.edges_to_input(np.zeros(32 * batch.n_eblocks, np.float32))
    nn = batch.n_nodes
    got, ref = s * nn + d, c["src"] * nn + c["dst"]
    og, orf = np.argsort(got, kind="stable"), np.argsort(ref, kind="stable")
    assert np.array_equal(got[og], ref[orf])
    to_case, to_batch = np.empty(len(ref), np.int64), np.empty(len(ref), np.int64)
    to_case[orf], to_batch[og] = og, orf
    if batch.node_perm is None:
        assert np.array_equal(to_case, np.arange(len(ref)))   # the plan's edge order is the input's
    return to_case, to_batch


def _slot_gates(c, batch, gate):
    return batch.edge_gates(torch.as_tensor(np.asarray(gate, np.float32)[_edge_maps(c, batch)[1]], device=DEV))


def _limit(wide):
    return E.wide_kernels() if wide else contextlib.nullcontext()


def _run(c, batch, math, gates=None, state=False, dstate=None):
    tgt = batch.to_plan_order(np.asarray(c["tgt"], np.float32).reshape(-1))
    if dstate is not None:
        dstate = torch.as_tensor(batch.to_plan_order(np.asarray(dstate, np.float32)), device=DEV)
    return TG._run(c, batch, math, gates, tgt=tgt, state=state, dstate=dstate)


# ------------------------------------------------------------------------------------ checks
def _check(what, c, batch, res, ref, state=False):
    """Every output against the fp64 reference at the module docstring's criteria; prints the figures first."""
    inp = batch.to_input_order
    z = inp(TG._np(res["z"]))
    ex = {"z": T.logit_excess(z, ref["z"])}
    g = P.from_flat(res["g"])
    ratio = {}
    for name in sorted(ref["g"]):
        ex["g:" + name] = T.tensor_excess(g[name], ref["g"][name])
        ratio["g:" + name] = np.abs(np.asarray(g[name], np.float64) - ref["g"][name]).max() / np.abs(ref["g"][name]).max()
    drel = res["drel"]
    pad = (batch.edge_src < 0) | (batch.edge_dst < 0)
    assert drel.shape == (32 * batch.n_eblocks,) and bool((drel[pad] == 0).all()), what + ": padding slots of drel"
    _, _, vals = batch.edges_to_input(TG._np(drel))
    outs = {"dprop": (inp(TG._np(res["dp"])), ref["dprop"]), "dobj": (inp(TG._np(res["dobj"])), ref["dobj"]),
            "dgate": (vals[_edge_maps(c, batch)[0]], ref["dgate"])}
    if state:
        outs["state"] = (inp(TG._np(res["state"])), ref["state"])
    for k, (got, want) in outs.items():
        ex[k] = T.tensor_excess(got, want)
        ratio[k] = np.abs(got - want).max() / np.abs(want).max()
    worst = max(ratio, key=ratio.get)
    print(f"TOPOLOGY {what}: max|dz| {np.abs(z - ref['z']).max():.2e} (max|z| {np.abs(ref['z']).max():.2f}), "
          f"worst gradient ratio {ratio[worst]:.2e} ({worst}), dgate {ratio['dgate']:.2e}")
    bad = {k: v for k, v in ex.items() if not v <= 1.0}
    assert not bad, (what, "times the criterion:", bad)


# ------------------------------------------------------------------------------------ 1. oracle parity
SMALL = [(n, k, w) for n in ("chain", "mixed", "ragged_mixed") for k, w in (("default", False), ("default", True))]
SMALL.append(("ragged_mixed", "packed", False))
BIG = [(n, k, w) for n in ("star_in", "star_out", "hubs", "dag")
       for k, w in (("tile32", False), ("tile32", True), ("recv", False))]
BIG += [("star32", "recv", False), ("star32", "tile32", False)]
PARITY = [(n, k, w, m) for n, k, w in SMALL + BIG for m in ("f32", "x6")]
PARITY += [(n, k, w, "h3") for n, k, w in SMALL + BIG if n in ("mixed", "star_in")]


@pytest.mark.parametrize("name,kind,wide,math", PARITY,
                         ids=[f"{n}-{k}-{'wide' if w else 'team'}-{m}" for n, k, w, m in PARITY])
def test_oracle_parity(name, kind, wide, math):
    c = T.case(name)
    ref = T.reference(name)
    with _limit(wide):
        batch = _batch(c, kind)
        run = E.RunConfig(c["S"], training=True, math=math)
        path = E.fused_path(batch, run)
        if kind in ("default", "packed") and not wide and math != "f32":
            assert path == 3, path              # the fused small-batch loops, forward and backward
        if wide or kind in ("tile32", "recv") and batch.nw_max > 16:
            assert path == 0, path
        res = _run(c, batch, math)
    _check(f"{name}/{kind}/{'wide' if wide else 'team'} {math}", c, batch, res, ref)


# ------------------------------------------------------------------------------------ 2. state
@pytest.mark.parametrize("name,kind,wide", [("mixed", "default", False), ("star_in", "tile32", True)])
def test_state_and_its_cotangent(name, kind, wide):
    c = T.case(name)
    dstate = np.random.default_rng(5).normal(0, 0.05, (int(c["sizes"].sum()), 100)).astype(np.float32)
    ref = T.reference(name, dstate=dstate)
    with _limit(wide):
        batch = _batch(c, kind)
        res = _run(c, batch, "x6", state=True, dstate=dstate)
    _check(f"{name}/{kind}/{'wide' if wide else 'team'} x6 + dstate", c, batch, res, ref, state=True)


# ------------------------------------------------------------------------------------ 3. gated
@pytest.mark.parametrize("name,kind,wide", [("mixed", "default", False), ("mixed", "default", True),
                                            ("star_in", "tile32", False), ("star_in", "recv", False)])
def test_gated(name, kind, wide):
    """Gates with a 0, a 1 and a −0.5 (`pick_gates`): a repeated pair's two slots carry different gates."""
    c, gate = T.case(name), T.gates(name)
    ref = T.reference(name, gated=True)
    with _limit(wide):
        batch = _batch(c, kind)
        if kind == "default" and not wide:
            assert E.fused_path(batch, E.RunConfig(c["S"], training=True, math="x6"), gated=True) == 3
        res = _run(c, batch, "x6", gates=_slot_gates(c, batch, gate))
    _check(f"{name}/{kind}/{'wide' if wide else 'team'} x6 gated", c, batch, res, ref)


# ------------------------------------------------------------------------------------ 4. bitwise properties
@pytest.mark.parametrize("name,kind", [("mixed", "default"), ("star_in", "tile32")])
def test_team_and_wide_agree_and_runs_repeat(name, kind, monkeypatch):
    """Team and wide kernels give equal logits and d/d'propagation'; two runs on poisoned workspaces are equal in
    every output and leave no NaN or poison pattern."""
    monkeypatch.setattr(E, "POISON_WORKSPACE", True)
    c = T.case(name)
    batch = _batch(c, kind)
    team, again = _run(c, batch, "x6", state=True), _run(c, batch, "x6", state=True)
    with E.wide_kernels():
        wide = _run(c, batch, "x6", state=True)
    TG._bits_equal(f"{name}: two runs", again, team)
    TG._bits_equal(f"{name}: team against wide", wide, team, keys=("z", "dp"))
    for k in ("z", "g", "dp", "dobj", "drel", "state"):
        x = team[k].cpu().numpy()
        assert np.isfinite(x).all() and not (x.view(np.uint32) == 0xFFFFFFFF).any(), k
    assert float(team["g"].abs().max()) > 0


@pytest.mark.parametrize("name,kind", [("star_in", "tile32"), ("mixed", "default")])
def test_stored_steps_do_not_change_the_gradients(name, kind):
    """spwgnn_da_stored_steps K = 0 against K = 2 on the wide kernels (star_in's 24-node tiles rebuild no dA, so K
    must not matter at all; mixed's S = 3 reads two stored steps back)."""
    c = T.case(name)
    with E.wide_kernels():
        batch = _batch(c, kind)
        with E.da_stored(2):
            k2 = _run(c, batch, "x6")
        with E.da_stored(0):
            k0 = _run(c, batch, "x6")
    TG._bits_equal(f"{name}: K = 0 against K = 2", k0, k2, keys=("z", "g", "dp", "dobj", "drel"))
    assert float(k2["g"].abs().max()) > 0


# ------------------------------------------------------------------------------------ 5. plans built on the device
@pytest.mark.parametrize("name", ["mixed", "star32"])
def test_device_built_plan(name):
    """`from_dense_device` on Rs / Rr whose columns are the case's edges in order: the arrays of the host capacity
    plan, and one forward and backward bitwise the host plan's."""
    c = T.case(name)
    Rs, Rr = T.dense_relations(c)
    dev = TowerBatch.from_dense_device(*(torch.as_tensor(np.asarray(a, np.float32), device=DEV)
                                         for a in (c["obj"], Rs, Rr, c["prop"])), check=True)
    host = _batch(c, "capacity")
    assert (dev.n_wtiles, dev.n_eblocks, dev.nw_max) == (host.n_wtiles, host.n_eblocks, host.nw_max)
    for k in ("edge_src", "edge_dst", "blk_csr", "wtile"):
        assert torch.equal(getattr(dev, k), getattr(host, k)), k
    assert np.array_equal(dev.src, c["src"]) and np.array_equal(dev.dst, c["dst"])
    assert np.array_equal(dev.tower_edges, c["te"]) and np.array_equal(dev.edge_id, host.edge_id)
    a, b = _run(c, dev, "x6", state=True), _run(c, host, "x6", state=True)
    TG._bits_equal(f"{name}: device-built against host plan", a, b)
    _check(f"{name}/device capacity plan x6", c, dev, a, T.reference(name))


# ------------------------------------------------------------------------------------ 6. x3 and bf16
@pytest.mark.parametrize("wide", [False, True], ids=["team", "wide"])
def test_lower_precision_maths(wide):
    c = T.case("mixed")
    ref = T.reference("mixed")
    rel = lambda got, want: float(np.linalg.norm(got - want) / np.linalg.norm(want))
    d = {}
    with _limit(wide):
        batch = _batch(c, "default")
        for math in ("x3", "bf16"):
            res = _run(c, batch, math)
            pad = (batch.edge_src < 0) | (batch.edge_dst < 0)
            assert bool((res["drel"][pad] == 0).all())
            _, _, vals = batch.edges_to_input(TG._np(res["drel"]))
            k = np.asarray(P.from_flat(res["g"])["rmp.1.kernel"], np.float64)
            d[math] = dict(z=float(np.abs(TG._np(res["z"]) - ref["z"]).max()), dobj=rel(TG._np(res["dobj"]), ref["dobj"]),
                           drel=rel(vals, ref["dgate"]), w2=rel(k, ref["g"]["rmp.1.kernel"]))
            print(f"TOPOLOGY mixed/{'wide' if wide else 'team'} {math}: max|dz| {d[math]['z']:.2e}, relative L2 error "
                  f"dobj {d[math]['dobj']:.2e}, dgate {d[math]['drel']:.2e}, rmp.1.kernel {d[math]['w2']:.2e}")
    for math in ("x3", "bf16"):
        assert d[math]["drel"] <= 2 * d[math]["w2"], (math, d[math])
    assert 32 * d["x3"]["z"] <= d["bf16"]["z"], d
    assert 32 * d["x3"]["dobj"] <= d["bf16"]["dobj"], d


# ------------------------------------------------------------------------------------ 7. DropEdge
KEY, RATE = 0x1234ABCD5, 0.5


def test_dropedge_on_a_directed_list():
    """The mask equals the NumPy restatement slot for slot; a repeated pair's slots share one decision; with
    SYMMETRIC a one-way edge takes the decision of its (min, max) key."""
    c = T.case("mixed")
    batch = _batch(c, "default")
    run = E.RunConfig(c["S"], training=True, seed=KEY)
    pad = ((batch.edge_src < 0) | (batch.edge_dst < 0)).cpu().numpy()
    pairs = list(zip(c["src"].tolist(), c["dst"].tolist()))
    got = {}
    for sym in (False, True):
        g = E.dropedge_gates(batch, run, RATE, symmetric=sym).cpu().numpy()
        want = DREF.batch_gates(batch, KEY, RATE, sym)
        assert np.array_equal(g.view(np.int32), want.view(np.int32)), sym
        assert np.all(g[pad].view(np.int32) == 0) and set(np.unique(g[~pad])) == {np.float32(0), np.float32(1)}
        _, _, got[sym] = batch.edges_to_input(g)   # per edge, the case's order
        for j, p in enumerate(pairs):               # a repeated pair: one decision
            assert got[sym][j] == got[sym][pairs.index(p)]
    one_way = [j for j, (s, d) in enumerate(pairs) if s != d and (d, s) not in pairs]
    both = [j for j, (s, d) in enumerate(pairs) if s != d and (d, s) in pairs]
    assert one_way and both
    for j in one_way + both:
        s, d = pairs[j]
        tower, a, b = s // 6, s % 6, d % 6
        assert got[True][j] == float(E.dropedge_keep_host(KEY, tower, min(a, b), max(a, b), RATE, symmetric=False))
        assert got[False][j] == float(E.dropedge_keep_host(KEY, tower, a, b, RATE, symmetric=False))
    for j in both:                                  # both directions of a contact share the symmetric draw
        assert got[True][j] == got[True][pairs.index((pairs[j][1], pairs[j][0]))]
    # the masked run is the run of the list without the dropped edges, to the criterion (gate 0 is deletion)
    res = _run(c, batch, "x6", gates=torch.as_tensor(DREF.batch_gates(batch, KEY, RATE, False), device=DEV))
    kept = got[False] != 0
    tw = np.repeat(np.arange(c["B"]), c["te"])
    cut = dict(c, src=c["src"][kept], dst=c["dst"][kept], te=np.bincount(tw[kept], minlength=c["B"]).astype(np.int32))
    z_ref = TG.GR.oracle(cut, T.ones(cut), "bce")["z"]
    assert T.logit_excess(TG._np(res["z"]), z_ref) <= 1.0
