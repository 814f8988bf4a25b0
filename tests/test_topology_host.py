"""CPU: relation sets outside the symmetric family (tests/topology_ref.py) — directed, uneven-degree,
reordered edge lists with repeated pairs and a→a — through the host planners, the dense conversion and the fp64
oracle; `edges_to_input(dense=True)` on a repeated pair; spwgnn_plan_order's guarantee (ADVICE.md's counterexample).

The plans are checked against a NumPy restatement written here (`_check_plan`), not against the library's own
arrays: every input edge in exactly one slot with its edge_id, padding −1, both halves of blk_csr the stable sort of
the block's local receiver / sender keys with 255 after the valid entries.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import relation_gates_ref as GR
import topology_ref as T
from oracle import model as O
from spwgnn_amd import _lib
from spwgnn_amd.batch import HostPlan, TowerBatch, pack_order

KINDS = ["nw16", "nw32", "capacity", "packed", "recv"]


# ------------------------------------------------------------------------------------ the cases themselves
@pytest.mark.parametrize("name", T.NAMES)
def test_case_margins_and_seed(name):
    """Every tower's ReLU margin exceeds TAU (no tower left out), the committed seed is the one `pick_seed` returns,
    and the case has the property its row of the table promises."""
    c = T.case(name)
    m = T.margins(c)
    print(f"{name}: seed {c['seed']}, ReLU margins per tower min {m.min():.2e} (TAU {T.TAU:g})")
    assert m.shape == (c["B"],) and np.all(m > T.TAU)
    assert T.pick_seed(name)[0] == T.SEEDS[name]
    nn = int(c["sizes"].sum())
    indeg, outdeg = np.bincount(c["dst"], minlength=nn), np.bincount(c["src"], minlength=nn)
    pairs = list(zip(c["src"].tolist(), c["dst"].tolist()))
    repeats, loops = len(pairs) - len(set(pairs)), int((c["src"] == c["dst"]).sum())
    assert not np.array_equal(indeg, outdeg)                                 # in-degree != out-degree somewhere
    assert set(pairs) != {(d, s) for s, d in pairs}                          # the edge set is not symmetric
    want = {"chain": (1, 0, 0), "star_in": (23, 0, 0), "star_out": (1, 0, 0), "star32": (32, 1, 0), "hubs": (16, 0, 0),
            "dag": (11, 0, 0), "mixed": (None, 2, 1), "ragged_mixed": (None, 1, 1)}[name]
    assert (repeats, loops) == want[1:] and (want[0] is None or indeg.max() == want[0])
    if name in ("chain", "star_out", "dag"):
        assert (indeg == 0).any()
    if name in ("chain", "star_in", "dag"):
        assert (outdeg == 0).any()
    if name == "dag":
        assert sorted(indeg.tolist()) == list(range(12))
    if name == "hubs":
        assert np.array_equal(indeg[:4], [16] * 4)


@pytest.mark.parametrize("name", ["mixed", "star_in"])
def test_gated_margins(name):
    c, g = T.case(name), T.gates(name)
    assert list(g[:3]) == [0.0, 1.0, -0.5] and len(g) == len(c["src"])
    assert np.all(GR.gated_margins(c, g, c["sizes"]) > T.TAU)


# ------------------------------------------------------------------------------------ plans
def _plan(c, kind):
    """The host plan of `kind`, or None where the case does not fit it."""
    nn = int(c["sizes"].sum())
    args = (c["obj"].reshape(nn, 3), c["sizes"], c["src"].astype(np.int32), c["dst"].astype(np.int32), c["te"],
            c["prop"].reshape(nn, 100))
    full = (c["sizes"].astype(np.int64) * (c["sizes"] - 1)).astype(np.int32)
    if kind == "nw16":
        return HostPlan.build(*args, nw_max=16, recv_blocks=False) if c["sizes"].max() <= 16 else None
    if kind == "nw32":
        return HostPlan.build(*args, nw_max=32, recv_blocks=False)
    if kind == "capacity":
        return HostPlan.build(*args, edge_cap=full) if np.all(c["te"] <= full) else None
    if kind == "packed":
        return HostPlan.build(*args, pack=True, recv_blocks=False)
    return HostPlan.build(*args, recv_blocks=True)


def _check_plan(c, plan, kind):
    """The NumPy restatement. Returns the number of edge slots checked."""
    pos4, node_tower, node_local, wtile, esrc, edst, csr = plan.arrays[:7]
    eid = np.asarray(plan.edge_id)
    ne, nn = len(c["src"]), int(c["sizes"].sum())
    assert esrc.shape == edst.shape == eid.shape == (32 * plan.n_eblocks,) and csr.shape == (plan.n_eblocks, 128)
    # every input edge in exactly one slot, with its edge_id; padding is −1 in all three arrays
    valid = eid >= 0
    assert np.array_equal(np.sort(eid[valid]), np.arange(ne))
    assert np.all(esrc[~valid] == -1) and np.all(edst[~valid] == -1) and np.all(eid[~valid] == -1)
    assert np.all(esrc[valid] >= 0) and np.all(edst[valid] >= 0)
    # the plan's own edge list is the case's (through node_perm for a packed plan, towers moved as wholes)
    perm = np.arange(nn) if plan.node_perm is None else np.asarray(plan.node_perm)
    assert np.array_equal(np.sort(perm), np.arange(nn))
    ps, pd = perm[np.asarray(plan.src, np.int64)], perm[np.asarray(plan.dst, np.int64)]
    if plan.node_perm is None:
        assert np.array_equal(ps, c["src"]) and np.array_equal(pd, c["dst"])
    else:
        assert np.array_equal(pos4[:, :3], c["obj"].reshape(nn, 3)[perm])
    assert sorted(zip(ps.tolist(), pd.tolist())) == sorted(zip(c["src"].tolist(), c["dst"].tolist()))
    assert np.array_equal(perm[esrc[valid]], ps[eid[valid]]) and np.array_equal(perm[edst[valid]], pd[eid[valid]])
    # a repeated pair sits in as many slots as the list names it
    slot_pairs = list(zip(perm[esrc[valid]].tolist(), perm[edst[valid]].tolist()))
    for pair in set(slot_pairs):
        assert slot_pairs.count(pair) == list(zip(c["src"].tolist(), c["dst"].tolist())).count(pair)
    # tiles: whole towers, every node once, every block once
    cover, bcover = np.zeros(nn, int), np.zeros(plan.n_eblocks, int)
    for b0, nb, n0, nw in wtile:
        cover[n0:n0 + nw] += 1
        bcover[b0:b0 + nb] += 1
        assert 1 <= nw <= plan.nw_max and node_local[n0] == 0 and (n0 + nw == nn or node_local[n0 + nw] == 0)
        if kind == "recv":
            assert nb == nw
        for blk in range(b0, b0 + nb):
            s, d = esrc[32 * blk:32 * blk + 32].astype(np.int64), edst[32 * blk:32 * blk + 32].astype(np.int64)
            v = s >= 0
            nv = int(v.sum())
            assert np.all(v[:nv]) and not np.any(v[nv:])              # padding only at the block's end
            assert np.all((s[v] >= n0) & (s[v] < n0 + nw) & (d[v] >= n0) & (d[v] < n0 + nw))
            assert np.array_equal(node_tower[s[v]], node_tower[d[v]])  # an edge stays inside its tower
            if kind == "recv":                                        # block bb holds node n0 + bb's in-edges, in input order
                assert np.all(d[v] == n0 + (blk - b0)) and np.all(np.diff(eid[32 * blk:32 * blk + nv]) > 0)
            else:                                                     # the tile's edges in input order, slot after slot
                assert np.all(np.diff(eid[32 * blk:32 * blk + nv]) == 1)
            for base, glob in ((0, d), (64, s)):
                key = np.where(v, glob - n0, 255)
                order = np.argsort(key, kind="stable")
                assert np.array_equal(csr[blk, base:base + 32], order.astype(np.uint8)), (kind, blk, base)
                assert np.array_equal(csr[blk, base + 32:base + 64], key[order].astype(np.uint8)), (kind, blk, base)
                assert np.all(csr[blk, base + 32 + nv:base + 64] == 255)
    assert np.all(cover == 1) and np.all(bcover == 1)
    return int(valid.sum())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", T.NAMES)
def test_plans(name, kind):
    c = T.case(name)
    plan = _plan(c, kind)
    if plan is None:   # towers of more than 16 nodes have no nw_max 16 plan; every other kind fits every case
        assert kind == "nw16" and c["sizes"].max() > 16
        with pytest.raises(_lib.SpwgnnError, match="status -2"):
            HostPlan.build(c["obj"].reshape(-1, 3), c["sizes"], c["src"], c["dst"], c["te"], nw_max=16, recv_blocks=False)
        return
    assert bool(plan.flags & _lib.BATCH_RECV_BLOCKS) == (kind == "recv")
    assert _check_plan(c, plan, kind) == len(c["src"])
    if kind == "packed" and name == "ragged_mixed":
        assert plan.node_perm is not None and not np.array_equal(plan.node_perm, np.arange(plan.n_nodes))
    if kind == "recv":
        nn = int(c["sizes"].sum())
        empty = np.bincount(c["dst"], minlength=nn) == 0
        blocks = np.asarray(plan.edge_id).reshape(-1, 32)
        assert plan.n_eblocks == nn and np.array_equal((blocks < 0).all(axis=1), empty)   # all-padding blocks


def test_plan_walk_runs():
    """What the cases promise the 17–32-node csr walk: receiver runs of 23 (star_in), four of 16 in one tile
    (hubs), a sender run of 23 (star_out), and on star32's receiver-block plan a run of 32 without a terminator."""
    def runs(plan, base):
        csr = plan.arrays[6]
        out = []
        for row in csr:
            keys = row[base + 32:base + 64]
            keys = keys[keys != 255]
            out.append(np.unique(keys, return_counts=True)[1].tolist() if len(keys) else [])
        return out
    r = runs(_plan(T.case("star_in"), "nw32"), 0)
    assert r[0] == [23] and max(map(max, runs(_plan(T.case("star_in"), "nw32"), 64))) == 1
    assert runs(_plan(T.case("star_out"), "nw32"), 64)[0] == [23]
    h = runs(_plan(T.case("hubs"), "nw32"), 0)
    assert h[0] == [16, 16] and h[1] == [16, 16]
    plan = _plan(T.case("star32"), "recv")
    csr = plan.arrays[6]
    assert np.all(csr[0, 32:64] == 0) and not np.any(csr[0] == 255) and np.all(csr[1:, 32:64] == 255)
    assert runs(_plan(T.case("star32"), "nw32"), 0) == [[32]]


def test_receiver_block_limit():
    """32 in-edges at one node fill its receiver block; a 33rd is SPWGNN_E_SHAPE, on every node and with a repeat."""
    c = T.case("star32")
    assert _plan(c, "recv").n_eblocks == 32
    for extra in ((6, 0), (0, 0)):
        src, dst = np.append(c["src"], extra[0]).astype(np.int32), np.append(c["dst"], extra[1]).astype(np.int32)
        with pytest.raises(_lib.SpwgnnError, match="status -2"):
            HostPlan.build(c["obj"].reshape(-1, 3), c["sizes"], src, dst, c["te"] + 1, recv_blocks=True)
        plain = HostPlan.build(c["obj"].reshape(-1, 3), c["sizes"], src, dst, c["te"] + 1, recv_blocks=False)
        assert plain.n_eblocks == 2   # the ordinary plan takes it


# ------------------------------------------------------------------------------------ dense round trip
@pytest.mark.parametrize("name", ["mixed", "star32"])
def test_dense_round_trip(name):
    """Rs / Rr with the columns in the case's edge order (a repeated pair is two columns, a→a a column whose sender
    row is its receiver row): the C conversion and the oracle's give the case's list back, and the literal dense
    graph computes what the edge list does."""
    c = T.case(name)
    Rs, Rr = T.dense_relations(c)
    B, N = c["B"], c["N"]
    src, dst = np.zeros(B * N * (N - 1), np.int32), np.zeros(B * N * (N - 1), np.int32)
    tec, n = np.zeros(B, np.int32), C.c_int64()
    st = _lib.lib().spwgnn_dense_to_edges(Rs.ctypes.data, Rr.ctypes.data, B, N, src.ctypes.data, dst.ctypes.data, None,
                                          len(src), C.byref(n), tec.ctypes.data)
    assert st == 0 and n.value == len(c["src"]) and np.array_equal(tec, c["te"])
    assert np.array_equal(src[:n.value], c["src"]) and np.array_equal(dst[:n.value], c["dst"])
    e = np.array(O.dense_to_edges(Rs, Rr), np.int64).reshape(-1, 4)
    assert np.array_equal(e[:, 0] * N + e[:, 2], c["src"]) and np.array_equal(e[:, 0] * N + e[:, 3], c["dst"])
    b = TowerBatch.from_dense(c["obj"], Rs, Rr, c["prop"], device="cpu")
    assert np.array_equal(b.src, c["src"]) and np.array_equal(b.dst, c["dst"])
    tp = O.to_torch(c["params"])
    f64 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    with torch.no_grad():
        zd = O.forward_dense(tp, f64(c["obj"]), f64(Rs), f64(Rr), f64(c["prop"]), c["S"]).reshape(-1)
        zg = O.forward_gather(tp, f64(c["obj"]).reshape(-1, 3), torch.as_tensor(c["src"]), torch.as_tensor(c["dst"]),
                              f64(c["prop"]).reshape(-1, 100), c["S"])
    assert float((zd - zg).abs().max()) <= 1e-12
    assert np.abs(zg.numpy() - T.reference(name)["z"]).max() <= 1e-12


# ------------------------------------------------------------------------------------ the cases are not vacuous
def _outputs(ref):
    out = {"z": ref["z"], "dprop": ref["dprop"], "dobj": ref["dobj"], "dgate": ref["dgate"]}
    out.update({"g:" + k: v for k, v in ref["g"].items()})
    return out


@pytest.mark.parametrize("name", T.NAMES)
def test_mutations_are_caught(name):
    """A kernel that read the senders as receivers, lost a repeated pair or the a→a edge, or returned per-edge values
    in sender-major order would leave at least one output more than 100× the GPU criterion away from the reference."""
    c = T.case(name)
    ref = _outputs(T.reference(name))
    muts = T.mutations(c)
    want = {"swapped"}
    if name in ("star32", "mixed", "ragged_mixed"):
        want.add("repeats_dropped")
    if name in ("mixed", "ragged_mixed"):
        want.add("self_loop_dropped")
    if name not in ("chain", "star_out", "star_in"):   # those lists are sender-major as they stand
        want.add("sender_major")
    assert set(muts) == want, (name, sorted(muts))
    for mname, (m, keep) in muts.items():
        got = _outputs(GR.oracle(m, T.ones(m), "bce"))
        excess = {}
        for k, r in ref.items():
            if k == "z":
                excess[k] = T.logit_excess(got[k], r)
            elif k == "dgate":   # per edge, entry by entry
                excess[k] = T.tensor_excess(got[k], r[keep])
            else:
                excess[k] = T.tensor_excess(got[k], r)
        worst = max(excess, key=excess.get)
        print(f"{name} / {mname}: largest excess {excess[worst]:.3g}× the criterion ({worst}); logits {excess['z']:.3g}×")
        assert excess[worst] > 100, (name, mname, excess)


# ------------------------------------------------------------------------------------ edges_to_input
def test_dense_edges_to_input_refuses_a_repeated_pair():
    c = T.case("mixed")
    b = TowerBatch.from_edges(c["obj"].reshape(-1, 3), c["sizes"], c["src"].astype(np.int32), c["dst"].astype(np.int32),
                              c["te"], device="cpu")
    vals = np.arange(32 * b.n_eblocks, dtype=np.float32)
    s, d, v = b.edges_to_input(vals)   # the 1-D form returns both entries of a repeated pair
    assert np.array_equal(s, c["src"]) and np.array_equal(d, c["dst"]) and len(np.unique(v)) == len(c["src"])
    key = c["src"] * 18 + c["dst"]
    rep = np.nonzero(np.bincount(key) > 1)[0][0]
    a, r = (rep // 18) % 6, (rep % 18) % 6
    with pytest.raises(ValueError, match=rf"relation {a} -> {r} of tower {rep // 18 // 6} appears 2 times"):
        b.edges_to_input(vals, dense=True)
    # without the repeats the dense form stands, the a→a value on the diagonal
    m, keep = T.mutations(c)["repeats_dropped"]
    b2 = TowerBatch.from_edges(m["obj"].reshape(-1, 3), m["sizes"], m["src"].astype(np.int32), m["dst"].astype(np.int32),
                               m["te"], device="cpu")
    dense = b2.edges_to_input(np.where(b2.edge_id >= 0, b2.edge_id + 1.0, 0.0), dense=True)
    assert dense.shape == (3, 6, 6)
    assert np.array_equal(dense[m["src"] // 6, m["src"] % 6, m["dst"] % 6], np.arange(len(m["src"])) + 1.0)
    assert np.count_nonzero(dense) == len(m["src"]) and np.count_nonzero(dense[:, np.arange(6), np.arange(6)]) == 1


# ------------------------------------------------------------------------------------ spwgnn_plan_order
def _blocks(tn, te, nw):
    sz = _lib.PlanSizes()
    tn, te = np.ascontiguousarray(tn, np.int32), np.ascontiguousarray(te, np.int32)
    _lib.check(_lib.lib().spwgnn_plan_size(len(tn), tn.ctypes.data, te.ctypes.data, nw, C.byref(sz)), "plan_size")
    return sz.n_eblocks


def test_plan_order_never_needs_more_blocks():
    """ADVICE.md's counterexample: nw_max 16, towers (8,30), (2,2), (8,32) plan in 2 blocks as given; towers by
    decreasing edge count — (8,32), (8,30), (2,2) — plan in 3, since the in-order packing puts the two 8-node towers
    in one tile. spwgnn_plan_order sizes both and returns the identity then."""
    tn, te = np.array([8, 2, 8], np.int32), np.array([30, 2, 32], np.int32)
    assert _blocks(tn, te, 16) == 2 and _blocks(tn[[2, 0, 1]], te[[2, 0, 1]], 16) == 3
    o = pack_order(tn, te, 16)
    assert np.array_equal(np.sort(o), np.arange(3))
    assert _blocks(tn[o], te[o], 16) <= 2
    assert np.array_equal(o, [0, 1, 2])
    # the same towers given in the greedy order: any order of 3 blocks or fewer will do, never more
    tn2, te2 = tn[[2, 0, 1]], te[[2, 0, 1]]
    o2 = pack_order(tn2, te2, 16)
    assert _blocks(tn2[o2], te2[o2], 16) <= 3
    # exhaustively over small batches: a permutation, and never more blocks than the given order
    rng = np.random.default_rng(11)
    for _ in range(300):
        T_ = int(rng.integers(1, 7))
        tn = rng.integers(1, 17, T_).astype(np.int32)
        te = np.array([rng.integers(0, min(n * (n - 1), 40) + 1) for n in tn], np.int32)
        o = pack_order(tn, te, 16)
        assert np.array_equal(np.sort(o), np.arange(T_))
        assert _blocks(tn[o], te[o], 16) <= _blocks(tn, te, 16), (tn, te, o)
