"""GPU: batch plans filled on the device (k_plan_device; TowerBatch.from_positions / from_dense_device /
refill, GraphNetwork.forward_positions and plan="device").

The yardstick everywhere is the host planner: `HostPlan.build(..., edge_cap=cap)` on the edge list the
host enumerates from the same towers (the float64 distance test of `data.relation_matrices` /
`TowerBatch.ragged`, or spwgnn_dense_to_edges on the same matrices). Its arrays are compared bitwise
with what the kernel wrote; nothing is compared against a second run of the new code, except where a
test is about exactly that (a captured replay against the eager call)."""
import ctypes as C

import numpy as np
import pytest
import torch

from spwgnn_amd import GraphNetwork, TowerBatch, _lib, data as D, engine as E
from spwgnn_amd.batch import HostPlan

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 4096          # sentinel bytes on each side of a guarded output array
SENTINEL = 0xA5


# ------------------------------------------------------------------------------------ the yardstick
def _enumerate(raw_list, thr):
    """Tower-major, sender-major edges with global node ids; thresholded like main.py:71-81."""
    srcs, dsts, tes, off = [], [], [], 0
    for r in raw_list:
        n = len(r)
        m, j = np.nonzero(~np.eye(n, dtype=bool))
        if thr is not None:
            keep = np.linalg.norm(r[m, 0:2] - r[j, 0:2], axis=1) < thr
            m, j = m[keep], j[keep]
        srcs.append(off + m)
        dsts.append(off + j)
        tes.append(len(m))
        off += n
    return (np.concatenate(srcs).astype(np.int32), np.concatenate(dsts).astype(np.int32), np.array(tes, np.int32))


def _host_plan(raw_list, thr, nw_max, cap=None, ids=None) -> HostPlan:
    tn = np.array([len(r) for r in raw_list], np.int32)
    src, dst, te = _enumerate(raw_list, thr)
    pos = np.concatenate(raw_list)[:, :3] / 170          # float64 division, cast by the planner (main.py:91)
    return HostPlan.build(pos, tn, src, dst, te, nw_max=nw_max, edge_cap=tn * (tn - 1) if cap is None else cap,
                          tower_ids=ids)


def _dense_host_plan(obj, Rs, Rr, nw_max) -> HostPlan:
    """spwgnn_dense_to_edges on the host matrices, then the capacity plan of N(N−1) slots per tower."""
    B, N = obj.shape[:2]
    Ecap = B * N * (N - 1)
    src, dst, tec = np.zeros(max(Ecap, 1), np.int32), np.zeros(max(Ecap, 1), np.int32), np.zeros(B, np.int32)
    ne = C.c_int64(0)
    Rs, Rr = np.ascontiguousarray(Rs, np.float32), np.ascontiguousarray(Rr, np.float32)
    _lib.check(_lib.lib().spwgnn_dense_to_edges(Rs.ctypes.data, Rr.ctypes.data, B, N, src.ctypes.data, dst.ctypes.data,
                                                None, Ecap, C.byref(ne), tec.ctypes.data), "dense_to_edges")
    n = int(ne.value)
    return HostPlan.build(obj.reshape(B * N, 3), np.full(B, N, np.int32), src[:n], dst[:n], tec, nw_max=nw_max,
                          edge_cap=N * (N - 1))


def _same_bits(a: torch.Tensor, b: np.ndarray) -> bool:
    a = a.detach().cpu().contiguous().numpy()
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == np.ascontiguousarray(b).tobytes()


def _assert_arrays(batch, hp: HostPlan, pos=True):
    assert (batch.n_towers, batch.n_nodes, batch.n_wtiles, batch.n_eblocks, batch.nw_max) == \
        (hp.n_towers, hp.n_nodes, hp.n_wtiles, hp.n_eblocks, hp.nw_max)
    assert int(batch.status.item()) == 0
    assert _same_bits(batch.wtile, hp.arrays[3]) and _same_bits(batch.node_tower, hp.arrays[1])
    assert _same_bits(batch.node_local, hp.arrays[2])
    assert _same_bits(batch.edge_src, hp.arrays[4]), "edge_src"
    assert _same_bits(batch.edge_dst, hp.arrays[5]), "edge_dst"
    assert _same_bits(batch.blk_csr, hp.arrays[6]), "blk_csr"
    assert _same_bits(batch.tower_edges_dev, hp.tower_edges), "tower_edges"
    if pos:
        assert _same_bits(batch.pos, hp.arrays[0]), "pos"
    # the lazily fetched host fields are the host planner's too
    assert np.array_equal(batch.src, hp.src) and np.array_equal(batch.dst, hp.dst)
    assert np.array_equal(batch.edge_id, hp.edge_id) and batch.n_edges == len(hp.src)


# name → (raw (B, N, 3) float64, nw_max); the towers every test shares
_UNIFORM = {"n6": (6, 5, 0, 16), "n3": (3, 64, 1, 16), "n1": (1, 7, 0, None), "n32": (32, 3, 0, None),
            "n17": (17, 2, 0, None)}
_RAW = {}


def _raw(name):
    if name not in _RAW:
        n, b, seed, nw = _UNIFORM[name]
        raw = D.synthetic_towers(b, n, seed=seed)
        assert np.array_equal(raw, raw.astype(np.float32))   # fp32-exact pixels: the device sees the same numbers
        _RAW[name] = (raw, nw)
    return _RAW[name]


def _ragged():
    if "ragged" not in _RAW:
        sizes = np.random.default_rng(3).integers(4, 17, 40)
        _RAW["ragged"] = [D.synthetic_towers(1, int(n), seed=100 + k)[0] for k, n in enumerate(sizes)]
    return _RAW["ragged"]


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


# ------------------------------------------------------------------------------------ 1. positions
@pytest.mark.parametrize("name,thr", [("n6", None), ("n6", 170.0), ("n3", 170.0), ("n1", 170.0), ("n1", None),
                                      ("n32", None), ("n32", 170.0), ("n17", 170.0)])
def test_arrays_from_positions(name, thr):
    raw, nw = _raw(name)
    hp = _host_plan(list(raw), thr, nw)
    if name == "n3":
        assert int((hp.tower_edges == 0).sum()) >= 20       # many towers without a relation: all-padding tiles
    if name == "n6":
        assert hp.n_wtiles == 3 and hp.arrays[3][2, 3] == 6  # two towers per tile, the last tile half-filled
    batch = TowerBatch.from_positions(_t(raw), thr, nw_max=nw)
    _assert_arrays(batch, hp)
    assert batch.node_shape == raw.shape[:2]


def test_thresholds_that_mean_fully_connected():
    raw, nw = _raw("n6")
    hp = _host_plan(list(raw), None, nw)
    for thr in (0.0, -1.0, float("nan")):
        _assert_arrays(TowerBatch.from_positions(_t(raw), thr, nw_max=nw), hp)


def test_arrays_from_ragged_positions_with_tower_ids():
    rl = _ragged()
    ids = np.random.default_rng(9).permutation(500)[:len(rl)]
    hp = _host_plan(rl, 170.0, 16, ids=ids)
    tn = np.array([len(r) for r in rl], np.int32)
    batch = TowerBatch.from_positions(_t(np.concatenate(rl)), 170.0, tower_nodes=tn, nw_max=16, tower_ids=ids)
    _assert_arrays(batch, hp)
    assert batch.node_shape is None


def test_edge_cap_below_every_slot():
    """A capacity below N(N−1) but above every tower's count: fewer blocks, the same edges."""
    rl = _ragged()
    tn = np.array([len(r) for r in rl], np.int32)
    te = _enumerate(rl, 170.0)[2]
    cap = np.maximum(te + (np.arange(len(te)) % 3), 1).astype(np.int32)    # tight: 0..2 spare slots per tower
    assert np.any(cap < tn * (tn - 1)) and np.any(cap == te)
    hp = _host_plan(rl, 170.0, 16, cap=cap)
    assert hp.n_eblocks < _host_plan(rl, 170.0, 16).n_eblocks
    batch = TowerBatch.from_positions(_t(np.concatenate(rl)), 170.0, tower_nodes=tn, nw_max=16, edge_cap=cap, check=True)
    _assert_arrays(batch, hp)


# ------------------------------------------------------------------------------------ 2. dense relations
@pytest.mark.parametrize("name,thr", [("n6", None), ("n6", 170.0), ("n3", 170.0), ("n1", 170.0), ("n32", None),
                                      ("n32", 170.0), ("n17", 170.0)])
def test_arrays_from_dense_relations(name, thr):
    raw, nw = _raw(name)
    Rs, Rr = D.relation_matrices(raw, thr)
    obj = (raw / 170).astype(np.float32)
    hp = _dense_host_plan(obj, Rs, Rr, nw)
    batch = TowerBatch.from_dense_device(_t(obj), _t(Rs), _t(Rr), nw_max=nw)
    _assert_arrays(batch, hp)


def test_dense_columns_permuted_per_tower():
    """The sender is the row holding the 1, not the slot's sender-major node."""
    raw, nw = _raw("n6")
    Rs, Rr = D.relation_matrices(raw, 170.0)
    rng = np.random.default_rng(2)
    for b in range(len(raw)):
        perm = rng.permutation(Rs.shape[2])
        Rs[b], Rr[b] = Rs[b][:, perm], Rr[b][:, perm]
    obj = (raw / 170).astype(np.float32)
    hp = _dense_host_plan(obj, Rs, Rr, nw)
    assert np.any(np.diff(hp.src) < 0)                     # not sender-major any more
    _assert_arrays(TowerBatch.from_dense_device(_t(obj), _t(Rs), _t(Rr), nw_max=nw), hp)


# ------------------------------------------------------------------------------------ 3. errors without damage
def _guard(batch):
    """Move the batch's own output arrays into the middle of sentinel-filled buffers."""
    bufs = {}
    for name in ("edge_src", "edge_dst", "blk_csr", "pos", "tower_edges_dev"):
        t = getattr(batch, name)
        nbytes = t.numel() * t.element_size()
        big = torch.full((nbytes + 2 * PAD,), SENTINEL, dtype=torch.uint8, device=DEV)
        setattr(batch, name, big[PAD:PAD + nbytes].view(t.dtype).view(t.shape))
        bufs[name] = big
    batch._cstruct = None
    return bufs


def _assert_intact(bufs):
    for name, big in bufs.items():
        assert bool((big[:PAD] == SENTINEL).all()) and bool((big[-PAD:] == SENTINEL).all()), name


def _bad_matrices(kind):
    raw, nw = _raw("n6")
    Rs, Rr = D.relation_matrices(raw, None)
    if kind == "half":
        Rs[1, 2, 7] = 0.5
    elif kind == "two_ones":
        Rr[3, :2, 11] = 1.0
        assert Rr[3, :, 11].sum() == 2
    else:   # a receiver without a sender
        Rs[4, :, 29] = 0.0
    return raw, nw, Rs, Rr


@pytest.mark.parametrize("kind", ["half", "two_ones", "no_sender"])
def test_relation_errors_leave_memory_intact(kind):
    raw, nw, Rs, Rr = _bad_matrices(kind)
    obj = _t((raw / 170).astype(np.float32))
    with pytest.raises(_lib.SpwgnnError):     # the host conversion refuses the same matrices
        _dense_host_plan((raw / 170).astype(np.float32), Rs, Rr, nw)
    good = D.relation_matrices(raw, None)
    batch = TowerBatch.from_dense_device(obj, _t(good[0]), _t(good[1]), nw_max=nw, check=True)
    bufs = _guard(batch)
    batch.refill((_t(Rs), _t(Rr)))            # check=False: no error here, the status stays on the device
    torch.cuda.synchronize()
    assert int(batch.status.item()) == -_lib.E_RELATION
    _assert_intact(bufs)
    with pytest.raises(_lib.SpwgnnError, match="one-hot"):
        batch.check()
    with pytest.raises(_lib.SpwgnnError, match="one-hot"):
        batch.n_edges
    with pytest.raises(_lib.SpwgnnError, match="one-hot"):
        TowerBatch.from_dense_device(obj, _t(Rs), _t(Rr), nw_max=nw, check=True)
    batch.refill((_t(good[0]), _t(good[1])), check=True)      # and the batch is usable again
    _assert_arrays(batch, _dense_host_plan((raw / 170).astype(np.float32), good[0], good[1], nw), pos=False)
    _assert_intact(bufs)


def test_capacity_overflow_leaves_memory_intact():
    raw, nw = _raw("n6")
    te = _enumerate(list(raw), 170.0)[2]
    cap = int(te.max()) - 2                   # at least one tower holds more relations than this
    x = _t(raw)
    fits = _t(raw * np.array([4.0, 4.0, 1.0]))   # the same towers spread out: fewer relations under the threshold
    te_fit = _enumerate(list(raw * np.array([4.0, 4.0, 1.0])), 170.0)[2]
    assert te_fit.max() <= cap
    batch = TowerBatch.from_positions(fits, 170.0, nw_max=nw, edge_cap=cap, check=True)
    bufs = _guard(batch)
    batch.refill(x)
    torch.cuda.synchronize()
    assert int(batch.status.item()) == -_lib.E_CAPACITY
    _assert_intact(bufs)
    # no tower was written beyond its capacity, and the count reports what the positions hold
    es = batch.edge_src.cpu().numpy()
    per_tower = np.bincount(es[es >= 0] // 6, minlength=len(raw))
    assert per_tower.max() <= cap and np.array_equal(batch.tower_edges_dev.cpu().numpy(), te)
    with pytest.raises(_lib.SpwgnnError, match="capacity"):
        batch.check()
    with pytest.raises(_lib.SpwgnnError, match="capacity"):
        TowerBatch.from_positions(x, 170.0, nw_max=nw, edge_cap=cap, check=True)


# ------------------------------------------------------------------------------------ 4. end to end
_E2E = {}


def _e2e_inputs():
    if not _E2E:
        raw = D.synthetic_towers(40, 6, seed=7)
        src, dst, te = _enumerate(list(raw), 170.0)
        _E2E.update(raw=raw, src=src, dst=dst, te=te,
                    prop=np.random.default_rng(1).normal(0, 0.3, (240, 100)).astype(np.float32),
                    dz=np.random.default_rng(2).normal(0, 1, 240).astype(np.float32))
    return _E2E


@pytest.mark.parametrize("math", ["x6", "bf16"])
def test_forward_and_backward_equal_the_host_capacity_plan(math):
    c = _e2e_inputs()
    net = GraphNetwork(seed=3, device=DEV, math=math)
    run = E.RunConfig(net.mp_steps, training=True, dropout=0.1, seed=11, math=math)
    prop, dz = _t(c["prop"]), _t(c["dz"])
    host = TowerBatch.from_edges(c["raw"].reshape(-1, 3) / 170, np.full(40, 6, np.int32), c["src"], c["dst"], c["te"],
                                 c["prop"], DEV, nw_max=16, edge_cap=30)
    dev = TowerBatch.from_positions(_t(c["raw"]), 170.0, nw_max=16, propagation=prop)
    out = []
    for b in (host, dev):
        ws = E.Workspace(DEV)
        z = E.forward(net.flat.detach(), b, run, ws)
        grads, dprop = E.backward(net.flat.detach(), b, run, ws, dz, want_dprop=True)
        dobj = E.backward_inputs(net.flat.detach(), b, run, ws)
        out.append([t.cpu().numpy().copy() for t in (z, grads, dprop, dobj)])
    for name, a, b in zip(("logits", "weight gradients", "d/d propagation", "d/d objects"), *out):
        assert np.isfinite(a).all() and np.abs(a).max() > 0, name
        assert a.tobytes() == b.tobytes(), name
    # all 22 tensors of the flat gradient buffer were compared
    assert len(_lib.param_tensors()) == 22 and out[0][1].size == _lib.lib().spwgnn_param_count()


def test_forward_positions_gradient_is_dobjects_over_divisor():
    c = _e2e_inputs()
    net = GraphNetwork(seed=3, device=DEV)
    net.eval()                                  # no dropout: the two calls below run the same graph
    raw = _t(c["raw"]).requires_grad_(True)
    z = net.forward_positions(raw, 170.0, nw_max=16)
    assert z.shape == (40, 6)
    (z * _t(c["dz"]).reshape(40, 6)).sum().backward()
    obj = (_t(c["raw"]) / 170.0).requires_grad_(True)
    batch = TowerBatch.from_positions(_t(c["raw"]), 170.0, nw_max=16)
    z2 = net.forward_batch(batch, None, obj)
    (z2 * _t(c["dz"])).sum().backward()
    assert torch.equal(z.reshape(-1), z2)
    assert float(obj.grad.abs().max()) > 0
    assert torch.equal(raw.grad, obj.grad / 170.0)
    # and the relation set is the thresholded one: the host plan's logits, bit for bit
    host = TowerBatch.from_edges(c["raw"].reshape(-1, 3) / 170, np.full(40, 6, np.int32), c["src"], c["dst"], c["te"],
                                 None, DEV, nw_max=16, edge_cap=30)
    with torch.no_grad():
        assert torch.equal(net.forward_batch(host), net.forward_batch(batch))


@pytest.mark.parametrize("math", ["f32", "x6"])
def test_plan_device_equals_plan_host(math):
    c = _e2e_inputs()
    Rs, Rr = D.relation_matrices(c["raw"], 170.0)
    obj = (c["raw"] / 170).astype(np.float32)
    net = GraphNetwork(seed=3, device=DEV, math=math)
    net.eval()
    with torch.no_grad():
        zh = net.forward_logits(obj, Rs, Rr)
        zd = net.forward_logits(_t(obj), _t(Rs), _t(Rr), plan="device")
        ph = net.forward(_t(obj), _t(Rs), _t(Rr), plan="host")
        pd = net.forward(_t(obj), _t(Rs), _t(Rr), plan="device")
        qh = net.forward_pooled(obj, Rs, Rr, mode="sum_prob")
        qd = net.forward_pooled(_t(obj), _t(Rs), _t(Rr), mode="sum_prob", plan="device")
    diff = float((zh - zd).abs().max())
    print(f"{math}: max |plan=device − plan=host| logits {diff:.3e}")
    assert zd.shape == (40, 6) and pd.shape == (40, 6, 1) and qd.shape == (40,)
    if math == "f32":
        assert torch.equal(zh, zd) and torch.equal(ph, pd)
    else:   # the position-independence bound of the x6 receiver sums (DESIGN.md §3 "Determinism")
        assert diff <= 2e-6
        assert float((ph - pd).abs().max()) <= 2e-6
    assert float((qh - qd).abs().max()) <= 6 * 2e-6
    with pytest.raises(_lib.SpwgnnError, match="device"):
        net.forward_logits(obj, Rs, Rr, plan="device")       # host arrays: no quiet copy to the device
    with pytest.raises(ValueError):
        net.forward_logits(obj, Rs, Rr, plan="gpu")


# ------------------------------------------------------------------------------------ 5. capture
def test_refill_and_forward_replay_in_one_graph():
    net = GraphNetwork(seed=4, device=DEV)
    flat = net.flat.detach()
    run = net.run_config()
    sets = [D.synthetic_towers(12, 6, seed=s) for s in (21, 22, 23)]
    assert len({_enumerate(list(r), 170.0)[2].tobytes() for r in sets}) == 3      # three different relation sets
    static = _t(D.synthetic_towers(12, 6, seed=20))
    batch = TowerBatch.from_positions(static, 170.0, nw_max=16)
    ws = E.Workspace(DEV)
    out = torch.empty(batch.n_nodes, dtype=torch.float32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):               # warm-up: the workspace is allocated before the capture
        batch.refill(static)
        E.forward(flat, batch, run, ws, out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        batch.refill(static)
        E.forward(flat, batch, run, ws, out)
    for r in sets:
        static.copy_(_t(r))
        graph.replay()
        torch.cuda.synchronize()
        eager = E.forward(flat, TowerBatch.from_positions(_t(r), 170.0, nw_max=16), run, E.Workspace(DEV))
        assert torch.equal(out, eager)
        assert int(batch.status.item()) == 0
        batch.mark_refilled()                   # the replay refilled the arrays behind the object's back
        assert np.array_equal(batch.tower_edges, _enumerate(list(r), 170.0)[2])


def test_a_forward_stored_before_a_refill_is_refused():
    net = GraphNetwork(seed=4, device=DEV)
    flat = net.flat.detach()
    run = E.RunConfig(net.mp_steps, training=True, math="x6")
    raw = _t(D.synthetic_towers(12, 6, seed=21))
    batch = TowerBatch.from_positions(raw, 170.0, nw_max=16)
    ws = E.Workspace(DEV)
    z = E.forward(flat, batch, run, ws)
    assert ws.holds(batch, run)
    batch.refill(_t(D.synthetic_towers(12, 6, seed=22)))
    assert not ws.holds(batch, run)
    with pytest.raises(_lib.SpwgnnError, match="same batch"):
        E.backward(flat, batch, run, ws, torch.ones_like(z))
    z = E.forward(flat, batch, run, ws)          # a forward after the refill is good again
    E.backward(flat, batch, run, ws, torch.ones_like(z))


# ------------------------------------------------------------------------------------ 6. no sync
def test_from_positions_and_forward_do_not_synchronise():
    net = GraphNetwork(seed=4, device=DEV)
    net.eval()
    raw = _t(D.synthetic_towers(12, 6, seed=21))
    with torch.no_grad():
        net.forward_positions(raw, 170.0, nw_max=16)         # the geometry of this shape is cached now
        torch.cuda.synchronize()
        prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(RuntimeError):                # the mode is effective on this build
                raw.sum().item()
            batch = TowerBatch.from_positions(raw, 170.0, nw_max=16, check=False)
            z = net.forward_batch(batch)
            z2 = net.forward_positions(raw, 170.0, nw_max=16)
        finally:
            torch.cuda.set_sync_debug_mode(prev)
    assert torch.equal(z.reshape(12, 6), z2)
