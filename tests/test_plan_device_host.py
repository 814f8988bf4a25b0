"""CPU: the host side of the device-filled plans (spwgnn_plan_device_positions / _dense, added within
ABI 8) — the static geometry against the host planner run on real edges, the argument statuses that
come back before any device work, and the host fields of a device-built batch object. The arrays the
kernel writes are checked on the GPU (tests/test_gpu_plan_device.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from spwgnn_amd import _lib, batch as TB
from spwgnn_amd.batch import HostPlan, plan_geometry_host


def test_symbols_and_version():
    lib = _lib.lib()
    assert hasattr(lib, "spwgnn_plan_device_positions") and hasattr(lib, "spwgnn_plan_device_dense")
    assert lib.spwgnn_version() == 8 == _lib.ABI_VERSION
    assert _lib.K_PLAN_DEVICE == 13
    assert lib.spwgnn_struct_size(6) == C.sizeof(_lib.PlanDeviceC)
    assert b"capacity" in lib.spwgnn_strerror(_lib.E_CAPACITY)


def _random_edges(tn, cap, rng):
    """Per tower a random subset (≤ cap) of its N(N−1) sender-major slots, as global node ids."""
    srcs, dsts, tes, off = [], [], [], 0
    for n, c in zip(tn, cap):
        m, j = np.nonzero(~np.eye(int(n), dtype=bool))
        keep = np.sort(rng.permutation(len(m))[:rng.integers(0, min(len(m), int(c)) + 1)])
        srcs.append(off + m[keep])
        dsts.append(off + j[keep])
        tes.append(len(keep))
        off += int(n)
    return (np.concatenate(srcs).astype(np.int32), np.concatenate(dsts).astype(np.int32), np.array(tes, np.int32))


GEOMETRIES = [(np.full(7, n, np.int32), nw, None) for n in (1, 3, 6) for nw in (16, 32)] + [
    (np.full(3, 17, np.int32), 32, None), (np.full(3, 32, np.int32), 32, None),
    (np.full(40, 1, np.int32), None, None),                                    # default nw_max: a tile per tower
    (np.random.default_rng(5).integers(4, 17, 40).astype(np.int32), 16, None),
    (np.random.default_rng(6).integers(4, 17, 40).astype(np.int32), 32, None),
    (np.random.default_rng(7).integers(4, 17, 40).astype(np.int32), 16, "half"),
    (np.full(9, 6, np.int32), 16, 20),
]


@pytest.mark.parametrize("case", range(len(GEOMETRIES)))
def test_geometry_equals_the_host_planner_on_real_edges(case):
    tn, nw_max, cap = GEOMETRIES[case]
    full = tn * (tn - 1)
    capv = full if cap is None else (np.maximum(full // 2, 1) if cap == "half" else np.full(len(tn), cap, np.int32))
    rng = np.random.default_rng(100 + case)
    src, dst, te = _random_edges(tn, capv, rng)
    ids = rng.permutation(1000)[:len(tn)] if case % 2 else None   # custom tower ids in every other case
    want = HostPlan.build(np.zeros((int(tn.sum()), 3), np.float32), tn, src, dst, te, nw_max=nw_max, edge_cap=capv,
                          tower_ids=ids)
    g = plan_geometry_host(tn, nw_max, None if cap is None else capv, ids)
    assert (g.n_towers, g.n_nodes, g.n_wtiles, g.n_eblocks, g.nw_max) == \
        (want.n_towers, want.n_nodes, want.n_wtiles, want.n_eblocks, want.nw_max)
    assert np.array_equal(g.node_tower, want.arrays[1]) and np.array_equal(g.node_local, want.arrays[2])
    assert np.array_equal(g.wtile, want.arrays[3])
    assert g.default_cap == (cap is None) and np.array_equal(g.tower_cap, capv)
    # the first tower of each wave-tile: the tower whose first node is the tile's first node
    starts = np.concatenate([[0], np.cumsum(tn)[:-1]])
    assert np.array_equal(starts[g.wtile_tower], g.wtile[:, 2])
    assert g.dev is None   # nothing was uploaded


def _plan(fake=0x1000):
    """A well-formed spwgnn_plan_device whose pointers are never followed."""
    p = _lib.PlanDeviceC()
    p.n_towers, p.n_nodes, p.n_wtiles, p.n_eblocks, p.nw_max = 4, 24, 2, 4, 16
    p.wtile = p.node_local = p.wtile_tower = p.edge_src = p.edge_dst = p.blk_csr = p.status = fake
    return p


def test_statuses_without_a_device():
    lib = _lib.lib()
    fake = 0x1000
    pos = lambda p, raw=fake, stride=3, thr=170.0, div=170.0: lib.spwgnn_plan_device_positions(
        C.byref(p) if p is not None else None, raw, stride, thr, div, None)
    dense = lambda p, Rs=fake, Rr=fake, B=4, N=6: lib.spwgnn_plan_device_dense(
        C.byref(p) if p is not None else None, Rs, Rr, B, N, None)
    for call in (pos, dense):
        assert call(None) == _lib.E_ARG
        for name in ("wtile", "node_local", "wtile_tower", "edge_src", "edge_dst", "blk_csr", "status"):
            p = _plan()
            setattr(p, name, None)
            assert call(p) == _lib.E_ARG, name                      # null pointer
            setattr(p, name, fake + 2)
            assert call(p) == _lib.E_ARG, name                      # misaligned pointer
        p = _plan()
        p.blk_csr = fake + 4                                        # rows are stored as 16-byte aligned words
        assert call(p) == _lib.E_ARG
        p = _plan()
        p.tower_cap = fake + 1
        assert call(p) == _lib.E_ARG
        for nw in (0, 33, 64):
            p = _plan()
            p.nw_max = nw
            assert call(p) == _lib.E_SHAPE, nw
        for name in ("n_towers", "n_nodes", "n_wtiles", "n_eblocks"):
            p = _plan()
            setattr(p, name, 0)
            assert call(p) == _lib.E_ARG, name
        p = _plan()
        p.n_wtiles = 5                                              # more wave-tiles than towers
        assert call(p) == _lib.E_SHAPE
        p = _plan()
        p.n_eblocks = 1                                             # fewer blocks than wave-tiles
        assert call(p) == _lib.E_SHAPE
        p = _plan()
        p.n_nodes = 33                                              # more nodes than the tiles can hold
        assert call(p) == _lib.E_SHAPE
    # positions
    assert pos(_plan(), raw=None) == _lib.E_ARG
    assert pos(_plan(), raw=fake + 2) == _lib.E_ARG
    assert pos(_plan(), stride=1) == _lib.E_ARG
    assert pos(_plan(), div=0.0) == _lib.E_ARG
    assert pos(_plan(), div=float("nan")) == _lib.E_ARG
    p = _plan()
    p.pos = fake + 8                                                # pos rows are 16-byte vectors
    assert pos(p) == _lib.E_ARG
    p.pos = fake
    assert pos(p, stride=2) == _lib.E_ARG                           # pos needs (x, y, w)
    # dense
    assert dense(_plan(), Rs=None) == _lib.E_ARG
    assert dense(_plan(), Rr=None) == _lib.E_ARG
    assert dense(_plan(), Rr=fake + 1) == _lib.E_ARG
    assert dense(_plan(), N=0) == _lib.E_ARG
    assert dense(_plan(), N=-3) == _lib.E_ARG
    assert dense(_plan(), B=0) == _lib.E_ARG
    assert dense(_plan(), N=17) == _lib.E_SHAPE                     # a tower larger than a wave-tile
    assert dense(_plan(), B=3) == _lib.E_SHAPE                      # B != n_towers
    assert dense(_plan(), N=5) == _lib.E_SHAPE                      # B·N != n_nodes
    p = _plan()
    p.pos = fake
    assert dense(p) == _lib.E_ARG                                   # the dense source writes no pos


def test_host_tensors_are_refused():
    """The device constructors have no host path: a CPU tensor is an error that says so."""
    raw = torch.zeros(2, 3, 3)
    with pytest.raises(_lib.SpwgnnError, match="device"):
        TB.TowerBatch.from_positions(raw)
    with pytest.raises(_lib.SpwgnnError, match="device"):
        TB.TowerBatch.from_dense_device(raw, torch.zeros(2, 3, 6), torch.zeros(2, 3, 6))
    with pytest.raises(_lib.SpwgnnError, match="device"):
        TB.TowerBatch.from_positions(np.zeros((2, 3, 3), np.float32))


class _FakeDeviceBatch(TB.DeviceTowerBatch):
    """A DeviceTowerBatch over host tensors: what the kernel would have left for two 3-box towers in
    one wave-tile (tower 0: relations 0→1, 2→1; tower 1: none), to exercise the host fields."""

    def __init__(self, status=0):
        self.n_towers, self.n_nodes, self.n_wtiles, self.n_eblocks, self.nw_max = 2, 6, 1, 1, 6
        self.tower_nodes = np.array([3, 3], np.int32)
        es = np.full(32, -1, np.int32)
        ed = np.full(32, -1, np.int32)
        es[:2], ed[:2] = (0, 2), (1, 1)
        self.edge_src, self.edge_dst = torch.from_numpy(es), torch.from_numpy(ed)
        self.tower_edges_dev = torch.tensor([2, 0], dtype=torch.int32)
        self.status = torch.tensor([status], dtype=torch.int32)
        self.device = torch.device("cpu")
        self.generation, self._host, self._cstruct, self.prop, self.source = 0, None, None, None, ("positions", 170.0, 170.0)


def test_host_fields_are_fetched_lazily():
    b = _FakeDeviceBatch()
    assert b._host is None                       # nothing fetched at construction
    assert "DeviceTowerBatch" in repr(b) and b._host is None
    assert b.n_edges == 2                        # not a TypeError on None: fetched on first access
    assert b._host is not None
    assert b.src.tolist() == [0, 2] and b.dst.tolist() == [1, 1]
    assert b.tower_edges.tolist() == [2, 0]
    eid = b.edge_id
    assert eid.shape == (32,) and eid[:2].tolist() == [0, 1] and np.all(eid[2:] == -1)
    assert b.tower_offsets.tolist() == [0, 3, 6]
    # a refill invalidates what was fetched: the next access reads the arrays again
    b.generation += 1
    b.edge_src[2], b.edge_dst[2] = 3, 4
    assert b.n_edges == 3 and b.edge_id[2] == 2


def test_an_error_status_raises_with_a_clear_message():
    for code, word in ((3, "one-hot"), (5, "capacity")):
        b = _FakeDeviceBatch(status=code)
        with pytest.raises(_lib.SpwgnnError, match=word):
            b.check()
        with pytest.raises(_lib.SpwgnnError, match="batch.status"):
            b.src                                # the lazy fetch checks the status too
    assert _FakeDeviceBatch().check() is not None


def test_refill_is_for_device_built_batches():
    b = TB.TowerBatch.__new__(TB.TowerBatch)
    with pytest.raises(_lib.SpwgnnError, match="from_positions"):
        b.refill(None)
    assert TB.TowerBatch.generation == 0         # host batches keep generation 0 in Workspace.key
