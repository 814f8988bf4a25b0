"""GPU: guard bands (tests/guard.py) around `gates` and every input of spwgnn_dropedge_gates — the plan's edge and
node arrays, `base`, the device key word — at 32, 33 and 64 active edges (one full block; one edge into a second
block; two full blocks) and on a capacity plan with all-padding blocks. Every gate is written, nothing past them, no
input is touched; the values are the numpy restatement's (tests/dropedge_ref.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import dropedge_ref as REF
from guard import Arena
from spwgnn_amd import _lib
from spwgnn_amd.batch import HostPlan

pytestmark = pytest.mark.gpu

DEV = "cuda"
KEY = 0x0F1E2D3C4B5A6978
N = 9   # one tower of 9 boxes: 72 relation slots


def _plan(n_edges, edge_cap=None):
    m, j = np.nonzero(~np.eye(N, dtype=bool))
    src, dst = m[:n_edges].astype(np.int32), j[:n_edges].astype(np.int32)
    pos = np.random.default_rng(1).random((N, 3)).astype(np.float32)
    return HostPlan.build(pos, np.array([N], np.int32), src, dst, np.array([n_edges], np.int32), edge_cap=edge_cap)


@pytest.mark.parametrize("n_edges,edge_cap,blocks", [(32, None, 1), (33, None, 2), (64, None, 2), (10, 72, 3)])
@pytest.mark.parametrize("with_base,key_on_device", [(False, False), (True, True)])
def test_guard_bands(n_edges, edge_cap, blocks, with_base, key_on_device):
    plan = _plan(n_edges, edge_cap)
    assert plan.n_eblocks == blocks
    slots = 32 * blocks
    node_tower, node_local, es, ed = (np.asarray(plan.arrays[k], np.int32).reshape(-1) for k in (1, 2, 4, 5))
    assert int((es >= 0).sum()) == n_edges
    if edge_cap:
        assert (es.reshape(-1, 32) < 0).all(axis=1).sum() == 2     # two all-padding blocks
    ar = Arena(DEV)
    d_es, d_ed = ar.put(es, 4, "edge_src"), ar.put(ed, 4, "edge_dst")
    d_nt, d_nl = ar.put(node_tower, 4, "node_tower"), ar.put(node_local, 4, "node_local")
    base = np.linspace(0.5, 1.5, slots).astype(np.float32)
    d_base = ar.put(base, 4, "base") if with_base else None
    d_key = ar.put(np.array([KEY], np.uint64).view(np.int64), 8, "seed_dev") if key_on_device else None
    gates = ar.alloc(slots, torch.float32, 16, "gates", written=True)
    b = _lib.BatchC()
    b.n_towers, b.n_nodes, b.n_wtiles, b.n_eblocks, b.nw_max = 1, N, plan.n_wtiles, blocks, plan.nw_max
    b.edge_src, b.edge_dst, b.node_tower, b.node_local = (t.data_ptr() for t in (d_es, d_ed, d_nt, d_nl))
    r = _lib.RunC()
    r.seed = 1 if key_on_device else KEY
    if key_on_device:
        r.seed_dev = d_key.data_ptr()
    flags = _lib.DROPEDGE_SYMMETRIC | _lib.DROPEDGE_RESCALE
    st = _lib.lib().spwgnn_dropedge_gates(C.byref(b), C.byref(r), 0.25, flags, d_base.data_ptr() if with_base else None,
                                          gates.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert st == 0
    ar.check(f"dropedge {n_edges} edges")
    want = REF.slot_gates(es, ed, node_tower, node_local, KEY, 0.25, True, True, base if with_base else None)
    got = gates.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.all(got[es < 0].view(np.int32) == 0)
