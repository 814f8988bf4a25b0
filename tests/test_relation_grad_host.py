"""CPU: the host side of spwgnn_backward_relations (within ABI 8) — export, the argument statuses that come
back before any device work — the fp64 identities of the relation gradients on the gated oracle
(tests/relation_grad_ref.py) that the GPU tests rest on, and `TowerBatch.edges_to_input`."""
import ctypes as C

import numpy as np
import torch

import relation_grad_ref as RR
from oracle import model as O
from spwgnn_amd import _lib, batch as BT, data as D

F64 = torch.float64


def test_symbol_and_kernel_id():
    lib = _lib.lib()
    assert hasattr(lib, "spwgnn_backward_relations")
    assert lib.spwgnn_version() == 8 == _lib.ABI_VERSION
    assert _lib.K_REL_BWD == 15


def _structs(training=1):
    """A well-formed batch / run pair whose pointers are never followed."""
    b = _lib.BatchC()
    b.n_towers, b.n_nodes, b.n_wtiles, b.n_eblocks, b.nw_max, b.flags = 2, 12, 2, 2, 6, 0
    fake = 0x1000
    b.pos = b.node_tower = b.node_local = b.wtile = b.edge_src = b.edge_dst = b.blk_csr = fake
    r = _lib.RunC()
    r.mp_steps, r.training, r.dropout, r.math = 3, training, 0.0, _lib.MATH_X6
    return b, r, fake


def test_statuses_without_a_device():
    lib = _lib.lib()
    b, r, fake = _structs()
    need = lib.spwgnn_workspace_bytes(b.n_nodes, b.n_eblocks, r.mp_steps, 1)
    assert need > 0
    call = lambda params, bb, rr, ws, nbytes, drel, steps=None: lib.spwgnn_backward_relations(
        params, C.byref(bb) if bb is not None else None, C.byref(rr) if rr is not None else None, ws, nbytes, drel,
        steps, None)
    assert call(None, b, r, fake, need, fake) == _lib.E_ARG          # null params
    assert call(fake, b, r, None, need, fake) == _lib.E_ARG          # null workspace
    assert call(fake, b, r, fake, need, None) == _lib.E_ARG          # null drel
    assert call(fake, b, r, fake, need, None, fake) == _lib.E_ARG    # drel_steps does not replace drel
    assert call(fake, None, r, fake, need, fake) == _lib.E_ARG       # null batch
    assert call(fake, b, None, fake, need, fake) == _lib.E_ARG       # null run
    assert call(fake, b, r, fake, need - 1, fake) == _lib.E_WORKSPACE
    bi, ri, _ = _structs(training=0)
    assert call(fake, bi, ri, fake, need, fake) == _lib.E_NOTRAIN    # the same answer as spwgnn_backward_inputs
    assert lib.spwgnn_backward_inputs(fake, C.byref(bi), C.byref(ri), fake, need, fake, None) == _lib.E_NOTRAIN
    bad, _, _ = _structs()
    bad.n_eblocks = 0
    assert call(fake, bad, r, fake, need, fake) == _lib.E_SHAPE      # validate()
    for math in (_lib.MATH_F32, _lib.MATH_BF16, _lib.MATH_X3, _lib.MATH_H3):
        r.math = math
        assert call(fake, b, r, fake, need - 1, fake) == _lib.E_WORKSPACE   # every math is served
    r.math = 99
    assert call(fake, b, r, fake, need, fake) == _lib.E_ARG


def _inputs():
    B, N, S = 3, 5, 4
    params = O.random_params(8)
    obj, Rs, Rr, prop, tgt = D.synthetic_batch(B, N, seed=4, fully_connected=False)
    prop = np.random.default_rng(1).normal(0, 0.3, prop.shape)
    e = np.array(O.dense_to_edges(Rs, Rr), np.int64).reshape(-1, 4)
    return params, obj.reshape(-1, 3), e[:, 0] * N + e[:, 2], e[:, 0] * N + e[:, 3], prop.reshape(-1, 100), tgt, S


def test_gated_forward_at_one_is_forward_gather():
    params, pos, src, dst, prop, _, S = _inputs()
    tp = O.to_torch(params)
    x, pr = torch.as_tensor(pos, dtype=F64), torch.as_tensor(prop, dtype=F64)
    s, d = torch.as_tensor(src), torch.as_tensor(dst)
    with torch.no_grad():
        ref = O.forward_gather(tp, x, s, d, pr, S)
        got = RR.forward_gather_gated(tp, x, s, d, pr, S, [torch.ones(len(src), dtype=F64)] * S)
    assert torch.equal(got, ref)


def test_gate_gradient_is_the_closed_form_and_eulers_identity():
    """r_{k,s} from autograd (the gate as the leaf) = <g_s[dst_k], e_{k,s}> with g_s = d loss / d (receiver sum
    of step s) read off the graph, to 1e-12 relative; and, the sum being linear in the gates,
    Σ_k r_{k,s} = Σ_i <g_s[i], agg_s[i]>."""
    params, pos, src, dst, prop, tgt, S = _inputs()
    for loss in ("bce", "sum_prob"):
        keep = {}
        r, steps, _, _ = RR.relation_grads(params, pos, src, dst, prop, S, tgt, loss, keep=keep)
        assert steps.shape == (S, len(src)) and np.abs(r).max() > 0
        closed = np.stack([(keep["agg"][s].grad[torch.as_tensor(dst)] * keep["e"][s]).sum(1).numpy() for s in range(S)])
        scale = np.abs(steps).max()
        assert np.abs(closed - steps).max() <= 1e-12 * scale
        assert np.abs(closed.sum(0) - r).max() <= 1e-12 * np.abs(r).max()
        for s in range(S):
            euler = float((keep["agg"][s].grad * keep["agg"][s].detach()).sum())
            assert abs(steps[s].sum() - euler) <= 1e-12 * max(abs(euler), scale)


def test_gate_gradient_against_deleting_an_edge():
    """What the number means: removing relation k changes the loss by −r_k to first order — checked by a
    central difference on one gate (all steps together) in fp64."""
    params, pos, src, dst, prop, tgt, S = _inputs()
    r, _, _, _ = RR.relation_grads(params, pos, src, dst, prop, S, tgt, "bce")
    tp = O.to_torch(params)
    x, pr = torch.as_tensor(pos, dtype=F64), torch.as_tensor(prop, dtype=F64)
    s, d = torch.as_tensor(src), torch.as_tensor(dst)
    k, h = int(np.argmax(np.abs(r))), 1e-6

    def loss_at(w):
        g = torch.ones(len(src), dtype=F64)
        g[k] = w
        with torch.no_grad():
            return float(RR.loss_of(RR.forward_gather_gated(tp, x, s, d, pr, S, [g] * S), tgt, "bce"))
    fd = (loss_at(1 + h) - loss_at(1 - h)) / (2 * h)
    assert abs(fd - r[k]) <= 1e-7 * abs(r[k])


def test_edges_to_input_round_trip_on_a_packed_ragged_plan():
    """Slot values → (src, dst, values) in the input's node ids, the padding dropped, for a packed plan of
    towers of 1, 2, 4, 7 and 3 boxes (fully connected here); and the dense form of equal towers."""
    sizes = np.array([1, 2, 4, 7, 3], np.int32)
    off = np.concatenate([[0], np.cumsum(sizes)])
    src, dst = [], []
    for t, n in enumerate(sizes):
        m, j = np.nonzero(~np.eye(n, dtype=bool))
        src.append(off[t] + m)
        dst.append(off[t] + j)
    src, dst = np.concatenate(src).astype(np.int32), np.concatenate(dst).astype(np.int32)
    tes = (sizes * (sizes - 1)).astype(np.int32)
    pos = np.random.default_rng(0).random((int(off[-1]), 3)).astype(np.float32)
    plan = BT.HostPlan.build(pos, sizes, src, dst, tes, pack=True)
    assert plan.node_perm is not None and not np.array_equal(plan.node_perm, np.arange(off[-1]))
    # a value per slot that encodes the slot's own (input sender, input receiver), read off the slot arrays
    # the kernels index (edge_src / edge_dst of the upload); -7 in the padding
    perm = np.asarray(plan.node_perm, np.int64)
    esrc, edst = plan.arrays[4], plan.arrays[5]
    act = esrc >= 0
    assert np.array_equal(act, np.asarray(plan.edge_id) >= 0) and np.array_equal(act, edst >= 0)
    vals = np.full(len(esrc), -7.0)
    vals[act] = perm[esrc[act]] * 100.0 + perm[edst[act]]
    s_in, d_in, v = plan.edges_to_input(vals)
    assert len(v) == len(src) == int(act.sum()) and not np.any(v == -7.0)
    assert np.array_equal(v, s_in * 100.0 + d_in)
    # the same relation set as the input's, as a set of pairs
    assert sorted(zip(s_in.tolist(), d_in.tolist())) == sorted(zip(src.tolist(), dst.tolist()))
    # leading axes (the per-step rows) are kept
    s2, d2, v2 = plan.edges_to_input(np.stack([vals, 2 * vals]))
    assert v2.shape == (2, len(src)) and np.array_equal(v2[1], 2 * v)
    try:
        plan.edges_to_input(vals, dense=True)
        raise AssertionError("ragged towers have no dense form")
    except ValueError:
        pass
    # equal towers: (B, N, N) [sender, receiver], zero diagonal
    B, N = 3, 4
    m, j = np.nonzero(~np.eye(N, dtype=bool))
    src = np.concatenate([b * N + m for b in range(B)]).astype(np.int32)
    dst = np.concatenate([b * N + j for b in range(B)]).astype(np.int32)
    plan = BT.HostPlan.build(np.zeros((B * N, 3), np.float32), np.full(B, N, np.int32), src, dst,
                             np.full(B, N * (N - 1), np.int32))
    esrc, edst = plan.arrays[4], plan.arrays[5]
    vals = np.where(esrc >= 0, esrc * 100.0 + edst, -7.0)
    dense = plan.edges_to_input(vals, dense=True)
    assert dense.shape == (B, N, N)
    for b in range(B):
        for s in range(N):
            for r in range(N):
                assert dense[b, s, r] == (0.0 if s == r else (b * N + s) * 100.0 + b * N + r)
