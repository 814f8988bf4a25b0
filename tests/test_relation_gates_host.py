"""CPU: the host side of the relation gates (spwgnn_forward_gated / spwgnn_backward_gated / spwgnn_gates_supported,
within ABI 8) — exports and unchanged structs, the statuses that come back before any device work,
`edge_gates` as the inverse of `edges_to_input`, the fp64 identities of the gated oracle the GPU tests rest on, and
the ReLU margins of the GPU tests' inputs under their gates."""
import ctypes as C

import numpy as np
import pytest
import torch

import relation_gates_ref as GR
import relation_grad_ref as RR
import test_gpu_input_grad as IG
from oracle import model as O
from spwgnn_amd import _lib, batch as BT, data as D, engine as E

F64 = torch.float64
MATHS = {"f32": _lib.MATH_F32, "x6": _lib.MATH_X6, "bf16": _lib.MATH_BF16, "x3": _lib.MATH_X3, "h3": _lib.MATH_H3}


# ------------------------------------------------------------------------------------ the C ABI
def test_exports_version_and_struct_sizes():
    lib = _lib.lib()
    for name in ("spwgnn_gates_supported", "spwgnn_forward_gated", "spwgnn_backward_gated"):
        assert hasattr(lib, name)
    assert lib.spwgnn_version() == 8 == _lib.ABI_VERSION
    # no struct was added or changed: the ids in use answer their ctypes mirror's size, the free ones -1
    for which, st in ((0, _lib.BatchC), (1, _lib.RunC), (2, _lib.PlanSizes), (3, _lib.ParamInfo), (4, _lib.LossWeightsC),
                      (6, _lib.PlanDeviceC), (7, _lib.ClipC), (9, _lib.StepWeightsC), (10, _lib.EvalC),
                      (12, _lib.TowerLossC)):
        assert lib.spwgnn_struct_size(which) == C.sizeof(st)
    for which in (5, 8, 11, 13, 14):
        assert lib.spwgnn_struct_size(which) == -1
    # the sizes spwgnn_struct_size(0 .. 14) answered before this change
    assert [lib.spwgnn_struct_size(k) for k in range(15)] == [88, 64, 12, 24, 24, -1, 112, 32, -1, 264, 64, -1, 80, -1, -1]


def test_gates_supported_per_math():
    lib = _lib.lib()
    assert [lib.spwgnn_gates_supported(MATHS[m]) for m in ("x6", "x3", "h3")] == [1, 1, 1]
    assert [lib.spwgnn_gates_supported(MATHS[m]) for m in ("f32", "bf16")] == [0, 0]
    assert lib.spwgnn_gates_supported(99) == -1 and lib.spwgnn_gates_supported(-1) == -1
    assert E.gates_supported("x6") and E.gates_supported("h3") and not E.gates_supported("bf16")
    with pytest.raises(ValueError):
        E.gates_supported(99)


def _structs(training=1, math=_lib.MATH_X6):
    """A well-formed batch / run pair whose pointers are never followed (every status below comes back first)."""
    b = _lib.BatchC()
    b.n_towers, b.n_nodes, b.n_wtiles, b.n_eblocks, b.nw_max, b.flags = 2, 12, 2, 2, 6, 0
    fake = 0x1000
    b.pos = b.node_tower = b.node_local = b.wtile = b.edge_src = b.edge_dst = b.blk_csr = fake
    r = _lib.RunC()
    r.mp_steps, r.training, r.dropout, r.math = 3, training, 0.0, math
    return b, r, fake


def _fwd(lib, params, b, r, ws, nbytes, gates, logits, state=None):
    return lib.spwgnn_forward_gated(params, C.byref(b) if b is not None else None, C.byref(r) if r is not None else None,
                                    ws, nbytes, gates, logits, state, None)


def _bwd(lib, params, b, r, ws, nbytes, gates, dlogits, dstate, grads, dprop=None):
    return lib.spwgnn_backward_gated(params, C.byref(b) if b is not None else None,
                                     C.byref(r) if r is not None else None, ws, nbytes, gates, dlogits, dstate, grads,
                                     dprop, None)


def test_statuses_without_a_device():
    """Every argument error returns before any device work: the pointers here are never followed. One byte short
    of the workspace is the last check, so SPWGNN_E_WORKSPACE stands for "every argument was accepted"."""
    lib = _lib.lib()
    b, r, fake = _structs()
    need = lib.spwgnn_workspace_bytes(b.n_nodes, b.n_eblocks, r.mp_steps, 1)
    short = need - 1
    # an otherwise valid argument set, with gates, with a null gate pointer (= the ungated call)
    assert _fwd(lib, fake, b, r, fake, short, fake, fake) == _lib.E_WORKSPACE
    assert _fwd(lib, fake, b, r, fake, short, None, fake) == _lib.E_WORKSPACE
    assert _bwd(lib, fake, b, r, fake, short, fake, fake, None, fake) == _lib.E_WORKSPACE
    assert _bwd(lib, fake, b, r, fake, short, None, fake, None, fake) == _lib.E_WORKSPACE
    # misaligned gate, state and state-cotangent pointers
    for off in (4, 8, 12):
        assert _fwd(lib, fake, b, r, fake, need, fake + off, fake) == _lib.E_ARG
        assert _bwd(lib, fake, b, r, fake, need, fake + off, fake, None, fake) == _lib.E_ARG
    assert _fwd(lib, fake, b, r, fake, need, fake, fake, fake + 4) == _lib.E_ARG
    assert _bwd(lib, fake, b, r, fake, need, fake, fake, fake + 4, fake) == _lib.E_ARG
    # the arguments of spwgnn_forward_state / spwgnn_backward_state, checked as there
    assert _fwd(lib, None, b, r, fake, need, fake, fake) == _lib.E_ARG
    assert _fwd(lib, fake, b, r, fake, need, fake, None) == _lib.E_ARG
    assert _fwd(lib, fake, b, r, None, need, fake, fake) == _lib.E_ARG
    assert _fwd(lib, fake, None, r, fake, need, fake, fake) == _lib.E_ARG
    assert _fwd(lib, fake, b, None, fake, need, fake, fake) == _lib.E_ARG
    assert _bwd(lib, None, b, r, fake, need, fake, fake, None, fake) == _lib.E_ARG
    assert _bwd(lib, fake, b, r, fake, need, fake, None, None, fake) == _lib.E_ARG
    assert _bwd(lib, fake, b, r, fake, need, fake, fake, None, None) == _lib.E_ARG
    bi, ri, _ = _structs(training=0)
    assert _bwd(lib, fake, bi, ri, fake, need, fake, fake, None, fake) == _lib.E_NOTRAIN
    need_inf = lib.spwgnn_workspace_bytes(bi.n_nodes, bi.n_eblocks, ri.mp_steps, 0)
    assert _fwd(lib, fake, bi, ri, fake, need_inf - 1, fake, fake) == _lib.E_WORKSPACE   # inference takes gates too
    bad, _, _ = _structs()
    bad.n_eblocks = 0
    assert _fwd(lib, fake, bad, r, fake, need, fake, fake) == _lib.E_SHAPE
    r.math = 99
    assert _fwd(lib, fake, b, r, fake, need, fake, fake) == _lib.E_ARG


@pytest.mark.parametrize("math", sorted(MATHS))
def test_query_agrees_with_the_call(math):
    """spwgnn_gates_supported(math) == 1 exactly when a gated call with otherwise valid arguments is accepted
    (it then fails the last check, the workspace size); 0 exactly when it returns SPWGNN_E_SHAPE, whatever the
    workspace size. A null gate pointer is accepted in every math."""
    lib = _lib.lib()
    b, r, fake = _structs(math=MATHS[math])
    need = lib.spwgnn_workspace_bytes(b.n_nodes, b.n_eblocks, r.mp_steps, 1)
    want = _lib.E_WORKSPACE if lib.spwgnn_gates_supported(MATHS[math]) == 1 else _lib.E_SHAPE
    assert _fwd(lib, fake, b, r, fake, need - 1, fake, fake) == want
    assert _bwd(lib, fake, b, r, fake, need - 1, fake, fake, None, fake) == want
    assert _fwd(lib, fake, b, r, fake, need - 1, None, fake) == _lib.E_WORKSPACE
    assert _bwd(lib, fake, b, r, fake, need - 1, None, fake, None, fake) == _lib.E_WORKSPACE
    if want == _lib.E_SHAPE:   # refused with a workspace of the full size as well: still no device work
        assert _fwd(lib, fake, b, r, fake, need, fake, fake) == _lib.E_SHAPE
        assert _bwd(lib, fake, b, r, fake, need, fake, fake, None, fake) == _lib.E_SHAPE


# ------------------------------------------------------------------------------------ edge_gates
def _ragged_plan(pack, edge_cap=None):
    sizes = np.array([1, 2, 4, 7, 3], np.int32)
    off = np.concatenate([[0], np.cumsum(sizes)])
    src, dst = [], []
    for t, n in enumerate(sizes):
        m, j = np.nonzero(~np.eye(n, dtype=bool))
        src.append(off[t] + m)
        dst.append(off[t] + j)
    src, dst = np.concatenate(src).astype(np.int32), np.concatenate(dst).astype(np.int32)
    pos = np.random.default_rng(0).random((int(off[-1]), 3)).astype(np.float32)
    return BT.HostPlan.build(pos, sizes, src, dst, (sizes * (sizes - 1)).astype(np.int32), pack=pack, edge_cap=edge_cap)


@pytest.mark.parametrize("kind", ["plain", "packed", "capacity"])
def test_edge_gates_inverts_edges_to_input(kind):
    """1-D values in the input's edge order → slots → `edges_to_input` gives them back; the padding holds `fill`;
    the gradient of Σ c_slot·gates[slot] arrives at the right entries of `values`."""
    plan = _ragged_plan(kind == "packed", 64 if kind == "capacity" else None)
    if kind == "packed":
        assert plan.node_perm is not None and not np.array_equal(plan.node_perm, np.arange(plan.n_nodes))
    ne, eid = len(plan.src), np.asarray(plan.edge_id)
    if kind == "capacity":
        assert 32 * plan.n_eblocks >= 64 * 5 and int((eid < 0).sum()) > 32
    vals = torch.arange(1, ne + 1, dtype=F64, requires_grad=True)
    gates = plan.edge_gates(vals, fill=-7.0)
    assert gates.shape == (32 * plan.n_eblocks,) and gates.dtype == torch.float32 and gates.is_contiguous()
    g = gates.detach().numpy()
    assert np.all(g[eid < 0] == -7.0) and np.array_equal(g[eid >= 0], eid[eid >= 0] + 1.0)
    s_in, d_in, back = plan.edges_to_input(g)
    assert np.array_equal(back, np.arange(1, ne + 1))
    coef = torch.arange(len(eid), dtype=torch.float32)
    (gates * coef).sum().backward()
    want = np.zeros(ne)
    want[eid[eid >= 0]] = np.nonzero(eid >= 0)[0]
    assert vals.grad.dtype == F64 and np.array_equal(vals.grad.numpy(), want)
    assert np.all(plan.edge_gates(vals.detach()).numpy()[eid < 0] == 0.0)   # the default fill
    with pytest.raises(ValueError):
        plan.edge_gates(torch.zeros(ne + 1))
    with pytest.raises(ValueError):
        plan.edge_gates(torch.zeros(5, 7, 7))   # ragged towers have no dense form


def test_edge_gates_dense_form():
    """(B, N, N) [tower, sender, receiver] → slots; `edges_to_input(dense=True)` gives the matrix back (zero
    diagonal); thresholded towers read only their relations' entries."""
    B, N = 3, 5
    obj, Rs, Rr, _, _ = D.synthetic_batch(B, N, seed=4, fully_connected=False)
    e = np.array(O.dense_to_edges(Rs, Rr), np.int64).reshape(-1, 4)
    src, dst = (e[:, 0] * N + e[:, 2]).astype(np.int32), (e[:, 0] * N + e[:, 3]).astype(np.int32)
    te = np.bincount(e[:, 0], minlength=B).astype(np.int32)
    assert 0 < len(src) < B * N * (N - 1)
    plan = BT.HostPlan.build(obj.reshape(-1, 3), np.full(B, N, np.int32), src, dst, te)
    dense = torch.tensor(np.random.default_rng(2).normal(size=(B, N, N)), dtype=torch.float32, requires_grad=True)
    gates = plan.edge_gates(dense, fill=9.0)
    eid = np.asarray(plan.edge_id)
    g = gates.detach().numpy()
    assert np.all(g[eid < 0] == 9.0)
    assert np.array_equal(g[eid >= 0], dense.detach().numpy()[src // N, src % N, dst % N][eid[eid >= 0]])
    back = plan.edges_to_input(g, dense=True)
    mask = np.zeros((B, N, N), bool)
    mask[src // N, src % N, dst % N] = True
    assert np.array_equal(back, np.where(mask, dense.detach().numpy(), 0.0))
    gates.sum().backward()
    assert np.array_equal(dense.grad.numpy(), mask.astype(np.float32))   # entries without a relation are not read
    # the 1-D form of the same values gives the same slots
    one_d = dense.detach()[torch.as_tensor(src // N), torch.as_tensor(src % N), torch.as_tensor(dst % N)]
    assert torch.equal(plan.edge_gates(one_d, fill=9.0), gates.detach())


# ------------------------------------------------------------------------------------ oracle identities (fp64)
def _c64():
    return IG._case("team_a")


def test_shared_gate_forward_is_the_oracles():
    """`relation_gates_ref.forward` = `relation_grad_ref.forward_gather_gated` with the same gate at every step, bit
    for bit, and at gate ≡ 1 `forward_gather`."""
    c = _c64()
    tp = O.to_torch(c["params"])
    x, pr = torch.as_tensor(c["obj"].reshape(-1, 3), dtype=F64), torch.as_tensor(c["prop"].reshape(-1, 100), dtype=F64)
    s, d = torch.as_tensor(c["src"]), torch.as_tensor(c["dst"])
    w = torch.as_tensor(GR.gates_for(len(c["src"])), dtype=F64)
    with torch.no_grad():
        assert torch.equal(GR.forward(tp, x, s, d, pr, c["S"], w)[0], RR.forward_gather_gated(tp, x, s, d, pr, c["S"], [w] * c["S"]))
        assert torch.equal(GR.forward(tp, x, s, d, pr, c["S"], torch.ones_like(w))[0], O.forward_gather(tp, x, s, d, pr, c["S"]))


def test_central_difference_on_one_gate():
    """Autograd with one shared gate tensor as the leaf, at gates away from 1, against a central difference."""
    c = _c64()
    gate = GR.gates_for(len(c["src"])).astype(np.float64)
    ref = GR.oracle(c, gate, "bce")
    tp = O.to_torch(c["params"])
    x, pr = torch.as_tensor(c["obj"].reshape(-1, 3), dtype=F64), torch.as_tensor(c["prop"].reshape(-1, 100), dtype=F64)
    s, d = torch.as_tensor(c["src"]), torch.as_tensor(c["dst"])
    for k in (0, 2, int(np.argmax(np.abs(ref["dgate"])))):   # the zero gate, the negative one, the largest gradient
        def loss_at(wk):
            w = torch.as_tensor(gate.copy())
            w[k] = wk
            with torch.no_grad():
                return float(RR.loss_of(GR.forward(tp, x, s, d, pr, c["S"], w)[0], c["tgt"], "bce"))
        h = 1e-6
        fd = (loss_at(gate[k] + h) - loss_at(gate[k] - h)) / (2 * h)
        assert abs(fd - ref["dgate"][k]) <= 1e-7 * np.abs(ref["dgate"]).max(), (k, fd, ref["dgate"][k])


def test_gate_zero_deletes_the_edges():
    """Gate 0 on a subset of the edges = `forward_gather` on the batch without them, to 1e-12."""
    c = IG._case("wide")
    tp = O.to_torch(c["params"])
    x, pr = torch.as_tensor(c["obj"].reshape(-1, 3), dtype=F64), torch.as_tensor(c["prop"].reshape(-1, 100), dtype=F64)
    s, d = torch.as_tensor(c["src"]), torch.as_tensor(c["dst"])
    keep = np.arange(len(c["src"])) % 3 != 0
    w = torch.as_tensor(keep.astype(np.float64))
    with torch.no_grad():
        gated = GR.forward(tp, x, s, d, pr, c["S"], w)[0]
        cut = O.forward_gather(tp, x, s[torch.as_tensor(keep)], d[torch.as_tensor(keep)], pr, c["S"])
    assert float((gated - cut).abs().max()) <= 1e-12


def test_soft_threshold_formula():
    """sigmoid((threshold − distance) / tau): 1/2 on the threshold, the hard relation set as tau → 0, and its
    derivative in the positions against a central difference."""
    raw = torch.tensor(D.synthetic_towers(2, 5, seed=7).reshape(-1, 3)[:, :2], dtype=F64, requires_grad=True)
    N = 5
    m, j = np.nonzero(~np.eye(N, dtype=bool))
    src = torch.as_tensor(np.concatenate([b * N + m for b in range(2)]))
    dst = torch.as_tensor(np.concatenate([b * N + j for b in range(2)]))
    dist = (raw[src] - raw[dst]).norm(dim=-1).detach()
    g = GR.soft_threshold_gates(raw, src, dst, 170.0, 20.0)
    assert torch.allclose(g, 1.0 / (1.0 + torch.exp((dist - 170.0) / 20.0)), rtol=1e-12, atol=0)
    assert float(GR.soft_threshold_gates(torch.tensor([[0.0, 0.0], [170.0, 0.0]], dtype=F64), torch.tensor([0]),
                                         torch.tensor([1]), 170.0, 20.0)) == 0.5
    hard = GR.soft_threshold_gates(raw.detach(), src, dst, 170.0, 1e-3)
    assert torch.equal(hard.round(), (dist < 170.0).to(F64))
    g.sum().backward()
    k, h = 3, 1e-5
    up, dn = raw.detach().clone(), raw.detach().clone()
    up[k, 0] += h
    dn[k, 0] -= h
    fd = (GR.soft_threshold_gates(up, src, dst, 170.0, 20.0).sum() - GR.soft_threshold_gates(dn, src, dst, 170.0, 20.0).sum()) / (2 * h)
    assert abs(float(fd) - float(raw.grad[k, 0])) <= 1e-8 * max(1.0, abs(float(fd)))


# ------------------------------------------------------------------------------------ the GPU tests' inputs
@pytest.mark.parametrize("name", ["team_a", "team_b", "wide", "recv"])
def test_gated_margins_of_the_gpu_cases(name):
    """With the gates the GPU tests use (seed 1000) every tower's smallest ReLU pre-activation distance under the
    GATED fp64 forward exceeds TAU: no tower is left out of any parity test."""
    c = IG._case(name)
    gate = GR.gates_for(len(c["src"]))
    assert gate[0] == 0.0 and gate[1] == 1.0 and gate[2] == -0.5 and gate[3:].min() >= 0.25 and gate.max() < 1.5
    m = GR.gated_margins(c, gate)
    print(f"{name}: gated ReLU margins per tower, min {m.min():.2e} (TAU {GR.TAU:g})")
    assert m.shape == (c["B"],) and np.all(m > GR.TAU), m
    # at gate ≡ 1 the margins are the ungated function's
    assert np.array_equal(GR.gated_margins(c, np.ones(len(c["src"]))), IG._assert_margins(c))


def test_gated_margins_of_the_ragged_case():
    c, sizes, _ = IG._ragged_case()
    gate, seed = GR.pick_gates(c, sizes)
    m = GR.gated_margins(c, gate, sizes)
    print(f"ragged: gate seed {seed}, gated ReLU margins min {m.min():.2e}")
    assert np.all(m > GR.TAU)
