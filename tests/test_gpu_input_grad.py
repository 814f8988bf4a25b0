"""GPU: d(loss)/d(objects) — `engine.backward_inputs` (spwgnn_backward_inputs, k_input_bwd), the
autograd path of `GraphNetwork` and `demolish.stability_gradients` — against fp64 torch autograd
through the oracle with the objects as the leaf.

The relation set is a constant of the graph on both sides: the oracle takes the relation matrices /
edge lists as data, the engine its plan.

Criterion (f32 and x6 math): max|got − ref| <= 1e-5·max|ref| + 1e-8, the project's gradient criterion
(test_gpu_training.py). Plain fp32 torch against fp64 gives 1.4e-7 to 7.3e-7 of the max on these
inputs, the class of the rm.0 / om.0 kernel gradients.

ReLU kinks: the rule of test_gpu_chain_parity.py (TAU = 1e-6) with no tower left out — the data seeds
were picked on the CPU so that `oracle.model.relu_margins_gather` exceeds TAU for every tower, and
every case asserts it. The one exception is the committed dropout fixture (case 3), whose inputs are
given: its tower 0 sits 1.6e-7 from a kink, printed there; tests/test_gpu_training.py::
test_golden_dropout holds every parameter gradient of the same run to the same criterion.
"""
import os

import numpy as np
import pytest
import torch

from oracle import dropout as DR
from oracle import model as O
from spwgnn_amd import GraphNetwork, TowerBatch, _lib, data as D, demolish, engine as E, params as P

pytestmark = pytest.mark.gpu

TAU = 1e-6
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
F64 = torch.float64


# ------------------------------------------------------------------------------------ inputs
def _dense_case(B, N, seed, fully, pseed, S):
    """A `synthetic_batch` in dense and edge form with the non-zero propagation input the margins
    were measured with; asserts every tower's ReLU margin."""
    params = O.random_params(pseed)
    obj, Rs, Rr, prop, tgt = D.synthetic_batch(B, N, seed=seed, fully_connected=fully)
    prop = np.random.default_rng(1).normal(0, 0.3, prop.shape).astype(np.float32)
    e = np.array(O.dense_to_edges(Rs, Rr), np.int64).reshape(-1, 4)
    src, dst = e[:, 0] * N + e[:, 2], e[:, 0] * N + e[:, 3]
    c = dict(params=params, obj=obj, Rs=Rs, Rr=Rr, prop=prop, tgt=tgt, src=src, dst=dst, slots=e, S=S, B=B, N=N)
    _assert_margins(c)
    return c


def _assert_margins(c, drop_r=None, drop_o=None, sizes=None, assert_tau=True):
    sizes = np.full(c["B"], c["N"]) if sizes is None else np.asarray(sizes)
    m = O.relu_margins_gather(O.to_torch(c["params"]), c["obj"].reshape(-1, 3), c["src"], c["dst"],
                              c["prop"].reshape(-1, 100), np.repeat(np.arange(len(sizes)), sizes), len(sizes), c["S"],
                              drop_r=drop_r, drop_o=drop_o)
    print(f"ReLU margins per tower: min {m.min():.2e} (TAU {TAU:g})")
    if assert_tau:
        assert np.all(m > TAU), m
    return m


_CASES = {}


def _case(name):
    """The shared inputs (built once): name → dict."""
    if name not in _CASES:
        spec = {"team_a": (3, 5, 4, False, 8, 4), "team_b": (2, 6, 11, False, 3, 3),
                "wide": (4, 6, 2, True, 2, 5), "recv": (2, 9, 13, True, 5, 2)}[name]
        _CASES[name] = _dense_case(*spec)
    return _CASES[name]


# ------------------------------------------------------------------------------------ reference
_REFS = {}


def _oracle(c, key=None, drop_r=None, drop_o=None, loss="bce"):
    """fp64 autograd through `forward_gather` with the objects as the leaf: (dobj (Nn, 3), parameter
    gradients, logits). loss "bce": the Keras mean BCE; "sum": Σ z; "sum_prob": Σ sigmoid(z)."""
    if key is not None and key in _REFS:
        return _REFS[key]
    tp = O.to_torch(c["params"], requires_grad=True)
    x = torch.tensor(c["obj"].reshape(-1, 3), dtype=F64, requires_grad=True)
    as64 = lambda a: None if a is None else torch.as_tensor(np.asarray(a), dtype=F64)
    z = O.forward_gather(tp, x, torch.as_tensor(c["src"]), torch.as_tensor(c["dst"]), as64(c["prop"].reshape(-1, 100)),
                         c["S"], drop_r=as64(drop_r), drop_o=as64(drop_o))
    if loss == "bce":
        out = O.keras_bce_from_logits(z, as64(c["tgt"]).reshape(z.shape))
    elif loss == "sum":
        out = z.sum()
    else:
        out = torch.sigmoid(z).sum()
    out.backward()
    res = (x.grad.numpy().copy(), {k: v.grad.numpy().copy() for k, v in tp.items()}, z.detach().numpy().copy())
    if key is not None:
        _REFS[key] = res
    return res


def _dense_oracle_dobj(c):
    """The same derivative through the literal dense graph (`forward_dense`), objects (B, N, 3) as the leaf."""
    tp = O.to_torch(c["params"])
    x = torch.tensor(c["obj"], dtype=F64, requires_grad=True)
    z = O.forward_dense(tp, x, torch.tensor(c["Rs"], dtype=F64), torch.tensor(c["Rr"], dtype=F64),
                        torch.tensor(c["prop"], dtype=F64), c["S"])
    O.keras_bce_from_logits(z, torch.tensor(c["tgt"], dtype=F64)).backward()
    return x.grad.numpy().reshape(-1, 3)


# ------------------------------------------------------------------------------------ engine
def _engine(c, batch, math, tgt=None, dropout=0.0, seed=0, inputs=True, fused_bce=False):
    """One training step's forward + loss + backward (+ backward_inputs): (z, grads (flat, device), dprop, dobj)."""
    flat = P.to_flat(c["params"], device="cuda")
    ws = E.Workspace("cuda")
    run = E.RunConfig(c["S"], training=True, math=math, dropout=dropout, seed=seed)
    tgt = torch.as_tensor(np.asarray(c["tgt"] if tgt is None else tgt, np.float32), device="cuda").reshape(-1)
    want_dprop = batch.prop is not None
    z = E.forward(flat, batch, run, ws)
    if fused_bce:
        _, _, g, dp = E.bce_backward(flat, batch, run, ws, z, tgt, E.BceScratch("cuda"), want_dprop=want_dprop)
    else:
        _, dz = E.bce(z, tgt, E.BceScratch("cuda"))
        g, dp = E.backward(flat, batch, run, ws, dz, want_dprop=want_dprop)
    dobj = E.backward_inputs(flat, batch, run, ws) if inputs else None
    torch.cuda.synchronize()
    if dobj is not None:
        assert dobj.shape == (batch.n_nodes, 3)
        full = dobj._base if dobj._base is not None else dobj
        assert full.shape == (batch.n_nodes, 4) and bool((full[:, 3] == 0).all())   # column 3 is written as 0
        dobj = dobj.cpu().numpy()
    return z.cpu().numpy(), g, dp, dobj


def _close(what, got, ref, g=None, g_ref=None):
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    msg = f"{what}: max|dobj - ref| {err:.3e} = {err / scale:.2e} of max|ref| {scale:.3e}"
    if g is not None:   # the same run's rm.0 kernel gradient beside it
        k = P.from_flat(g)["rm.0.kernel"]
        msg += f"; rm.0.kernel {np.abs(k - g_ref['rm.0.kernel']).max() / np.abs(g_ref['rm.0.kernel']).max():.2e}"
    print(msg)
    assert err <= 1e-5 * scale + 1e-8, msg


def _tower_x_sums(what, dobj, sizes):
    """Translation invariance: per tower Σ_n d/dx = 0 in mathematics; the kernel adds the same fp32 q_e
    with both signs, so at most 2N(N−1) roundings remain (bound 1e-4 of the array's max|d/dx|)."""
    off = np.concatenate([[0], np.cumsum(sizes)])
    x = dobj[:, 0].astype(np.float64)
    sums = np.array([x[a:b].sum() for a, b in zip(off[:-1], off[1:])])
    print(f"{what}: max per-tower |sum d/dx| {np.abs(sums).max():.3e}, max |d/dx| {np.abs(x).max():.3e}")
    assert np.all(np.abs(sums) <= 1e-4 * np.abs(x).max()), (what, sums)


# ------------------------------------------------------------------------------------ cases
@pytest.mark.parametrize("math", ["f32", "x6"])
@pytest.mark.parametrize("name", ["team_a", "team_b"])
def test_oracle_parity_team_path(name, math):
    """Case 1: small thresholded batches on the team (small-batch) kernels; the parameter gradients and
    d/d'propagation' of the run are bitwise those of a run that never calls backward_inputs."""
    c = _case(name)
    batch = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], c["prop"], device="cuda")
    assert E.team_max_blocks() == 512 and batch.n_eblocks <= 512
    ref, g_ref, _ = _oracle(c, name)
    assert np.abs(ref - _dense_oracle_dobj(c)).max() <= 1e-12 * np.abs(ref).max()   # both oracle forms agree
    _, g, dp, dobj = _engine(c, batch, math)
    _close(f"{name} {math}", dobj, ref, g, g_ref)
    _, g0, dp0, _ = _engine(c, batch, math, inputs=False)
    assert torch.equal(g, g0) and torch.equal(dp, dp0)


@pytest.mark.parametrize("math,fused_bce", [("f32", False), ("x6", False), ("x6", True)])
def test_oracle_parity_wide_kernels(math, fused_bce):
    """Case 2: the wide (large-batch) kernels on a fully connected batch whose wave-tiles span more than
    one edge block; once more through bce_backward; translation invariance in x6."""
    c = _case("wide")
    ref, g_ref, _ = _oracle(c, "wide")
    with E.wide_kernels():
        batch = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], c["prop"], device="cuda", nw_max=16)
        assert batch.n_eblocks > batch.n_wtiles   # two towers per wave-tile: 60 edges, two blocks
        _, g, _, dobj = _engine(c, batch, math, fused_bce=fused_bce)
    _close(f"wide {math} bce_backward={fused_bce}", dobj, ref, g, g_ref)
    if math == "x6":
        _tower_x_sums("wide x6", dobj, np.full(c["B"], c["N"]))


def test_dropout_on():
    """Case 3: the committed dropout fixture's inputs, rate and seed; the oracle multiplies the engine's
    masks (oracle/dropout.py) in as drop_r / drop_o."""
    g = np.load(os.path.join(GOLDEN, "golden_dropout_N6_B2_S5.npz"))
    B, N = g["objects"].shape[:2]
    rate, seed = float(g["rate"]), int(g["seed"])
    e = np.array(O.dense_to_edges(g["Rs"], g["Rr"]), np.int64).reshape(-1, 4)
    c = dict(params=dict(np.load(os.path.join(GOLDEN, "golden_params.npz"))), obj=g["objects"], Rs=g["Rs"], Rr=g["Rr"],
             prop=g["prop"], tgt=g["target"], src=e[:, 0] * N + e[:, 2], dst=e[:, 0] * N + e[:, 3], S=int(g["mp_steps"]),
             B=B, N=N)
    drop_r = DR.relation_mask(seed, rate, B, N)[e[:, 0], e[:, 1]]
    drop_o = DR.object_mask(seed, rate, B, N).reshape(-1, 100)
    _assert_margins(c, drop_r, drop_o, assert_tau=False)   # given inputs (module docstring): printed
    ref, g_ref, z_ref = _oracle(c, None, drop_r, drop_o)
    assert np.abs(z_ref.reshape(g["logits"].shape) - g["logits"]).max() < 1e-12   # the fixture's own forward
    batch = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], None, device="cuda")
    _, gr, _, dobj = _engine(c, batch, "x6", dropout=rate, seed=seed)
    _close("dropout fixture x6", dobj, ref, gr, g_ref)


def _ragged_case():
    """Towers of 1, 2, 4, 7 and 3 boxes, relations thresholded on the raw positions (main.py:71-81)."""
    sizes = [1, 2, 4, 7, 3]
    raws = [D.synthetic_towers(1, n, seed=50 + k)[0] for k, n in enumerate(sizes)]
    srcs, dsts, tes, off, isolated = [], [], [], 0, False
    for raw in raws:
        n = len(raw)
        m_idx, j_idx = np.nonzero(~np.eye(n, dtype=bool))
        keep = np.linalg.norm(raw[m_idx, 0:2] - raw[j_idx, 0:2], axis=1) < D.RELATION_THRESHOLD
        m_idx, j_idx = m_idx[keep], j_idx[keep]
        isolated |= n > 1 and len(m_idx) > 0 and len(set(m_idx) | set(j_idx)) < n
        srcs.append(off + m_idx)
        dsts.append(off + j_idx)
        tes.append(len(m_idx))
        off += n
    assert isolated   # a multi-box tower with edges and a node that has none
    pos = (np.concatenate(raws) / D.RELATION_THRESHOLD).astype(np.float32)
    tgt = np.random.default_rng(3).integers(0, 2, size=off).astype(np.float32)
    c = dict(params=O.random_params(4), obj=pos, prop=np.zeros((off, 100), np.float32), tgt=tgt,
             src=np.concatenate(srcs).astype(np.int64), dst=np.concatenate(dsts).astype(np.int64), S=3, B=len(sizes), N=0)
    _assert_margins(c, sizes=sizes)
    return c, np.array(sizes, np.int32), np.array(tes, np.int32)


def test_ragged_batch_in_packed_order():
    """Case 4: a packed plan (towers reordered): the result goes back through to_input_order; single-box
    towers and nodes without edges get the object encoder's part alone."""
    c, sizes, tes = _ragged_case()
    batch = TowerBatch.from_edges(c["obj"], sizes, c["src"].astype(np.int32), c["dst"].astype(np.int32), tes,
                                  device="cuda", pack=True)
    assert batch.node_perm is not None and not np.array_equal(batch.node_perm, np.arange(batch.n_nodes))
    ref, g_ref, _ = _oracle(c)
    _, g, _, dobj = _engine(c, batch, "x6", tgt=batch.to_plan_order(c["tgt"]))
    dobj = batch.to_input_order(dobj)
    _close("ragged packed x6", dobj, ref, g, g_ref)
    assert dobj[0, 0] == 0.0 and dobj[0, 2] != 0.0   # the single-box tower: no edge term, a width term


def test_receiver_block_plan():
    """Case 5: a receiver-block plan — a node's out-edges lie in other nodes' blocks of its tile."""
    c = _case("recv")
    batch = TowerBatch.fully_connected(c["obj"], c["prop"], device="cuda", recv_blocks=True)
    assert batch.flags & _lib.BATCH_RECV_BLOCKS
    ref, g_ref, _ = _oracle(c, "recv")
    _, g, _, dobj = _engine(c, batch, "x6")
    _close("receiver blocks x6", dobj, ref, g, g_ref)


def test_bf16_math_wide_kernels():
    """Case 6: bf16 math stores dz1 as bf16; the kernel widens it on load. (a) translation invariance;
    (b) the relative L2 error against the fp64 oracle is at most twice that of the same run's rm.0 kernel
    gradient — both are fp32 linear maps of the same bf16-stored dz1 rows, and that gradient comes from a
    kernel of the parent commit. Measured on MI355X: DESIGN.md §3zj."""
    c = _case("wide")
    ref, g_ref, _ = _oracle(c, "wide")
    with E.wide_kernels():
        batch = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], c["prop"], device="cuda", nw_max=16)
        _, g, _, dobj = _engine(c, batch, "bf16")
    _tower_x_sums("wide bf16", dobj, np.full(c["B"], c["N"]))
    k = P.from_flat(g)["rm.0.kernel"].astype(np.float64)
    l2_obj = np.linalg.norm(dobj - ref) / np.linalg.norm(ref)
    l2_rm0 = np.linalg.norm(k - g_ref["rm.0.kernel"]) / np.linalg.norm(g_ref["rm.0.kernel"])
    print(f"bf16: relative L2 error dobj {l2_obj:.3e}, rm.0.kernel gradient {l2_rm0:.3e}")
    assert l2_obj <= 2 * l2_rm0


def test_deterministic_and_every_row_written(monkeypatch):
    """Case 7: 64 thresholded six-box towers, dropout 0.1, on a poisoned workspace and output: two runs
    agree bitwise; no element is NaN or the poison pattern."""
    monkeypatch.setattr(E, "POISON_WORKSPACE", True)
    obj, Rs, Rr, _, tgt = D.synthetic_batch(64, 6, seed=5, fully_connected=False)
    c = dict(params=O.random_params(2), tgt=tgt, S=5)
    batch = TowerBatch.from_dense(obj, Rs, Rr, None, device="cuda")
    a = _engine(c, batch, "x6", dropout=0.1, seed=99)[3]
    b = _engine(c, batch, "x6", dropout=0.1, seed=99)[3]
    assert a.shape == (64 * 6, 3) and np.isfinite(a).all()
    assert not (a.view(np.uint32) == 0xFFFFFFFF).any()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.abs(a).max() > 0


def test_autograd_objects_leaf():
    """Case 8: objects as a leaf tensor of the module (here fp64 on the CPU): the gradient arrives in
    the caller's shape, device and dtype; the parameter gradient is bitwise that of a run without it."""
    c = _case("team_b")
    net = GraphNetwork(mp_steps=c["S"], dropout=0.0, device="cuda", params=c["params"])
    net.train()
    obj_t = torch.tensor(c["obj"], dtype=F64, requires_grad=True)
    z = net.forward_logits(obj_t, c["Rs"], c["Rr"], c["prop"])
    assert z.shape == c["obj"].shape[:2]
    z.sum().backward()
    assert obj_t.grad is not None and obj_t.grad.shape == obj_t.shape
    assert obj_t.grad.dtype == F64 and obj_t.grad.device.type == "cpu"
    ref, _, z_ref = _oracle(c, "team_b/sum", loss="sum")
    assert np.abs(z.detach().cpu().numpy().reshape(-1) - z_ref).max() <= 1e-5
    _close("autograd sum(z)", obj_t.grad.numpy().reshape(-1, 3), ref)
    flat_grad = net.flat.grad.clone()
    net.flat.grad = None
    net.forward_logits(torch.tensor(c["obj"]), c["Rs"], c["Rr"], c["prop"]).sum().backward()
    assert torch.equal(net.flat.grad, flat_grad)


def test_stability_gradients():
    """Case 9: demolish.stability_gradients on three five-box candidates: the sums are stability_sums',
    the gradient is the oracle's d Σ sigmoid(z) / d raw towers."""
    raw = D.synthetic_towers(3, 5, seed=22)
    obj = (raw / D.RELATION_THRESHOLD).astype(np.float32)
    Rs, Rr = D.relation_matrices(raw, None)
    e = np.array(O.dense_to_edges(Rs, Rr), np.int64).reshape(-1, 4)
    c = dict(params=O.random_params(2), obj=obj, prop=np.zeros((3, 5, 100), np.float32), tgt=None,
             src=e[:, 0] * 5 + e[:, 2], dst=e[:, 0] * 5 + e[:, 3], S=5, B=3, N=5)
    _assert_margins(c)
    net = GraphNetwork(mp_steps=5, device="cuda", params=c["params"])
    sums, grads = demolish.stability_gradients(net, raw)
    assert grads.shape == (3, 5, 3)
    want = demolish.stability_sums(net, raw)
    print("stability sums:", sums.tolist(), "inference:", want.tolist())
    assert torch.equal(sums, want)
    ref, _, z_ref = _oracle(c, loss="sum_prob")
    # the oracle's leaf is objects = raw / 170 (as fp32): d/d raw = d/d objects / 170
    _close("stability_gradients", grads.cpu().numpy().reshape(-1, 3), ref / D.RELATION_THRESHOLD)
    with pytest.raises(ValueError):
        demolish.stability_gradients(net, raw, mode="max")


def test_errors():
    """Case 10: no backward on the workspace → SpwgnnError; an inference run → SPWGNN_E_NOTRAIN."""
    c = _case("team_b")
    batch = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], None, device="cuda")
    flat = P.to_flat(c["params"], device="cuda")
    ws = E.Workspace("cuda")
    run = E.RunConfig(c["S"], training=True)
    z = E.forward(flat, batch, run, ws)
    with pytest.raises(_lib.SpwgnnError, match="needs the backward"):
        E.backward_inputs(flat, batch, run, ws)
    E.backward(flat, batch, run, ws, torch.ones_like(z))
    E.backward_inputs(flat, batch, run, ws)
    E.forward(flat, batch, run, ws)   # a new forward discards what the backward left
    with pytest.raises(_lib.SpwgnnError, match="needs the backward"):
        E.backward_inputs(flat, batch, run, ws)
    infer = E.RunConfig(c["S"], training=False)
    with pytest.raises(_lib.SpwgnnError, match="status -6"):
        E.backward_inputs(flat, batch, infer, ws)
    import ctypes as C
    b, r = batch.cstruct(), infer.cstruct()
    out = torch.zeros(batch.n_nodes, 4, device="cuda")
    st = _lib.lib().spwgnn_backward_inputs(flat.data_ptr(), C.byref(b), C.byref(r), ws.buf.data_ptr(), ws.buf.numel(),
                                           out.data_ptr(), 0)
    assert st == _lib.E_NOTRAIN
    torch.cuda.synchronize()
