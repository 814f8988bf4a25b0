"""GPU: relation gradients — `engine.backward_relations` (spwgnn_backward_relations, k_rel_bwd), `GraphNetwork.
relation_gradients` and `demolish.relation_gradients` — against fp64 torch autograd through the gated oracle
(tests/relation_grad_ref.py: a scalar gate on every message of the receiver sum of Networks.py:88, the
gates as leaves, taken at gate ≡ 1). DESIGN.md §3zy.

Inputs: the shapes, data seeds and parameter seeds of tests/test_gpu_input_grad.py (its case builders are
imported), picked there so that every tower's ReLU margin exceeds 1e-6; each case asserts the margins again.

Criterion (f32, x6 and h3 math): max|got − ref| <= 1e-5·max|ref| + 1e-8, the project's gradient criterion.
x3 and bf16: the relative L2 error is at most 2× that of the same run's rmp.1.kernel gradient against the same
reference — that gradient comes from a kernel of the parent commit and is bilinear in the same stored rows
(factor 2: the precedent of test_gpu_input_grad.py case 6).
Measured on MI355X (r_k relative L2 / rmp.1.kernel relative L2): see DESIGN.md §3zy.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

import relation_grad_ref as RR
import test_gpu_input_grad as IG
from oracle import dropout as DR
from oracle import model as O
from spwgnn_amd import GraphNetwork, TowerBatch, _lib, data as D, demolish, engine as E, params as P

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
EXACT = ["f32", "x6", "h3"]


# ------------------------------------------------------------------------------------ reference
_REFS = {}


def _ref(c, key, loss, drop_r=None, drop_o=None):
    """(r (Ne,), r_steps (S, Ne), parameter gradients) of the case, edges in the order of c["src"] / c["dst"]."""
    k = None if key is None else (key, loss)
    if k is not None and k in _REFS:
        return _REFS[k]
    r, steps, g, _ = RR.relation_grads(c["params"], c["obj"], c["src"], c["dst"], c["prop"], c["S"], c["tgt"], loss,
                                       drop_r, drop_o)
    assert np.abs(r).max() > 0
    if k is not None:
        _REFS[k] = (r, steps, g)
    return r, steps, g


# ------------------------------------------------------------------------------------ engine
def _engine(c, batch, math, loss="bce", tgt=None, dropout=0.0, seed=0, relations=True, inputs=False, first="rel",
            keep_ws=False):
    """One training step's forward + loss + backward, then backward_relations (and backward_inputs, in the
    order `first` says). Returns a dict of device tensors."""
    flat = P.to_flat(c["params"], device="cuda")
    ws = E.Workspace("cuda")
    run = E.RunConfig(c["S"], training=True, math=math, dropout=dropout, seed=seed)
    z = E.forward(flat, batch, run, ws)
    if loss == "bce":
        t = torch.as_tensor(np.asarray(c["tgt"] if tgt is None else tgt, np.float32), device="cuda").reshape(-1)
        _, dz = E.bce(z, t, E.BceScratch("cuda"))
    else:
        p = E.sigmoid(z)
        dz = p * (1.0 - p)
    g, dp = E.backward(flat, batch, run, ws, dz, want_dprop=batch.prop is not None)
    out = dict(z=z, g=g, dp=dp, flat=flat, run=run, ws=ws)
    before = ws.buf.clone() if keep_ws else None
    for what in (("rel", "inp") if first == "rel" else ("inp", "rel")):
        if what == "rel" and relations:
            out["drel"], out["steps"] = E.backward_relations(flat, batch, run, ws, per_step=True)
        if what == "inp" and inputs:
            out["dobj"] = E.backward_inputs(flat, batch, run, ws).clone()
    torch.cuda.synchronize()
    if keep_ws:
        out["ws_equal"] = torch.equal(before, ws.buf)
    return out


def _to_ref_order(c, batch, values):
    """Slot values → the order of the reference's edge list (matched by the (sender, receiver) pair)."""
    s, d, v = batch.edges_to_input(values)
    nn = batch.n_nodes
    got_key, ref_key = s * nn + d, np.asarray(c["src"], np.int64) * nn + np.asarray(c["dst"], np.int64)
    assert len(np.unique(ref_key)) == len(ref_key) and np.array_equal(np.sort(got_key), np.sort(ref_key))
    pos = np.argsort(got_key, kind="stable")[np.searchsorted(np.sort(got_key), ref_key)]
    return v[..., pos]


def _padding_is_zero(batch, out):
    pad = (batch.edge_src < 0) | (batch.edge_dst < 0)
    assert out["drel"].shape == (32 * batch.n_eblocks,) and out["steps"].shape == (out["run"].mp_steps, 32 * batch.n_eblocks)
    assert bool((out["drel"][pad] == 0).all()) and bool((out["steps"][:, pad] == 0).all())


def _close(what, got, ref):
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    msg = f"{what}: max|got - ref| {err:.3e} = {err / scale:.2e} of max|ref| {scale:.3e}"
    print(msg)
    assert err <= 1e-5 * scale + 1e-8, msg


def _check_exact(what, c, batch, out, ref):
    """drel and every drel_steps row meet the criterion; Σ_s drel_steps = drel to 1e-6 of the max."""
    r, steps, _ = ref
    _padding_is_zero(batch, out)
    drel, dsteps = out["drel"].cpu().numpy(), out["steps"].cpu().numpy()
    _close(what + " r_k", _to_ref_order(c, batch, drel), r)
    got_steps = _to_ref_order(c, batch, dsteps)
    for s in range(c["S"]):   # each row against its own maximum
        err, scale = np.abs(got_steps[s] - steps[s]).max(), np.abs(steps[s]).max()
        assert err <= 1e-5 * scale + 1e-8, (what, s, err, scale)
    assert np.abs(dsteps.astype(np.float64).sum(0) - drel).max() <= 1e-6 * np.abs(drel).max()


# ------------------------------------------------------------------------------------ cases
@pytest.mark.parametrize("math", EXACT)
@pytest.mark.parametrize("name", ["team_a", "team_b"])
def test_oracle_parity_team_path(name, math):
    """Small thresholded batches on the team (small-batch, fused) kernels, BCE and Σ sigmoid(z)."""
    c = IG._case(name)
    batch = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], c["prop"], device="cuda")
    assert E.team_max_blocks() == 512 and batch.n_eblocks <= 512
    for loss in ("bce", "sum_prob"):
        _check_exact(f"{name} {math} {loss}", c, batch, _engine(c, batch, math, loss), _ref(c, name, loss))


@pytest.mark.parametrize("math", EXACT)
def test_oracle_parity_wide_kernels(math):
    """The wide (large-batch) kernels on a fully connected batch whose wave-tiles span more than one block."""
    c = IG._case("wide")
    with E.wide_kernels():
        batch = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], c["prop"], device="cuda", nw_max=16)
        assert batch.n_eblocks > batch.n_wtiles
        outs = {loss: _engine(c, batch, math, loss) for loss in ("bce", "sum_prob")}
    for loss, out in outs.items():
        _check_exact(f"wide {math} {loss}", c, batch, out, _ref(c, "wide", loss))


@pytest.mark.parametrize("math", EXACT)
def test_receiver_block_plan(math):
    """A receiver-block plan: every node owns one block of its in-edges."""
    c = IG._case("recv")
    batch = TowerBatch.fully_connected(c["obj"], c["prop"], device="cuda", recv_blocks=True)
    assert batch.flags & _lib.BATCH_RECV_BLOCKS
    for loss in ("bce", "sum_prob"):
        _check_exact(f"recv {math} {loss}", c, batch, _engine(c, batch, math, loss), _ref(c, "recv", loss))


_RAGGED = []


@pytest.mark.parametrize("math", EXACT)
def test_ragged_batch_in_packed_order(math):
    """Towers of 1, 2, 4, 7 and 3 boxes in a packed plan with a null propagation input (step 0 reads no U, V
    row): the single-box tower has no edge and one node has none; node ids go back through node_perm."""
    if not _RAGGED:
        _RAGGED.append(IG._ragged_case())
    c, sizes, tes = _RAGGED[0]
    batch = TowerBatch.from_edges(c["obj"], sizes, c["src"].astype(np.int32), c["dst"].astype(np.int32), tes,
                                  device="cuda", pack=True)
    assert batch.node_perm is not None and batch.prop is None
    assert tes[0] == 0 and len(np.union1d(c["src"], c["dst"])) < batch.n_nodes - 1
    for loss in ("bce", "sum_prob"):
        out = _engine(c, batch, math, loss, tgt=batch.to_plan_order(c["tgt"]))
        _check_exact(f"ragged packed {math} {loss}", c, batch, out, _ref(c, "ragged", loss))


def test_dropout_on():
    """The committed dropout fixture's inputs, rate and seed; the oracle multiplies the engine's masks in."""
    g = np.load(os.path.join(GOLDEN, "golden_dropout_N6_B2_S5.npz"))
    B, N = g["objects"].shape[:2]
    rate, seed = float(g["rate"]), int(g["seed"])
    e = np.array(O.dense_to_edges(g["Rs"], g["Rr"]), np.int64).reshape(-1, 4)
    c = dict(params=dict(np.load(os.path.join(GOLDEN, "golden_params.npz"))), obj=g["objects"], Rs=g["Rs"], Rr=g["Rr"],
             prop=g["prop"], tgt=g["target"], src=e[:, 0] * N + e[:, 2], dst=e[:, 0] * N + e[:, 3], S=int(g["mp_steps"]),
             B=B, N=N)
    drop_r = DR.relation_mask(seed, rate, B, N)[e[:, 0], e[:, 1]]
    drop_o = DR.object_mask(seed, rate, B, N).reshape(-1, 100)
    IG._assert_margins(c, drop_r, drop_o, assert_tau=False)   # given inputs (test_gpu_input_grad.py): printed
    batch = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], None, device="cuda")
    out = _engine(c, batch, "x6", dropout=rate, seed=seed)
    _check_exact("dropout fixture x6", c, batch, out, _ref(c, None, "bce", drop_r, drop_o))


@pytest.mark.parametrize("name", ["wide", "team_b"])
@pytest.mark.parametrize("math", ["x3", "bf16"])
def test_lower_precision_maths(math, name):
    """x3 and bf16 (bf16 on the wide kernels stores A, U, V and g as bf16, on the team kernels A alone; the
    kernel widens them on load): relative L2 error at most 2× the same run's rmp.1.kernel gradient's."""
    c = IG._case(name)
    r, _, g_ref = _ref(c, name, "bce")
    if name == "wide":
        with E.wide_kernels():
            batch = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], c["prop"], device="cuda", nw_max=16)
            out = _engine(c, batch, math)
    else:
        batch = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], c["prop"], device="cuda")
        out = _engine(c, batch, math)
    _padding_is_zero(batch, out)
    got = _to_ref_order(c, batch, out["drel"].cpu().numpy())
    k = P.from_flat(out["g"])["rmp.1.kernel"].astype(np.float64)
    l2_rel = np.linalg.norm(got - r) / np.linalg.norm(r)
    l2_w2 = np.linalg.norm(k - g_ref["rmp.1.kernel"]) / np.linalg.norm(g_ref["rmp.1.kernel"])
    print(f"{math} {name}: relative L2 error r_k {l2_rel:.3e}, rmp.1.kernel gradient {l2_w2:.3e}, ratio {l2_rel / l2_w2:.2f}")
    assert l2_rel <= 2 * l2_w2


@pytest.mark.parametrize("math,name", [("x6", "team_a"), ("x6", "wide"), ("bf16", "wide")])
def test_no_side_effects(math, name):
    """The parameter gradients, d/d'propagation' and the backward_inputs result are bitwise those of a run
    that never calls backward_relations, in either call order; the workspace bytes do not change; a second
    call gives the first one's bits."""
    c = IG._case(name)
    with (E.wide_kernels() if name == "wide" else contextlib.nullcontext()):
        batch = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], c["prop"], device="cuda",
                                      nw_max=16 if name == "wide" else None)
        base = _engine(c, batch, math, relations=False, inputs=True)
        a = _engine(c, batch, math, inputs=True, first="rel", keep_ws=True)
        b = _engine(c, batch, math, inputs=True, first="inp", keep_ws=True)
        again = E.backward_relations(b["flat"], batch, b["run"], b["ws"])
        torch.cuda.synchronize()
    for o in (a, b):
        assert o["ws_equal"]
        assert torch.equal(o["g"], base["g"]) and torch.equal(o["dp"], base["dp"]) and torch.equal(o["dobj"], base["dobj"])
    assert torch.equal(a["drel"], b["drel"]) and torch.equal(a["steps"], b["steps"]) and torch.equal(again, b["drel"])


def test_deterministic_and_every_slot_written(monkeypatch):
    """64 thresholded six-box towers, dropout 0.1, on a poisoned workspace and poisoned outputs: two runs
    agree bitwise; every slot is written; padding slots are exactly 0; no NaN or poison pattern."""
    monkeypatch.setattr(E, "POISON_WORKSPACE", True)
    obj, Rs, Rr, _, tgt = D.synthetic_batch(64, 6, seed=5, fully_connected=False)
    c = dict(params=O.random_params(2), tgt=tgt, S=5)
    batch = TowerBatch.from_dense(obj, Rs, Rr, None, device="cuda")
    a = _engine(c, batch, "x6", dropout=0.1, seed=99)
    b = _engine(c, batch, "x6", dropout=0.1, seed=99)
    _padding_is_zero(batch, a)
    assert bool(((batch.edge_src < 0).sum() > 0))   # the plan has padding slots
    for k in ("drel", "steps"):
        x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
        assert np.isfinite(x).all() and not (x.view(np.uint32) == 0xFFFFFFFF).any()
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert float(a["drel"].abs().max()) > 0


def _candidates():
    raw = D.synthetic_towers(3, 5, seed=22)
    obj = (raw / D.RELATION_THRESHOLD).astype(np.float32)
    Rs, Rr = D.relation_matrices(raw, None)
    e = np.array(O.dense_to_edges(Rs, Rr), np.int64).reshape(-1, 4)
    c = dict(params=O.random_params(2), obj=obj, Rs=Rs, Rr=Rr, prop=np.zeros((3, 5, 100), np.float32), tgt=None,
             src=e[:, 0] * 5 + e[:, 2], dst=e[:, 0] * 5 + e[:, 3], slots=e, S=5, B=3, N=5)
    IG._assert_margins(c)
    return raw, c


def test_demolish_relation_gradients():
    """Three five-box candidates: the sums are stability_sums'; the (C, N, N) [sender, receiver] matrix is
    the oracle's d Σ sigmoid(z) / d gate, zero on the diagonal."""
    raw, c = _candidates()
    net = GraphNetwork(mp_steps=5, device="cuda", params=c["params"])
    sums, rel = demolish.relation_gradients(net, raw)
    assert torch.equal(sums, demolish.stability_sums(net, raw)) and tuple(rel.shape) == (3, 5, 5)
    assert rel.device.type == "cuda" and rel.dtype == torch.float32
    rel = rel.cpu().numpy()
    r, _, _ = _ref(c, "candidates", "sum_prob")
    want = np.zeros((3, 5, 5))
    want[c["slots"][:, 0], c["slots"][:, 2], c["slots"][:, 3]] = r
    _close("demolish.relation_gradients", rel, want)
    assert all(rel[b, i, i] == 0 for b in range(3) for i in range(5))
    with pytest.raises(ValueError):
        demolish.relation_gradients(net, raw, mode="max")


def test_graph_network_relation_gradients():
    """A tensor shaped like receiver_relations: r_k at [b, dst_k, k], exact zeros everywhere else — for
    thresholded relation matrices with inactive columns, the default loss, a dlogits and a callable."""
    c = IG._case("team_b")
    net = GraphNetwork(mp_steps=c["S"], dropout=0.0, device="cuda", params=c["params"])
    e = c["slots"]   # (tower, column, sender, receiver) of the active columns
    assert len(e) < c["Rr"].shape[0] * c["Rr"].shape[2]   # some columns are inactive
    def bce(z):
        return O.keras_bce_from_logits(z.double(), torch.as_tensor(c["tgt"], dtype=torch.float64, device=z.device).reshape(z.shape))

    for loss, kw in (("sum_prob", {}), ("sum", dict(dlogits=torch.ones(c["B"], c["N"]))), ("bce", dict(loss=bce))):
        got = net.relation_gradients(c["obj"], c["Rs"], c["Rr"], c["prop"], **kw)
        assert tuple(got.shape) == c["Rr"].shape
        got = got.cpu().numpy()
        r, _, _ = _ref(c, "team_b", loss)
        want = np.zeros(c["Rr"].shape)
        want[e[:, 0], e[:, 3], e[:, 1]] = r
        _close(f"GraphNetwork.relation_gradients {loss}", got, want)
        assert np.all(got[want == 0] == 0) and np.all(got[c["Rr"] == 0] == 0)


def test_errors():
    """No backward on the workspace → SpwgnnError, after a new forward the same; an inference run → −6."""
    c = IG._case("team_b")
    batch = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], None, device="cuda")
    flat = P.to_flat(c["params"], device="cuda")
    ws = E.Workspace("cuda")
    run = E.RunConfig(c["S"], training=True)
    z = E.forward(flat, batch, run, ws)
    with pytest.raises(_lib.SpwgnnError, match="needs the backward"):
        E.backward_relations(flat, batch, run, ws)
    E.backward(flat, batch, run, ws, torch.ones_like(z))
    E.backward_relations(flat, batch, run, ws)
    with pytest.raises(ValueError):
        E.backward_relations(flat, batch, run, ws, drel=torch.zeros(32 * batch.n_eblocks + 1, device="cuda"))
    E.forward(flat, batch, run, ws)   # a new forward discards what the backward left
    with pytest.raises(_lib.SpwgnnError, match="needs the backward"):
        E.backward_relations(flat, batch, run, ws)
    infer = E.RunConfig(c["S"], training=False)
    with pytest.raises(_lib.SpwgnnError, match="status -6"):
        E.backward_relations(flat, batch, infer, ws)
    b, r = batch.cstruct(), infer.cstruct()
    out = torch.zeros(32 * batch.n_eblocks, device="cuda")
    st = _lib.lib().spwgnn_backward_relations(flat.data_ptr(), C.byref(b), C.byref(r), ws.buf.data_ptr(), ws.buf.numel(),
                                              out.data_ptr(), None, 0)
    assert st == _lib.E_NOTRAIN
    torch.cuda.synchronize()
