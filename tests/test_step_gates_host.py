"""CPU: the host side of the per-step relation gates and layer-wise DropEdge (spwgnn_forward_step_gated /
spwgnn_backward_step_gated / spwgnn_dropedge_step_gates / spwgnn_dropedge_keep_host_step, within ABI 8; DESIGN.md
§3zzc) — exports and the statuses that come back before any device work, `edge_step_gates` against a loop over
`edge_gates`, the per-step draw of the DropEdge key, the fp64 identities of the oracle the GPU tests rest on, the ReLU
margins of every GPU case under its per-step gates, the separation of the two mutants the GPU criteria must catch
(gate rows rotated by one step; row 0 at every step), and the Trainer's control flow with an fp64 oracle engine."""
import ctypes as C

import numpy as np
import pytest
import torch

import dropedge_ref as DREF
import relation_gates_ref as GR
import relation_grad_ref as RR
import step_gates_ref as SR
import test_dropedge_host as DH
from oracle import dropout as DR
from oracle import model as O
from spwgnn_amd import _lib, batch as BT, data as D, engine as E, params as P
from spwgnn_amd.trainer import Trainer, dropout_key

F64 = torch.float64
MATHS = {"f32": _lib.MATH_F32, "x6": _lib.MATH_X6, "bf16": _lib.MATH_BF16, "x3": _lib.MATH_X3, "h3": _lib.MATH_H3}
SYM, RESCALE = _lib.DROPEDGE_SYMMETRIC, _lib.DROPEDGE_RESCALE


# ------------------------------------------------------------------------------------ the C ABI
def _structs(training=1, math=_lib.MATH_X6):
    """A well-formed batch / run pair whose pointers are never followed (every status below comes back first)."""
    b = _lib.BatchC()
    b.n_towers, b.n_nodes, b.n_wtiles, b.n_eblocks, b.nw_max, b.flags = 2, 12, 2, 2, 6, 0
    fake = 0x1000
    b.pos = b.node_tower = b.node_local = b.wtile = b.edge_src = b.edge_dst = b.blk_csr = fake
    r = _lib.RunC()
    r.mp_steps, r.training, r.dropout, r.math = 3, training, 0.0, math
    return b, r, fake


def _ref(x):
    return C.byref(x) if x is not None else None


def _fwd(lib, params, b, r, ws, nbytes, gates, step, logits, state=None):
    return lib.spwgnn_forward_step_gated(params, _ref(b), _ref(r), ws, nbytes, gates, step, logits, state, None)


def _bwd(lib, params, b, r, ws, nbytes, gates, step, dlogits, dstate, grads, dprop=None):
    return lib.spwgnn_backward_step_gated(params, _ref(b), _ref(r), ws, nbytes, gates, step, dlogits, dstate, grads,
                                          dprop, None)


def test_exports_and_version():
    lib = _lib.lib()
    for name in ("spwgnn_forward_step_gated", "spwgnn_backward_step_gated", "spwgnn_dropedge_step_gates",
                 "spwgnn_dropedge_keep_host_step"):
        assert hasattr(lib, name)
    assert lib.spwgnn_version() == 8 == _lib.ABI_VERSION
    # new symbols only: the struct sizes of before
    assert [lib.spwgnn_struct_size(k) for k in range(15)] == [88, 64, 12, 24, 24, -1, 112, 32, -1, 264, 64, -1, 80, -1, -1]


def test_statuses_without_a_device():
    """Every argument error returns before any device work: the pointers here are never followed. One byte short of
    the workspace is the last check, so SPWGNN_E_WORKSPACE stands for "every argument was accepted"."""
    lib = _lib.lib()
    b, r, fake = _structs()
    slots = 32 * b.n_eblocks
    need = lib.spwgnn_workspace_bytes(b.n_nodes, b.n_eblocks, r.mp_steps, 1)
    short = need - 1
    for step in (slots, slots + 4, slots + 64):   # the smallest stride and padded rows
        assert _fwd(lib, fake, b, r, fake, short, fake, step, fake) == _lib.E_WORKSPACE
        assert _bwd(lib, fake, b, r, fake, short, fake, step, fake, None, fake) == _lib.E_WORKSPACE
    # a bad gate_step: shorter than the plan's slots, not a multiple of 4 (a row would lose its 16-byte alignment)
    for step in (0, -4, slots - 4, slots - 1, slots + 1, slots + 2, slots + 3, 4):
        assert _fwd(lib, fake, b, r, fake, need, fake, step, fake) == _lib.E_ARG, step
        assert _bwd(lib, fake, b, r, fake, need, fake, step, fake, None, fake) == _lib.E_ARG, step
    # misaligned gate, state and state-cotangent pointers
    for off in (4, 8, 12):
        assert _fwd(lib, fake, b, r, fake, need, fake + off, slots, fake) == _lib.E_ARG
        assert _bwd(lib, fake, b, r, fake, need, fake + off, slots, fake, None, fake) == _lib.E_ARG
    assert _fwd(lib, fake, b, r, fake, need, fake, slots, fake, fake + 4) == _lib.E_ARG
    assert _bwd(lib, fake, b, r, fake, need, fake, slots, fake, fake + 4, fake) == _lib.E_ARG
    # the arguments of spwgnn_forward_state / spwgnn_backward_state, checked as there
    assert _fwd(lib, None, b, r, fake, need, fake, slots, fake) == _lib.E_ARG
    assert _fwd(lib, fake, b, r, fake, need, fake, slots, None) == _lib.E_ARG
    assert _fwd(lib, fake, b, r, None, need, fake, slots, fake) == _lib.E_ARG
    assert _fwd(lib, fake, None, r, fake, need, fake, slots, fake) == _lib.E_ARG
    assert _fwd(lib, fake, b, None, fake, need, fake, slots, fake) == _lib.E_ARG
    assert _bwd(lib, fake, b, r, fake, need, fake, slots, None, None, fake) == _lib.E_ARG
    assert _bwd(lib, fake, b, r, fake, need, fake, slots, fake, None, None) == _lib.E_ARG
    bi, ri, _ = _structs(training=0)
    assert _bwd(lib, fake, bi, ri, fake, need, fake, slots, fake, None, fake) == _lib.E_NOTRAIN
    need_inf = lib.spwgnn_workspace_bytes(bi.n_nodes, bi.n_eblocks, ri.mp_steps, 0)
    assert _fwd(lib, fake, bi, ri, fake, need_inf - 1, fake, slots, fake) == _lib.E_WORKSPACE   # inference takes them too
    bad, _, _ = _structs()
    bad.n_eblocks = 0
    assert _fwd(lib, fake, bad, r, fake, need, fake, slots, fake) == _lib.E_SHAPE


@pytest.mark.parametrize("math", sorted(MATHS))
def test_maths_and_null_gates(math):
    """f32 / bf16: SPWGNN_E_SHAPE right after validate, whatever else is wrong. NULL gates: the state call's status,
    gate_step not looked at."""
    lib = _lib.lib()
    b, r, fake = _structs(math=MATHS[math])
    slots = 32 * b.n_eblocks
    need = lib.spwgnn_workspace_bytes(b.n_nodes, b.n_eblocks, r.mp_steps, 1)
    want = _lib.E_WORKSPACE if lib.spwgnn_gates_supported(MATHS[math]) == 1 else _lib.E_SHAPE
    assert _fwd(lib, fake, b, r, fake, need - 1, fake, slots, fake) == want
    assert _bwd(lib, fake, b, r, fake, need - 1, fake, slots, fake, None, fake) == want
    if want == _lib.E_SHAPE:   # the math is asked before the call's own arguments
        assert _fwd(lib, None, b, r, fake, need, fake, 3, None) == _lib.E_SHAPE
    for step in (slots, 0, 3, -1):
        for nbytes in (need - 1,):
            assert _fwd(lib, fake, b, r, fake, nbytes, None, step, fake) == \
                lib.spwgnn_forward_state(fake, C.byref(b), C.byref(r), fake, nbytes, fake, None, None) == _lib.E_WORKSPACE
            assert _bwd(lib, fake, b, r, fake, nbytes, None, step, fake, None, fake) == \
                lib.spwgnn_backward_state(fake, C.byref(b), C.byref(r), fake, nbytes, fake, None, fake, None, None) \
                == _lib.E_WORKSPACE
        assert _fwd(lib, None, b, r, fake, need, None, step, fake) == \
            lib.spwgnn_forward_state(None, C.byref(b), C.byref(r), fake, need, fake, None, None) == _lib.E_ARG


def test_dropedge_step_gates_statuses_without_a_device():
    lib = _lib.lib()
    b, r, fake = DH._structs()
    slots = 32 * b.n_eblocks
    call = lambda bb, rr, rate, flags, base, bstep, gates, gstep: lib.spwgnn_dropedge_step_gates(
        _ref(bb), _ref(rr), rate, flags, base, bstep, gates, gstep, None)
    for rate in (float("nan"), -0.1, 1.0, float("inf")):
        assert call(b, r, rate, SYM, None, 0, fake, slots) == _lib.E_ARG
        assert lib.spwgnn_dropedge_keep_host_step(1, 0, 0, 1, 2, rate, 0) == _lib.E_ARG
    assert lib.spwgnn_dropedge_keep_host_step(1, 0, 0, 1, 2, 0.25, 8) == _lib.E_ARG
    assert call(None, r, 0.25, SYM, None, 0, fake, slots) == _lib.E_ARG
    assert call(b, None, 0.25, SYM, None, 0, fake, slots) == _lib.E_ARG
    assert call(b, r, 0.25, SYM, None, 0, None, slots) == _lib.E_ARG
    assert call(b, r, 0.25, 4, None, 0, fake, slots) == _lib.E_ARG
    for gstep in (0, -4, slots - 4, slots + 1, slots + 2):          # rows shorter than the plan, or unaligned rows
        assert call(b, r, 0.25, SYM, None, 0, fake, gstep) == _lib.E_ARG, gstep
    for bstep in (-4, slots - 4, slots + 2, 4):                     # per-step base rows: the same rule
        assert call(b, r, 0.25, SYM, fake, bstep, fake, slots) == _lib.E_ARG, bstep
    for off in (4, 8, 12):
        assert call(b, r, 0.25, SYM, None, 0, fake + off, slots) == _lib.E_ARG
    assert call(b, r, 0.25, SYM, fake + 2, 0, fake, slots) == _lib.E_ARG
    bad, _, _ = DH._structs()
    bad.n_eblocks = 0
    assert call(bad, r, 0.25, SYM, None, 0, fake, slots) == _lib.E_SHAPE
    r0 = _lib.RunC()
    r0.mp_steps = 0
    assert call(b, r0, 0.25, SYM, None, 0, fake, slots) == _lib.E_SHAPE


# ------------------------------------------------------------------------------------ the per-step draw
def _keep_ref(key, tower, a, b, step, rate, symmetric=True):
    """drop_keep(rowkey(key, kind 3, tower, a, b), feature step, thresh) from oracle.dropout's mix32 / row_key."""
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    if symmetric:
        a, b = np.minimum(a, b), np.maximum(a, b)
    rk = DR.row_key(int(key) & 0xFFFFFFFFFFFFFFFF, DREF.KIND, tower, a, b)
    return DR.mix32(rk ^ np.uint64(step)) >= np.uint64(DREF.thresh(rate))


def test_step_zero_is_the_shared_draw_and_steps_follow_the_key():
    keys = [0, 1, 0x9E3779B97F4A7C15, (1 << 64) - 1, dropout_key(7, 3, 1, 2)]
    ab = [(a, b) for a in (0, 1, 5, 31) for b in (0, 2, 5, 30)]
    a, b = np.array([p[0] for p in ab]), np.array([p[1] for p in ab])
    for key in keys:
        for tw in (0, 3, 65536):
            for sym in (True, False):
                shared = [E.dropedge_keep_host(key, tw, x, y, 0.3, symmetric=sym) for x, y in ab]
                assert shared == [E.dropedge_keep_host(key, tw, x, y, 0.3, symmetric=sym, step=0) for x, y in ab]
                for step in (0, 1, 4, 31):
                    got = [E.dropedge_keep_host(key, tw, x, y, 0.3, symmetric=sym, step=step) for x, y in ab]
                    assert got == list(_keep_ref(key, np.full(len(ab), tw), a, b, step, 0.3, sym)), (hex(key), tw, step)
    with pytest.raises(ValueError):
        E.dropedge_keep_host(1, 0, 0, 1, 0.3, step=-1)


def test_rows_differ_and_symmetric_pairs_share_their_draw_per_step():
    """Rate 0.3 on a 6-node fully connected tower, S = 5: the five masks are pairwise different; under `symmetric`
    both directions of a contact share the draw at every step."""
    N, S, key = 6, 5, dropout_key(3, 0, 0, 0)
    pairs = [(a, b) for a in range(N) for b in range(N) if a != b]
    rows = [[E.dropedge_keep_host(key, 0, a, b, 0.3, step=s) for a, b in pairs] for s in range(S)]
    for s in range(S):
        assert 0 < sum(rows[s]) < len(pairs)
        for t in range(s + 1, S):
            assert rows[s] != rows[t], (s, t)
        back = [E.dropedge_keep_host(key, 0, b, a, 0.3, step=s) for a, b in pairs]
        assert back == rows[s]
    asym = [[E.dropedge_keep_host(key, 0, a, b, 0.3, symmetric=False, step=s) for a, b in pairs] for s in range(S)]
    assert any(E.dropedge_keep_host(key, 0, b, a, 0.3, symmetric=False, step=2) != k for (a, b), k in zip(pairs, asym[2]))


# ------------------------------------------------------------------------------------ edge_step_gates
def _plans():
    obj, Rs, Rr, prop, _ = D.synthetic_batch(3, 5, seed=4, fully_connected=False)
    dense = BT.TowerBatch.from_dense(obj, Rs, Rr, prop, device="cpu")
    sizes = [1, 2, 4, 7, 3]
    raws = [D.synthetic_towers(1, n, seed=50 + k)[0] for k, n in enumerate(sizes)]
    srcs, dsts, tes, off = [], [], [], 0
    for raw in raws:
        n = len(raw)
        m, j = np.nonzero(~np.eye(n, dtype=bool))
        srcs.append(off + m), dsts.append(off + j), tes.append(len(m))
        off += n
    pos = (np.concatenate(raws) / D.RELATION_THRESHOLD).astype(np.float32)
    packed = BT.TowerBatch.from_edges(pos, np.array(sizes, np.int32), np.concatenate(srcs).astype(np.int32),
                                      np.concatenate(dsts).astype(np.int32), np.array(tes, np.int32), device="cpu", pack=True)
    assert packed.node_perm is not None and not np.array_equal(packed.node_perm, np.arange(packed.n_nodes))
    obj2, Rs2, Rr2, prop2, _ = D.synthetic_batch(5, 4, seed=6, fully_connected=True)
    return dense, packed, (obj2, Rs2, Rr2, prop2)


def test_edge_step_gates_is_a_loop_over_edge_gates():
    dense, packed, _ = _plans()
    S = 4
    for batch in (dense, packed):
        v = torch.as_tensor(SR.step_gates_for(batch.n_edges, S, 7))
        got = batch.edge_step_gates(v, fill=-2.0)
        assert got.shape == (S, 32 * batch.n_eblocks) and got.dtype == torch.float32 and got.is_contiguous()
        for s in range(S):
            assert torch.equal(got[s], batch.edge_gates(v[s], fill=-2.0))
            _, _, back = batch.edges_to_input(got[s])
            assert np.array_equal(back, v[s].numpy())
    # the dense form [step, tower, sender, receiver]
    B, N = dense.node_shape
    w = torch.as_tensor(np.random.default_rng(2).uniform(0.1, 2.0, (S, B, N, N)).astype(np.float32))
    got = dense.edge_step_gates(w)
    for s in range(S):
        assert torch.equal(got[s], dense.edge_gates(w[s]))
    src, dst = np.asarray(dense.src), np.asarray(dense.dst)
    _, _, back = dense.edges_to_input(got[2])
    assert np.array_equal(back, w[2].numpy()[src // N, src % N, dst % N])
    for bad in (w[0], torch.ones(dense.n_edges), torch.ones(S, dense.n_edges + 1)):
        with pytest.raises(ValueError):
            dense.edge_step_gates(bad)


def test_edge_step_gates_dense_form_through_node_perm():
    _, _, (obj, Rs, Rr, prop) = _plans()
    B, N = obj.shape[:2]
    e = np.array(O.dense_to_edges(Rs, Rr), np.int64).reshape(-1, 4)
    src, dst = (e[:, 0] * N + e[:, 2]).astype(np.int32), (e[:, 0] * N + e[:, 3]).astype(np.int32)
    te = np.bincount(e[:, 0], minlength=B).astype(np.int32)
    plan = BT.HostPlan.build(obj.reshape(-1, 3), np.full(B, N, np.int32), src, dst, te, pack=True)
    w = torch.as_tensor(np.random.default_rng(3).uniform(0.1, 2.0, (3, B, N, N)).astype(np.float32))
    got = plan.edge_step_gates(w)
    for s in range(3):
        assert torch.equal(got[s], plan.edge_gates(w[s]))


def test_autograd_reaches_the_values():
    dense, _, _ = _plans()
    v = torch.ones(3, dense.n_edges, requires_grad=True)
    coef = torch.arange(3 * 32 * dense.n_eblocks, dtype=torch.float32).reshape(3, -1)
    (dense.edge_step_gates(v) * coef).sum().backward()
    for s in range(3):
        _, _, want = dense.edges_to_input(coef[s])
        assert np.array_equal(v.grad[s].numpy(), want)


def test_gates_and_step_gates_are_exclusive():
    with pytest.raises(ValueError, match="mutually exclusive"):
        E._gate_args(None, None, torch.ones(4), torch.ones(2, 4))


# ------------------------------------------------------------------------------------ the oracle's identities
def test_the_reference_forward_is_the_oracle_and_equal_rows_are_the_shared_gates():
    c, _, gates, _ = SR.case("team_b")
    tp = O.to_torch(c["params"])
    src, dst = SR._tensors(c)
    x = torch.as_tensor(np.asarray(c["obj"], np.float64).reshape(-1, 3))
    pr = torch.as_tensor(np.asarray(c["prop"], np.float64).reshape(-1, 100))
    w = torch.as_tensor(gates, dtype=F64)
    with torch.no_grad():
        z, state = SR.forward(tp, x, src, dst, pr, c["S"], w)
        assert torch.equal(z, RR.forward_gather_gated(tp, x, src, dst, pr, c["S"], list(w)))
        z1, s1 = SR.forward(tp, x, src, dst, pr, c["S"], w[:1].expand(c["S"], -1))
        z0, s0 = GR.forward(tp, x, src, dst, pr, c["S"], w[0])
        assert torch.equal(z1, z0) and torch.equal(s1, s0) and not torch.equal(z, z0)


def test_the_gate_gradient_is_relation_grads_at_unit_gates():
    """d loss / d w_{k,s} at w ≡ 1 is r_{k,s} of relation_grad_ref (what k_rel_bwd's drel_steps is held to)."""
    c, _, _, _ = SR.case("team_b")
    ones = np.ones((c["S"], len(c["src"])))
    ref = SR.oracle(c, ones, "bce")
    r, r_steps, g, z = RR.relation_grads(c["params"], c["obj"], c["src"], c["dst"], c["prop"], c["S"], c["tgt"])
    assert np.array_equal(ref["dgate"], r_steps) and np.array_equal(ref["z"], z)


# ------------------------------------------------------------------------------------ margins and mutants
@pytest.mark.parametrize("name", SR.CASES)
def test_margins_and_mutants(name):
    """Every tower's ReLU / BCE-clip margin under the per-step gated forward exceeds TAU (no tower is left out), every
    row holds 0, 1 and −0.5, no two rows are equal — and the two mutant oracles (rows rotated by one step; row 0 at
    every step) miss the GPU criteria in the logits and in at least one gradient tensor, for both losses the GPU
    parity tests use."""
    c, sizes, gates, seed = SR.case(name)
    m = SR.step_gated_margins(c, gates, sizes)
    print(f"{name}: gate seed {seed}, margins min {m.min():.2e} (TAU {SR.TAU:g})")
    assert np.all(m > SR.TAU), m
    assert gates.shape == (c["S"], len(c["src"])) and gates.dtype == np.float32
    for s in range(c["S"]):
        assert list(gates[s, :3]) == [0.0, 1.0, -0.5]
        for t in range(s + 1, c["S"]):
            assert not np.array_equal(gates[s], gates[t])
    for loss in ("bce", "sum_prob"):
        true = SR.oracle(c, gates, loss, key=name)
        for mutate in (SR.rotated, SR.row0):
            mut = SR.oracle(c, mutate(gates), loss)
            dz = np.abs(mut["z"] - true["z"]).max()
            print(f"{name} {loss} {mutate.__name__}: max|dz| {dz:.2e}")
            assert SR.mutant_separated(true, mut), (name, loss, mutate.__name__)
        # the gate gradient itself is indexed by step: the rotated rows' gradient, rotated back, is not the true one
        assert not SR.tensor_within(SR.rotated(true["dgate"]), true["dgate"])


def test_the_x3_gate_sets_keep_the_ungated_distance_to_the_kinks():
    """`pick_x3_gates` (the x3 comparison's gate sets): per layer group the gated forward is no closer to a ReLU kink
    than the ungated one, or farther than X3_EPS; every tower clears TAU. And why it matters: on `wide` with the
    parity tests' gate set, parameters moved by 1e-5 of their size — x3's rounding class — flip a ReLU and move the
    fp64 gradient by more than 1e-3 of its norm, a hundred times the disturbance; a comparison of rounding errors
    cannot be made across that."""
    for name in ("wide", "team_a"):
        c, sizes, _, _ = SR.case(name)
        g, seed = SR.pick_x3_gates(c, sizes)
        floor = SR.step_gated_margins(c, np.ones_like(g), sizes, groups=True)
        m = SR.step_gated_margins(c, g, sizes, groups=True)
        print(f"{name}: x3 gate seed {seed}, kink distances {m} (ungated {floor})")
        assert all(m[k] >= min(floor[k], SR.X3_EPS) for k in floor) and np.all(SR.step_gated_margins(c, g, sizes) > SR.TAU)
        for s in range(c["S"]):
            assert list(g[s, :3]) == [0.0, 1.0, -0.5]
    c, sizes, gates, _ = SR.case("wide")
    flat = lambda o: np.concatenate([o["g"][k].reshape(-1) for k in sorted(o["g"])])
    base = flat(SR.oracle(c, gates, "bce", key="wide"))
    rng = np.random.default_rng(0)
    moved = dict(c, params={k: v * (1 + 1e-5 * rng.standard_normal(v.shape)) for k, v in c["params"].items()})
    jump = float(np.linalg.norm(flat(SR.oracle(moved, gates, "bce")) - base) / np.linalg.norm(base))
    print(f"wide, parity gate set: 1e-5 parameter noise moves the fp64 gradient by {jump:.2e} of its norm")
    assert jump > 1e-3


# ------------------------------------------------------------------------------------ the Trainer's control flow
def _step_mask(batch, key, rate, steps, symmetric=True, rescale=False, base=None):
    """The (S, slots) per-step masks of a batch from the restated key."""
    arr = lambda t: np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, np.int64)
    es, ed, nt, nl = arr(batch.edge_src), arr(batch.edge_dst), arr(batch.node_tower), arr(batch.node_local)
    ok = (es >= 0) & (ed >= 0)
    s, d = np.where(ok, es, 0), np.where(ok, ed, 0)
    rows = []
    for t in range(steps):
        g = np.where(_keep_ref(key, nt[s], nl[s], nl[d], t, rate, symmetric), DREF.scale(rate, rescale), np.float32(0))
        g = g.astype(np.float32)
        if base is not None:
            bb = np.asarray(base, np.float32)
            g = (bb[t] if bb.ndim == 2 else bb) * g
        rows.append(np.where(ok, g, np.float32(0)).astype(np.float32))
    return np.stack(rows)


class StepGatedOracleEngine(DH.GatedOracleEngine):
    """The gated fp64 oracle engine with ``per_step=`` on dropedge_gates and a 2-D gate tensor on forward."""

    def dropedge_gates(self, batch, run, rate, symmetric=True, rescale=False, base=None, per_step=False):
        if not per_step:
            return super().dropedge_gates(batch, run, rate, symmetric, rescale, base)
        g = torch.from_numpy(_step_mask(batch, run.seed, rate, run.mp_steps, symmetric, rescale,
                                        None if base is None else base.numpy()))
        self.log.append(("mask", run.seed, g))
        return g

    def forward(self, flat, batch, run, **kw):
        if "gates" not in kw or kw["gates"].dim() == 1:
            return super().forward(flat, batch, run, **kw)
        self.log.append(("fwd", run.training, kw))
        w = np.stack([batch.edges_to_input(row)[2] for row in kw["gates"]])
        self.p = self._params(flat)
        src, dst = torch.as_tensor(batch.src, dtype=torch.long), torch.as_tensor(batch.dst, dtype=torch.long)
        self.z, _ = SR.forward(self.p, batch.pos[:, :3].to(F64), src, dst, torch.zeros(batch.n_nodes, 100, dtype=F64),
                               run.mp_steps, torch.as_tensor(w, dtype=F64))
        return self.z.detach()


def _trainer(**kw):
    params = P.to_flat(O.random_params(11), dtype=F64)
    tr = Trainer(params, engine=StepGatedOracleEngine(), mp_steps=DH.S, dropout=0.0, seed=DH.SEED, dropedge=DH.RATE, **kw)
    tr.m, tr.v = torch.zeros_like(params), torch.zeros_like(params)
    return tr


def test_trainer_draws_a_mask_per_step_and_hands_it_to_both_calls():
    tr = _trainer(dropedge_per_step=True)
    batch, tgt = DH._batch()
    tr.step([batch, batch], [tgt, tgt])
    w = torch.linspace(0.5, 1.5, batch.n_edges)
    tr.step(batch, tgt, relation_weights=w)
    log = tr.engine.log
    assert [e[0] for e in log] == ["mask", "fwd", "bwd"] * 3
    keys = [dropout_key(DH.SEED, 0, 0, 0), dropout_key(DH.SEED, 0, 0, 1), dropout_key(DH.SEED, 1, 0, 0)]
    for k in range(3):
        mask, fwd, bwd = log[3 * k:3 * k + 3]
        assert mask[1] == keys[k] and fwd[2]["gates"] is mask[2] and bwd[2]["gates"] is mask[2]
        assert mask[2].shape == (DH.S, 32 * batch.n_eblocks)
        base = batch.edge_gates(w).numpy() if k == 2 else None   # relation_weights: the shared base of every row
        assert np.array_equal(mask[2].numpy(), _step_mask(batch, keys[k], DH.RATE, DH.S, base=base))
        assert not np.array_equal(mask[2][0].numpy(), mask[2][1].numpy())
    # row 0 is the shared mask of the same key
    assert np.array_equal(log[0][2][0].numpy(), DREF.batch_gates(batch, keys[0], DH.RATE))
    # per_step False (the default): the call of before, a 1-D mask
    tr1 = _trainer()
    tr1.step(batch, tgt)
    assert tr1.engine.log[0][2].dim() == 1 and np.array_equal(tr1.engine.log[0][2].numpy(), log[0][2][0].numpy())
    # dropedge 0: dropedge_per_step is inert, no gated call
    tr0 = Trainer(P.to_flat(O.random_params(11), dtype=F64), engine=StepGatedOracleEngine(), mp_steps=DH.S, dropout=0.0,
                  seed=DH.SEED, dropedge=0.0, dropedge_per_step=True)
    tr0.step(batch, tgt)
    assert [e[0] for e in tr0.engine.log] == ["fwd", "bwd"] and all(e[2] == {} for e in tr0.engine.log)
    tr.engine.log.clear()
    tr.evaluate(batch, tgt)
    assert [e[0] for e in tr.engine.log] == ["fwd"] and tr.engine.log[0][2] == {}
    assert tr._dropedge_options() == (DH.RATE, True, False, True) and tr1._dropedge_options() == (DH.RATE, True, False)


def test_two_per_step_steps_match_a_hand_rolled_fp64_loop():
    tr = _trainer(dropedge_per_step=True)
    batch, tgt = DH._batch()
    for _ in range(2):
        tr.step(batch, tgt)
    layout = P.layout()
    flat = P.to_flat(O.random_params(11), dtype=F64)
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    src, dst = np.asarray(batch.src, np.int64), np.asarray(batch.dst, np.int64)
    pos = batch.pos[:, :3].to(F64)
    for it in range(2):
        key = dropout_key(DH.SEED, it, 0, 0)
        w = np.stack([[float(E.dropedge_keep_host(key, int(a // DH.N), int(a % DH.N), int(b % DH.N), DH.RATE, step=s))
                       for a, b in zip(src, dst)] for s in range(DH.S)])
        assert not np.array_equal(w[0], w[1]) and 0 < w.sum() < w.size
        p = {n: flat[o:o + int(np.prod(s))].reshape(s).clone().requires_grad_(True) for n, o, s in layout}
        z, _ = SR.forward(p, pos, torch.as_tensor(src), torch.as_tensor(dst), torch.zeros(len(pos), 100, dtype=F64), DH.S,
                          torch.as_tensor(w))
        _, dz = O.keras_bce_grad(z.detach().numpy(), tgt.numpy())
        z.backward(torch.tensor(dz, dtype=F64))
        g = torch.zeros_like(flat)
        for n, o, s in layout:
            g[o:o + int(np.prod(s))] = p[n].grad.reshape(-1)
        t = it + 1
        m = 0.9 * m + 0.1 * g
        v = 0.999 * v + 0.001 * g * g
        flat = flat - 5e-4 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t) * m / (torch.sqrt(v) + 1e-7)
    err = float((tr.params - flat).abs().max())
    print(f"two per-step DropEdge steps against the hand-rolled loop: max|Δparam| {err:.2e}")
    assert err <= 1e-12
