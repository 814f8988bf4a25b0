"""CPU: DropEdge (spwgnn_dropedge_gates / spwgnn_dropedge_keep_host, within ABI 8) — the key
against its numpy restatement (tests/dropedge_ref.py, from oracle.dropout's mix32 / row_key with kind 3), the
statuses that come back before any device work, and the Trainer's control flow with an fp64 oracle engine on the
gated oracle (tests/relation_gates_ref.py): which gates reach which call, which key draws them, and two optimizer
steps against a hand-rolled fp64 loop."""
import ctypes as C

import numpy as np
import pytest
import torch

import dropedge_ref as REF
import relation_gates_ref as GR
from oracle import model as O
from spwgnn_amd import _lib, data as D, engine as E, params as P
from spwgnn_amd.batch import TowerBatch
from spwgnn_amd.trainer import Trainer, dropout_key
from test_distributed import OracleEngine
from test_eval_host import EvalOracleEngine

F64 = torch.float64
ALMOST_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))   # the largest float below 1
SYM, RESCALE = _lib.DROPEDGE_SYMMETRIC, _lib.DROPEDGE_RESCALE


# ------------------------------------------------------------------------------------ the key
@pytest.mark.parametrize("rate", [0.0, 0.25, ALMOST_ONE])
@pytest.mark.parametrize("flags", [0, SYM, RESCALE, SYM | RESCALE])
def test_keep_host_equals_the_numpy_restatement(rate, flags):
    lib = _lib.lib()
    keys = [0, 1, 0xFFFFFFFF, 1 << 32, 0x9E3779B97F4A7C15, (1 << 64) - 1, dropout_key(7, 3, 1, 2)]
    towers = [0, 1, 31, 65535, 65536, (1 << 31) - 1]
    ab = [(a, b) for a in (0, 1, 5, 31) for b in (0, 2, 5, 30)]
    a, b = np.array([p[0] for p in ab]), np.array([p[1] for p in ab])
    kept = 0
    for key in keys:
        for tw in towers:
            want = REF.keep(key, np.full(len(ab), tw), a, b, rate, bool(flags & SYM))
            got = np.array([lib.spwgnn_dropedge_keep_host(key, tw, int(x), int(y), rate, flags) for x, y in ab])
            assert np.array_equal(got, want.astype(np.int64)), (hex(key), tw)
            kept += int(got.sum())
            if flags & SYM:   # both directions of a contact share their fate
                back = np.array([lib.spwgnn_dropedge_keep_host(key, tw, int(y), int(x), rate, flags) for x, y in ab])
                assert np.array_equal(got, back)
    n = len(keys) * len(towers) * len(ab)
    if rate == 0.0:
        assert kept == n                      # rate 0 keeps all
    elif rate == 0.25:
        assert 0.65 * n < kept < 0.85 * n     # 672 draws at p = 0.75: ± 6 sigma
    else:
        assert kept < 0.01 * n


def test_asymmetric_directions_draw_separately():
    """Without SYMMETRIC the two directions of a contact are two draws: over many contacts some disagree."""
    lib = _lib.lib()
    pairs = [(t, a, b) for t in range(40) for a in range(4) for b in range(a + 1, 5)]
    differ = sum(lib.spwgnn_dropedge_keep_host(5, t, a, b, 0.5, 0) != lib.spwgnn_dropedge_keep_host(5, t, b, a, 0.5, 0)
                 for t, a, b in pairs)
    assert 0.35 * len(pairs) < differ < 0.65 * len(pairs)


def test_kind_3_is_independent_of_the_dropout_masks():
    """The draw is feature 0 of a kind-3 row key: the kind-1 and kind-2 row keys of the same (tower, a, b) differ."""
    from oracle import dropout as DR
    tw, a, b = np.arange(50), np.arange(50) % 7, np.arange(50) % 5
    k3 = DR.row_key(99, 3, tw, a, b)
    assert not np.any(k3 == DR.row_key(99, 1, tw, a, b)) and not np.any(k3 == DR.row_key(99, 2, tw, a, b))


def _structs():
    b = _lib.BatchC()
    b.n_towers, b.n_nodes, b.n_wtiles, b.n_eblocks, b.nw_max, b.flags = 2, 12, 2, 2, 6, 0
    fake = 0x1000
    b.pos = b.node_tower = b.node_local = b.wtile = b.edge_src = b.edge_dst = b.blk_csr = fake
    r = _lib.RunC()
    r.mp_steps, r.training, r.dropout, r.math = 3, 1, 0.0, _lib.MATH_X6
    return b, r, fake


def test_exports_and_statuses_without_a_device():
    """Every refusal returns before any device work: the pointers here are never followed (no accepted call is made)."""
    lib = _lib.lib()
    assert hasattr(lib, "spwgnn_dropedge_gates") and hasattr(lib, "spwgnn_dropedge_keep_host")
    assert lib.spwgnn_version() == 8 and _lib.K_DROPEDGE == 16
    b, r, fake = _structs()
    call = lambda bb, rr, rate, flags, base, gates: lib.spwgnn_dropedge_gates(
        C.byref(bb) if bb is not None else None, C.byref(rr) if rr is not None else None, rate, flags, base, gates, None)
    for rate in (float("nan"), -0.1, 1.0, 1.5, float("inf")):
        assert call(b, r, rate, SYM, None, fake) == _lib.E_ARG
        assert lib.spwgnn_dropedge_keep_host(1, 0, 0, 1, rate, 0) == _lib.E_ARG
    assert call(None, r, 0.25, SYM, None, fake) == _lib.E_ARG
    assert call(b, None, 0.25, SYM, None, fake) == _lib.E_ARG
    assert call(b, r, 0.25, SYM, None, None) == _lib.E_ARG
    for off in (4, 8, 12):
        assert call(b, r, 0.25, SYM, None, fake + off) == _lib.E_ARG       # gates: 16-byte aligned
    assert call(b, r, 0.25, SYM, fake + 2, fake) == _lib.E_ARG             # base: a float pointer
    assert call(b, r, 0.25, 4, None, fake) == _lib.E_ARG                   # an unknown flag
    assert lib.spwgnn_dropedge_keep_host(1, 0, 0, 1, 0.25, 8) == _lib.E_ARG
    for field in ("edge_src", "edge_dst", "node_tower", "node_local"):
        bad, _, _ = _structs()
        setattr(bad, field, None)
        assert call(bad, r, 0.25, SYM, None, fake) == _lib.E_ARG
    rd = _lib.RunC()
    rd.seed_dev = fake + 4
    assert call(b, rd, 0.25, SYM, None, fake) == _lib.E_ARG                # the device key word: 8-byte aligned
    bad, _, _ = _structs()
    bad.n_eblocks = 0
    assert call(bad, r, 0.25, SYM, None, fake) == _lib.E_SHAPE
    with pytest.raises(ValueError):
        E.check_dropedge(1.0)
    with pytest.raises(ValueError):
        E.check_dropedge(float("nan"))


def test_fused_path_gated_answers_without_a_device():
    """spwgnn_fused_path_gated: spwgnn_fused_path's bits for a gated call — the same launches in the split maths,
    SPWGNN_E_SHAPE where gates are refused, the ungated query's statuses otherwise. No pointer is followed."""
    lib = _lib.lib()
    b, r, _ = _structs()
    for math in (_lib.MATH_X6, _lib.MATH_X3, _lib.MATH_H3):
        r.math = math
        for training in (0, 1):
            r.training = training
            want = lib.spwgnn_fused_path(C.byref(b), C.byref(r))
            assert lib.spwgnn_fused_path_gated(C.byref(b), C.byref(r)) == want == (3 if training else 1)
        prev = lib.spwgnn_team_max_blocks(0)      # the wide kernels for the process: no fused loop, gated or not
        try:
            assert lib.spwgnn_fused_path_gated(C.byref(b), C.byref(r)) == 0 == lib.spwgnn_fused_path(C.byref(b), C.byref(r))
        finally:
            lib.spwgnn_team_max_blocks(prev)
    for math in (_lib.MATH_F32, _lib.MATH_BF16):
        r.math = math
        assert lib.spwgnn_fused_path_gated(C.byref(b), C.byref(r)) == _lib.E_SHAPE
        assert lib.spwgnn_fused_path(C.byref(b), C.byref(r)) >= 0
    r.math = 99
    assert lib.spwgnn_fused_path_gated(C.byref(b), C.byref(r)) == _lib.E_ARG
    assert lib.spwgnn_fused_path_gated(None, C.byref(r)) == _lib.E_ARG


# ------------------------------------------------------------------------------------ the Trainer's control flow
B, N, S, RATE, SEED = 4, 5, 2, 0.25, 3


def _problem():
    obj, Rs, Rr, prop, tgt = D.synthetic_batch(B, N, seed=9, fully_connected=False)
    return obj, Rs, Rr, tgt


class GatedOracleEngine(EvalOracleEngine):
    """The fp64 oracle engine with the optional protocol methods of DropEdge: `dropedge_gates` (the numpy
    restatement on the batch's slot arrays) and ``gates=`` on forward / backward (the gated oracle). Logs every call."""

    def __init__(self):
        super().__init__()
        self.log = []

    def dropedge_gates(self, batch, run, rate, symmetric=True, rescale=False, base=None):
        g = torch.from_numpy(REF.batch_gates(batch, run.seed, rate, symmetric, rescale, base))
        self.log.append(("mask", run.seed, g))
        return g

    def forward(self, flat, batch, run, **kw):
        self.log.append(("fwd", run.training, kw))
        if "gates" not in kw:
            return super().forward(flat, batch, run)
        _, _, w = batch.edges_to_input(kw["gates"])   # slot order → the order of batch.src / batch.dst
        self.p = self._params(flat)
        src, dst = torch.as_tensor(batch.src, dtype=torch.long), torch.as_tensor(batch.dst, dtype=torch.long)
        self.z, _ = GR.forward(self.p, batch.pos[:, :3].to(F64), src, dst, torch.zeros(batch.n_nodes, 100, dtype=F64),
                               run.mp_steps, torch.as_tensor(w, dtype=F64))
        return self.z.detach()

    def backward(self, flat, batch, run, dlogits, **kw):
        self.log.append(("bwd", run.training, kw))
        return super().backward(flat, batch, run, dlogits)


def _trainer(dropedge=RATE, **kw):
    params = P.to_flat(O.random_params(11), dtype=F64)
    tr = Trainer(params, engine=GatedOracleEngine(), mp_steps=S, dropout=0.0, seed=SEED, dropedge=dropedge, **kw)
    tr.m, tr.v = torch.zeros_like(params), torch.zeros_like(params)
    return tr


def _batch(sl=slice(0, B), tower_ids=None):
    obj, Rs, Rr, tgt = _problem()
    e = np.array(O.dense_to_edges(Rs[sl], Rr[sl]), np.int64).reshape(-1, 4)
    n = obj[sl].shape[0]
    src, dst = (e[:, 0] * N + e[:, 2]).astype(np.int32), (e[:, 0] * N + e[:, 3]).astype(np.int32)
    te = np.bincount(e[:, 0], minlength=n).astype(np.int32)
    batch = TowerBatch.from_edges(obj[sl].reshape(-1, 3), np.full(n, N, np.int32), src, dst, te, None, "cpu",
                                  tower_ids=tower_ids)
    return batch, torch.tensor(tgt[sl].reshape(-1), dtype=F64)


def test_the_backward_receives_the_forwards_gates_and_the_key_is_the_steps():
    tr = _trainer()
    batch, tgt = _batch()
    tr.step([batch, batch], [tgt, tgt])
    tr.step(batch, tgt)
    log = tr.engine.log
    kinds = [e[0] for e in log]
    assert kinds == ["mask", "fwd", "bwd"] * 3
    for k in range(3):
        mask, fwd, bwd = log[3 * k:3 * k + 3]
        assert fwd[2]["gates"] is mask[2] and bwd[2]["gates"] is mask[2]     # the same tensor, forward and backward
    # the key: (seed, iteration, rank, micro-batch) — the feature dropout's, drawn with kind 3
    assert [e[1] for e in log[0::3]] == [dropout_key(SEED, 0, 0, 0), dropout_key(SEED, 0, 0, 1), dropout_key(SEED, 1, 0, 0)]
    m00, m01, m10 = (e[2].numpy() for e in log[0::3])
    assert not np.array_equal(m00, m01) and not np.array_equal(m00, m10) and not np.array_equal(m01, m10)
    active = np.asarray(batch.edge_id) >= 0
    for m in (m00, m01, m10):   # 0 / 1 gates, both present, the padding 0
        assert set(np.unique(m[active])) == {0.0, 1.0} and np.all(m[~active] == 0.0)
    tr2 = _trainer()
    tr2.rank = 1                # another rank of the same step draws another mask
    tr2.step(batch, tgt)
    assert tr2.engine.log[0][1] == dropout_key(SEED, 0, 1, 0) and not np.array_equal(tr2.engine.log[0][2].numpy(), m00)


def test_rescale_and_relation_weights_reach_the_mask():
    tr = _trainer(dropedge_rescale=True, dropedge_symmetric=False)
    batch, tgt = _batch()
    w = torch.linspace(0.5, 1.5, batch.n_edges)
    tr.step(batch, tgt, relation_weights=w)
    got = tr.engine.log[0][2].numpy()
    base = batch.edge_gates(w)
    want = REF.batch_gates(batch, dropout_key(SEED, 0, 0, 0), RATE, False, True, base)
    assert np.array_equal(got, want)
    kept = got[np.asarray(batch.edge_id) >= 0] != 0
    assert kept.any() and not kept.all()
    assert np.array_equal(got[np.asarray(batch.edge_id) >= 0][kept],
                          (base.numpy() * REF.scale(RATE, True))[np.asarray(batch.edge_id) >= 0][kept])
    # a slot tensor is taken as it is; without DropEdge the weights alone are the gates
    tr0 = _trainer(dropedge=0.0)
    tr0.step(batch, tgt, relation_weights=base)
    assert tr0.engine.log[0][0] == "fwd" and tr0.engine.log[0][2]["gates"] is base and tr0.engine.log[1][2]["gates"] is base
    with pytest.raises(ValueError):
        tr0.step([batch, batch], [tgt, tgt], relation_weights=[base])


def test_a_shards_towers_get_the_whole_batchs_masks():
    """The key is tower id + local indices: a shard cut with `tower_ids` draws, under one key, its towers' part of the
    whole batch's mask — whatever its own plan looks like."""
    eng = GatedOracleEngine()
    run = E.RunConfig(S, training=True, seed=dropout_key(SEED, 5, 0, 0))
    whole, _ = _batch()
    shard, _ = _batch(slice(2, 4), tower_ids=np.array([2, 3]))
    unnamed, _ = _batch(slice(2, 4))
    sw, dw, vw = whole.edges_to_input(eng.dropedge_gates(whole, run, RATE))
    ss, ds, vs = shard.edges_to_input(eng.dropedge_gates(shard, run, RATE))
    _, _, vu = unnamed.edges_to_input(eng.dropedge_gates(unnamed, run, RATE))
    sel = sw >= 2 * N
    assert np.array_equal(sw[sel] - 2 * N, ss) and np.array_equal(dw[sel] - 2 * N, ds)
    assert np.array_equal(vw[sel], vs) and 0 < vs.sum() < len(vs)
    assert not np.array_equal(vu, vs)   # the same towers under ids 0, 1: another draw


def test_evaluate_draws_nothing():
    tr = _trainer()
    batch, tgt = _batch()
    tr.evaluate(batch, tgt)
    assert [e[0] for e in tr.engine.log] == ["fwd"] and tr.engine.log[0][1] is False and tr.engine.log[0][2] == {}


def test_dropedge_zero_issues_no_gated_call():
    tr = _trainer(dropedge=0.0)
    batch, tgt = _batch()
    tr.step(batch, tgt)
    tr.step([batch, batch], [tgt, tgt])
    assert [e[0] for e in tr.engine.log] == ["fwd", "bwd"] * 3
    assert all(e[2] == {} for e in tr.engine.log)          # the engine never sees a gates argument
    ref = Trainer(P.to_flat(O.random_params(11), dtype=F64), engine=OracleEngine(), mp_steps=S, dropout=0.0, seed=SEED)
    ref.m, ref.v = torch.zeros_like(ref.params), torch.zeros_like(ref.params)
    ref.step(batch, tgt)
    ref.step([batch, batch], [tgt, tgt])
    assert torch.equal(ref.params, tr.params)


def test_construction_errors():
    params = P.to_flat(O.random_params(11), dtype=F64)
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            Trainer(params, engine=GatedOracleEngine(), dropedge=bad)
    for math in ("f32", "bf16"):     # spwgnn_gates_supported answers 0
        with pytest.raises(ValueError):
            Trainer(params, engine=GatedOracleEngine(), dropedge=0.25, math=math)
    with pytest.raises(ValueError):  # an engine without the optional methods
        Trainer(params, engine=OracleEngine(), dropedge=0.25)
    with pytest.raises(ValueError):  # gated per-step logits are not built
        Trainer(params, engine=GatedOracleEngine(), dropedge=0.25, mp_steps=S, step_loss_weights=(0.5, 1.0))


def test_two_steps_match_a_hand_rolled_fp64_loop():
    tr = _trainer()
    batch, tgt = _batch()
    for _ in range(2):
        tr.step(batch, tgt)
    # by hand: the mask per input edge from the restated key, the gated oracle, the Keras BCE, Adam
    layout = P.layout()
    flat = P.to_flat(O.random_params(11), dtype=F64)
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    src, dst = np.asarray(batch.src, np.int64), np.asarray(batch.dst, np.int64)
    pos = batch.pos[:, :3].to(F64)
    kept_counts = []
    for it in range(2):
        key = dropout_key(SEED, it, 0, 0)
        w = REF.keep(key, src // N, src % N, dst % N, RATE, True).astype(np.float64)
        kept_counts.append(int(w.sum()))
        p = {n: flat[o:o + int(np.prod(s))].reshape(s).clone().requires_grad_(True) for n, o, s in layout}
        z, _ = GR.forward(p, pos, torch.as_tensor(src), torch.as_tensor(dst), torch.zeros(len(pos), 100, dtype=F64), S,
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
    assert all(0 < k < len(src) for k in kept_counts)
    err = float((tr.params - flat).abs().max())
    print(f"two DropEdge steps against the hand-rolled loop: max|Δparam| {err:.2e}")
    assert err <= 1e-12
