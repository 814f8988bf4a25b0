"""Node rows gathered through buffer descriptors in the wide edge-side kernels: the
W2 gradient (`k_w2grad_ws`: U_s[src], V_s[dst], G3_s[dst] through per-step descriptors, the lane's
node offsets and the block's src / dst once per 32-edge block, zero-length U / V descriptors at step
0 of a null 'propagation'), the ≤ 16-node edge forward (A, U, V) and the edge backward (G3). dA's
G3 ring measured slower through descriptors and keeps its pointers.

The conversion is exact — same products, k order and rounding — so every check but the oracle's is
bitwise. Every case runs the wide kernels (team limit 0) on a workspace pre-filled with 0xFF bytes
and NaN-filled outputs, with dropout 0.1. Shapes: the smallest at which the addressing can go wrong —
5 six-box towers (30 nodes: a partial last 32-node block; three wave-tiles, one holding a single
tower), 8 six-box towers (two edge blocks per tile: the once-per-block index reuse crosses block
boundaries inside a tile and between tiles), 5 twelve-box towers, 24 ragged thresholded 4–16-box
towers (padding edges with index −1, blocks with few real edges), 3 towers of 32 boxes (the 32-row
path, which keeps the pointer form in the edge forward / backward). S = 1 makes every U / V gather of
the W2 gradient a zero-length-descriptor one; bf16 math covers the 2-byte U / V offsets.

The range guard's host function (path.hip: gather_desc_fits) has no entry point reachable without a
device; it is covered by reading (one comparison of RN · 152 · 4 against 2^31).
"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import dropout as DR
from oracle import model as O
from spwgnn_amd import TowerBatch, data as D, engine as E, params as P

gpu = pytest.mark.gpu

SHAPES = ["six5", "six8", "twelve", "ragged", "box32"]
PTR_SWITCH = "SPWGNN_GATHER_PTR"   # mask of kernels forced to the 64-bit pointer form (7: all three)
DROPOUT, SEED = 0.1, 5


@functools.lru_cache(maxsize=None)
def _batch(shape: str) -> TowerBatch:
    if shape == "ragged":
        pos, sizes, src, dst, tower_edges, _ = D.ragged_batch(24, 4, 16, seed=7)
        return TowerBatch.from_edges(pos, sizes, src, dst, tower_edges, None, device="cuda")
    T, N = {"six5": (5, 6), "six8": (8, 6), "twelve": (5, 12), "box32": (3, 32)}[shape]
    raw = D.synthetic_towers(T, N, seed=4)
    return TowerBatch.fully_connected((raw / D.RELATION_THRESHOLD).astype(np.float32), device="cuda")


@functools.lru_cache(maxsize=None)
def _flat():
    return P.to_flat(O.random_params(seed=29), device="cuda")


def _targets(batch):
    rng = np.random.default_rng(batch.n_nodes)
    return torch.tensor(rng.integers(0, 2, size=batch.n_nodes).astype(np.float32), device="cuda")


def _prop(batch, zero: bool):
    if zero:
        return torch.zeros(batch.n_nodes, 100, device="cuda")
    rng = np.random.default_rng(3)
    return torch.tensor(rng.normal(0, 0.3, size=(batch.n_nodes, 100)).astype(np.float32), device="cuda")


def _step(batch, S, math, want_dprop=False, flat=None, targets=None):
    """One forward + loss + backward on the wide kernels, 0xFF-filled workspace, NaN-filled outputs;
    (logits, flat gradient, dprop or None, loss) as numpy arrays."""
    flat = _flat() if flat is None else flat
    run = E.RunConfig(S, training=True, math=math, dropout=DROPOUT, seed=SEED)
    with E.wide_kernels():
        assert E.fused_path(batch, run) == 0
        ws = E.Workspace("cuda")
        ws.buf = torch.full((E.workspace_bytes(batch, run),), 0xFF, dtype=torch.uint8, device="cuda")
        z = E.forward(flat, batch, run, ws, logits=torch.full((batch.n_nodes,), float("nan"), device="cuda"))
        out3, dz = E.bce(z, _targets(batch) if targets is None else targets, E.BceScratch("cuda"))
        g = torch.full_like(flat, float("nan"))
        _, dp = E.backward(flat, batch, run, ws, dz, grads=g, want_dprop=want_dprop)
        torch.cuda.synchronize()
    return z.cpu().numpy(), g.cpu().numpy(), None if dp is None else dp.cpu().numpy(), float(out3[0])


class _pointer_form:
    """`with _pointer_form(): ...` — every call inside takes the 64-bit pointer form of all three kernels."""

    def __enter__(self):
        self._prev = os.environ.get(PTR_SWITCH)
        os.environ[PTR_SWITCH] = "7"

    def __exit__(self, *exc):
        if self._prev is None:
            del os.environ[PTR_SWITCH]
        else:
            os.environ[PTR_SWITCH] = self._prev
        return False


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("S", [1, 2, 5])
@pytest.mark.parametrize("math", ["x6", "bf16"])
def test_null_prop_equals_zero_prop(math, S, shape):
    """Test 1: null prop ≡ an all-zero prop array ≡ null prop with dprop requested, on logits, the whole
    flat gradient and dprop: the zero-length descriptors give exactly what the stored zero rows give."""
    base = _batch(shape)
    za, ga, _, _ = _step(base, S, math)
    zb, gb, pb, _ = _step(base.with_prop(_prop(base, zero=True)), S, math, want_dprop=True)
    zc, gc, pc, _ = _step(base, S, math, want_dprop=True)
    assert np.isfinite(zb).all() and np.isfinite(gb).all() and np.isfinite(pb).all()
    assert _same_bits(za, zb) and _same_bits(zc, zb)
    assert np.array_equal(ga, gb) and np.array_equal(gc, gb)   # −0 == +0, as in test_gpu_loop_ends.py
    assert _same_bits(pc, pb)


@gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("S", [1, 2, 5])
@pytest.mark.parametrize("math", ["x6", "bf16"])
def test_nonzero_prop_with_and_without_dprop(math, S, shape):
    """Test 2: with a non-zero prop step 0's descriptors must not be nulled — the runs with and without
    a dprop request agree, and differ from the null-prop run's W2 gradient."""
    b0 = _batch(shape)
    b = b0.with_prop(_prop(b0, zero=False))
    z0, g0, _, _ = _step(b, S, math)
    z1, g1, p1, _ = _step(b, S, math, want_dprop=True)
    assert np.isfinite(g0).all() and np.isfinite(g1).all() and np.isfinite(p1).all()
    assert _same_bits(z0, z1) and _same_bits(g0, g1)
    _, gn, _, _ = _step(b0, S, math)
    w2 = P.from_flat(torch.from_numpy(g0))["rmp.1.kernel"]
    assert not np.array_equal(w2, P.from_flat(torch.from_numpy(gn))["rmp.1.kernel"])


@gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("S", [1, 2, 5])
@pytest.mark.parametrize("math", ["x6", "bf16"])
@pytest.mark.parametrize("prop", ["null", "nonzero"])
def test_pointer_form_equals_descriptor_form(prop, math, S, shape):
    """Test 3: the forced pointer form (the range guard's fallback) ≡ the descriptor form, bitwise."""
    b = _batch(shape)
    if prop == "nonzero":
        b = b.with_prop(_prop(b, zero=False))
    zd, gd, pd, _ = _step(b, S, math, want_dprop=True)
    with _pointer_form():
        zp, gp, pp, _ = _step(b, S, math, want_dprop=True)
    assert np.isfinite(gd).all() and np.isfinite(pd).all()
    assert _same_bits(zd, zp) and _same_bits(gd, gp) and _same_bits(pd, pp)


@gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("math", ["x6", "bf16"])
def test_two_runs_are_bitwise_equal(math, shape):
    """Test 5: deterministic — two runs give the same bits."""
    b = _batch(shape)
    z0, g0, _, _ = _step(b, 5, math)
    z1, g1, _, _ = _step(b, 5, math)
    assert np.isfinite(g0).all()
    assert _same_bits(z0, z1) and _same_bits(g0, g1)


# ---- Test 4: x6 against the fp64 oracle (tests/test_gpu_chain_parity.py's criterion: per tensor
# max|Δ| ≤ 1e-5·max|g| and relative L2 ≤ 5e-6; logits 1e-5 + 1e-5·|z|; loss 1e-5), on the six-box and
# ragged shapes with the engine's dropout masks. Towers with a ReLU pre-activation within TAU of its
# kink in the oracle (oracle.model.relu_margins_gather) are left out as there: candidates are drawn
# with a quarter to spare, the first n_keep kink-free ones are kept, and the seeds are chosen so that
# the oracle alone leaves out at most a quarter of the candidates at every S (checked on the CPU).
TAU = 1e-6
GRAD_MAX_REL, GRAD_L2_REL = 1e-5, 5e-6
ORACLE_CASES = {"six8": dict(cand=10, keep=8, towers=2, params=7), "ragged": dict(cand=32, keep=24, towers=5, params=7)}
ORACLE_S = [1, 2, 5]


def _candidates(shape):
    c = ORACLE_CASES[shape]
    if shape == "ragged":
        pos, sizes, src, dst, te, _ = D.ragged_batch(c["cand"], 4, 16, seed=c["towers"])
    else:
        N = 6
        raw = D.synthetic_towers(c["cand"], N, seed=c["towers"])
        pos = (raw / D.RELATION_THRESHOLD).astype(np.float32).reshape(-1, 3)
        m_idx, j_idx = np.nonzero(~np.eye(N, dtype=bool))
        base = (np.arange(c["cand"], dtype=np.int64) * N)[:, None]
        src, dst = (base + m_idx[None]).reshape(-1).astype(np.int32), (base + j_idx[None]).reshape(-1).astype(np.int32)
        sizes, te = np.full(c["cand"], N, np.int32), np.full(c["cand"], N * (N - 1), np.int32)
    return pos, np.asarray(sizes, np.int32), src, dst, np.asarray(te, np.int32)


def _masks(sizes, src, dst, te, tower_ids):
    """The engine's dropout masks (rows keyed by tower id and the boxes' indices within the tower)."""
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(DROPOUT))
    et = np.repeat(np.arange(len(sizes)), te)
    kr = DR.row_key(SEED, 1, tower_ids[et], src - off[et], dst - off[et])
    nt = np.repeat(np.arange(len(sizes)), sizes)
    ko = DR.row_key(SEED, 2, tower_ids[nt], np.arange(off[-1]) - off[nt], np.full(off[-1], 0xFFFF))
    return DR.keep(kr, 150, DROPOUT).astype(np.float32) * scale, DR.keep(ko, 100, DROPOUT).astype(np.float32) * scale


def _slice(pos, sizes, src, dst, te, keep):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    eoff = np.concatenate([[0], np.cumsum(te)]).astype(np.int64)
    n_rows = np.concatenate([np.arange(off[t], off[t + 1]) for t in keep])
    e_rows = np.concatenate([np.arange(eoff[t], eoff[t + 1]) for t in keep])
    new_off = np.concatenate([[0], np.cumsum(sizes[keep])]).astype(np.int64)
    shift = np.repeat(new_off[:-1] - off[keep], te[keep])
    return (pos[n_rows], sizes[keep], (src[e_rows] + shift).astype(np.int32), (dst[e_rows] + shift).astype(np.int32),
            te[keep], n_rows, e_rows)


@functools.lru_cache(maxsize=None)
def _oracle_case(shape, S):
    c = ORACLE_CASES[shape]
    params = O.random_params(seed=c["params"])
    pos, sizes, src, dst, te = _candidates(shape)
    T = len(sizes)
    dr, do = _masks(sizes, src, dst, te, np.arange(T))
    marg = O.relu_margins_gather(O.to_torch(params), pos, src, dst, np.zeros((len(pos), 100)),
                                 np.repeat(np.arange(T), sizes), T, S, drop_r=dr, drop_o=do)
    ok = np.nonzero(marg > TAU)[0]
    left_out = T - len(ok)
    keep = ok[:c["keep"]]
    kpos, ksz, ksrc, kdst, kte, n_rows, e_rows = _slice(pos, sizes, src, dst, te, keep)
    tgt = np.random.default_rng(12).integers(0, 2, size=len(kpos)).astype(np.float32)
    ref = O.loss_and_grads(params, kpos, None, None, np.zeros((len(kpos), 100)), tgt, S, form="gather",
                           src=ksrc.astype(np.int64), dst=kdst.astype(np.int64), drop_r=dr[e_rows], drop_o=do[n_rows])
    return dict(params=params, left_out=left_out, cand=T, keep=keep, edges=(kpos, ksz, ksrc, kdst, kte), tgt=tgt, ref=ref)


@pytest.mark.parametrize("shape", sorted(ORACLE_CASES))
@pytest.mark.parametrize("S", ORACLE_S)
def test_oracle_seeds_leave_most_towers_in(S, shape):
    """(CPU) The fp64 oracle alone: at the chosen seeds at most a quarter of the candidate towers sit
    within TAU of a kink, the kept batch has the shape's tower count, and every gradient is non-zero."""
    c = _oracle_case(shape, S)
    assert 4 * c["left_out"] <= c["cand"], (c["left_out"], c["cand"])
    assert len(c["keep"]) == ORACLE_CASES[shape]["keep"]
    loss, z, g = c["ref"]
    assert np.isfinite(loss) and np.isfinite(np.asarray(z)).all()
    for k, v in g.items():
        assert np.isfinite(v).all() and np.abs(v).max() > 0, k


@gpu
@pytest.mark.parametrize("shape", sorted(ORACLE_CASES))
@pytest.mark.parametrize("S", ORACLE_S)
def test_descriptor_form_matches_oracle(S, shape):
    c = _oracle_case(shape, S)
    kpos, ksz, ksrc, kdst, kte = c["edges"]
    batch = TowerBatch.from_edges(kpos, ksz, ksrc, kdst, kte, None, device="cuda", tower_ids=c["keep"])
    tgt = torch.tensor(batch.to_plan_order(c["tgt"]), device="cuda")
    z, g, _, loss = _step(batch, S, "x6", flat=P.to_flat(c["params"], device="cuda"), targets=tgt)
    z = batch.to_input_order(z)
    loss_r, z_r, g_r = c["ref"]
    z_r = np.asarray(z_r).reshape(-1)
    dz = np.abs(z - z_r)
    print(f"{shape} S={S}: max|dz| {dz.max():.3e} loss {loss:.7f} (oracle {float(loss_r):.7f})")
    assert np.all(dz <= 1e-5 + 1e-5 * np.abs(z_r))
    assert abs(loss - float(loss_r)) < 1e-5
    got = P.from_flat(torch.from_numpy(g))
    for k, r in g_r.items():
        d = got[k].astype(np.float64) - r
        rel_max, rel_l2 = np.abs(d).max() / np.abs(r).max(), np.linalg.norm(d) / np.linalg.norm(r)
        print(f"{k:14s} max|dg|/max|g| {rel_max:.3e} rel-L2 {rel_l2:.3e}")
        assert rel_max <= GRAD_MAX_REL and rel_l2 <= GRAD_L2_REL, (k, rel_max, rel_l2)
