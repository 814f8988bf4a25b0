"""GPU: relation gates on the small-batch kernels — the gated team kernels (k_edge_fwd_team, k_edge_bwd_team,
k_dA_team, k_bwd_enc_pair_team) and the gated fused step loops (k_fwd_fused_team, k_bwd_fused_team), DESIGN.md §3zzb.

The team forms compute the wide kernels' products in the wide kernels' order, so a gated call on them must equal
the gated call on the wide kernels (`engine.wide_kernels()`) BIT FOR BIT: logits, final state, every gradient, dprop,
`backward_inputs` and `backward_relations`, in x6, x3 and h3. Every case first asserts, through
`engine.fused_path(gated=True)`, which launches it took.

Shapes: the team cases of tests/test_gpu_input_grad.py; the packed ragged batch (1, 2, 4, 7, 3 boxes) with a null
propagation input; two fully connected 12-box towers (5 blocks per wave-tile, past the 4 blocks whose dA sums the
fused backward keeps in LDS: the rebuild's team body runs) — also with the team limit at the wave-tile count (the
per-phase team edge kernels beside wide encoders and the wide rebuild) and as a receiver-block plan (no fused loop:
the whole per-phase team chain with k_dA_team); one 16-node wave-tile of two 8-box towers (4 blocks: both operand
buffers, the LDS dA sums).

Oracle parity at the criteria of tests/test_gpu_relation_gates.py: logits |Δ| <= 1e-5 + 1e-5·|z|, every tensor
max|Δ| <= 1e-5·max|ref| + 1e-8; gates and margins as there (tests/test_relation_gates_host.py holds team_a's gated
ReLU margins above TAU)."""
import numpy as np
import pytest
import torch

import relation_gates_ref as GR
import test_gpu_input_grad as IG
import test_gpu_relation_gates as RG
from oracle import model as O
from spwgnn_amd import TowerBatch, _lib, data as D, engine as E

pytestmark = pytest.mark.gpu

DEV = "cuda"
SPLIT = ["x6", "x3", "h3"]


# ------------------------------------------------------------------------------------ inputs
def _towers(B, N, seed, S=3):
    """B fully connected N-box towers with a non-zero propagation input, in the form of IG._case."""
    obj, Rs, Rr, prop, tgt = D.synthetic_batch(B, N, seed=seed, fully_connected=True)
    prop = np.random.default_rng(seed).normal(0, 0.3, prop.shape).astype(np.float32)
    return dict(params=O.random_params(seed + 1), obj=obj, Rs=Rs, Rr=Rr, prop=prop, tgt=tgt, S=S, B=B, N=N)


_BUILT = {}


def _shape(name):
    """name → (case dict, batch, targets in plan order, the fused-path bits it must take, team limit or None)."""
    if name in _BUILT:
        return _BUILT[name]
    limit = None
    if name in ("team_a", "team_b"):
        c = IG._case(name)
        batch, want = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], c["prop"], device=DEV), 3
    elif name == "ragged":
        c, sizes, tes = IG._ragged_case()
        batch = TowerBatch.from_edges(c["obj"], sizes, c["src"].astype(np.int32), c["dst"].astype(np.int32), tes,
                                      device=DEV, pack=True)
        assert batch.prop is None and batch.node_perm is not None
        want = 3
    elif name in ("tall", "tall_phases", "tall_recv"):
        c = _towers(2, 12, 21)
        if name == "tall_recv":   # a receiver-block plan: no fused loop, every phase its own team launch
            batch, want = TowerBatch.fully_connected(c["obj"], c["prop"], device=DEV, recv_blocks=True), 0
            assert batch.flags & _lib.BATCH_RECV_BLOCKS
        else:
            batch = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], c["prop"], device=DEV)
            blocks = batch.wtile.cpu().numpy().reshape(-1, 4)[:, 1]
            assert batch.n_wtiles == 2 and np.all(blocks == 5)      # past kTeamDaBlocks = 4
            want = 3
            if name == "tall_phases":   # team tiles, but edge blocks past the limit: no fused loop, no team encoders
                limit, want = batch.n_wtiles, 0
                assert batch.n_eblocks > limit
    elif name == "pair16":
        c = _towers(2, 8, 22)
        batch = TowerBatch.from_dense(c["obj"], c["Rs"], c["Rr"], c["prop"], device=DEV, nw_max=16)
        assert batch.n_wtiles == 1 and batch.n_eblocks == 4 and batch.n_nodes == 16
        want = 3
    else:
        raise ValueError(name)
    tgt = batch.to_plan_order(np.asarray(c["tgt"], np.float32).reshape(-1))
    _BUILT[name] = (c, batch, tgt, want, limit)
    return _BUILT[name]


class _team_limit:
    """The library's team limit set to `n` (None: left alone) inside the block."""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        self.prev = E.team_max_blocks(self.n) if self.n is not None else None

    def __exit__(self, *exc):
        if self.n is not None:
            E.team_max_blocks(self.prev)
        return False


def _gates(batch, fill=0.0, seed=GR.GATE_SEED):
    return batch.edge_gates(torch.as_tensor(GR.gates_for(batch.n_edges, seed), device=DEV), fill=fill)


SHAPES = ["team_a", "team_b", "ragged", "tall", "tall_phases", "tall_recv", "pair16"]


# ------------------------------------------------------------------------------------ 1. team / fused == wide, bit for bit
@pytest.mark.parametrize("math", SPLIT)
@pytest.mark.parametrize("name", SHAPES)
def test_gated_team_run_is_the_gated_wide_run(name, math):
    c, batch, tgt, want, limit = _shape(name)
    run = E.RunConfig(c["S"], training=True, math=math)
    gates = _gates(batch)
    dstate = torch.as_tensor(np.random.default_rng(3).normal(0, 0.1, (batch.n_nodes, 100)).astype(np.float32), device=DEV)
    with _team_limit(limit):
        assert E.fused_path(batch, run, gated=True) == want == E.fused_path(batch, run)
        assert E.fused_path(batch, E.RunConfig(c["S"], training=False, math=math), gated=True) == (want & 1)
        team = RG._run(c, batch, math, gates, tgt=tgt, state=True, dstate=dstate)
    with E.wide_kernels():
        assert E.fused_path(batch, run, gated=True) == 0
        wide = RG._run(c, batch, math, gates, tgt=tgt, state=True, dstate=dstate)
    assert E.team_max_blocks() == 512
    RG._bits_equal(f"{name} {math} team vs wide", team, wide)
    assert bool(torch.isfinite(team["z"]).all()) and float(team["g"].abs().max()) > 0 and float(team["drel"].abs().max()) > 0
    pad = (batch.edge_src < 0) | (batch.edge_dst < 0)
    assert bool((team["drel"][pad] == 0).all())


def test_gates_change_the_team_result():
    """The gates are read: against unit gates the logits and the gradients move (x6, the fused loops)."""
    c, batch, tgt, want, _ = _shape("team_a")
    ones = batch.edge_gates(torch.ones(batch.n_edges, device=DEV))
    a = RG._run(c, batch, "x6", _gates(batch), tgt=tgt)
    b = RG._run(c, batch, "x6", ones, tgt=tgt)
    assert not torch.equal(a["z"], b["z"]) and not torch.equal(a["g"], b["g"])


# ------------------------------------------------------------------------------------ 2. parity with the fp64 oracle
@pytest.mark.parametrize("math", ["x6", "h3"])
def test_oracle_parity_on_the_fused_loops(math):
    c, batch, tgt, want, _ = _shape("team_a")
    assert E.fused_path(batch, E.RunConfig(c["S"], training=True, math=math), gated=True) == 3
    gate = GR.gates_for(len(c["src"]))
    gates = RG._slot_gates(c, batch, gate)
    for loss in ("bce", "sum_prob"):
        ref = GR.oracle(c, gate, loss, key="team_a")
        RG._check(f"team_a fused {math} {loss}", c, batch, RG._run(c, batch, math, gates, loss), ref)


# ------------------------------------------------------------------------------------ 3. padding, inference
@pytest.mark.parametrize("name", ["team_a", "ragged", "tall_recv"])
def test_nan_in_the_padding_slots_changes_nothing(name):
    c, batch, tgt, want, _ = _shape(name)
    assert int(((batch.edge_src < 0) | (batch.edge_dst < 0)).sum()) > 0
    clean = RG._run(c, batch, "x6", _gates(batch, 0.0), tgt=tgt, state=True)
    dirty = RG._run(c, batch, "x6", _gates(batch, float("nan")), tgt=tgt, state=True)
    RG._bits_equal(f"{name} NaN padding", dirty, clean)
    assert bool(torch.isfinite(dirty["z"]).all()) and bool(torch.isfinite(dirty["g"]).all())


@pytest.mark.parametrize("math", SPLIT)
def test_inference_forward_is_the_training_forward(math):
    """Dropout 0: the inference instantiation of the gated fused loop gives the training one's logits and state."""
    c, batch, tgt, want, _ = _shape("pair16")
    gates = _gates(batch)
    train = RG._run(c, batch, math, gates, tgt=tgt, state=True)
    infer = RG._run(c, batch, math, gates, state=True, training=False)
    RG._bits_equal(f"pair16 {math} inference", infer, train, keys=("z", "state"))


def test_errors():
    c, batch, tgt, want, _ = _shape("team_a")
    for math in ("f32", "bf16"):
        with pytest.raises(_lib.SpwgnnError):
            E.fused_path(batch, E.RunConfig(c["S"], training=True, math=math), gated=True)
