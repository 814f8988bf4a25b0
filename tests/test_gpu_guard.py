"""GPU: the memory contract of include/spwgnn.h — outputs written in full and nothing past them, inputs
const, a workspace of exactly spwgnn_workspace_bytes() — at the shapes where the hand-written row guards of
the kernels decide. Every device buffer of every call comes from a guard-band arena
(tests/guard.py): params, the batch's eight arrays, prop, targets, weights and every cotangent are frozen
inputs; the workspace holds exactly engine.workspace_bytes(); every output and every scratch lies between two
64 KiB bands of sentinel bytes at the alignment the header asks for and no more. `Arena.check` runs after EACH
call, so a failure names the call and the buffer.

Shapes (the towers, the plan, what they reach; asserted with engine.fused_path for the split-bf16 maths):
  box1        one 1-box tower                    n_nodes = 1, no edge, one all-padding block
  pair        one 2-box tower                    2 nodes, 2 edges
  n6x5        5 x 6 fully connected              30 nodes: the fused loops, a node block that is not full
  n31 / n32   one fully connected tower          31 nodes; 32 nodes and 992 edges = 31 blocks exactly, no padding
                                                 slot, a full node block
  n33         a 32-box and a 1-box tower         the second node block holds one row
  e32         towers of 4 and 5 boxes, one tile  12 + 20 = 32 edges: one block without padding
  e33         e32 + a 2-box tower, one of its    33 edges: the second block holds one edge (the removed relation
              two relations removed              is a zeroed column of both Rs and Rr)
  thr9_recv   5 x 9 thresholded, receiver blocks the per-phase team kernels
  thr20       3 x 20 thresholded                 17-32-node tiles (the LDS csr path)
  packed      towers of 4, 7, 12, pack=True      plan order differs from input order
  wide138 / wide_box1 / wide_n33                 the wide kernels (engine.wide_kernels()): 5 node blocks in two
                                                 workgroups, the last partial; a single row; a one-row second block
  fold256 / fold257  32 x 8 boxes (+ a 1-box     either side of the folded-loss switch n <= 256 of
              tower)                             spwgnn_bce_backward
x6 and f32 on every shape, bf16 / x3 / h3 on n6x5, n33 and wide138; S = 1 and 3; dropout 0.1 for x6 on n6x5 and
wide138 (the mask arrays live in the workspace next to the slabs).

Each case makes the same calls twice, once with every buffer from the arena and once with the engine's
default allocations and an ordinary batch, and asserts the same bits in every output: results do not depend
on where the buffers lie. On the shapes new to the suite (box1, pair, n31, n32, n33, e32, e33) x6 and f32 are
also held to the fp64 oracle (forward_dense per group of equal towers; the loss is the mean over all nodes, i.e.
the per-tower oracle with node-count weights) at the project's tolerances: logits and state
1e-5 + 1e-5·|ref|, gradients 1e-5·max|g| + 1e-7 per tensor, loss 1e-5; with x3_emu.kink_free_params and the
oracle's ReLU margins asserted first. The whole file also passes under SPWGNN_POISON_WORKSPACE=1 (arena
workspaces are then 0xFF-filled, as engine.Workspace fills its own).

Entry point -> guarded buffers -> where (calls 1-8 are test_guarded_calls' sequence, run by every case):
  every forward / backward call  params, spwgnn_batch's pos, prop, node_tower, node_local, wtile, edge_src,
                                 edge_dst, blk_csr (frozen), workspace (exact size)          calls 1-7
  spwgnn_forward                 logits                                                      calls 1, 7
  spwgnn_forward_state           logits, state_out                                           calls 1, 7c
  spwgnn_forward_steps           step_logits, state_out                                      call 2
  spwgnn_bce_steps               step_logits, targets, out3s, out3, dlogits, scratch,        call 3 (lw.w, lw.norm_dev:
                                 weights3, total3, total3s                                   n6x5)
  spwgnn_backward_steps          dstep_logits, dstate, grads, dprop                          call 4
  spwgnn_backward_inputs         dpos                                                        call 5
  spwgnn_sigmoid                 logits, probs                                               call 6
  spwgnn_tower_readout           logits, tower_offsets, out                                  call 6
  spwgnn_bce_backward            logits, targets, out3, dlogits, bce_scratch, grads, dprop   call 7 (weights3, total3:
                                                                                             the fold test)
  spwgnn_bce_backward_weighted   the same + lw.w, lw.norm_dev                                call 7 on n6x5
  spwgnn_backward_state          dlogits, dstate, grads, dprop                               call 7c
  spwgnn_backward                dlogits, grads, dprop                                       the fold test
  spwgnn_bce, _bce_accumulate    logits, targets, out3, dlogits, scratch (weights3, total3)  the geometry / fold tests
  spwgnn_bce_weighted            + lw.w, lw.norm_dev                                         the geometry test
  spwgnn_adam                    params, m, v (in place), grads (frozen)                     call 8
  spwgnn_adam_clipped            the same + clip.out4, clip.total4, scratch                  call 8
  spwgnn_step_advance            key_dev, step_dev                                           the replay test
  spwgnn_run.seed_dev, spwgnn_prologue (copy_dst, key, step), spwgnn_copy_in (dev)           the replay test
  spwgnn_accumulate_out3         out3, weights3, total3                                      the replay test
  spwgnn_adam_dev, spwgnn_adam_clipped_dev   + step_dev, lr_table                            the replay test
  spwgnn_plan_device_positions / _dense      tests/test_gpu_plan_device.py's own sentinel test (unchanged)"""
import functools

import numpy as np
import pytest
import torch

import guard as G
import steps_ref as SR
import test_gpu_state as TS
import x3_emu as X
from oracle import model as O
from spwgnn_amd import TowerBatch, _lib, data as D, engine as E, params as P
from spwgnn_amd.batch import HostPlan

pytestmark = pytest.mark.gpu

F64 = torch.float64
DEV = "cuda"
DROP_SEED = 77
CLIPNORM = 1e-3          # call 8's clipnorm; whether or not a case's norm exceeds it, the same buffers are written

#        id           tower sizes        fully   plan      nw_max  wide
SHAPES = {
    "box1":      ((1,),              True,  "dense",  None, False),
    "pair":      ((2,),              True,  "dense",  None, False),
    "n6x5":      ((6,) * 5,          True,  "dense",  None, False),
    "n31":       ((31,),             True,  "dense",  None, False),
    "n32":       ((32,),             True,  "dense",  None, False),
    "n33":       ((32, 1),           True,  "dense",  None, False),
    "e32":       ((4, 5),            True,  "dense",  16,   False),
    "e33":       ((4, 5, 2),         True,  "dense",  16,   False),
    "thr9_recv": ((9,) * 5,          False, "recv",   None, False),
    "thr20":     ((20,) * 3,         False, "dense",  None, False),
    "packed":    ((4, 7, 12),        True,  "packed", None, False),
    "wide138":   ((6,) * 23,         True,  "dense",  None, True),
    "wide_box1": ((1,),              True,  "dense",  None, True),
    "wide_n33":  ((32, 1),           True,  "dense",  None, True),
    "fold256":   ((8,) * 32,         True,  "dense",  None, False),
    "fold257":   ((8,) * 32 + (1,),  True,  "dense",  None, False),
}
# engine.fused_path of a training run in a split-bf16 math: bit 0 the forward's fused loop, bit 1 the backward's
FUSED = {"box1": 3, "pair": 3, "n6x5": 3, "n31": 0, "n32": 0, "n33": 0, "e32": 3, "e33": 3, "thr9_recv": 0, "thr20": 0,
         "packed": 3, "wide138": 0, "wide_box1": 0, "wide_n33": 0, "fold256": 3, "fold257": 3}
# (n_nodes, n_edges, n_eblocks) the table above promises
GEOMETRY = {"box1": (1, 0, 1), "pair": (2, 2, 1), "n6x5": (30, 150, 5), "n31": (31, 930, 30), "n32": (32, 992, 31),
            "n33": (33, 992, 32), "e32": (9, 32, 1), "e33": (11, 33, 2), "wide138": (138, 690, 23),
            "wide_box1": (1, 0, 1), "wide_n33": (33, 992, 32)}
ORACLE_SHAPES = ["box1", "pair", "n31", "n32", "n33", "e32", "e33"]
ALL_MATH_SHAPES = ["n6x5", "n33", "wide138"]
DROPOUT_SHAPES = ["n6x5", "wide138"]


# ------------------------------------------------------------------------------------------ cases
class Case:
    """A batch in the input's node order: one group (objects (1, N, 3), Rs, Rr) per tower for the dense
    oracle — test_gpu_state.Case's interface, so its oracle helpers and steps_ref's take it."""

    def __init__(self, name):
        sizes, fully, self.plan, self.nw_max, self.wide = SHAPES[name]
        self.name = name
        self.groups = []
        for i, n in enumerate(sizes):
            raw = D.synthetic_towers(1, n, seed=31 + i)
            Rs, Rr = O.relation_matrices(raw, None if fully else D.RELATION_THRESHOLD)
            if name == "e33" and i == 2:        # the removed relation: a zeroed column of both matrices
                Rs[:, :, 1] = 0.0
                Rr[:, :, 1] = 0.0
            self.groups.append(((raw / D.RELATION_THRESHOLD).astype(np.float32), Rs, Rr))
        self.n = int(sum(sizes))
        rng = np.random.default_rng(17)
        self.prop = rng.normal(0, 0.3, (self.n, 100)).astype(np.float32)
        self.tgt = rng.integers(0, 2, self.n).astype(np.float32)
        self.w = rng.normal(0, 1.0 / self.n, (self.n, 100)).astype(np.float32)     # a loss on the state, BCE-sized
        self.node_w = rng.choice([0.5, 1.0, 2.5], size=self.n).astype(np.float32)
        self.node_w[self.n // 2] = 0.0
        self.pos = np.concatenate([g[0].reshape(-1, 3) for g in self.groups])

    edges = TS.Case.edges

    def host_plan(self) -> HostPlan:
        src, dst, te, tn = self.edges()
        hp = HostPlan.build(self.pos, tn, src, dst, te, self.prop, nw_max=self.nw_max,
                            recv_blocks=self.plan == "recv", pack=self.plan == "packed")
        assert (hp.flags == 1) == (self.plan == "recv") and (hp.node_perm is not None) == (self.plan == "packed")
        if self.plan == "packed":
            assert not np.array_equal(hp.node_perm, np.arange(self.n))
        if self.name in GEOMETRY:
            assert (hp.n_nodes, len(hp.src), hp.n_eblocks) == GEOMETRY[self.name], (hp.n_nodes, len(hp.src), hp.n_eblocks)
        if self.name in ("e32", "e33"):
            assert hp.n_wtiles == 1                  # every tower in one wave-tile
        return hp


@functools.lru_cache(maxsize=None)
def _case(name):
    return Case(name)


def _lam(S):
    return (1.0,) if S == 1 else tuple([0.25] * (S - 2) + [0.5, 1.0])


def _params(oracle):
    return X.kink_free_params(1) if oracle else O.random_params(5)


# ----------------------------------------------------------------------------------------- oracle
@functools.lru_cache(maxsize=None)
def _ref(name, S):
    """fp64: the step-logit rows, P_S, and the loss + gradients of (a) Σ_s λ_s·BCE(z_s) + Σ w ⊙ P_S — calls 2-5 —
    and (b) BCE(z_S) — call 7 — in the input's node order; and the ReLU / clip margin."""
    case = _case(name)
    params = _params(True)
    tgt = torch.as_tensor(case.tgt, dtype=F64)
    out = {}
    for which in ("deep", "plain"):
        tp, objs, p = TS._leaves(case, params, True, True)
        if which == "deep":
            Z = SR.step_logits(tp, case.groups, objs, p, S)
            st = SR.final_state(tp, case.groups, objs, p, S)
            bce = SR.deep_loss(Z, tgt, _lam(S))
            loss = bce + (torch.as_tensor(case.w, dtype=F64) * st).sum()
            out["Z"], out["state"] = Z.detach().numpy().copy(), st.detach().numpy().copy()
        else:
            bce = loss = O.keras_bce_from_logits(SR._forward(tp, case.groups, objs, p, S), tgt)
        loss.backward()
        g = {k: v.grad.numpy().copy() for k, v in tp.items()}
        g["dprop"] = p.grad.numpy().copy()
        g["dpos"] = np.concatenate([o.grad.numpy().reshape(-1, 3) for o in objs])
        out[which] = (float(bce.detach()), g)
    out["margin"] = TS._margin(case, params, True, S)
    return out


# ----------------------------------------------------------------------------------------- engine
class _Bufs:
    """Where a sequence of calls gets its buffers: an arena (guarded) or None (the engine's defaults)."""

    def __init__(self, arena):
        self.ar = arena

    def out(self, shape, name, dtype=torch.float32):
        return None if self.ar is None else self.ar.alloc(shape, dtype, name=name, written=True)

    def put(self, x, name, frozen=True):
        x = torch.as_tensor(np.ascontiguousarray(x)) if not isinstance(x, torch.Tensor) else x
        if self.ar is None:
            return x.to(DEV).clone()
        return self.ar.put(x.to(DEV), name=name, frozen=frozen)

    def freeze(self, *ts):
        if self.ar is not None:
            for t in ts:
                self.ar.freeze(t)

    def check(self, what):
        if self.ar is not None:
            self.ar.check(what)

    def workspace(self, batch, run, name):
        """Exactly engine.workspace_bytes() bytes, 256-aligned and no more (Workspace.get keeps a buffer that
        is large enough)."""
        ws = E.Workspace(DEV)
        if self.ar is not None:
            ws.buf = self.ar.alloc(E.workspace_bytes(batch, run), torch.uint8, align=256, name=name)
            if E.POISON_WORKSPACE:
                ws.buf.fill_(0xFF)
        return ws

    def scratch(self, sc, outs):
        """Replace a scratch object's attributes by arena views of exactly the advertised sizes."""
        if self.ar is not None:
            kind = type(sc).__name__
            sc.scratch = self.ar.alloc(sc.scratch.numel(), torch.uint8, name=f"{kind}.scratch")
            for k in outs:
                t = getattr(sc, k)
                setattr(sc, k, self.ar.alloc(tuple(t.shape), t.dtype, name=f"{kind}.{k}", written=True))
        return sc

    def batch(self, hp: HostPlan):
        if self.ar is None:
            return TowerBatch.from_plan(hp, DEV)
        names = ["pos", "node_tower", "node_local", "wtile", "edge_src", "edge_dst", "blk_csr", "prop"]
        b = TowerBatch.from_plan(hp, DEV, dev_arrays=[self.put(a, "batch." + k) for a, k in zip(hp.arrays, names)])
        off = np.concatenate([[0], np.cumsum(hp.tower_nodes)]).astype(np.int32)
        b._tower_offsets = self.put(off, "batch.tower_offsets")      # tower_readout's offsets
        return b


def _np(t):
    return None if t is None else t.detach().cpu().numpy().copy()


def _sequence(case, math, S, rate, arena, oracle_params=False, weighted=False):
    """The calls of one case in order; every output as numpy, in the plan's node order."""
    B = _Bufs(arena)
    hp = case.host_plan()
    batch = B.batch(hp)
    n, T = batch.n_nodes, batch.n_towers
    flat = B.put(P.to_flat(_params(oracle_params)), "params")
    plan_rows = lambda x: np.asarray(x)[hp.node_perm] if hp.node_perm is not None else np.asarray(x)
    tgt = B.put(plan_rows(case.tgt), "targets")
    dstate = B.put(plan_rows(case.w), "dstate")
    r = {"batch": batch}

    # 1. inference forward on an inference-sized workspace
    run_i = E.RunConfig(S, training=False, math=math)
    ws_i = B.workspace(batch, run_i, "workspace(inference)")
    z_inf = E.forward(flat, batch, run_i, ws_i, logits=B.out(n, "logits(inference)"))
    B.check("1 forward (inference)")
    r["z_inf"] = _np(z_inf)
    z_inf2, st_inf = E.forward(flat, batch, run_i, ws_i, logits=B.out(n, "logits(inference, state)"), return_state=True,
                               state=B.out((n, 100), "state_out(inference)"))
    B.check("1 forward (inference, return_state)")
    r["z_inf2"], r["state_inf"] = _np(z_inf2), _np(st_inf)
    assert r["z_inf2"].tobytes() == r["z_inf"].tobytes()

    # 2. training forward_steps with the state
    run = E.RunConfig(S, training=True, math=math, dropout=rate, seed=DROP_SEED)
    if math != "f32":
        assert E.fused_path(batch, run) == FUSED[case.name], (case.name, E.fused_path(batch, run))
    ws = B.workspace(batch, run, "workspace(training)")
    Z, st = E.forward_steps(flat, batch, run, ws, step_logits=B.out((S, n), "step_logits"), return_state=True,
                            state=B.out((n, 100), "state_out"))
    B.check("2 forward_steps")
    B.freeze(Z, st)
    r["Z"], r["state"] = _np(Z), _np(st)

    # 3. the deep-supervision loss
    sc = B.scratch(E.BceStepsScratch(DEV, S), ("out3", "out3s"))
    w3 = B.put(torch.tensor([float(n), 1.0, 1.0], dtype=torch.float64), "weights3")
    tot3 = B.put(torch.ones(3, dtype=torch.float64), "total3", frozen=False)
    tot3s = B.put(torch.ones(S, 3, dtype=torch.float64), "total3s", frozen=False)
    o3, o3s, dZ = E.bce_steps(Z, tgt, _lam(S), sc, dlogits=B.out((S, n), "dstep_logits"), total3=tot3, weights3=w3,
                              total3s=tot3s)
    B.check("3 bce_steps")
    B.freeze(dZ)
    r["steps_out3"], r["steps_out3s"], r["dZ"] = _np(o3), _np(o3s), _np(dZ)
    r["total3"], r["total3s"] = _np(tot3), _np(tot3s)
    assert np.array_equal(r["total3"], 1.0 + r["steps_out3"].astype(np.float64) * _np(w3))
    assert np.array_equal(r["total3s"], 1.0 + r["steps_out3s"].astype(np.float64) * _np(w3))
    if weighted:        # the same loss with guarded node weights and a guarded device norm (spwgnn_loss_weights)
        nw = B.put(plan_rows(case.node_w), "node_weights(steps)")
        norm = B.put(np.array([np.count_nonzero(case.node_w)], np.float32), "norm_dev(steps)")
        scw = B.scratch(E.BceStepsScratch(DEV, S), ("out3", "out3s"))
        o3w, o3sw, dZw = E.bce_steps(Z, tgt, _lam(S), scw, dlogits=B.out((S, n), "dstep_logits(weighted)"),
                                     node_weights=nw, norm=norm)
        B.check("3 bce_steps (weighted)")
        r["w_steps_out3"], r["w_steps_out3s"], r["w_dZ"] = _np(o3w), _np(o3sw), _np(dZw)
        assert r["w_steps_out3"][2] == np.count_nonzero(case.node_w)

    # 4. backward_steps with a state cotangent and dprop
    g, dp = E.backward_steps(flat, batch, run, ws, dZ, grads=B.out(flat.numel(), "grads(steps)"), dstate=dstate,
                             want_dprop=True, dprop=B.out((n, 100), "dprop(steps)"))
    B.check("4 backward_steps")
    r["g"], r["dprop"] = _np(g), _np(dp)

    # 5. d/d objects
    dpos4 = B.out((n, 4), "dpos")
    dpos = E.backward_inputs(flat, batch, run, ws, dpos=dpos4)
    B.check("5 backward_inputs")
    r["dpos"] = _np(dpos)
    if dpos4 is not None:
        assert dpos.data_ptr() == dpos4.data_ptr()
        assert not _np(dpos4)[:, 3].any(), "dpos column 3 must be exactly zero"

    # 6. readouts of the last row (an address that is only 4-byte aligned when S·n is odd)
    sig = E.sigmoid(Z[-1], out=B.out(n, "sigmoid.out"))
    B.check("6 sigmoid")
    ro = E.tower_readout(Z[-1], batch, "sum_prob", out=B.out(T, "tower_readout.out"))
    B.check("6 tower_readout")
    r["sigmoid"], r["readout"] = _np(sig), _np(ro)

    # 7. a second workspace: forward, then the loss and the backward in one call
    ws2 = B.workspace(batch, run, "workspace(second)")
    for wtd in ([False, True] if weighted else [False]):
        tag = "weighted " if wtd else ""
        z = E.forward(flat, batch, run, ws2, logits=B.out(n, f"logits({tag}training)"))
        B.check(f"7 {tag}forward")
        B.freeze(z)
        bsc = B.scratch(E.BceScratch(DEV), ("out3",))
        nw = B.put(plan_rows(case.node_w), "node_weights") if wtd else None
        norm = B.put(np.array([np.count_nonzero(case.node_w)], np.float32), "norm_dev") if wtd else None
        o3b, dzb, gb, dpb = E.bce_backward(flat, batch, run, ws2, z, tgt, bsc, dlogits=B.out(n, f"dlogits({tag}bce_backward)"),
                                           grads=B.out(flat.numel(), f"grads({tag}bce_backward)"),
                                           want_dprop=True, dprop=B.out((n, 100), f"dprop({tag}bce_backward)"),
                                           node_weights=nw, norm=norm)
        B.check(f"7 {tag}bce_backward")
        k = "w_" if wtd else ""
        r[k + "z"], r[k + "out3"], r[k + "dz"], r[k + "g2"], r[k + "dprop2"] = _np(z), _np(o3b), _np(dzb), _np(gb), _np(dpb)
        if not wtd:
            grads = gb
    B.freeze(grads)

    # 7c. the state-carrying pair of the plain calls: forward(return_state) and backward(dstate)
    z, st2 = E.forward(flat, batch, run, ws2, logits=B.out(n, "logits(state pair)"), return_state=True,
                       state=B.out((n, 100), "state_out(state pair)"))
    B.check("7c forward (return_state)")
    assert _np(z).tobytes() == r["z"].tobytes()                      # the same logits with and without the state
    r["state2"] = _np(st2)
    g3, dp3 = E.backward(flat, batch, run, ws2, dzb, grads=B.out(flat.numel(), "grads(backward)"), dstate=dstate,
                         want_dprop=True, dprop=B.out((n, 100), "dprop(backward)"))
    B.check("7c backward (dstate)")
    r["g3"], r["dprop3"] = _np(g3), _np(dp3)

    # 8. Adam, plain and clipped, on the returned gradients: params, m and v are outputs
    p1 = B.put(P.to_flat(_params(oracle_params)), "adam.params", frozen=False)
    m = B.put(torch.zeros(flat.numel()), "adam.m", frozen=False)
    v = B.put(torch.zeros(flat.numel()), "adam.v", frozen=False)
    E.adam(p1, grads, m, v, 1)
    B.check("8 adam")
    r["p1"], r["m1"], r["v1"] = _np(p1), _np(m), _np(v)
    clip = B.scratch(E.ClipScratch(DEV, totals=True), ("out4",))
    if arena is not None:
        clip.total4 = B.put(torch.zeros(4, dtype=torch.float64), "ClipScratch.total4", frozen=False)
    out4 = E.adam_clipped(p1, grads, m, v, 2, clip, clipnorm=CLIPNORM, accumulate=True)
    B.check("8 adam_clipped")
    r["p2"], r["m2"], r["v2"], r["out4"], r["total4"] = _np(p1), _np(m), _np(v), _np(out4), _np(clip.total4)
    return r


def _same_bits(a, b, what):
    for k, x in a.items():
        if k == "batch":
            continue
        assert x.dtype == b[k].dtype and x.shape == b[k].shape, (what, k)
        assert x.tobytes() == b[k].tobytes(), f"{what}: '{k}' differs between arena buffers and ordinary ones"


def _guarded_and_plain(name, math, S, rate=0.0, oracle_params=False):
    case = _case(name)
    with TS._limit(case.wide):
        got = _sequence(case, math, S, rate, G.Arena(DEV), oracle_params, weighted=name == "n6x5")
        plain = _sequence(case, math, S, rate, None, oracle_params, weighted=name == "n6x5")
    _same_bits(got, plain, f"{name} {math} S={S} dropout={rate}")
    for k, x in got.items():
        if k != "batch":
            assert np.isfinite(x).all(), k
    return case, got


# --------------------------------------------------------------------------- 1. the call sequence
def _close(got, ref):
    return np.all(np.abs(got - ref) <= 1e-5 + 1e-5 * np.abs(ref))


def _against_oracle(case, got, S):
    ref = _ref(case.name, S)
    assert ref["margin"] >= TS.MIN_RELU_MARGIN, ref["margin"]
    assert np.abs(ref["Z"]).max() <= O.LOGIT_CLIP - 1.0              # no step's logit near the BCE clip
    back = got["batch"].to_input_order
    rows = lambda Zp: back(Zp.T).T
    worst = float(np.abs(rows(got["Z"]) - ref["Z"]).max())
    for s in range(S):
        assert _close(rows(got["Z"])[s], ref["Z"][s]), (s, np.abs(rows(got["Z"])[s] - ref["Z"][s]).max())
    assert _close(back(got["z_inf"]), ref["Z"][-1]) and _close(back(got["z"]), ref["Z"][-1])
    assert _close(back(got["state"]), ref["state"]), np.abs(back(got["state"]) - ref["state"]).max()
    flat_of = lambda a: P.from_flat(torch.as_tensor(a))
    for which, loss, g, dprop, dpos in (("deep", got["steps_out3"][0], got["g"], got["dprop"], got["dpos"]),
                                        ("plain", got["out3"][0], got["g2"], got["dprop2"], None)):
        rloss, rg = ref[which]
        print(f"guard {case.name} S={S} {which}: loss {float(loss):.7f} oracle {rloss:.7f}")
        assert abs(float(loss) - rloss) <= 1e-5, (which, float(loss), rloss)
        have = dict(flat_of(g), dprop=back(dprop))
        if dpos is not None:
            have["dpos"] = back(dpos)
        for k, x in have.items():
            err, bound = TS._maxabs(x, rg[k]), 1e-5 * np.abs(rg[k]).max() + 1e-7
            worst = max(worst, err / bound)
            assert err <= bound, (which, k, err, bound)
    assert got["steps_out3"][2] == case.n and got["out3"][2] == case.n
    if case.name == "box1":        # no relation: nothing reaches the relation encoder or the relation model
        for g in (flat_of(got["g"]), flat_of(got["g2"])):
            for k, x in g.items():
                if k.startswith("rm.") or k.startswith("rmp."):
                    assert not x.any(), k
                else:
                    assert x.any(), k
    print(f"guard {case.name} S={S}: ReLU margin {ref['margin']:.3f}, worst err / bound {worst:.3f}")


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("math", ["x6", "f32"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_guarded_calls(name, math, S):
    oracle = name in ORACLE_SHAPES
    case, got = _guarded_and_plain(name, math, S, oracle_params=oracle)
    if oracle:
        _against_oracle(case, got, S)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("math", ["bf16", "x3", "h3"])
@pytest.mark.parametrize("name", ALL_MATH_SHAPES)
def test_guarded_calls_other_maths(name, math, S):
    _guarded_and_plain(name, math, S)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("name", DROPOUT_SHAPES)
def test_guarded_calls_with_dropout(name, S):
    case, got = _guarded_and_plain(name, "x6", S, rate=0.1)
    assert not np.array_equal(got["Z"][-1], got["z_inf"])            # the masks were drawn and applied


# ------------------------------------------------------------------ 2. the folded-loss switch n <= 256
@pytest.mark.parametrize("math", ["x6", "f32"])
@pytest.mark.parametrize("name", ["fold256", "fold257"])
def test_bce_backward_equals_bce_then_backward_at_the_fold_boundary(name, math):
    """tests/test_gpu_training.py::test_bce_backward_equals_bce_then_backward at n = 256 (the loss folded into
    the fused backward loop) and n = 257 (the loss launch first, two workgroups), every buffer guarded."""
    case = _case(name)
    assert case.n == (256 if name == "fold256" else 257)
    ar = G.Arena(DEV)
    B = _Bufs(ar)
    batch = B.batch(case.host_plan())
    n = batch.n_nodes
    flat = B.put(P.to_flat(O.random_params(2)), "params")
    tgt = B.put(case.tgt, "targets")
    run = E.RunConfig(5, training=True, math=math, dropout=0.1, seed=3)
    if math != "f32":
        assert E.fused_path(batch, run) == 3          # the fused backward: n <= 256 alone decides the fold
    w3 = B.put(torch.tensor([float(n), 1.0, 1.0], dtype=torch.float64), "weights3")
    out = []
    for fold in (False, True):
        tag = "folded" if fold else "two calls"
        ws = B.workspace(batch, run, f"workspace({tag})")
        tot = B.put(torch.zeros(3, dtype=torch.float64), f"total3({tag})", frozen=False)
        z = E.forward(flat, batch, run, ws, logits=B.out(n, f"logits({tag})"))
        B.check(f"{tag}: forward")
        B.freeze(z)
        sc = B.scratch(E.BceScratch(DEV), ("out3",))
        # (an output is allocated right before the call that writes it: check() holds every one to "written")
        dlogits = B.out(n, f"dlogits({tag})")
        if not fold:
            o3, dz = E.bce(z, tgt, sc, dlogits=dlogits, total3=tot, weights3=w3)
            B.check("bce")
            B.freeze(dz)
        grads, dprop = B.out(flat.numel(), f"grads({tag})"), B.out((n, 100), f"dprop({tag})")
        if fold:
            o3, dz, g, dp = E.bce_backward(flat, batch, run, ws, z, tgt, sc, dlogits=dlogits, total3=tot, weights3=w3,
                                           grads=grads, dprop=dprop)
            B.check("bce_backward")
        else:
            g, dp = E.backward(flat, batch, run, ws, dz, grads=grads, dprop=dprop)
            B.check("backward")
        out.append([_np(t) for t in (o3, tot, dz, g, dp)])
    for a, b, what in zip(out[0], out[1], ("out3", "total3", "dlogits", "grads", "dprop")):
        assert a.tobytes() == b.tobytes(), what
        assert np.isfinite(a).all() and np.abs(a).max() > 0, what


# ---------------------------------------------------------------------- 3. the loss launch geometry
@pytest.mark.parametrize("n", [1, 255, 256, 257, 65536, 65537])
def test_bce_launch_geometry(n):
    """Guarded spwgnn_bce on either side of one / two workgroups (256 | 257) and of the 256-workgroup cap
    (65536 | 65537), against a float64 numpy restatement of Keras's clipped BCE (oracle.model.keras_bce_grad).
    dlogits within 1e-6/n of (σ(z) − t)/n: fp32 sigmoid is good to a few ulp of 1 (6e-8 each), and the division
    by n scales that. Logits from N(0, 3), max|z| < 15 asserted, so the probability clip decides nothing."""
    rng = np.random.default_rng(1000 + n)
    z = rng.normal(0.0, 3.0, n).astype(np.float32)
    t = rng.integers(0, 2, n).astype(np.float32)
    assert np.abs(z).max() < 15.0 < O.LOGIT_CLIP
    loss_ref, g_ref = O.keras_bce_grad(z, t)
    z64 = z.astype(np.float64)
    assert np.array_equal(g_ref, (1.0 / (1.0 + np.exp(-z64)) - t) / n)            # the restatement is (σ(z) − t)/n here
    correct_ref = int(((z > 0).astype(np.float32) == t).sum())
    ar = G.Arena(DEV)
    B = _Bufs(ar)
    zt, tt = B.put(z, "logits"), B.put(t, "targets")
    sc = B.scratch(E.BceScratch(DEV), ("out3",))
    out3, dz = E.bce(zt, tt, sc, dlogits=B.out(n, "dlogits"))
    B.check(f"bce n={n}")
    out3, dz = _np(out3), _np(dz).astype(np.float64)
    plain3, plain_dz = E.bce(zt.clone(), tt.clone(), E.BceScratch(DEV))
    assert np.array_equal(_np(plain_dz).astype(np.float64), dz), "dlogits differ between arena buffers and ordinary ones"
    assert np.array_equal(_np(plain3), out3), "out3 differs between arena buffers and ordinary ones"
    err = np.abs(dz - g_ref).max()
    print(f"bce n={n}: loss {out3[0]:.7f} ref {loss_ref:.7f}; max|ddlogits|·n {err * n:.2e}")
    assert abs(float(out3[0]) - loss_ref) <= 1e-5
    assert float(out3[1]) == correct_ref and float(out3[2]) == n
    assert err <= 1e-6 / n, (err, 1e-6 / n)
    # the weighted launch (spwgnn_bce_weighted) with guarded weights and a guarded device norm: with w ≡ 1 and
    # norm = n < 2^24 every output equals the unweighted call's bit for bit (spwgnn.h)
    wt = B.put(np.ones(n, np.float32), "node_weights")
    norm = B.put(np.array([n], np.float32), "norm_dev")
    sc2 = B.scratch(E.BceScratch(DEV), ("out3",))
    w_out3, w_dz = E.bce(zt, tt, sc2, dlogits=B.out(n, "dlogits(weighted)"), node_weights=wt, norm=norm)
    B.check(f"bce weighted n={n}")
    assert np.array_equal(_np(w_out3), out3) and np.array_equal(_np(w_dz).astype(np.float64), dz)


# ------------------------------------------------------- 4. the entry points of a replayed step
def test_replay_entry_points_guarded():
    """The remaining launch functions, on n6x5: spwgnn_step_advance, spwgnn_run.seed_dev, spwgnn_copy_in and the
    forward's prologue, spwgnn_accumulate_out3, spwgnn_adam_dev, spwgnn_adam_clipped_dev — against the eager
    calls they restate, bit for bit."""
    case = _case("n6x5")
    ar = G.Arena(DEV)
    B = _Bufs(ar)
    hp = case.host_plan()
    batch = B.batch(hp)
    n = batch.n_nodes
    flat = B.put(P.to_flat(O.random_params(5)), "params")
    tgt = B.put(case.tgt, "targets")
    key = B.put(torch.tensor([DROP_SEED - 1], dtype=torch.int64), "key_dev", frozen=False)
    step = B.put(torch.tensor([0], dtype=torch.int32), "step_dev", frozen=False)
    E.step_advance(key, step)
    B.check("step_advance")
    assert int(key.item()) == DROP_SEED and int(step.item()) == 1
    B.freeze(key, step)

    # a forward that reads its dropout key from the device word
    run_dev = E.RunConfig(3, training=True, dropout=0.1, seed_dev=key)
    run = E.RunConfig(3, training=True, dropout=0.1, seed=DROP_SEED)
    flat_plain, batch_plain = P.to_flat(O.random_params(5), device=DEV), TowerBatch.from_plan(hp, DEV)
    z_ref = E.forward(flat_plain, batch_plain, run, E.Workspace(DEV))
    ws = B.workspace(batch, run_dev, "workspace")
    z = E.forward(flat, batch, run_dev, ws, logits=B.out(n, "logits(seed_dev)"))
    B.check("forward (seed_dev)")
    assert torch.equal(z, z_ref)

    # copy_in, alone and as the forward's prologue together with the key / step advance
    host = torch.arange(n * 4, dtype=torch.float32).reshape(n, 4).pin_memory()
    src = _lib.host_device_ptr(host.data_ptr())
    dst = ar.alloc((n, 4), torch.float32, name="copy_in.dst", written=True)
    E.copy_in(host, dst, n * 16, src_dev_ptr=src)
    B.check("copy_in")
    assert torch.equal(dst.cpu(), host)
    ar.rearm(dst)
    ar.thaw(key), ar.thaw(step)
    run_dev.prologue = E.Prologue(dst=dst, src_dev_ptr=src, nbytes=n * 16, key=key, step=step)
    z2 = E.forward(flat, batch, run_dev, ws, logits=B.out(n, "logits(prologue)"))
    B.check("forward (prologue)")
    assert torch.equal(dst.cpu(), host) and int(key.item()) == DROP_SEED + 1 and int(step.item()) == 2
    run.seed = DROP_SEED + 1
    assert torch.equal(z2, E.forward(flat_plain, batch_plain, run, E.Workspace(DEV))) and not torch.equal(z2, z_ref)
    B.freeze(key, step, z2)
    run_dev.prologue = None

    # the loss, its epoch sums in a launch of their own, and the gradients
    sc = B.scratch(E.BceScratch(DEV), ("out3",))
    out3, dz = E.bce(z2, tgt, sc, dlogits=B.out(n, "dlogits"))
    B.check("bce")
    B.freeze(out3, dz)
    w3 = B.put(torch.tensor([float(n), 1.0, 1.0], dtype=torch.float64), "weights3")
    tot = B.put(torch.ones(3, dtype=torch.float64), "total3", frozen=False)
    E.accumulate_out3(tot, out3, w3)
    B.check("accumulate_out3")
    assert np.array_equal(_np(tot), 1.0 + _np(out3).astype(np.float64) * _np(w3))
    g, _ = E.backward(flat, batch, run_dev, ws, dz, grads=B.out(flat.numel(), "grads"))
    B.check("backward")
    B.freeze(g)

    # Adam with the step word and the lr table, plain and clipped, against the eager calls at step 2
    table = B.put(E.adam_lr_table(8, device=DEV), "lr_table")
    state = lambda tag: [B.put(x, f"adam.{k}({tag})", frozen=False) for k, x in
                         (("params", flat), ("m", torch.zeros_like(flat)), ("v", torch.full_like(flat, 1e-6)))]
    eager, dev = state("eager"), state("dev")
    E.adam(*eager[:1], g, *eager[1:], 2)
    E.adam_dev(*dev[:1], g, *dev[1:], step, table)
    B.check("adam_dev")
    for a, b in zip(eager, dev):
        assert torch.equal(a, b) and torch.isfinite(a).all()
    assert not torch.equal(eager[0], flat)
    clips = []
    for tag in ("eager", "dev"):
        c = B.scratch(E.ClipScratch(DEV, totals=True), ("out4",))
        c.total4 = B.put(torch.zeros(4, dtype=torch.float64), f"ClipScratch.total4({tag})", frozen=False)
        clips.append(c)
    E.adam_clipped(*eager[:1], g, *eager[1:], 2, clips[0], clipnorm=CLIPNORM, clipvalue=1e-4, accumulate=True)
    E.adam_clipped_dev(*dev[:1], g, *dev[1:], step, table, clips[1], clipnorm=CLIPNORM, clipvalue=1e-4, accumulate=True)
    B.check("adam_clipped_dev")
    for a, b in zip(eager + [clips[0].out4, clips[0].total4], dev + [clips[1].out4, clips[1].total4]):
        assert torch.equal(a, b) and torch.isfinite(a).all()


# ------------------------------------------------------------------------- 5. the new arguments
def test_output_buffer_arguments_are_validated():
    case = _case("pair")
    batch = TowerBatch.from_plan(case.host_plan(), DEV)
    n = batch.n_nodes
    flat = P.to_flat(O.random_params(5), device=DEV)
    run, ws = E.RunConfig(2, training=True), E.Workspace(DEV)
    z = E.forward(flat, batch, run, ws)
    dz = torch.zeros_like(z)
    good = torch.empty(n, 100, device=DEV)
    for bad in (torch.empty(n + 1, 100, device=DEV), good.double(), good.cpu(), torch.empty(100, n, device=DEV).T):
        with pytest.raises((ValueError, _lib.SpwgnnError)):
            E.backward(flat, batch, run, ws, dz, dprop=bad)
        with pytest.raises((ValueError, _lib.SpwgnnError)):
            E.backward_steps(flat, batch, run, ws, torch.zeros(2, n, device=DEV), dprop=bad)
        with pytest.raises((ValueError, _lib.SpwgnnError)):
            E.bce_backward(flat, batch, run, ws, z, dz, E.BceScratch(DEV), dprop=bad)
    g, dp = E.backward(flat, batch, run, ws, dz, dprop=good)              # dprop= implies want_dprop
    assert dp is good
    for bad in (torch.empty(n, 3, device=DEV), torch.empty(n, 4, device=DEV).double(), torch.empty(n, 4)):
        with pytest.raises((ValueError, _lib.SpwgnnError)):
            E.backward_inputs(flat, batch, run, ws, dpos=bad)
    for bad in (torch.empty(n + 1, device=DEV), torch.empty(n, device=DEV).double(), torch.empty(n)):
        with pytest.raises((ValueError, _lib.SpwgnnError)):
            E.sigmoid(z, out=bad)
    for bad in (torch.empty(batch.n_towers + 1, device=DEV), torch.empty(batch.n_towers)):
        with pytest.raises((ValueError, _lib.SpwgnnError)):
            E.tower_readout(z, batch, out=bad)
    for wrong in (torch.zeros(n + 1, device=DEV), torch.zeros(n - 1, device=DEV)):
        with pytest.raises(ValueError, match="one value per node"):
            E.bce_backward(flat, batch, run, ws, wrong, wrong, E.BceScratch(DEV))
    torch.cuda.synchronize()
