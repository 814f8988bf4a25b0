"""GPU: the final propagation state and its gradient (spwgnn_forward_state / spwgnn_backward_state,
DESIGN.md §3zo) against the fp64 oracle (oracle.model.forward_dense(return_state=True)).

Shapes — the smallest that reach each path (asserted with engine.fused_path in the split-bf16 maths):
  n6_full      (8, 6, full)                      the fused small-batch loops
  n9_thr       (5, 9, thresholded)               the fused loops again (at the default team limit a dense
                                                 plan of ≤ 16-node tiles takes them), partly filled blocks
  n9_thr_recv  the same towers on a receiver-    the per-phase team kernels
               block plan
  n20_thr      (3, 20, thresholded)              17–32-node wave-tiles
  n12_recv     (4, 12, full), receiver blocks    forward only
  n6_wide8 / n6_wide23  (8, 6) / (23, 6, full)   the wide kernels (engine.wide_kernels()); 138 nodes = 5
                                                 node blocks, two workgroups, the last block partial
  packed       towers of 4 / 7 / 12 nodes        a packed plan (node order ≠ input order)
S ∈ {1, 2, 4}, with and without a 'propagation' input. Gradient tests use x3_emu.kink_free_params and
assert the oracle's ReLU margins first, so that no kink decides a result.

Tolerances. Forward: the project's logit criterion c = 1e-5 + 1e-5·|ref|. Gradients: the project's
1e-5·max|g| (+ 1e-7 against the oracle). A run chained from n calls is held to n·c (errors of valid
evaluations add). x3 and bf16 are not fp32-class: they are held to 3·d, d that math's own single-call
distance to the oracle on the same case (two valid evaluations differ by at most the sum of their
distances; a lost state gives errors of order 0.1).
The whole file also passes under SPWGNN_POISON_WORKSPACE=1."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import x3_emu as X
from oracle import dropout as DR
from oracle import model as O
from spwgnn_amd import TowerBatch, _lib, data as D, engine as E, params as P
from spwgnn_amd.network import GraphNetwork

pytestmark = pytest.mark.gpu

TEAM_LIMIT = 512
MIN_RELU_MARGIN = 0.1       # far above the rounding of any math's pre-activations (bf16: ≈ 1e-2)
F64 = torch.float64

#        id            T   N   fully  plan     wide   backward
SHAPES = {
    "n6_full":      (8,  6,  True,  "dense", False, True),
    "n9_thr":       (5,  9,  False, "dense", False, True),
    "n9_thr_recv":  (5,  9,  False, "recv",  False, True),
    "n20_thr":      (3,  20, False, "dense", False, True),
    "n12_recv":     (4,  12, True,  "recv",  False, False),
    "n6_wide8":     (8,  6,  True,  "dense", True,  True),
    "n6_wide23":    (23, 6,  True,  "dense", True,  True),
    "packed":       (0,  0,  True,  "packed", False, True),
}
FUSED = {"n6_full": 3, "n9_thr": 3, "n9_thr_recv": 0, "n20_thr": 0, "n12_recv": 0, "n6_wide8": 0, "n6_wide23": 0}
BWD_SHAPES = [k for k, v in SHAPES.items() if v[5]]
PACKED_NODES = (4, 7, 12)


class _limit:
    def __init__(self, wide):
        self.n = 0 if wide else TEAM_LIMIT

    def __enter__(self):
        self.prev = E.team_max_blocks(self.n)

    def __exit__(self, *exc):
        E.team_max_blocks(self.prev)


# ------------------------------------------------------------------------------------------ cases
class Case:
    """A batch in the input's node order: groups of equal-size towers for the dense oracle."""

    def __init__(self, name):
        T, N, fully, self.plan, self.wide, _ = SHAPES[name]
        self.name = name
        if self.plan == "packed":
            self.groups = []
            for i, n in enumerate(PACKED_NODES):
                raw = D.synthetic_towers(1, n, seed=11 + i)
                Rs, Rr = O.relation_matrices(raw, None)
                self.groups.append(((raw / D.RELATION_THRESHOLD).astype(np.float32), Rs, Rr))
        else:
            obj, Rs, Rr = X.dense_case(T, N, fully)[:3]
            self.groups = [(obj, Rs, Rr)]
        self.n = sum(g[0].shape[0] * g[0].shape[1] for g in self.groups)
        rng = np.random.default_rng(17)
        self.prop = rng.normal(0, 0.3, (self.n, 100)).astype(np.float32)
        self.tgt = rng.integers(0, 2, self.n).astype(np.float32)
        self.w = rng.normal(0, 1.0 / self.n, (self.n, 100)).astype(np.float32)   # a loss on the state, BCE-sized
        self.pos = np.concatenate([g[0].reshape(-1, 3) for g in self.groups])

    def edges(self):
        src, dst, te, tn, off = [], [], [], [], 0
        for obj, Rs, Rr in self.groups:
            B, N = obj.shape[:2]
            e = np.array(O.dense_to_edges(Rs, Rr), np.int64).reshape(-1, 4)
            src.append(off + e[:, 0] * N + e[:, 2])
            dst.append(off + e[:, 0] * N + e[:, 3])
            te.append(np.bincount(e[:, 0], minlength=B))
            tn.append(np.full(B, N))
            off += B * N
        cat = lambda a: np.concatenate(a).astype(np.int32)
        return cat(src), cat(dst), cat(te), cat(tn)

    def batch(self, prop=True):
        """The device batch; per-node rows go in through to_plan / come back through to_input."""
        src, dst, te, tn = self.edges()
        b = TowerBatch.from_edges(self.pos, tn, src, dst, te, self.prop if prop else None, device="cuda",
                                  recv_blocks=True if self.plan == "recv" else None, pack=self.plan == "packed")
        assert (b.flags == 1) == (self.plan == "recv") and (b.node_perm is not None) == (self.plan == "packed")
        if self.plan == "packed":
            assert not np.array_equal(b.node_perm, np.arange(self.n))     # the order really differs
        return b


@functools.lru_cache(maxsize=None)
def _case(name):
    return Case(name)


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


# ----------------------------------------------------------------------------------------- oracle
def _oracle_forward(tp, case, objs, prop, S, drop_seed=None, rate=0.0):
    """(logits (n,), P_S (n, 100)) in the input's node order, fp64 torch (autograd through tp, objs, prop)."""
    zs, sts, off, t0 = [], [], 0, 0
    for (obj, Rs, Rr), o in zip(case.groups, objs):
        B, N = obj.shape[:2]
        dr = do = None
        if rate:     # the engine's own masks, restated (oracle/dropout.py), keyed by the tower's index in the batch
            dr = torch.as_tensor(DR.relation_mask_towers(drop_seed, rate, t0 + np.arange(B), N), dtype=F64)
            do = torch.as_tensor(DR.object_mask_towers(drop_seed, rate, t0 + np.arange(B), N), dtype=F64)
        t0 += B
        z, states = O.forward_dense(tp, o, torch.as_tensor(Rs, dtype=F64), torch.as_tensor(Rr, dtype=F64),
                                    prop[off:off + B * N].reshape(B, N, 100), S, dr, do, return_state=True)
        zs.append(z.reshape(-1))
        sts.append(states[-1].reshape(-1, 100))
        off += B * N
    return torch.cat(zs), torch.cat(sts)


def _leaves(case, params, prop, grad):
    tp = O.to_torch(params, requires_grad=grad)
    objs = [torch.tensor(g[0], dtype=F64, requires_grad=grad) for g in case.groups]
    p = torch.tensor(case.prop if prop else np.zeros_like(case.prop), dtype=F64, requires_grad=grad)
    return tp, objs, p


@functools.lru_cache(maxsize=None)
def _fwd_ref(name, S, prop, pseed=5, drop_seed=None, rate=0.0):
    case = _case(name)
    tp, objs, p = _leaves(case, O.random_params(pseed), prop, False)
    with torch.no_grad():
        z, st = _oracle_forward(tp, case, objs, p, S, drop_seed, rate)
    return z.numpy(), st.numpy()


def _margin(case, params, prop, S):
    src, dst, _, tn = case.edges()
    tower = np.repeat(np.arange(len(tn)), tn)
    m = O.relu_margins_gather(O.to_torch(params), case.pos.astype(np.float64), src, dst,
                              (case.prop if prop else np.zeros_like(case.prop)).astype(np.float64), tower, len(tn), S)
    return float(m.min())


@functools.lru_cache(maxsize=None)
def _grad_ref(name, S, prop, state_loss=True, pseed=1):
    """fp64 gradients of L = BCE(z) [+ Σ w ⊙ P_S]: ({tensor: g}, dprop, dpos, ReLU margin), input node order."""
    case = _case(name)
    params = X.kink_free_params(pseed)
    tp, objs, p = _leaves(case, params, prop, True)
    z, st = _oracle_forward(tp, case, objs, p, S)
    loss = O.keras_bce_from_logits(z, torch.as_tensor(case.tgt, dtype=F64))
    if state_loss:
        loss = loss + (torch.as_tensor(case.w, dtype=F64) * st).sum()
    loss.backward()
    g = {k: v.grad.numpy().copy() for k, v in tp.items()}
    dpos = np.concatenate([o.grad.numpy().reshape(-1, 3) for o in objs])
    return g, p.grad.numpy().copy(), dpos, _margin(case, params, prop, S)


# ----------------------------------------------------------------------------------------- engine
def _run(S, math, training=True, dropout=0.0, seed=0):
    return E.RunConfig(S, training=training, math=math, dropout=dropout, seed=seed)


def _assert_path(name, batch, run):
    if run.math != "f32" and run.training and name in FUSED:
        assert E.fused_path(batch, run) == FUSED[name], (name, E.fused_path(batch, run))


def _step(params, case, S, math, prop=True, state_loss=True, dlogits="bce", dstate="w", dropout=0.0, seed=0, batch=None,
          prop_t=None, check_path=True):
    """One training forward (with the state) and its backward, per-node results in the input's node order:
    dict z, state, g (tensors), dprop, dpos. dlogits: "bce" | "zero"; dstate: "w" | None | an (n, 100) array
    in input order. prop_t: a device 'propagation' in PLAN order replacing the case's."""
    batch = batch if batch is not None else case.batch(prop)
    if prop_t is not None:
        batch = batch.with_prop(prop_t)
    flat = P.to_flat(params, device="cuda")
    ws = E.Workspace("cuda")
    run = _run(S, math, dropout=dropout, seed=seed)
    if check_path:
        _assert_path(case.name, batch, run)
    z, st = E.forward(flat, batch, run, ws, return_state=True)
    if dlogits == "bce":
        _, dz = E.bce(z, _dev(batch.to_plan_order(case.tgt)), E.BceScratch("cuda"))
    else:
        dz = torch.zeros_like(z)
    ds = None
    if dstate is not None and state_loss:
        ds = _dev(batch.to_plan_order(case.w if isinstance(dstate, str) else np.asarray(dstate, np.float32)))
    g, dp = E.backward(flat, batch, run, ws, dz, want_dprop=True, dstate=ds)
    dpos = E.backward_inputs(flat, batch, run, ws)
    torch.cuda.synchronize()
    back = lambda t: batch.to_input_order(t.cpu().numpy())
    return {"z": back(z), "state": back(st), "state_plan": st, "g": P.from_flat(g), "dprop": back(dp),
            "dpos": back(dpos), "batch": batch}


def _close(got, ref, factor=1.0):
    return np.all(np.abs(got - ref) <= factor * (1e-5 + 1e-5 * np.abs(ref)))


# ------------------------------------------------------------------ 1. the state against the oracle
@pytest.mark.parametrize("math", ["f32", "x6"])
@pytest.mark.parametrize("prop", [True, False], ids=["prop", "noprop"])
@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("name", list(SHAPES))
def test_state_against_oracle(name, S, prop, math):
    case = _case(name)
    zref, sref = _fwd_ref(name, S, prop)
    flat = P.to_flat(O.random_params(5), device="cuda")
    with _limit(case.wide):
        batch = case.batch(prop)
        for training in (True, False):
            run = _run(S, math, training)
            _assert_path(name, batch, run)
            state = torch.full((batch.n_nodes, 100), float("nan"), device="cuda")
            z, st = E.forward(flat, batch, run, E.Workspace("cuda"), return_state=True, state=state)
            z0 = E.forward(flat, batch, run, E.Workspace("cuda"))
            torch.cuda.synchronize()
            assert st is state
            got_s, got_z = batch.to_input_order(st.cpu().numpy()), batch.to_input_order(z.cpu().numpy())
            np.testing.assert_array_equal(z.cpu().numpy(), z0.cpu().numpy())     # the same logits, bit for bit
            assert np.isfinite(got_s).all(), "a state row was left unwritten"
            err = np.abs(got_s - sref).max()
            print(f"state {name} S={S} prop={prop} {math} training={training}: max|dP_S| {err:.2e}, "
                  f"max|dz| {np.abs(got_z - zref).max():.2e}")
            assert _close(got_s, sref), err
            assert _close(got_z, zref)


# ----------------------------------------------------------------------------------- 2. chaining
CHAIN_SHAPES = ["n6_full", "n9_thr_recv", "n20_thr", "n12_recv", "n6_wide23"]
DROP_SEED = 77


def _chain(case, batch, flat, math, rate):
    """S = 2, then S = 2 with prop = the state (plan order, as the engine returned it); and one S = 4 call."""
    r2, r4 = _run(2, math, dropout=rate, seed=DROP_SEED), _run(4, math, dropout=rate, seed=DROP_SEED)
    _, st = E.forward(flat, batch, r2, E.Workspace("cuda"), return_state=True)
    z2, st2 = E.forward(flat, batch.with_prop(st), r2, E.Workspace("cuda"), return_state=True)
    z4, st4 = E.forward(flat, batch, r4, E.Workspace("cuda"), return_state=True)
    torch.cuda.synchronize()
    back = lambda t: batch.to_input_order(t.cpu().numpy()).astype(np.float64)
    return back(z2), back(st2), back(z4), back(st4)


@pytest.mark.parametrize("rate", [0.0, 0.1], ids=["nodrop", "drop"])
@pytest.mark.parametrize("math", ["f32", "x6", "x3", "bf16"])
@pytest.mark.parametrize("name", CHAIN_SHAPES + ["packed"])
def test_chained_calls_equal_one_long_call(name, math, rate):
    case = _case(name)
    flat = P.to_flat(O.random_params(5), device="cuda")
    with _limit(case.wide):
        batch = case.batch(True)
        _assert_path(name, batch, _run(2, math, dropout=rate, seed=DROP_SEED))
        z2, st2, z4, st4 = _chain(case, batch, flat, math, rate)
    if math in ("f32", "x6"):
        print(f"chain {name} {math} rate={rate}: max|dz| {np.abs(z2 - z4).max():.2e}, max|dP| {np.abs(st2 - st4).max():.2e}")
        assert _close(z2, z4, 2), np.abs(z2 - z4).max()
        assert _close(st2, st4, 2), np.abs(st2 - st4).max()
        return
    zref, sref = _fwd_ref(name, 4, True, 5, DROP_SEED if rate else None, rate)
    d = np.abs(z4 - zref).max()
    got = np.abs(z2 - zref).max()
    print(f"chain {name} {math} rate={rate}: d (single S=4 call to the oracle) {d:.3e}, chained {got:.3e}, ratio {got / d:.2f}; "
          f"state d {np.abs(st4 - sref).max():.3e}, chained {np.abs(st2 - sref).max():.3e}")
    assert got <= 3 * d, (got, d)
    assert np.abs(st2 - sref).max() <= 3 * np.abs(st4 - sref).max()


# ----------------------------------------------------------------------- 3. gradient composition
def _maxabs(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max())


@pytest.mark.parametrize("math", ["f32", "x6", "x3", "bf16"])
@pytest.mark.parametrize("name", BWD_SHAPES)
def test_gradients_compose_across_two_calls(name, math):
    """S = 4 gradients of BCE(z) against call 2's (S = 2, prop = call 1's state) plus call 1's
    backward(dlogits = 0, dstate = call 2's dprop): every weight tensor, dprop and dpos."""
    case = _case(name)
    params = X.kink_free_params(1)
    ref_g, ref_dprop, ref_dpos, margin = _grad_ref(name, 4, True, state_loss=False)
    assert margin >= MIN_RELU_MARGIN, margin
    with _limit(case.wide):
        one = _step(params, case, 4, math, state_loss=False)
        c1 = case.batch(True)
        flat = P.to_flat(params, device="cuda")
        ws1, r2 = E.Workspace("cuda"), _run(2, math)
        _assert_path(name, c1, r2)
        _, st1 = E.forward(flat, c1, r2, ws1, return_state=True)
        two = _step(params, case, 2, math, state_loss=False, batch=c1, prop_t=st1)
        dz0 = torch.zeros(c1.n_nodes, device="cuda")
        g1, dp1 = E.backward(flat, c1, r2, ws1, dz0, want_dprop=True, dstate=_dev(c1.to_plan_order(two["dprop"])))
        dpos1 = E.backward_inputs(flat, c1, r2, ws1)
        torch.cuda.synchronize()
    g1 = P.from_flat(g1)
    comp = {k: g1[k].astype(np.float64) + two["g"][k] for k in g1}
    comp["dprop"] = c1.to_input_order(dp1.cpu().numpy())
    comp["dpos"] = c1.to_input_order(dpos1.cpu().numpy()).astype(np.float64) + two["dpos"]
    single = dict(one["g"], dprop=one["dprop"], dpos=one["dpos"])
    ref = dict(ref_g, dprop=ref_dprop, dpos=ref_dpos)
    worst = 0.0
    for k in ref:
        scale = np.abs(ref[k]).max()
        assert scale > 0, k
        if math in ("f32", "x6"):
            err, bound = _maxabs(comp[k], np.asarray(single[k], np.float64)), 2e-5 * np.abs(single[k]).max()
        else:
            d = _maxabs(single[k], ref[k])
            err, bound = _maxabs(comp[k], ref[k]), 3 * d
        worst = max(worst, err / bound)
        assert err <= bound, (k, err, bound)
    print(f"compose {name} {math}: ReLU margin {margin:.3f}, worst err / bound {worst:.3f}")


# ------------------------------------------------------------------ 4. gradients against the oracle
@pytest.mark.parametrize("math", ["f32", "x6"])
@pytest.mark.parametrize("prop", [True, False], ids=["prop", "noprop"])
@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("name", BWD_SHAPES)
def test_state_loss_gradients_against_oracle(name, S, prop, math):
    """L = BCE(z) + Σ w ⊙ P_S with a fixed random w."""
    case = _case(name)
    ref_g, ref_dprop, ref_dpos, margin = _grad_ref(name, S, prop)
    assert margin >= MIN_RELU_MARGIN, margin
    with _limit(case.wide):
        got = _step(X.kink_free_params(1), case, S, math, prop=prop)
    worst = 0.0
    # (without a 'propagation' input dprop is the gradient at the zero state: compared too)
    ref = dict(ref_g, dpos=ref_dpos, dprop=ref_dprop)
    have = dict(got["g"], dpos=got["dpos"], dprop=got["dprop"])
    for k in ref:
        err, bound = _maxabs(have[k], ref[k]), 1e-5 * np.abs(ref[k]).max() + 1e-7
        worst = max(worst, err / bound)
        assert err <= bound, (k, err, bound)
    print(f"state-loss gradients {name} S={S} prop={prop} {math}: margin {margin:.3f}, worst err / bound {worst:.3f}")


# ------------------------------------------------------------------------------ 5. invariants
def _bits(a, b, what):
    for k in ("z", "state", "dprop", "dpos"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")
    for k in a["g"]:
        np.testing.assert_array_equal(a["g"][k], b["g"][k], err_msg=f"{what}: {k}")


INV_SHAPES = ["n6_full", "n9_thr_recv", "n6_wide23"]


@pytest.mark.parametrize("math", ["f32", "x6", "x3", "bf16"])
@pytest.mark.parametrize("name", INV_SHAPES)
def test_zero_and_null_state_cotangents_are_the_plain_backward(name, math):
    """dstate = zeros, dstate = NULL through spwgnn_backward_state and state_out = NULL through
    spwgnn_forward_state give the bits of spwgnn_forward / spwgnn_backward."""
    case = _case(name)
    params = O.random_params(5)
    flat = P.to_flat(params, device="cuda")
    L = _lib.lib()
    with _limit(case.wide):
        zeros = _step(params, case, 4, math, dstate=np.zeros((case.n, 100)), dropout=0.1, seed=3)
        none = _step(params, case, 4, math, dstate=None, dropout=0.1, seed=3)
        _bits(zeros, none, "dstate = zeros vs none")
        # the plain calls, and the new symbols with NULL, on workspaces whose forward kept no state
        batch = case.batch(True)
        run = _run(4, math, dropout=0.1, seed=3)
        tgt = _dev(batch.to_plan_order(case.tgt))
        outs = []
        for null_calls in (False, True):
            ws = E.Workspace("cuda")
            z = E.forward(flat, batch, run, ws)                 # sizes the workspace; the plain forward
            stream = torch.cuda.current_stream().cuda_stream
            b, r = batch.cstruct(), run.cstruct()
            if null_calls:
                z = torch.full_like(z, float("nan"))
                _lib.check(L.spwgnn_forward_state(flat.data_ptr(), C.byref(b), C.byref(r), ws.buf.data_ptr(),
                                                  ws.buf.numel(), z.data_ptr(), None, stream), "forward_state(NULL)")
            _, dz = E.bce(z, tgt, E.BceScratch("cuda"))
            if null_calls:
                g = torch.full_like(flat, float("nan"))
                dp = torch.full((batch.n_nodes, 100), float("nan"), device="cuda")
                _lib.check(L.spwgnn_backward_state(flat.data_ptr(), C.byref(b), C.byref(r), ws.buf.data_ptr(),
                                                   ws.buf.numel(), dz.data_ptr(), None, g.data_ptr(), dp.data_ptr(),
                                                   stream), "backward_state(NULL)")
                ws.bwd_key = ws.fwd_key
            else:
                g, dp = E.backward(flat, batch, run, ws, dz, want_dprop=True)
            dpos = E.backward_inputs(flat, batch, run, ws)
            torch.cuda.synchronize()
            back = lambda t: batch.to_input_order(t.cpu().numpy())
            outs.append({"z": back(z), "state": none["state"], "g": P.from_flat(g), "dprop": back(dp), "dpos": back(dpos)})
    _bits(outs[0], outs[1], "plain calls vs NULL through the state symbols")
    _bits(outs[0], none, "plain forward / backward vs the state-keeping forward")


@pytest.mark.parametrize("math", ["f32", "x6", "x3", "bf16"])
@pytest.mark.parametrize("name", INV_SHAPES + ["packed"])
def test_two_runs_on_poisoned_workspaces_agree_bitwise(name, math, monkeypatch):
    monkeypatch.setattr(E, "POISON_WORKSPACE", True)     # every fresh workspace byte 0xFF, outputs NaN-filled
    case = _case(name)
    params = O.random_params(5)
    with _limit(case.wide):
        a = _step(params, case, 4, math, dropout=0.1, seed=3)
        b = _step(params, case, 4, math, dropout=0.1, seed=3)
    _bits(a, b, "two runs")
    for k in ("z", "state", "dprop", "dpos"):
        assert np.isfinite(a[k]).all() and np.abs(a[k]).max() > 0, k
    assert all(np.isfinite(v).all() for v in a["g"].values())


@pytest.mark.parametrize("math", ["x6", "x3", "bf16"])
def test_team_and_wide_kernels_agree_bitwise(math):
    case = _case("n6_full")
    params = O.random_params(5)
    outs = []
    for wide in (False, True):
        with _limit(wide):
            batch = case.batch(True)
            assert (E.fused_path(batch, _run(4, math, dropout=0.1, seed=3)) != 0) == (not wide)
            outs.append(_step(params, case, 4, math, dropout=0.1, seed=3, batch=batch, check_path=False))
    _bits(outs[0], outs[1], "team vs wide")


@pytest.mark.parametrize("math", ["x6", "x3"])
def test_stored_dh1pre_steps_agree_bitwise(math):
    case = _case("n6_wide23")
    params = O.random_params(5)
    outs = []
    with E.wide_kernels():
        for k in (0, 3):
            with E.da_stored(k):
                assert E.da_stored_steps() == k
                outs.append(_step(params, case, 4, math, dropout=0.1, seed=3))
    _bits(outs[0], outs[1], "stored dh1pre steps K = 0 vs 3")


@pytest.mark.parametrize("training", [False, True], ids=["inference", "training"])
@pytest.mark.parametrize("name", ["n6_full", "n6_wide23"])
def test_captured_forward_state_replays_identically(name, training):
    case = _case(name)
    flat = P.to_flat(O.random_params(5), device="cuda")
    with _limit(case.wide):
        batch = case.batch(True)
        run = _run(4, "x6", training)
        ws = E.Workspace("cuda")
        ez, es = E.forward(flat, batch, run, ws, return_state=True)
        ez, es = ez.clone(), es.clone()
        z, st = torch.empty_like(ez), torch.empty_like(es)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):      # warm-up on the capture stream's side: nothing allocates inside the capture
            E.forward(flat, batch, run, ws, logits=z, return_state=True, state=st)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            E.forward(flat, batch, run, ws, logits=z, return_state=True, state=st)
        for _ in range(2):
            z.fill_(float("nan"))
            st.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(z, ez) and torch.equal(st, es)


def test_backward_refuses_a_state_cotangent_without_the_state():
    case = _case("n6_full")
    flat = P.to_flat(O.random_params(5), device="cuda")
    batch, run, ws = case.batch(True), _run(2, "x6"), E.Workspace("cuda")
    z = E.forward(flat, batch, run, ws)
    ds = torch.zeros(batch.n_nodes, 100, device="cuda")
    with pytest.raises(ValueError, match="return_state"):
        E.backward(flat, batch, run, ws, torch.zeros_like(z), dstate=ds)
    E.forward(flat, batch, run, ws, return_state=True)
    for bad in (ds[:-1], ds.double(), ds.cpu()):
        with pytest.raises((ValueError, _lib.SpwgnnError)):
            E.backward(flat, batch, run, ws, torch.zeros_like(z), dstate=bad)
    E.backward(flat, batch, run, ws, torch.zeros_like(z), dstate=ds)
    E.forward(flat, batch, run, ws)                     # a plain forward forgets the state again
    with pytest.raises(ValueError, match="return_state"):
        E.backward(flat, batch, run, ws, torch.zeros_like(z), dstate=ds)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------- 6. GraphNetwork
def _net(params, S, math="x6"):
    net = GraphNetwork(mp_steps=S, dropout=0.0, device="cuda", params=params, math=math)
    net.train()
    return net


def test_graph_network_return_state_autograd():
    name, S = "n6_full", 4
    case = _case(name)
    params = X.kink_free_params(1)
    ref_g, ref_dprop, ref_dpos, margin = _grad_ref(name, S, True)
    assert margin >= MIN_RELU_MARGIN
    obj, Rs, Rr = case.groups[0]
    B, N = obj.shape[:2]
    net = _net(params, S)
    o = torch.tensor(obj, device="cuda", requires_grad=True)
    p = torch.tensor(case.prop.reshape(B, N, 100), device="cuda", requires_grad=True)
    z, st = net.forward_logits(o, Rs, Rr, p, return_state=True)
    assert z.shape == (B, N) and st.shape == (B, N, 100)
    prob, st_b = net.forward(o, Rs, Rr, p, return_state=True)
    assert prob.shape == (B, N, 1) and torch.equal(st_b, st) and torch.equal(prob[..., 0], torch.sigmoid(z))
    tp0, objs0, p0 = _leaves(case, params, True, False)
    with torch.no_grad():
        zref, sref = (t.numpy() for t in _oracle_forward(tp0, case, objs0, p0, S))
    assert _close(z.detach().cpu().numpy().reshape(-1), zref) and _close(st.detach().cpu().numpy().reshape(-1, 100), sref)
    tgt = _dev(case.tgt).reshape(B, N)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(z, tgt) + (st.reshape(-1, 100) * _dev(case.w)).sum()
    loss.backward()
    torch.cuda.synchronize()
    got = dict(P.from_flat(net.flat.grad), dprop=p.grad.cpu().numpy().reshape(-1, 100), dpos=o.grad.cpu().numpy().reshape(-1, 3))
    ref = dict(ref_g, dprop=ref_dprop, dpos=ref_dpos)
    for k in ref:
        assert _maxabs(got[k], ref[k]) <= 1e-5 * np.abs(ref[k]).max() + 1e-7, k
    # a loss on the state alone (no logits gradient) and on the logits alone (no state gradient)
    for use_z, use_s in ((False, True), (True, False)):
        net.zero_grad()
        z, st = net.forward_logits(o, Rs, Rr, p, return_state=True)
        l = (st.reshape(-1, 100) * _dev(case.w)).sum() if use_s else torch.nn.functional.binary_cross_entropy_with_logits(z, tgt)
        l.backward()
        torch.cuda.synchronize()
        assert torch.isfinite(net.flat.grad).all() and net.flat.grad.abs().max() > 0
        if use_z:
            net2 = _net(params, S)
            torch.nn.functional.binary_cross_entropy_with_logits(net2.forward_logits(o, Rs, Rr, p), tgt).backward()
            assert torch.equal(net2.flat.grad, net.flat.grad)       # the plain call's gradients, bit for bit


ROLL = (2, 6, 6, 3)     # S, towers, nodes per tower, frames


@functools.lru_cache(maxsize=None)
def _rollout_ref():
    """Three frames of moving towers and the fp64 oracle's chain over them: L = Σ_k BCE(z_k) + Σ w ⊙ P_final."""
    S, B, N, F = ROLL
    params = X.kink_free_params(2)
    rng = np.random.default_rng(23)
    raw0 = D.synthetic_towers(B, N, seed=9).astype(np.float32)
    raws = [raw0]
    for _ in range(F - 1):
        step = np.zeros_like(raw0)
        step[..., :2] = rng.normal(0, 6.0, raw0.shape[:2] + (2,))
        raws.append((raws[-1] + step).astype(np.float32))
    thr = float(D.RELATION_THRESHOLD)
    for raw in raws:     # no pair sits on the threshold: fp32 and fp64 select the same relation set
        d = np.linalg.norm(raw[:, :, None, :2].astype(np.float64) - raw[:, None, :, :2], axis=-1)
        assert np.abs(d - thr)[~np.eye(N, dtype=bool)[None].repeat(B, 0)].min() > 1e-2
    tgts = [rng.integers(0, 2, B * N).astype(np.float32) for _ in range(F)]
    w = rng.normal(0, 1.0 / (B * N), (B * N, 100)).astype(np.float32)
    prop0 = rng.normal(0, 0.3, (B * N, 100)).astype(np.float32)
    # the oracle's chain (fp64)
    tp = O.to_torch(params, requires_grad=True)
    objs = [torch.tensor(r.astype(np.float64) / 170.0, dtype=F64, requires_grad=(k == 0)) for k, r in enumerate(raws)]
    state = torch.tensor(prop0.reshape(B, N, 100), dtype=F64)
    loss, zrefs, margin = 0.0, [], np.inf
    for k, raw in enumerate(raws):
        Rs, Rr = O.relation_matrices(raw.astype(np.float64), thr)
        e = np.array(O.dense_to_edges(Rs, Rr), np.int64).reshape(-1, 4)
        margin = min(margin, O.relu_margins_gather(O.to_torch(params), objs[k].detach().numpy().reshape(-1, 3),
                                                   e[:, 0] * N + e[:, 2], e[:, 0] * N + e[:, 3],
                                                   state.detach().numpy().reshape(-1, 100), np.repeat(np.arange(B), N), B, S).min())
        z, states = O.forward_dense(tp, objs[k], torch.as_tensor(Rs, dtype=F64), torch.as_tensor(Rr, dtype=F64), state, S,
                                    return_state=True)
        state = states[-1]
        zrefs.append(z.detach().numpy().reshape(-1))
        loss = loss + O.keras_bce_from_logits(z.reshape(-1), torch.as_tensor(tgts[k], dtype=F64))
    loss = loss + (torch.as_tensor(w, dtype=F64) * state.reshape(-1, 100)).sum()
    loss.backward()
    grads = {k: v.grad.numpy().copy() for k, v in tp.items()}
    return (params, raws, tgts, w, prop0, zrefs, state.detach().numpy().reshape(-1, 100), grads,
            objs[0].grad.numpy().reshape(-1, 3).copy(), float(margin))


def test_rollout_three_moving_frames_against_the_oracle_chain():
    S, B, N, F = ROLL
    params, raws, tgts, w, prop0, zrefs, sref, ref_g, ref_dobj, margin = _rollout_ref()
    thr = float(D.RELATION_THRESHOLD)
    assert margin >= MIN_RELU_MARGIN, margin
    # the engine: device-filled capacity plans from the raw positions, one per frame
    net = _net(params, S)
    raw_t = [torch.tensor(r, device="cuda") for r in raws]
    batches = [TowerBatch.from_positions(r, thr, 170.0, check=True) for r in raw_t]
    assert len({(b.n_wtiles, b.n_eblocks) for b in batches}) == 1      # one capacity geometry for every frame
    o0 = (raw_t[0].reshape(-1, 3) / 170.0).detach().requires_grad_(True)
    logits, final = net.rollout(batches, torch.tensor(prop0, device="cuda"), objects=[o0, None, None])
    assert len(logits) == F and final.shape == (B * N, 100)
    l = (final * _dev(w)).sum()
    for k in range(F):
        l = l + torch.nn.functional.binary_cross_entropy_with_logits(logits[k], _dev(tgts[k]))
    l.backward()
    torch.cuda.synchronize()
    for k in range(F):       # frame k went through k + 1 calls
        assert _close(logits[k].detach().cpu().numpy(), zrefs[k], k + 1), (k, np.abs(logits[k].detach().cpu().numpy() - zrefs[k]).max())
    assert _close(final.detach().cpu().numpy(), sref, F), np.abs(final.detach().cpu().numpy() - sref).max()
    got = P.from_flat(net.flat.grad)
    for k, ref in ref_g.items():  # three composed backwards: three times the single-call criterion
        assert _maxabs(got[k], ref) <= F * (1e-5 * np.abs(ref).max() + 1e-7), k
    assert np.abs(ref_dobj).max() > 0
    assert _maxabs(o0.grad.cpu().numpy(), ref_dobj) <= F * (1e-5 * np.abs(ref_dobj).max() + 1e-7)


def test_packed_state_rows_map_back_to_input_order():
    case = _case("packed")
    zref, sref = _fwd_ref("packed", 2, True)
    net = GraphNetwork(mp_steps=2, device="cuda", params=O.random_params(5))
    net.eval()
    batch = case.batch(False)
    prop_plan = _dev(batch.to_plan_order(case.prop))
    with torch.no_grad():
        z, st = net.forward_batch(batch, prop_plan, return_state=True)
    torch.cuda.synchronize()
    assert st.shape == (case.n, 100)
    assert _close(batch.to_input_order(st).cpu().numpy(), sref) and _close(batch.to_input_order(z).cpu().numpy(), zref)
    assert not _close(st.cpu().numpy(), sref)            # plan order is not input order for this batch
