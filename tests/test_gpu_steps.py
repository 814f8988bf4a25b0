"""GPU: per-step logits and deep supervision (spwgnn_forward_steps, spwgnn_backward_steps, spwgnn_bce_steps;
DESIGN.md §3zr) against the fp64 oracle (tests/steps_ref.py: step s's logit of an S-step run is the final
logit of the same network at mp_steps = s + 1) and against the existing forward / bce / backward chain.

Shapes: those of tests/test_gpu_state.py (the smallest that reach each path; its Case and its path assertion
with engine.fused_path are reused): n6_full, n9_thr fused loops; n9_thr_recv team kernels; n20_thr 17-32-node
tiles; n12_recv forward only; n6_wide8 / n6_wide23 wide kernels; packed a packed plan. S in {1, 2, 4}
(S = 1: the first backward step is step 0; S = 2: no middle step; S = 4: true middle steps), with and without a
'propagation' input, all five maths.

Tolerances. Logits: the project's 1e-5 + 1e-5·|ref| for f32, x6, h3. Gradients: the project's
1e-5·max|g| + 1e-7 for f32, x6, h3. x3 and bf16 are not fp32-class: a row s is held to 3·d_s, d_s that math's
own distance to the oracle from the EXISTING engine.forward / backward at mp_steps = s + 1 on the same case
(test_gpu_state.py's rule), and a gradient of Σ_s λ_s·BCE(z_s) to 3·Σ_s λ_s·d_s (+ 3·d_state with a state
cotangent, d_state the existing backward_state's distance on Σ w ⊙ P_S alone): the gradient is linear in the
cotangents, so the errors of the terms add with their weights. λ_s·d_s is MEASURED with the weight inside: the
existing backward at mp_steps = s + 1 is run on the cotangent row λ_s·dBCE(z_s) that the per-step backward is
given for that step, and compared with λ_s times the oracle's term. In exact arithmetic that is λ_s times the
distance at λ = 1; in x3 / bf16 it is not, because the two-part split of an operand is not scale-invariant and at
λ = 1 some sums happen to be exactly representable (n6_full, S = 1, x3, omp.1.bias: distance 1.2e-9 at λ = 1
and 2.6e-7 at λ = 0.78 from the very same launches — at S = 1 the per-step backward IS the existing one).
The oracle gradient of the sum is assembled from per-term autograd gradients (autograd is linear too), which
the d_s need anyway. Gradient tests use x3_emu.kink_free_params and assert, on the oracle, ReLU margins
>= 0.1 and every |z_s| at least 1 away from the BCE clip: conditions on the inputs, no case is skipped.
The whole file also passes under SPWGNN_POISON_WORKSPACE=1."""
import functools

import numpy as np
import pytest
import torch

import steps_ref as SR
import test_gpu_state as TS
import x3_emu as X
from oracle import model as O
from spwgnn_amd import TowerBatch, data as D, engine as E, params as P
from spwgnn_amd.keras_api import CompactDataset, PropagationNetwork
from spwgnn_amd.network import GraphNetwork
from spwgnn_amd.trainer import Trainer

pytestmark = pytest.mark.gpu

F64 = torch.float64
MATHS = ["f32", "x6", "h3", "x3", "bf16"]
FP32_CLASS = ("f32", "x6", "h3")
SHAPES, BWD_SHAPES = list(TS.SHAPES), TS.BWD_SHAPES
DROP_SEED, RATE = 77, 0.1
_case, _limit, _run, _dev, _close, _maxabs = TS._case, TS._limit, TS._run, TS._dev, TS._close, TS._maxabs


def _rows(batch, Z):
    """(S, n) device rows in the plan's node order -> numpy in the input's."""
    return batch.to_input_order(Z.detach().cpu().numpy().T).T


def _plan(batch, x):
    return _dev(batch.to_plan_order(np.asarray(x, np.float32)))


def _lams(S, which):
    if which == "uniform":
        return tuple([1.0 / S] * S)
    lam = np.random.default_rng(40 + S).uniform(0.2, 1.0, S)
    if S >= 3:
        lam[1] = 0.0          # a step of zero weight between weighted ones (>= 2 stay non-zero)
    return tuple(float(x) for x in lam.astype(np.float32))


@functools.lru_cache(maxsize=None)
def _node_w(name):
    case = _case(name)
    w = np.random.default_rng(23).choice([0.5, 1.0, 2.5], size=case.n).astype(np.float32)
    w[case.n // 2] = 0.0
    return w


# ----------------------------------------------------------------------------------------- oracle
@functools.lru_cache(maxsize=None)
def _steps_ref(name, prop, train):
    """(4, n) oracle rows, input node order (the rows of an S-step run are its first S)."""
    case = _case(name)
    tp, objs, p = TS._leaves(case, O.random_params(5), prop, False)
    with torch.no_grad():
        return SR.step_logits(tp, case.groups, objs, p, 4, DROP_SEED if train else None, RATE if train else 0.0).numpy()


def _collect(tp, objs, p):
    g = {k: v.grad.numpy().copy() for k, v in tp.items()}
    g["dprop"] = p.grad.numpy().copy()
    g["dpos"] = np.concatenate([o.grad.numpy().reshape(-1, 3) for o in objs])
    return g


@functools.lru_cache(maxsize=None)
def _term_ref(name, k, prop, weighted):
    """fp64 gradient of BCE(z of the k-step network) — one term of the deep loss — and that z."""
    case = _case(name)
    tp, objs, p = TS._leaves(case, X.kink_free_params(1), prop, True)
    z = SR._forward(tp, case.groups, objs, p, k)
    w = torch.as_tensor(_node_w(name), dtype=F64) if weighted else None
    norm = float(np.count_nonzero(_node_w(name))) if weighted else None
    SR.bce_row(z, torch.as_tensor(case.tgt, dtype=F64), w, norm).backward()
    return _collect(tp, objs, p), z.detach().numpy()


@functools.lru_cache(maxsize=None)
def _state_ref(name, S, prop):
    case = _case(name)
    tp, objs, p = TS._leaves(case, X.kink_free_params(1), prop, True)
    (torch.as_tensor(case.w, dtype=F64) * SR.final_state(tp, case.groups, objs, p, S)).sum().backward()
    return _collect(tp, objs, p)


def _assert_inputs_clear_of_kinks(name, S, prop):
    case = _case(name)
    margin = TS._margin(case, X.kink_free_params(1), prop, S)      # mp_steps = S covers every step's ReLUs
    assert margin >= TS.MIN_RELU_MARGIN, margin
    for k in range(1, S + 1):
        z = _term_ref(name, k, prop, False)[1]
        assert np.abs(np.abs(z) - O.LOGIT_CLIP).min() >= 1.0, (k, np.abs(z).max())
    return margin


# ----------------------------------------------------------------------------------------- engine
def _out(batch, g, dp, dpos):
    back = lambda t: batch.to_input_order(t.cpu().numpy())
    return dict(P.from_flat(g), dprop=back(dp), dpos=back(dpos))


def _steps_grads(case, S, math, prop, lam, weighted=False, dstate=False):
    """forward_steps -> bce_steps -> backward_steps (-> backward_inputs) with kink-free parameters."""
    batch = case.batch(prop)
    flat = P.to_flat(X.kink_free_params(1), device="cuda")
    ws, run = E.Workspace("cuda"), _run(S, math)
    TS._assert_path(case.name, batch, run)
    out = E.forward_steps(flat, batch, run, ws, return_state=dstate)
    Z = out[0] if dstate else out
    w = _plan(batch, _node_w(case.name)) if weighted else None
    o3, o3s, dZ = E.bce_steps(Z, _plan(batch, case.tgt), lam, E.BceStepsScratch("cuda", S), node_weights=w)
    g, dp = E.backward_steps(flat, batch, run, ws, dZ, want_dprop=True, dstate=_plan(batch, case.w) if dstate else None)
    dpos = E.backward_inputs(flat, batch, run, ws)
    torch.cuda.synchronize()
    return _out(batch, g, dp, dpos), _rows(batch, Z), o3.cpu().numpy().copy()


def _plain_grads(case, k, math, prop, weighted=False, scale=1.0, state_only=False):
    """The EXISTING chain at mp_steps = k: forward -> bce -> backward (dlogits·scale) -> backward_inputs; with
    state_only the existing backward_state of Σ w ⊙ P_S alone (zero dlogits)."""
    batch = case.batch(prop)
    flat = P.to_flat(X.kink_free_params(1), device="cuda")
    ws, run = E.Workspace("cuda"), _run(k, math)
    z = E.forward(flat, batch, run, ws, return_state=state_only)
    if state_only:
        dz, ds = torch.zeros_like(z[0]), _plan(batch, case.w)
    else:
        w = _plan(batch, _node_w(case.name)) if weighted else None
        dz, ds = E.bce(z, _plan(batch, case.tgt), E.BceScratch("cuda"), node_weights=w)[1] * scale, None
    g, dp = E.backward(flat, batch, run, ws, dz, want_dprop=True, dstate=ds)
    dpos = E.backward_inputs(flat, batch, run, ws)
    torch.cuda.synchronize()
    return _out(batch, g, dp, dpos)


@functools.lru_cache(maxsize=None)
def _term_dist(name, k, prop, math, weighted, lam_k):
    """λ_k·d_k per tensor: the existing backward's distance to the oracle on λ_k·BCE(z at mp_steps = k), run
    with the cotangent row the per-step backward is given for that step (see the module docstring)."""
    case = _case(name)
    with _limit(case.wide):
        got = _plain_grads(case, k, math, prop, weighted, scale=lam_k)
    ref = _term_ref(name, k, prop, weighted)[0]
    return {key: _maxabs(got[key], lam_k * ref[key]) for key in ref}


@functools.lru_cache(maxsize=None)
def _state_dist(name, S, prop, math):
    case = _case(name)
    with _limit(case.wide):
        got = _plain_grads(case, S, math, prop, state_only=True)
    ref = _state_ref(name, S, prop)
    return {key: _maxabs(got[key], ref[key]) for key in ref}


# ------------------------------------------------------------------------------ 1. forward parity
@pytest.mark.parametrize("prop", [True, False], ids=["prop", "noprop"])
@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("name", SHAPES)
def test_step_logits_against_oracle(name, S, prop):
    """Every row, every math, inference and training with dropout 0.1 (the restated masks); the last row is
    engine.forward's logits bit for bit."""
    case = _case(name)
    flat = P.to_flat(O.random_params(5), device="cuda")
    with _limit(case.wide):
        batch = case.batch(prop)
        for train in (False, True):
            ref = _steps_ref(name, prop, train)[:S]
            for math in MATHS:
                mk = lambda k: _run(k, math, train, dropout=RATE if train else 0.0, seed=DROP_SEED)
                TS._assert_path(name, batch, mk(S))
                Z = torch.full((S, batch.n_nodes), float("nan"), device="cuda")
                assert E.forward_steps(flat, batch, mk(S), E.Workspace("cuda"), step_logits=Z) is Z
                z = E.forward(flat, batch, mk(S), E.Workspace("cuda"))
                assert torch.equal(Z[-1], z), (math, train)
                got = _rows(batch, Z)
                assert np.isfinite(got).all(), "a row was left unwritten"
                for s in range(S):
                    err = np.abs(got[s] - ref[s]).max()
                    if math in FP32_CLASS:
                        assert _close(got[s], ref[s]), (math, train, s, err)
                        continue
                    zs = E.forward(flat, batch, mk(s + 1), E.Workspace("cuda"))
                    d = np.abs(batch.to_input_order(zs.cpu().numpy()) - ref[s]).max()
                    print(f"steps fwd {name} S={S} prop={prop} {math} train={train} s={s}: err {err:.3e} d_s {d:.3e}")
                    assert err <= 3 * d, (math, train, s, err, d)


# ------------------------------------------------------------------ 2. bitwise ties to the existing path
@pytest.mark.parametrize("poison", [False, True], ids=["clean", "poisoned"])
@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("name", BWD_SHAPES)
def test_last_step_weight_alone_is_the_existing_chain_bitwise(name, S, poison, monkeypatch):
    """λ = e_{S-1}: out3, the last dlogits row, grads, dprop and backward_inputs carry the bits of
    forward -> bce -> backward; with and without a 'propagation' input / dprop request, plain and node-weighted."""
    monkeypatch.setattr(E, "POISON_WORKSPACE", poison)
    case = _case(name)
    flat = P.to_flat(O.random_params(5), device="cuda")
    lam = tuple([0.0] * (S - 1) + [1.0])
    with _limit(case.wide):
        for math in MATHS:
            for prop, weighted in ((True, False), (False, False), (True, True)):
                batch = case.batch(prop)
                run = _run(S, math, dropout=RATE, seed=3)
                TS._assert_path(name, batch, run)
                tgt = _plan(batch, case.tgt)
                w = _plan(batch, _node_w(name)) if weighted else None
                ws = E.Workspace("cuda")
                z = E.forward(flat, batch, run, ws)
                out3, dz = E.bce(z, tgt, E.BceScratch("cuda"), node_weights=w)
                out3 = out3.clone()
                g, dp = E.backward(flat, batch, run, ws, dz, want_dprop=prop)
                dpos = E.backward_inputs(flat, batch, run, ws).clone()
                ws2 = E.Workspace("cuda")
                Z = E.forward_steps(flat, batch, run, ws2)
                o3, o3s, dZ = E.bce_steps(Z, tgt, lam, E.BceStepsScratch("cuda", S), node_weights=w)
                g2, dp2 = E.backward_steps(flat, batch, run, ws2, dZ, want_dprop=prop)
                dpos2 = E.backward_inputs(flat, batch, run, ws2)
                torch.cuda.synchronize()
                what = (math, prop, weighted)
                assert torch.equal(Z[-1], z), what
                assert torch.equal(o3, out3) and torch.equal(o3s[-1], out3), what
                assert torch.equal(dZ[-1], dz), what
                assert not dZ[:-1].any() and not torch.signbit(dZ[:-1]).any(), what      # +0 rows
                assert torch.equal(g2, g), what
                assert (dp2 is None and dp is None) or torch.equal(dp2, dp), what
                assert torch.equal(dpos2, dpos), what
                assert torch.isfinite(g2).all(), what


# ------------------------------------------------------------------------------ 3. gradient parity
def _bound(math, ref, terms):
    """fp32-class: the project's criterion on the total; x3 / bf16: 3·Σ (weight · that term's own distance)."""
    if math in FP32_CLASS:
        return {k: 1e-5 * np.abs(ref[k]).max() + 1e-7 for k in ref}
    return {k: 3.0 * sum(wt * d[k] for wt, d in terms) for k in ref}


@pytest.mark.parametrize("prop", [True, False], ids=["prop", "noprop"])
@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("name", BWD_SHAPES)
def test_deep_supervision_gradients_against_oracle(name, S, prop):
    """Weights, dprop and d objects of Σ_s λ_s·BCE(z_s): a random λ (a zero in it for S >= 3), the uniform
    λ = 1/S together with a state cotangent, and random per-node weights, one of them zero."""
    case = _case(name)
    margin = _assert_inputs_clear_of_kinks(name, S, prop)
    worst = 0.0
    for which, weighted, dstate in (("random", False, False), ("uniform", False, True), ("random", True, False)):
        lam = _lams(S, which)
        ref = None
        for s, l in enumerate(lam):
            if l == 0:
                continue
            term = _term_ref(name, s + 1, prop, weighted)[0]
            ref = {k: l * term[k] + (ref[k] if ref else 0.0) for k in term}
        if dstate:
            st = _state_ref(name, S, prop)
            ref = {k: ref[k] + st[k] for k in ref}
        for math in MATHS:
            with _limit(case.wide):
                got, _, _ = _steps_grads(case, S, math, prop, lam, weighted, dstate)
            terms = []
            if math not in FP32_CLASS:
                terms = [(1.0, _term_dist(name, s + 1, prop, math, weighted, l)) for s, l in enumerate(lam) if l != 0]
                if dstate:
                    terms.append((1.0, _state_dist(name, S, prop, math)))
            bound = _bound(math, ref, terms)
            for k in ref:
                assert np.abs(ref[k]).max() > 0, k
                err = _maxabs(got[k], ref[k])
                worst = max(worst, err / bound[k])
                if err > bound[k]:
                    print(f"MISS deep gradients {name} S={S} prop={prop} {which} w={weighted} st={dstate} {math} {k}: "
                          f"err {err:.3e} bound {bound[k]:.3e} ratio {err / bound[k]:.2f}")
                assert err <= bound[k], (which, weighted, dstate, math, k, err, bound[k])
    print(f"deep gradients {name} S={S} prop={prop}: ReLU margin {margin:.3f}, worst err / bound {worst:.3f}")


# ---------------------------------------------------------------------- 4. decomposition on the device
@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("name", BWD_SHAPES)
def test_backward_steps_is_the_sum_of_the_existing_backwards(name, S):
    """backward_steps with cotangent rows c_s = λ_s·dBCE(z_s) equals Σ_s of the existing backward at
    mp_steps = s + 1 with c_s, within the sum of the per-term criteria (fp32-class: 1e-5·max|g_s| + 1e-7 per
    term; x3 / bf16: 3·λ_s·d_s per term)."""
    case = _case(name)
    _assert_inputs_clear_of_kinks(name, S, True)
    lam = _lams(S, "random")
    for math in MATHS:
        with _limit(case.wide):
            got, _, _ = _steps_grads(case, S, math, True, lam)
            parts = [_plain_grads(case, s + 1, math, True, scale=l) for s, l in enumerate(lam) if l != 0]
        for k in got:
            total = sum(np.asarray(p[k], np.float64) for p in parts)
            if math in FP32_CLASS:
                bound = sum(1e-5 * np.abs(p[k]).max() + 1e-7 for p in parts)
            else:
                bound = sum(3.0 * _term_dist(name, s + 1, True, math, False, l)[k] for s, l in enumerate(lam) if l != 0)
            err = _maxabs(got[k], total)
            assert err <= bound, (math, k, err, bound)


# ------------------------------------------------------------------------------- 5. the loss kernel
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "node_weights"])
@pytest.mark.parametrize("n", [18, 256, 257, 1000, 70001])
def test_bce_steps_against_fp64(n, weighted):
    """n = 18 under one wave, 256 one workgroup exactly (the one-launch form), 257 two workgroups, 1000 not a
    multiple of the 256-node tile, 70,001 the 256 capped workgroups with a grid stride. Row 1 has λ = 0 over NaN
    logits. 1e-6 relative: the bound tests/test_gpu_loss_weights.py derives for this reduction scheme (fp32
    strided sums, 256-wide tree, fp64 final; expf / log1pf a few ulp per term). Counts are exact; two runs agree
    bit for bit; the epoch sums equal the host's fp64 products bit for bit."""
    S, lam = 3, (0.5, 0.0, 2.0)
    rng = np.random.default_rng(n)
    Z = rng.normal(scale=3.0, size=(S, n)).astype(np.float32)
    Z[0, 0], Z[2, n - 1] = 20.0, -17.5          # beyond the clip: zero gradient there
    assert np.abs(Z).min() > 1e-6
    t = rng.integers(0, 2, n).astype(np.float32)
    w = rng.choice([0.0, 0.5, 1.0, 2.5], size=n).astype(np.float32) if weighted else None
    norm = float(max(np.count_nonzero(w), 1)) if weighted else None
    o3s_ref, o3_ref, dl_ref = SR.bce_steps_numpy(Z[[0, 2]], t, (lam[0], lam[2]), w, norm)
    Zn = Z.copy()
    Zn[1] = np.nan
    w3 = torch.tensor([float(n), 1.0, 1.0], dtype=torch.float64, device="cuda")
    runs = []
    for _ in range(2):
        tot, tots = torch.zeros(3, dtype=F64, device="cuda"), torch.zeros(S, 3, dtype=F64, device="cuda")
        sc = E.BceStepsScratch("cuda", S)
        for _ in range(2):      # two batches into the same sums
            o3, o3s, dl = E.bce_steps(_dev(Zn), _dev(t), lam, sc, total3=tot, weights3=w3, total3s=tots,
                                      node_weights=None if w is None else _dev(w))
        torch.cuda.synchronize()
        runs.append([x.cpu().numpy().copy() for x in (o3, o3s, dl, tot, tots)])
    for a, b in zip(*runs):
        np.testing.assert_array_equal(a, b)
    o3, o3s, dl, tot, tots = runs[0]
    assert np.all(dl[1] == 0.0) and not np.signbit(dl[1]).any()            # +0 under the zero step weight
    for row, r in ((0, 0), (2, 1)):
        assert abs(o3s[row, 0] - o3s_ref[r, 0]) <= 1e-6 * max(1.0, abs(o3s_ref[r, 0]))
        assert o3s[row, 1] == o3s_ref[r, 1] and o3s[row, 2] == o3s_ref[r, 2]
        assert np.abs(dl[row] - dl_ref[r]).max() <= 1e-6 * np.abs(dl_ref[r]).max()
    assert dl[0, 0] == 0.0 and dl[2, n - 1] == 0.0
    assert abs(o3[0] - o3_ref[0]) <= 1e-6 * max(1.0, abs(o3_ref[0])) and np.isfinite(o3).all()
    assert o3[1] == o3_ref[1] and o3[2] == o3_ref[2] and o3[2] == (norm if weighted else n)
    print(f"bce_steps n={n} weighted={weighted}: combined {o3[0]:.9g} ref {o3_ref[0]:.9g}")
    host = 2 * o3.astype(np.float64) * np.array([float(n), 1.0, 1.0])
    np.testing.assert_array_equal(tot, host)
    for row in (0, 2):
        np.testing.assert_array_equal(tots[row], 2 * o3s[row].astype(np.float64) * np.array([float(n), 1.0, 1.0]))
    # λ = e_{S-1} carries spwgnn_bce / spwgnn_bce_weighted's bits
    o3b, dzb = E.bce(_dev(Z[2]), _dev(t), E.BceScratch("cuda"), node_weights=None if w is None else _dev(w))
    o3e, _, dle = E.bce_steps(_dev(Zn), _dev(t), (0.0, 0.0, 1.0), E.BceStepsScratch("cuda", S),
                              node_weights=None if w is None else _dev(w))
    assert torch.equal(o3e, o3b) and torch.equal(dle[2], dzb)


# ----------------------------------------------------------------------------- 6. the Python surface
@pytest.mark.parametrize("name", ["n6_full", "packed", "n6_wide23"])
def test_graph_network_return_steps_autograd(name):
    """forward_batch(return_steps=True): rows in the input's node order, autograd in the weights, 'propagation'
    and objects equal to the engine calls bit for bit and to the oracle of case 3; combines with return_state."""
    S, case = 4, _case(name)
    lam = _lams(S, "random")
    _assert_inputs_clear_of_kinks(name, S, True)
    tgt = torch.as_tensor(case.tgt, device="cuda")
    with _limit(case.wide):
        net = GraphNetwork(mp_steps=S, dropout=0.0, params=X.kink_free_params(1), math="x6")
        batch = case.batch(False)
        prop = torch.tensor(batch.to_plan_order(case.prop), device="cuda", requires_grad=True)   # plan order, as forward_batch takes it
        objects = torch.tensor(case.pos, device="cuda", requires_grad=True)                      # input order
        Z = net.forward_batch(batch, prop, objects, return_steps=True)
        assert Z.shape == (S, case.n)
        SR.deep_loss(Z, tgt, lam).backward()
        # the engine calls with the same cotangent rows
        flat = net.flat.detach()
        b2 = batch.with_prop(prop.detach())
        ws, run = E.Workspace("cuda"), _run(S, "x6")
        Z2 = E.forward_steps(flat, b2, run, ws)
        np.testing.assert_array_equal(Z.detach().cpu().numpy(), _rows(b2, Z2))
        Zi = torch.tensor(_rows(b2, Z2), device="cuda", requires_grad=True)
        SR.deep_loss(Zi, tgt, lam).backward()
        dZ = _dev(batch.to_plan_order(Zi.grad.cpu().numpy().T).T)
        g, dp = E.backward_steps(flat, b2, run, ws, dZ, want_dprop=True)
        dpos = E.backward_inputs(flat, b2, run, ws)
        assert torch.equal(net.flat.grad, g) and torch.equal(prop.grad, dp)
        np.testing.assert_array_equal(objects.grad.cpu().numpy(), batch.to_input_order(dpos.cpu().numpy()))
        # the oracle (case 3's criterion for x6)
        ref = None
        for s, l in enumerate(lam):
            if l:
                term = _term_ref(name, s + 1, True, False)[0]
                ref = {k: l * term[k] + (ref[k] if ref else 0.0) for k in term}
        got = _out(batch, net.flat.grad, prop.grad, batch.to_plan_order(objects.grad))
        for k in ref:
            assert _maxabs(got[k], ref[k]) <= 1e-5 * np.abs(ref[k]).max() + 1e-7, k
        # with the state, and without autograd
        with torch.no_grad():
            Zs, st = net.forward_batch(batch, prop.detach(), return_state=True, return_steps=True)
            z1, st1 = net.forward_batch(batch, prop.detach(), return_state=True)
        assert Zs.shape == (S, case.n) and torch.equal(st, st1)
        np.testing.assert_array_equal(batch.to_input_order(z1.cpu().numpy()), Zs[-1].cpu().numpy())


def test_dense_front_ends_return_steps():
    obj, Rs, Rr, prop, _ = D.synthetic_batch(3, 5, seed=3, fully_connected=False)
    net = GraphNetwork(mp_steps=3, dropout=0.0, seed=2).eval()
    with torch.no_grad():
        Z = net.forward_logits(obj, Rs, Rr, prop, return_steps=True)
        z = net.forward_logits(obj, Rs, Rr, prop)
        Pz = net(obj, Rs, Rr, prop, return_steps=True)
        Pst = net(obj, Rs, Rr, prop, return_steps=True, return_state=True)
    assert Z.shape == (3, 3, 5) and torch.equal(Z[-1], z)
    assert Pz.shape == (3, 3, 5, 1) and torch.equal(Pz, torch.sigmoid(Z)[..., None])
    assert torch.equal(Pst[0], Pz) and Pst[1].shape == (3, 5, 100)
    model = PropagationNetwork(seed=2, mp_steps=3).getModel(5)
    x = {"objects": obj, "sender_relations": Rs, "receiver_relations": Rr, "propagation": prop}
    ps, p = model.predict(x, return_steps=True), model.predict(x)
    assert ps.shape == (3, 5, 3) and np.array_equal(ps[..., -1], p[..., 0])
    assert np.abs(ps[..., 0] - ps[..., -1]).max() > 0


FIT_B, FIT_N, FIT_BATCH, FIT_EPOCHS = 64, 6, 32, 2


@functools.lru_cache(maxsize=None)
def _fit_data():
    obj, Rs, Rr, prop, tgt = D.synthetic_batch(FIT_B, FIT_N, seed=7, fully_connected=False)
    return ({"objects": obj, "sender_relations": Rs, "receiver_relations": Rr, "propagation": prop},
            {"target": tgt.reshape(FIT_B, FIT_N, 1)})


def _fit(graph, lam, **opt):
    x, y = _fit_data()
    model = PropagationNetwork(seed=4, step_loss_weights=lam, **opt).getModel(FIT_N)
    h = model.fit(x, y, batch_size=FIT_BATCH, epochs=FIT_EPOCHS, verbose=0, graph=graph)
    torch.cuda.synchronize()
    return h, model.net.flat.detach().cpu().numpy().copy(), model


def _hand_loop(lam, **opt):
    """fit's batches through train_on_batch, the sums taken on the host in fit's arithmetic."""
    x, y = _fit_data()
    tgt = y["target"].reshape(FIT_B, FIT_N)
    ds = CompactDataset(x["objects"], x["sender_relations"], x["receiver_relations"], x["propagation"])
    model = PropagationNetwork(seed=4, step_loss_weights=lam, **opt).getModel(FIT_N)
    rng = np.random.default_rng(0)
    hist = {"loss": [], "binary_accuracy": [], "step_loss": [], "step_binary_accuracy": []}
    for _ in range(FIT_EPOCHS):
        order = rng.permutation(FIT_B)
        tot, tots = np.zeros(3), np.zeros((5, 3))
        for b0 in range(0, FIT_B, FIT_BATCH):
            idx = order[b0:b0 + FIT_BATCH]
            w3 = np.array([float(len(idx)), 1.0, 1.0])
            batch = TowerBatch.from_plan(ds.subset_plan(idx, edge_cap=True), "cuda")
            out3 = model.train_on_batch(batch, _dev(tgt[idx].reshape(-1)))
            tot += out3.double().cpu().numpy() * w3
            if lam is not None:
                tots += model.step_out3.double().cpu().numpy() * w3
        hist["loss"].append(tot[0] / FIT_B)
        hist["binary_accuracy"].append(tot[1] / tot[2])
        hist["step_loss"].append([r[0] / FIT_B for r in tots.tolist()])
        hist["step_binary_accuracy"].append([r[1] / max(r[2], 1) for r in tots.tolist()])
    torch.cuda.synchronize()
    return hist, model.net.flat.detach().cpu().numpy().copy()


def test_fit_with_step_loss_weights():
    """64 towers of 6, 2 epochs, uniform λ: eager and graph=True agree bit for bit; the history has the per-step
    keys; loss, binary_accuracy, step_loss and the final parameters equal a host-driven train_on_batch loop bit
    for bit; the options of the Adam step keep working with it."""
    lam = [0.2] * 5
    h_eager, p_eager, m = _fit(False, lam)
    h_graph, p_graph, mg = _fit(True, lam)
    assert h_eager == h_graph and np.array_equal(p_eager, p_graph)
    assert sum(s.replays for s in mg._replays.steps.values()) > 0
    assert set(h_eager) == {"loss", "binary_accuracy", "step_loss", "step_binary_accuracy"}
    assert all(len(r) == 5 for r in h_eager["step_loss"] + h_eager["step_binary_accuracy"]) and len(h_eager["step_loss"]) == 2
    hand, p_hand = _hand_loop(lam)
    assert hand == h_eager and np.array_equal(p_hand, p_eager)
    # loss is the weighted sum of the step losses (each a quotient of fp64 sums: equal to rounding), the
    # accuracy the last step's
    for ep in range(FIT_EPOCHS):
        assert abs(h_eager["loss"][ep] - sum(l * s for l, s in zip(lam, h_eager["step_loss"][ep]))) <= 1e-6
        assert h_eager["binary_accuracy"][ep] == h_eager["step_binary_accuracy"][ep][-1]
    # clipnorm / decay / skip_nonfinite with it: eager == graph == hand loop, and the history keeps both sets of keys
    opt = dict(clipnorm=0.05, decay=1e-3, skip_nonfinite=True)
    hc, pc, _ = _fit(False, lam, **opt)
    hg, pg, _ = _fit(True, lam, **opt)
    assert hc == hg and np.array_equal(pc, pg) and not np.array_equal(pc, p_eager)
    assert {"grad_norm", "clipped_steps", "skipped_steps", "step_loss"} <= set(hc)
    hh, ph = _hand_loop(lam, **opt)
    assert all(hh[k] == hc[k] for k in hh) and np.array_equal(ph, pc)


def test_fit_without_step_loss_weights_is_the_plain_fit():
    """None: the history keys and the trajectory of the plain step (forward, bce, backward, Adam through
    train_on_batch), bit for bit; and the weights do change the trajectory."""
    h0, p0, m0 = _fit(False, None)
    assert set(h0) == {"loss", "binary_accuracy"} and m0._tot_s is None
    hand, p_hand = _hand_loop(None)
    assert hand["loss"] == h0["loss"] and hand["binary_accuracy"] == h0["binary_accuracy"] and np.array_equal(p_hand, p0)
    _, p1, _ = _fit(False, [0.2] * 5)
    assert not np.array_equal(p0, p1)
    # λ = e_{S-1} is the plain loss through the per-step path: the same trajectory bit for bit
    h2, p2, _ = _fit(False, [0, 0, 0, 0, 1.0])
    assert h2["loss"] == h0["loss"] and h2["binary_accuracy"] == h0["binary_accuracy"] and np.array_equal(p2, p0)


def test_trainer_step_and_replay_with_step_loss_weights():
    """Single rank: Trainer.step equals KerasModel.train_on_batch's arithmetic (same forward_steps / bce_steps /
    backward_steps / Adam; the dropout keys differ, so dropout is off) and its replayed body equals step."""
    from spwgnn_amd.replay import ReplayStep
    lam = [0.1, 0.2, 0.7]
    x, y = _fit_data()
    ds = CompactDataset(x["objects"], x["sender_relations"], x["receiver_relations"], x["propagation"])
    tgt = y["target"].reshape(FIT_B, FIT_N)
    plans = [ds.subset_plan(np.arange(k * 16, k * 16 + 16), edge_cap=True) for k in range(3)]
    tgts = [tgt[k * 16:k * 16 + 16].reshape(-1) for k in range(3)]
    params = O.random_params(4)
    net = GraphNetwork(mp_steps=3, dropout=0.0, params=params)
    from spwgnn_amd.keras_api import KerasModel
    km = KerasModel(net, FIT_N, step_loss_weights=lam)
    ta = Trainer(P.to_flat(params, device="cuda"), mp_steps=3, dropout=0.0, seed=11, step_loss_weights=lam)
    tb = Trainer(P.to_flat(params, device="cuda"), mp_steps=3, dropout=0.0, seed=11, step_loss_weights=lam)
    rs = ReplayStep(plans[0], "cuda", tb.replay_body(plans[0].n_nodes))
    for p, t in zip(plans, tgts):
        b = TowerBatch.from_plan(p, "cuda")
        o_k = km.train_on_batch(b, _dev(t)).clone()
        o_t = ta.step(b, _dev(t))
        assert torch.equal(o_k, o_t)
        tb.replay_step(rs, p, t)
    torch.cuda.synchronize()
    assert rs.replays == 2 and tb.iterations == 3
    assert torch.equal(net.flat.detach(), ta.params) and torch.equal(km.m, ta.m) and torch.equal(km.v, ta.v)
    assert torch.equal(ta.params, tb.params) and torch.equal(ta.m, tb.m) and torch.equal(ta.v, tb.v)
    assert ta.engine.out3s.shape == (3, 3)
