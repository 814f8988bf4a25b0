"""fp64 reference of the per-step relation gates — TEST INFRASTRUCTURE ONLY, a plain module like
relation_gates_ref.py. The oracle is relation_grad_ref.forward_gather_gated, which takes gates[s] per step; `forward`
below is that function with the final state returned beside the logits (tests/test_step_gates_host.py holds the two
equal bit for bit).

Gate sets: row s is relation_gates_ref.gates_for(E, seed + s), so every row holds 0, 1 and −0.5 and no two rows are
equal. `step_gated_margins` is relation_gates_ref.gated_margins under the per-step gated forward; no tower is ever
left out: a case whose margin falls below TAU takes the next seed (`pick_step_gates`).

The mutants the GPU criteria must catch: `rotated` (row s−1 used at step s) and `row0` (row 0 used at every step).
"""
import numpy as np
import torch

import relation_gates_ref as GR
import relation_grad_ref as RR
from oracle import model as O

F64 = torch.float64
TAU = GR.TAU
GATE_SEED = GR.GATE_SEED


def step_gates_for(n_edges: int, steps: int, seed: int = GATE_SEED) -> np.ndarray:
    """(S, E) fp32: row s is GR.gates_for(E, seed + s)."""
    return np.stack([GR.gates_for(n_edges, seed + s) for s in range(steps)])


def rotated(gates: np.ndarray) -> np.ndarray:
    """The mutant of a wrong step index: step s reads row s − 1 (step 0 the last row)."""
    return np.roll(np.asarray(gates), 1, axis=0)


def row0(gates: np.ndarray) -> np.ndarray:
    """The mutant of a stride that is not applied: every step reads row 0."""
    g = np.asarray(gates)
    return np.repeat(g[:1], g.shape[0], axis=0)


def forward(p, pos, src, dst, prop, mp_steps, gates, drop_r=None, drop_o=None):
    """(logits (Nn,), final state (Nn, 100)): RR.forward_gather_gated, gates[s] (Ne,) at step s."""
    diff = pos[dst, 0:2] - pos[src, 0:2]
    c_r = torch.relu(O._mlp(diff, p, "rm"))
    c_o = torch.relu(O._mlp(pos[:, 1:3], p, "om"))
    if drop_r is not None:
        c_r = c_r * drop_r
    if drop_o is not None:
        c_o = c_o * drop_o
    P, x = prop, None
    for s in range(mp_steps):
        x = O._mlp(torch.cat([c_r, P[src], P[dst]], dim=-1), p, "rmp")
        agg = torch.zeros(P.shape[0], x.shape[1], dtype=x.dtype).index_add_(0, dst, x * gates[s][:, None])
        x = O._mlp(torch.cat([c_o, torch.tanh(agg), P], dim=-1), p, "omp")
        P = torch.tanh(x[:, 1:] + P)
    return x[:, 0], P


def _tensors(c):
    return torch.as_tensor(np.asarray(c["src"], np.int64)), torch.as_tensor(np.asarray(c["dst"], np.int64))


def step_gated_margins(c, gates, sizes=None, groups: bool = False):
    """Per tower: the smallest ReLU pre-activation distance (and logit-to-clip distance) of the per-step gated fp64
    forward — GR.gated_margins with gates[s] at step s. ``groups``: instead a dict {layer group: the smallest distance
    over all towers} for the groups "encoders" (rm, om), "rmp" and "omp" (the step loop's two kinds of ReLU)."""
    sizes = np.full(c["B"], c["N"]) if sizes is None else np.asarray(sizes)
    tower = torch.as_tensor(np.repeat(np.arange(len(sizes)), sizes))
    p = O.to_torch(c["params"])
    src, dst = _tensors(c)
    x = torch.as_tensor(np.asarray(c["obj"], np.float64).reshape(-1, 3))
    P = torch.as_tensor(np.asarray(c["prop"], np.float64).reshape(-1, 100))
    w = torch.as_tensor(np.asarray(gates, np.float64))
    assert w.shape == (c["S"], len(src))
    et = tower[dst]
    marg = torch.full((len(sizes),), float("inf"), dtype=F64)
    by_group = {"encoders": float("inf"), "rmp": float("inf"), "omp": float("inf")}
    group = ["encoders"]

    def note(pre, rows_tower):
        marg.scatter_reduce_(0, rows_tower, pre.abs().amin(dim=1), reduce="amin")
        if group[0] is not None:
            by_group[group[0]] = min(by_group[group[0]], float(pre.abs().min()))

    with torch.no_grad():
        h = x[dst, 0:2] - x[src, 0:2]
        for i in range(4):
            h = h @ p[f"rm.{i}.kernel"] + p[f"rm.{i}.bias"]
            note(h, et)
            h = torch.relu(h)
        c_r = h
        h = x[:, 1:3]
        for i in range(2):
            h = h @ p[f"om.{i}.kernel"] + p[f"om.{i}.bias"]
            note(h, tower)
            h = torch.relu(h)
        c_o, z = h, None
        for s in range(c["S"]):
            h = torch.cat([c_r, P[src], P[dst]], dim=-1)
            group[0] = "rmp"
            for i in range(2):
                h = h @ p[f"rmp.{i}.kernel"] + p[f"rmp.{i}.bias"]
                note(h, et)
                h = torch.relu(h)
            msg = (h @ p["rmp.2.kernel"] + p["rmp.2.bias"]) * w[s][:, None]
            agg = torch.zeros(len(x), msg.shape[1], dtype=F64).index_add_(0, dst, msg)
            h = torch.cat([c_o, torch.tanh(agg), P], dim=-1) @ p["omp.0.kernel"] + p["omp.0.bias"]
            group[0] = "omp"
            note(h, tower)
            xo = torch.relu(h) @ p["omp.1.kernel"] + p["omp.1.bias"]
            P = torch.tanh(xo[:, 1:] + P)
            z = xo[:, 0]
        group[0] = None
        note((z.abs() - O.LOGIT_CLIP)[:, None], tower)
    return by_group if groups else marg.numpy()


def pick_step_gates(c, sizes=None, seed: int = GATE_SEED, separated=None, tries: int = 40):
    """(gates (S, E), seed): the first seed from `seed` on whose per-step gated margins all exceed TAU and, with
    ``separated`` (a predicate on (case, gates)), for which it holds — the mutant separation of the host test."""
    for s in range(seed, seed + tries):
        g = step_gates_for(len(c["src"]), c["S"], s)
        if np.all(step_gated_margins(c, g, sizes) > TAU) and (separated is None or separated(c, g)):
            return g, s
    raise AssertionError("no gate seed gives every tower a ReLU margin above TAU")


X3_EPS = 2.0 ** -16


def pick_x3_gates(c, sizes=None, seed: int = GATE_SEED, tries: int = 4000):
    """(gates (S, E), seed) for the x3 comparison, which holds the per-step gated x3 run to twice the error of the
    UNGATED x3 run of the same case. That comparison is one of rounding errors: it presumes that rounding moves no ReLU
    across its kink in either run, and one flipped unit changes the gradients by up to 1e-2 of their norm on these
    inputs (tests/test_step_gates_host.py shows it in fp64), 500 times x3's rounding error. TAU covers fp32-class
    rounding, not x3's (16 mantissa bits per operand), and no fixed margin can: a case has a few units within any
    margin x3 would need. What the comparison can and must ask is that the gated inputs are no closer to a kink than
    the inputs of the run that sets the yardstick: the first seed whose gated forward, in each layer group (encoders;
    the step loop's rmp layers; omp.0), keeps at least the smallest pre-activation distance the ungated forward
    (gates ≡ 1) has in that group, or X3_EPS = 2^-16 where that is smaller — the relative rounding of an operand kept
    in 16 mantissa bits, on pre-activations of order 1; a group whose ungated distance happens to be far larger
    need not be matched (team_a's omp.0 has a unit at 2.0e-5 under every gate set, its first three gates being
    fixed) — and TAU per tower, as everywhere."""
    n = len(c["src"])
    floor = step_gated_margins(c, np.ones((c["S"], n), np.float32), sizes, groups=True)
    for s in range(seed, seed + tries):
        g = step_gates_for(n, c["S"], s)
        m = step_gated_margins(c, g, sizes, groups=True)
        if all(m[k] >= min(floor[k], X3_EPS) for k in floor) and np.all(step_gated_margins(c, g, sizes) > TAU):
            return g, s
    raise AssertionError("no gate seed keeps the ungated forward's distance to the ReLU kinks")


_REFS = {}


def oracle(c, gates, loss="bce", key=None, dstate=None):
    """fp64 autograd with the parameters, the objects, the propagation input and the (S, E) gate tensor as leaves.
    Returns a dict: z, state, g (parameter gradients), dprop, dobj, dgate (S, E) — numpy. ``dstate`` (Nn, 100): the
    loss gains Σ dstate·P_S. Computed once per ``key`` and shared; callers leave it unchanged."""
    k = None if key is None else (key, loss, dstate is not None)
    if k is not None and k in _REFS:
        return _REFS[k]
    tp = O.to_torch(c["params"], requires_grad=True)
    src, dst = _tensors(c)
    x = torch.tensor(np.asarray(c["obj"], np.float64).reshape(-1, 3), requires_grad=True)
    pr = torch.tensor(np.asarray(c["prop"], np.float64).reshape(-1, 100), requires_grad=True)
    w = torch.tensor(np.asarray(gates, np.float64), requires_grad=True)
    z, state = forward(tp, x, src, dst, pr, c["S"], w)
    L = RR.loss_of(z, c["tgt"], loss)
    if dstate is not None:
        L = L + (torch.as_tensor(np.asarray(dstate, np.float64)) * state).sum()
    L.backward()
    out = dict(z=z.detach().numpy().copy(), state=state.detach().numpy().copy(),
               g={n: v.grad.numpy().copy() for n, v in tp.items()}, dprop=pr.grad.numpy().copy(),
               dobj=x.grad.numpy().copy(), dgate=w.grad.numpy().copy())
    if k is not None:
        _REFS[k] = out
    return out


def logits_within(z, z_ref) -> bool:
    """The GPU logit criterion: |Δ| <= 1e-5 + 1e-5·|z_ref| everywhere."""
    return bool(np.all(np.abs(z - z_ref) <= 1e-5 + 1e-5 * np.abs(z_ref)))


def tensor_within(got, ref) -> bool:
    """The GPU gradient criterion: max|Δ| <= 1e-5·max|ref| + 1e-8."""
    return bool(np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max() + 1e-8)


def mutant_separated(true, mutant) -> bool:
    """A mutant oracle misses the GPU criteria in the logits AND in at least one gradient tensor of the true one."""
    grads = [tensor_within(mutant["g"][n], true["g"][n]) for n in true["g"]]
    grads += [tensor_within(mutant[k], true[k]) for k in ("dprop", "dobj")]
    return not logits_within(mutant["z"], true["z"]) and not all(grads)


# ------------------------------------------------------------------------------------ the cases of the GPU tests
# name → (case dict with src / dst, tower sizes or None). The inputs are those of tests/test_gpu_input_grad.py and the
# batch builders of tests/test_gpu_gated_team.py; building them needs no GPU.
_CASES = {}


def towers_case(B, N, seed, S=3):
    """test_gpu_gated_team._towers with the edge list of IG._dense_case beside the dense form."""
    import test_gpu_gated_team as GT
    c = dict(GT._towers(B, N, seed, S))
    e = np.array(O.dense_to_edges(c["Rs"], c["Rr"]), np.int64).reshape(-1, 4)
    c["src"], c["dst"] = e[:, 0] * N + e[:, 2], e[:, 0] * N + e[:, 3]
    return c


def case(name):
    """(c, sizes, gates (S, E), seed): the inputs and the picked per-step gates of a GPU case, built once."""
    import test_gpu_input_grad as IG

    def separated(cc, g):
        true = oracle(cc, g, "bce")
        return all(mutant_separated(true, oracle(cc, m(g), "bce")) for m in (rotated, row0))

    if name not in _CASES:
        sizes = None
        if name in ("team_a", "team_b", "wide", "recv"):
            c = IG._case(name)
        elif name == "ragged":
            c, sizes, tes = IG._ragged_case()
            c = dict(c, tes=tes)
        elif name in TOWERS:
            # the shapes of test_gpu_gated_team's `tall` / `pair16`. Their own data seeds (21, 22) leave an encoder
            # ReLU within TAU of its kink whatever the gates are, so the parity cases take the next data seed whose
            # towers all clear TAU (the rule of pick_gates, applied to the inputs)
            B, N, seed0 = TOWERS[name]
            for data_seed in range(seed0, seed0 + 20):
                c = towers_case(B, N, data_seed)
                try:
                    pick_step_gates(c, tries=2)
                    break
                except AssertionError:
                    continue
            else:
                raise AssertionError(f"{name}: no data seed gives every tower a ReLU margin above TAU")
            c["data_seed"] = data_seed
        else:
            raise ValueError(name)
        gates, seed = pick_step_gates(c, sizes, separated=separated)
        _CASES[name] = (c, sizes, gates, seed)
    return _CASES[name]


TOWERS = {"tall": (2, 12, 21), "pair16": (2, 8, 22)}   # name → (B, N, first data seed)
CASES = ["team_a", "team_b", "wide", "recv", "ragged", "tall", "pair16"]
