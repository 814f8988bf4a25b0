"""The order of calls one optimizer step makes, pinned per front end (no GPU).

(a) `Trainer.step` over a recording engine: the ordered engine-protocol calls and the `micro` each
`run_config` call gets, for one batch, two micro-batches and their weighted forms, with and without the
engine's `early_event` (the overlapped two-piece all-reduce, on CPU tensors in a one-rank gloo group).
(b) the `engine.*` launch wrappers replaced by recorders: the ordered wrapper calls of
`KerasModel.train_on_batch`, `KerasModel.evaluate_batch`, `KerasModel._replay_body()` and
`Trainer.replay_body()`, each plain, weighted, clipped and deep-supervised, the replay bodies with the
prologue folded into the forward and as a launch of its own.

The expected lists are literals read from the code as it stood before the front ends shared one step
body: a fold that reorders, drops or adds a call fails here."""
import types

import pytest
import torch
import torch.distributed as dist

from spwgnn_amd import engine as E
from spwgnn_amd.keras_api import PropagationNetwork
from spwgnn_amd.trainer import HipEngine, Trainer

N_NODES, N_PARAMS, STEPS = 5, 8, 5
LAM = (0.1, 0.1, 0.1, 0.2, 0.5)


def _batch():
    return types.SimpleNamespace(n_nodes=N_NODES, n_towers=1, device=torch.device("cpu"))


# ------------------------------------------------------------------------------- (a) Trainer.step
class RecordingEngine:
    """The engine protocol as fake arithmetic on zero tensors; every call is appended to `calls`."""

    def __init__(self):
        self.calls = []
        self.grads = torch.zeros(N_PARAMS)          # one persistent buffer, as HipEngine.grads
        self.out3 = torch.tensor([0.5, 3.0, float(N_NODES)])

    def forward(self, params, batch, run):
        self.calls.append("forward")
        return torch.zeros(batch.n_nodes)

    def loss(self, logits, target):
        self.calls.append("loss")
        return self.out3, torch.zeros_like(logits)

    def loss_weighted(self, logits, target, weights, norm):
        self.calls.append(("loss_weighted", norm))
        return self.out3, torch.zeros_like(logits)

    def backward(self, params, batch, run, dlogits):
        self.calls.append("backward")
        return self.grads

    def adam(self, params, grads, m, v, step, lr, b1, b2, eps, l2, gscale):
        self.calls.append(("adam", step, gscale))


class EarlyRecordingEngine(RecordingEngine):
    def early_event(self):
        self.calls.append("early_event")
        return "reached"


class UnweightedEngine:
    """An engine without loss_weighted (the CPU oracle engines): unweighted steps must not ask for it."""

    def __init__(self):
        inner = RecordingEngine()
        self.calls = inner.calls
        self.forward, self.loss, self.backward, self.adam = inner.forward, inner.loss, inner.backward, inner.adam


@pytest.fixture(scope="module")
def one_rank_group(tmp_path_factory):
    store = dist.FileStore(str(tmp_path_factory.mktemp("gloo") / "store"), 1)
    dist.init_process_group("gloo", store=store, rank=0, world_size=1)
    yield
    dist.destroy_process_group()


W_NODES = [1.0, 0.0, 2.0, 1.0, 1.0]      # 4 non-zero weights
_F, _L, _B, _EV = "forward", "loss", "backward", "early_event"
_LW = ("loss_weighted", 4)
STEP_CASES = {
    # name: (micro-batches, weighted, the calls without early_event)
    "one": (1, False, [_F, _L, _B, ("adam", 1, 1.0)]),
    "two": (2, False, [_F, _L, _B, _F, _L, _B, ("adam", 1, 1.0)]),
    "one_weighted": (1, True, [_F, _LW, _B, ("adam", 1, 1.0)]),
    "two_weighted": (2, True, [_F, _LW, _B, _F, _LW, _B, ("adam", 1, 1.0)]),
}


@pytest.mark.parametrize("early", [False, True], ids=["late", "early"])
@pytest.mark.parametrize("case", list(STEP_CASES))
def test_trainer_step_call_order(one_rank_group, case, early):
    k, weighted, want = STEP_CASES[case]
    if early:   # the event is asked for once, right before the last micro-batch's backward
        at = len(want) - 2
        want = want[:at] + [_EV] + want[at:]
    eng = EarlyRecordingEngine() if early else RecordingEngine()
    tr = Trainer(torch.zeros(N_PARAMS), engine=eng, dropout=0.0)
    tr._early_lo = 4                                 # the early range of this 8-float gradient
    assert tr.distributed and tr._split() is early
    micros, make = [], tr.run_config

    def run_config(micro=0):
        micros.append(micro)
        return make(micro)

    tr.run_config = run_config
    batches, targets = [_batch() for _ in range(k)], [torch.zeros(N_NODES) for _ in range(k)]
    weights = [torch.tensor(W_NODES) for _ in range(k)] if weighted else None
    if k == 1:
        out = tr.step(batches[0], targets[0], weights=weights[0] if weighted else None)
    else:
        out = tr.step(batches, targets, weights=weights)
    assert eng.calls == want
    assert micros == list(range(k))
    assert tr.iterations == 1 and out.shape == (3,) and out.dtype == torch.float32
    # Σ loss_i·n_i / Σ n_i with n_i = 5 nodes, or the 4 non-zero weights over the fake engine's count of 5
    loss = 0.5 * 4 / N_NODES if weighted else 0.5
    assert torch.equal(out, torch.tensor([loss, 3.0 * k, float(N_NODES * k)]))


def test_unweighted_step_needs_no_loss_weighted():
    eng = UnweightedEngine()
    tr = Trainer(torch.zeros(N_PARAMS), engine=eng, dropout=0.0)
    tr.step([_batch(), _batch()], [torch.zeros(N_NODES)] * 2)
    tr.step(_batch(), torch.zeros(N_NODES))
    assert eng.calls == [_F, _L, _B, _F, _L, _B, ("adam", 1, 1.0), _F, _L, _B, ("adam", 2, 1.0)]


# ----------------------------------------------------------------- (b) the engine launch wrappers
def _flags(**kw):
    return "+".join(k for k, v in kw.items() if v is not None and v is not False)


@pytest.fixture
def launches(monkeypatch):
    """Every engine launch wrapper a step can reach, replaced by a recorder (no GPU work): the list of
    "name" or "name:flag+flag" entries — which optional buffers were passed, `accumulate`, and whether the
    forward's RunConfig carries a prologue."""
    seen = []

    def note(name, **kw):
        f = _flags(**kw)
        seen.append(f"{name}:{f}" if f else name)

    def forward(flat, batch, run, ws, logits=None, return_state=False):
        note("forward", prologue=run.prologue)
        return logits if logits is not None else torch.zeros(batch.n_nodes)

    def forward_steps(flat, batch, run, ws, step_logits=None, return_state=False, state=None):
        note("forward_steps", prologue=run.prologue)
        return step_logits if step_logits is not None else torch.zeros(run.mp_steps, batch.n_nodes)

    def bce(logits, targets, scratch, dlogits=None, total3=None, weights3=None, node_weights=None, norm=None):
        assert (total3 is None) == (weights3 is None)
        note("bce", total3=total3, node_weights=node_weights, norm=norm)
        return scratch.out3, dlogits if dlogits is not None else torch.zeros_like(logits)

    def bce_steps(step_logits, targets, step_weights, scratch, dlogits=None, total3=None, weights3=None, total3s=None,
                  node_weights=None, norm=None):
        assert (total3 is None) == (weights3 is None) and tuple(step_weights) == LAM
        note("bce_steps", total3=total3, total3s=total3s, node_weights=node_weights, norm=norm)
        return scratch.out3, scratch.out3s, dlogits if dlogits is not None else torch.zeros_like(step_logits)

    def bce_backward(flat, batch, run, ws, logits, targets, scratch, dlogits=None, total3=None, weights3=None,
                     grads=None, want_dprop=False, node_weights=None, norm=None, dprop=None):
        assert (total3 is None) == (weights3 is None) and grads is not None and dlogits is not None
        note("bce_backward", total3=total3, node_weights=node_weights, norm=norm)
        return scratch.out3, dlogits, grads, None

    def backward(flat, batch, run, ws, dlogits, grads=None, want_dprop=False, dstate=None):
        note("backward")
        return grads, None

    def backward_steps(flat, batch, run, ws, dstep_logits, grads=None, want_dprop=False, dstate=None, dprop=None):
        note("backward_steps")
        return grads, None

    def adam(params, grads, m, v, step, lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-7, l2=0.0, grad_scale=1.0):
        note("adam")

    def adam_clipped(params, grads, m, v, step, clip, lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-7, l2=0.0,
                     grad_scale=1.0, clipnorm=0.0, clipvalue=0.0, skip_nonfinite=False, accumulate=False):
        assert clipnorm == 1.0
        note("adam_clipped", accumulate=accumulate)
        return clip.out4

    def adam_dev(params, grads, m, v, step_dev, lr_table, beta1=0.9, beta2=0.999, eps=1e-7, l2=0.0, grad_scale=1.0):
        note("adam_dev")

    def adam_clipped_dev(params, grads, m, v, step_dev, lr_table, clip, beta1=0.9, beta2=0.999, eps=1e-7, l2=0.0,
                         grad_scale=1.0, clipnorm=0.0, clipvalue=0.0, skip_nonfinite=False, accumulate=False):
        assert clipnorm == 1.0
        note("adam_clipped_dev", accumulate=accumulate)
        return clip.out4

    def step_advance(key_dev, step_dev, mode=0, seed=0, rank=0):
        note("step_advance")

    for fn in (forward, forward_steps, bce, bce_steps, bce_backward, backward, backward_steps, adam, adam_clipped,
               adam_dev, adam_clipped_dev, step_advance):
        monkeypatch.setattr(E, fn.__name__, fn)
    return seen


OPTIONS = {"plain": {}, "weighted": {}, "clipnorm": {"clipnorm": 1.0}, "steps": {"step_loss_weights": LAM}}

TRAIN_ON_BATCH = {
    "plain": ["forward", "bce", "backward", "adam"],
    "weighted": ["forward", "bce:node_weights", "backward", "adam"],
    "clipnorm": ["forward", "bce", "backward", "adam_clipped"],
    "steps": ["forward_steps", "bce_steps", "backward_steps", "adam"],
}
EVALUATE_BATCH = {
    "plain": ["forward", "bce"],
    "weighted": ["forward", "bce:node_weights+norm"],
    "clipnorm": ["forward", "bce"],
    "steps": ["forward_steps", "bce_steps"],
}
# the replay bodies with the prologue folded; unfolded, "step_advance" leads and the forward carries none
KERAS_REPLAY = {
    "plain": ["forward:prologue", "bce_backward:total3", "adam_dev"],
    "weighted": ["forward:prologue", "bce_backward:total3+node_weights+norm", "adam_dev"],
    "clipnorm": ["forward:prologue", "bce_backward:total3", "adam_clipped_dev:accumulate"],
    "steps": ["forward_steps:prologue", "bce_steps:total3+total3s", "backward_steps", "adam_dev"],
}
TRAINER_REPLAY = {
    "plain": ["forward:prologue", "bce_backward", "adam_dev"],
    "weighted": ["forward:prologue", "bce_backward:node_weights+norm", "adam_dev"],
    "clipnorm": ["forward:prologue", "bce_backward", "adam_clipped_dev"],
    "steps": ["forward_steps:prologue", "bce_steps", "backward_steps", "adam_dev"],
}


def _unfolded(want):
    return ["step_advance"] + [w.replace(":prologue", "") for w in want]


def _model(opt):
    return PropagationNetwork(device="cpu", **OPTIONS[opt]).getModel(4)


def _w(opt):
    return torch.tensor(W_NODES) if opt == "weighted" else None


@pytest.mark.parametrize("opt", list(OPTIONS))
def test_train_on_batch_launch_order(launches, opt):
    model = _model(opt)
    out3 = model.train_on_batch(_batch(), torch.zeros(N_NODES), _w(opt))
    assert launches == TRAIN_ON_BATCH[opt]
    assert out3.shape == (3,) and model.iterations == 1


@pytest.mark.parametrize("opt", list(OPTIONS))
def test_evaluate_batch_launch_order(launches, opt):
    model = _model(opt)
    out3 = model.evaluate_batch(_batch(), torch.zeros(N_NODES), _w(opt), 4 if opt == "weighted" else None)
    assert launches == EVALUATE_BATCH[opt]
    assert out3.shape == (3,) and model.iterations == 0


def _replay_args(opt):
    z, dz = torch.zeros(N_NODES), torch.zeros(N_NODES)
    kw = {"weights": torch.tensor(W_NODES), "norm": torch.tensor([4.0])} if opt == "weighted" else {}
    return (_batch(), torch.zeros(N_NODES), E.Workspace("cpu"), E.BceScratch("cpu"), z, dz), kw


@pytest.mark.parametrize("fold", [True, False], ids=["folded", "unfolded"])
@pytest.mark.parametrize("opt", list(OPTIONS))
def test_keras_replay_body_launch_order(launches, monkeypatch, opt, fold):
    monkeypatch.setattr(E, "FOLD_PROLOGUE", fold)
    model = _model(opt)
    model._ctr = types.SimpleNamespace(key=torch.zeros(1, dtype=torch.int64), step=torch.zeros(1, dtype=torch.int32),
                                       lr_table=torch.zeros(4))
    model._w3[1] = torch.tensor([1.0, 1.0, 1.0], dtype=torch.float64)
    body = model._replay_body()
    args, kw = _replay_args(opt)
    body(*args, **kw)
    want = KERAS_REPLAY[opt] if fold else _unfolded(KERAS_REPLAY[opt])
    assert launches == want
    del launches[:]
    body(*args, pre=E.Prologue() if fold else None, **kw)      # a later step of the same geometry: the same launches
    assert launches == want


@pytest.mark.parametrize("fold", [True, False], ids=["folded", "unfolded"])
@pytest.mark.parametrize("opt", list(OPTIONS))
def test_trainer_replay_body_launch_order(launches, monkeypatch, opt, fold):
    monkeypatch.setattr(E, "FOLD_PROLOGUE", fold)
    tr = Trainer(torch.zeros(N_PARAMS), engine=HipEngine("cpu"), **OPTIONS[opt])
    body = tr.replay_body(N_NODES, weighted=opt == "weighted")
    args, kw = _replay_args(opt)
    body(*args, **kw)
    want = TRAINER_REPLAY[opt] if fold else _unfolded(TRAINER_REPLAY[opt])
    assert launches == want
    del launches[:]
    body(*args, pre=E.Prologue() if fold else None, **kw)
    assert launches == want
