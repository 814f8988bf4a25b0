"""Host side of the final-state interface (spwgnn_forward_state / spwgnn_backward_state):
the exported symbols, the contract engine.backward enforces for a state cotangent, and how
_PropagationFn hands the two output gradients to the engine. No GPU."""
import ctypes as C
import re
import types
from pathlib import Path

import pytest
import torch

from spwgnn_amd import _lib, engine as E
from spwgnn_amd import network as NW
from spwgnn_amd.network import GraphNetwork

HEADER = Path(__file__).resolve().parents[1] / "include" / "spwgnn.h"


def _header_args(name):
    """The parameter count of `name`'s declaration in include/spwgnn.h (comments removed)."""
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    m = re.search(r"\bint32_t\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared in spwgnn.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name,nargs", [("spwgnn_forward_state", 8), ("spwgnn_backward_state", 10)])
def test_symbols_exported_with_documented_argument_counts(name, nargs):
    L = _lib.lib()
    assert L.spwgnn_version() == 8                      # added within ABI 8: no version change
    fn = getattr(L, name)                               # AttributeError: the library does not export it
    assert C.cast(fn, C.c_void_p).value
    assert len(fn.argtypes) == nargs and fn.restype is C.c_int32
    assert _header_args(name) == nargs
    # one argument more than the call each extends, in the documented place (before the outputs / stream)
    assert _header_args("spwgnn_forward") == 7 and _header_args("spwgnn_backward") == 9
    assert _lib.K_STATE == 14 and "#define SPWGNN_K_STATE 14" in HEADER.read_text()


def test_null_arguments_are_rejected_before_any_device_work():
    L = _lib.lib()
    assert L.spwgnn_forward_state(None, None, None, None, 0, None, None, None) == _lib.E_ARG
    assert L.spwgnn_backward_state(None, None, None, None, 0, None, None, None, None, None) == _lib.E_ARG


def _stub_batch(n):
    return types.SimpleNamespace(n_nodes=n, device=torch.device("cpu"))


def test_backward_dstate_needs_a_forward_that_returned_the_state():
    ws = E.Workspace("cpu")
    assert ws.has_state is False
    run = E.RunConfig(2, training=True)
    with pytest.raises(ValueError, match="return_state"):
        E.backward(torch.zeros(4), _stub_batch(7), run, ws, torch.zeros(7), dstate=torch.zeros(7, 100))


def test_backward_dstate_shape_dtype_device_errors():
    ws = E.Workspace("cpu")
    ws.has_state = True          # as forward(..., return_state=True) leaves it
    run = E.RunConfig(2, training=True)
    b = _stub_batch(7)
    flat, dz = torch.zeros(4), torch.zeros(7)
    for bad in (torch.zeros(7, 99), torch.zeros(6, 100), torch.zeros(700), torch.zeros(1, 7, 100), [[0.0] * 100] * 7):
        with pytest.raises(ValueError, match=r"\(7, 100\)"):
            E.backward(flat, b, run, ws, dz, dstate=bad)
    for bad in (torch.zeros(7, 100, dtype=torch.float64), torch.zeros(7, 100, dtype=torch.bfloat16),
                torch.zeros(7, 100, dtype=torch.int32)):
        with pytest.raises(ValueError, match="float32"):
            E.backward(flat, b, run, ws, dz, dstate=bad)
    with pytest.raises(_lib.SpwgnnError, match="HIP device tensor"):      # _require_gpu's error
        E.backward(flat, b, run, ws, dz, dstate=torch.zeros(7, 100))


def test_inference_backward_still_refused_first():
    ws = E.Workspace("cpu")
    with pytest.raises(_lib.SpwgnnError, match="training forward"):
        E.backward(torch.zeros(4), _stub_batch(7), E.RunConfig(2), ws, torch.zeros(7), dstate=torch.zeros(7, 100))


@pytest.fixture
def engine_calls(monkeypatch):
    """engine.forward / backward / backward_inputs replaced by recorders (no GPU work)."""
    seen = {"forward": [], "backward": []}

    def forward(flat, batch, run, ws, logits=None, return_state=False):
        seen["forward"].append(return_state)
        z = torch.zeros(batch.n_nodes)
        return (z, torch.zeros(batch.n_nodes, 100)) if return_state else z

    def backward(flat, batch, run, ws, dlogits, grads=None, want_dprop=False, dstate=None):
        seen["backward"].append((dlogits.clone(), None if dstate is None else dstate.clone(), want_dprop))
        return torch.zeros_like(flat), (torch.zeros(batch.n_nodes, 100) if want_dprop else None)

    monkeypatch.setattr(E, "forward", forward)
    monkeypatch.setattr(E, "backward", backward)
    return seen


def _apply(want_state, prop_grad=False):
    flat = torch.zeros(8, requires_grad=True)
    prop = torch.zeros(5, 100, requires_grad=prop_grad)
    run = E.RunConfig(2, training=True)
    out = NW._PropagationFn.apply(flat, prop, torch.zeros(0), _stub_batch(5), run, E.Workspace("cpu"), want_state)
    return flat, prop, out


def test_propagation_fn_none_state_gradient_is_dstate_none(engine_calls):
    flat, _, (z, state) = _apply(True)
    assert engine_calls["forward"] == [True] and state.shape == (5, 100) and state.requires_grad
    (z * torch.arange(5.0)).sum().backward()            # the state is unused: its gradient is missing
    (dz, dstate, want_dprop), = engine_calls["backward"]
    assert dstate is None and not want_dprop
    assert torch.equal(dz, torch.arange(5.0))
    assert flat.grad is not None


def test_propagation_fn_none_logits_gradient_is_zeros(engine_calls):
    _, prop, (z, state) = _apply(True, prop_grad=True)
    w = torch.arange(500.0).reshape(5, 100)
    (state * w).sum().backward()                        # the logits are unused
    (dz, dstate, want_dprop), = engine_calls["backward"]
    assert torch.equal(dz, torch.zeros(5)) and dz.dtype == torch.float32
    assert torch.equal(dstate, w) and want_dprop
    assert prop.grad is not None and prop.grad.shape == (5, 100)


def test_propagation_fn_both_gradients_and_the_plain_form(engine_calls):
    _, _, (z, state) = _apply(True)
    (z.sum() + 2 * state.sum()).backward()
    (dz, dstate, _), = engine_calls["backward"]
    assert torch.equal(dz, torch.ones(5)) and torch.equal(dstate, torch.full((5, 100), 2.0))
    engine_calls["backward"].clear()
    _, _, z = _apply(False)                             # one output, as before the state existed
    assert isinstance(z, torch.Tensor) and engine_calls["forward"] == [True, False]
    z.sum().backward()
    (dz, dstate, _), = engine_calls["backward"]
    assert dstate is None and torch.equal(dz, torch.ones(5))


def test_rollout_argument_checks():
    net = GraphNetwork(device="cpu")
    with pytest.raises(ValueError, match="at least one frame"):
        net.rollout([])
    with pytest.raises(ValueError, match="same nodes"):
        net.rollout([_stub_batch(5), _stub_batch(6)])
    with pytest.raises(ValueError, match="one entry"):
        net.rollout([_stub_batch(5), _stub_batch(5)], objects=[None])
