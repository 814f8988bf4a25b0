"""CPU: the host side of spwgnn_backward_inputs (ABI 8) — export, version, the argument statuses that
come back before any device work — and the fp64 identities of d(loss)/d(objects) on the oracle that
the GPU tests (tests/test_gpu_input_grad.py) rest on."""
import ctypes as C

import numpy as np
import torch

from oracle import model as O
from spwgnn_amd import _lib, data as D


def test_symbol_and_version():
    lib = _lib.lib()
    assert hasattr(lib, "spwgnn_backward_inputs")
    assert lib.spwgnn_version() == 8 == _lib.ABI_VERSION
    assert _lib.K_INPUT_BWD == 12


def _structs(training=1):
    """A well-formed batch / run pair whose pointers are never followed: every check below fails (or
    would pass) before the library touches the device."""
    b = _lib.BatchC()
    b.n_towers, b.n_nodes, b.n_wtiles, b.n_eblocks, b.nw_max, b.flags = 2, 12, 2, 2, 6, 0
    fake = 0x1000
    b.pos = b.node_tower = b.node_local = b.wtile = b.edge_src = b.edge_dst = b.blk_csr = fake
    r = _lib.RunC()
    r.mp_steps, r.training, r.dropout, r.math = 3, training, 0.0, _lib.MATH_X6
    return b, r, fake


def test_statuses_without_a_device():
    lib = _lib.lib()
    b, r, fake = _structs()
    need = lib.spwgnn_workspace_bytes(b.n_nodes, b.n_eblocks, r.mp_steps, 1)
    assert need > 0
    call = lambda params, bb, rr, ws, nbytes, dpos: lib.spwgnn_backward_inputs(
        params, C.byref(bb) if bb is not None else None, C.byref(rr) if rr is not None else None, ws, nbytes, dpos, None)
    assert call(None, b, r, fake, need, fake) == _lib.E_ARG          # null params
    assert call(fake, b, r, None, need, fake) == _lib.E_ARG          # null workspace
    assert call(fake, b, r, fake, need, None) == _lib.E_ARG          # null dpos
    assert call(fake, b, r, fake, need, fake + 4) == _lib.E_ARG      # dpos rows are 16-byte vectors
    assert call(fake, None, r, fake, need, fake) == _lib.E_ARG       # null batch
    assert call(fake, b, None, fake, need, fake) == _lib.E_ARG       # null run
    assert call(fake, b, r, fake, need - 1, fake) == _lib.E_WORKSPACE
    bi, ri, _ = _structs(training=0)
    assert call(fake, bi, ri, fake, need, fake) == _lib.E_NOTRAIN    # the same answer as spwgnn_backward
    assert lib.spwgnn_backward(fake, C.byref(bi), C.byref(ri), fake, need, fake, fake, None, None) == _lib.E_NOTRAIN
    bad, _, _ = _structs()
    bad.n_wtiles = 0
    assert call(fake, bad, r, fake, need, fake) == -2                # validate(): SPWGNN_E_SHAPE
    assert b"training" in lib.spwgnn_strerror(_lib.E_NOTRAIN)


def test_oracle_identities_of_the_position_gradient():
    """fp64, thresholded 5-box towers with a non-zero propagation input:
      * the formulas of DESIGN.md §3zj — dobj from q_e = dz1_e·W_rm0ᵀ (+ at the receiver, − at the
        sender) and p_n = dzo1_n·W_om0ᵀ, with dz1 / dzo1 taken from autograd — equal autograd's d/d objects;
      * translation invariance: per tower Σ_n dobj[n].x = 0;
      * Euler's identity: Σ obj·dobj = <W_rm0, dW_rm0> + <W_om0, dW_om0>."""
    B, N, S = 3, 5, 4
    params = O.random_params(8)
    obj, Rs, Rr, prop, tgt = D.synthetic_batch(B, N, seed=4, fully_connected=False)
    prop = np.random.default_rng(1).normal(0, 0.3, prop.shape)
    e = np.array(O.dense_to_edges(Rs, Rr), np.int64).reshape(-1, 4)
    src, dst = torch.as_tensor(e[:, 0] * N + e[:, 2]), torch.as_tensor(e[:, 0] * N + e[:, 3])
    tp = O.to_torch(params, requires_grad=True)
    x = torch.tensor(obj.reshape(-1, 3), dtype=torch.float64, requires_grad=True)
    # forward_gather with its two first layers spelled out, so their pre-activations can be read
    z1 = (x[dst, 0:2] - x[src, 0:2]) @ tp["rm.0.kernel"] + tp["rm.0.bias"]
    zo1 = x[:, 1:3] @ tp["om.0.kernel"] + tp["om.0.bias"]
    z1.retain_grad()
    zo1.retain_grad()
    h = torch.relu(z1)
    for i in (1, 2, 3):
        h = h @ tp[f"rm.{i}.kernel"] + tp[f"rm.{i}.bias"]
        if i < 3:
            h = torch.relu(h)
    c_r = torch.relu(h)
    c_o = torch.relu(torch.relu(zo1) @ tp["om.1.kernel"] + tp["om.1.bias"])
    Pm = torch.as_tensor(prop.reshape(-1, 100))
    for _ in range(S):
        m = O._mlp(torch.cat([c_r, Pm[src], Pm[dst]], dim=-1), tp, "rmp")
        agg = torch.zeros(Pm.shape[0], m.shape[1], dtype=m.dtype).index_add(0, dst, m)
        xo = O._mlp(torch.cat([c_o, torch.tanh(agg), Pm], dim=-1), tp, "omp")
        Pm = torch.tanh(xo[:, 1:] + Pm)
    zl = xo[:, 0]
    with torch.no_grad():   # the spelled-out forward is forward_gather
        ref = O.forward_gather(O.to_torch(params), x.detach(), src, dst, torch.as_tensor(prop.reshape(-1, 100)), S)
    assert torch.allclose(zl.detach(), ref, rtol=0, atol=1e-13)
    O.keras_bce_from_logits(zl, torch.as_tensor(tgt, dtype=torch.float64).reshape(-1)).backward()
    dobj = x.grad.numpy()
    q = (z1.grad @ tp["rm.0.kernel"].detach().T).numpy()     # (Ne, 2)
    p = (zo1.grad @ tp["om.0.kernel"].detach().T).numpy()    # (Nn, 2)
    want = np.zeros_like(dobj)
    np.add.at(want[:, 0:2], dst.numpy(), q)
    np.subtract.at(want[:, 0:2], src.numpy(), q)
    want[:, 1] += p[:, 0]
    want[:, 2] = p[:, 1]
    scale = np.abs(dobj).max()
    assert scale > 0 and np.abs(want - dobj).max() <= 1e-14 * scale
    assert np.abs(dobj[:, 0].reshape(B, N).sum(1)).max() <= 1e-14 * scale
    euler = float((x.detach().numpy() * dobj).sum())
    rhs = float((tp["rm.0.kernel"].detach() * tp["rm.0.kernel"].grad).sum()
                + (tp["om.0.kernel"].detach() * tp["om.0.kernel"].grad).sum())
    assert abs(euler - rhs) <= 1e-13 * max(abs(rhs), scale)
